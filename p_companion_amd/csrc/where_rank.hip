// The rank of a known product among the products of its type that pass the row's predicate on per-product attributes, over
// the fp32 table (pc_rank_grouped_where; ops.rank_grouped_where, PCompanionInference.rank_targets_where /
// evaluate_catalogue_where and SimilarProducts.rank_pairs_where / evaluate_pairs_where in inference.py): for row r with type
// c = types[r], target y = targets[r] and predicate w_r (pc_row_where: a band on value[p], masks on flags[p]),
//   s_p = fl(d(r, p) + bias[p])  (bias null: s_p = d(r, p)),   g = s_y,
//   rank_out[r] = #{ p of type c : p passes w_r, p not in the row's list : s_p > g  or  (s_p == g and p < y) },
// the position y takes in the list pc_retrieve_list_grouped_where / pc_retrieve_list_grouped_biased_where serves for the row,
// and -1 where the unfiltered ranks give -1 or y itself fails w_r.  rank.hip's / nearest.hip's schedule and count with the
// test INSIDE the count: a predicate can fail 99 % of a type, so nothing is counted over the whole type and subtracted.
// A unit of its own, as rank_exclude.hip: inside rank.hip or nearest.hip the new kernels would move the existing ones.
//
//   plan     grouped_plan.hip as it is (tiles of TM = 8192 / D rows); rank_out[r] = 0, or -1 for a row without a type or with
//            an id out of range (counted in *bad_count)
//   rank     wr_rank_kernel: grid-stride over the work items (type, slice, tile): query tile -> LDS; the tile's own targets
//            scored first (wave w: the 16 targets of row group w as one MFMA column block, g = its diagonal, plus bias[y]); the
//            rows' lo / hi / need / deny read through order[p0 + row] once per work item into LDS beside gs / ys (a part that is
//            not given: -inf, +inf, 0, 0); then the slice's candidates in chunks of 64, value[pid] / flags[pid] (and bias[pid])
//            gathered a chunk ahead with the product id; a candidate is counted where its score beats (or ties and precedes) the
//            row's g AND it passes that row's predicate (wr_count, where_rank.h); integer counts per lane, a 16-lane sum, the
//            four waves' sums through LDS, one integer atomic per (row, slice)
//   post     wr_post_kernel, one wave per row, in EVERY call: -1 for a target that fails its own predicate (written here, after
//            all slices' atomics have landed: the launch order on the stream) and, with lists, rk_exclude_kernel's post-pass
//            through the same chain, which decrements only for list entries that pass the predicate -- a failing entry was never
//            counted
//
// Determinism: d is rk_chain (rank_chain.h), the dimensions in index order, so a (row, product) score has the bits of
// pc_retrieve_list_grouped[_biased][_where] and of pc_rank_grouped / _biased; the predicate reads no score; the count is a sum
// of integers: it does not depend on the slices, on the order of the rows in a tile or on the order of type_col inside a type.
// With every array of the filter absent every product passes: the unfiltered entries' output.  No float atomics, no readback.
#include "common.h"
#include "grouped_rank.h"          // rk_rank_body, wr_stream, rk_post: the fp32 skeleton, the stream with the test, the post-pass

// Work item w = (type t, slice s, tile j) (rg_decode).  The four waves' counts meet in LDS: one integer atomic per (row, slice).
// Waves per SIMD as rk_rank_kernel / nb_rank_kernel: three at D = 128, two at D = 256.
template <int D, bool BIAS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(D == 128 ? 3 : 2))) void wr_rank_kernel(
    const float* __restrict__ proj, const int32_t* __restrict__ targets, const int32_t* __restrict__ type_rowptr,
    const int32_t* __restrict__ type_col, const float* __restrict__ table, const float* __restrict__ bias, int n_types, int S,
    const int32_t* __restrict__ cnt, const int32_t* __restrict__ row_start, const int64_t* __restrict__ item_start,
    const int32_t* __restrict__ order, int32_t* __restrict__ rank_out, pc_row_where wh) {
    rk_rank_body<D, BIAS, true>(proj, targets, type_rowptr, type_col, table, bias, n_types, S, cnt, row_start, item_start, order,
                                rank_out, wh);
}

// The row post-pass, one wave per row, after wr_rank_kernel on the stream: every slice's atomic has landed.
//   A row the plan left at -1 stays so.  With lists (row_key != null; wave-uniform): a key outside [-1, n_keys) is no list and
//   is counted in *bad_count, and cand_type[y] != types[r] is rank -1, as in rk_exclude_kernel.  A target that fails its own
//   row's predicate: rank -1.  Then rk_exclude_kernel's pass: the row's proj is row 0 of the A operand, the B operand blocks of
//   16 columns -- column 0 of the first block the target y, then the row's list ex_col[elo, ehi) -- through rk_chain, so g and
//   every s_e are the bits wr_rank_kernel compared.  A list entry e with cand_type[e] == types[r] that passes the predicate and
//   has rg_better(s_e, e, g, y) was counted there: one off (a failing entry never was).  e == y: rank -1.  An id outside
//   [0, num_products) is passed over.  Integer work, the row's wave the one writer.
template <int D, bool BIAS>
__global__ __launch_bounds__(64) void wr_post_kernel(const float* __restrict__ proj, const int32_t* __restrict__ types,
                                                     const int32_t* __restrict__ targets, const int32_t* __restrict__ row_key,
                                                     const int32_t* __restrict__ ex_rowptr, const int32_t* __restrict__ ex_col,
                                                     int n_keys, const int32_t* __restrict__ cand_type,
                                                     const float* __restrict__ table, const float* __restrict__ bias,
                                                     int num_products, pc_row_where wh, int32_t* __restrict__ rank_out,
                                                     int32_t* __restrict__ bad_count) {
    __shared__ __attribute__((aligned(16))) typename RkScoreF32<D>::Image q;
    rk_post<D, RkScoreF32<D>, BIAS, true>(q, proj, types, targets, row_key, ex_rowptr, ex_col, n_keys, cand_type, table, bias,
                                          num_products, wh, rank_out, bad_count);
}

extern "C" size_t pc_rank_grouped_where_workspace_bytes(int rows, int n_types, int slices) {
    return pc_rank_grouped_workspace_bytes(rows, n_types, slices);
}

extern "C" int pc_rank_grouped_where(const float* proj, const int32_t* types, const int32_t* targets, const int32_t* row_key,
                                     int rows, const int32_t* type_rowptr, const int32_t* type_col, const float* table,
                                     const float* bias, int n_types, int num_products, const int32_t* ex_rowptr,
                                     const int32_t* ex_col, int n_keys, const int32_t* cand_type, int dim, int slices,
                                     int32_t* rank_out, int32_t* bad_count, const pc_row_where* where, void* ws, size_t ws_bytes,
                                     void* stream) {
    RkStart s;
    // (args_ok: a null filter, or a half-given one, too)
    PC_TRY(rk_begin(s, proj && table && wr_where_ok(where), nullptr, types, targets, row_key, rows, type_rowptr, type_col, n_types,
                    num_products, ex_rowptr, ex_col, n_keys, cand_type, dim, slices, rank_out, bad_count, ws, ws_bytes, stream));
    const RgPlan& pl = s.w.plan;
    rk_dispatch(dim, bias != nullptr, [&](auto d, auto b) {
        constexpr int D = decltype(d)::value;
        constexpr bool BIAS = decltype(b)::value;
        PC_LAUNCH((wr_rank_kernel<D, BIAS>), dim3(s.grid), dim3(256), 0, s.st, proj, targets, type_rowptr, type_col, table, bias,
                  n_types, s.S, pl.cnt, pl.row_start, pl.item_start, pl.order, rank_out, *where);
        PC_LAUNCH((wr_post_kernel<D, BIAS>), dim3(rows), dim3(64), 0, s.st, proj, types, targets, row_key, ex_rowptr, ex_col,
                  n_keys, cand_type, table, bias, num_products, *where, rank_out, bad_count);
    });
    return pc_launch_status();
}
