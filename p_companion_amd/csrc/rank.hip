// The rank of a known product among all products of its type (PCompanionInference.rank_targets / evaluate_catalogue): for
// row r with type c = types[r] and target y = targets[r], g = <proj[r], table[y]> and
//   rank_out[r] = #{ p of type c : s_p > g  or  (s_p == g and p < y) },   s_p = <proj[r], table[p]>,
// the position y takes in the list pc_retrieve_topk_grouped serves for the row (score descending, product index ascending).
// retrieve.hip's schedule with its selection replaced by a compare and an integer add: no score matrix, no partial lists.
//
//   plan    (grouped_plan.hip: count, scan, place) the rows grouped by type, the work items; rank_out[r] = 0, or -1 for a
//           row without a type (types[r] < 0) or with an id out of range (counted in *bad_count)
//   rank    grid-stride over the work items (type, slice, tile): query tile -> LDS; the tile's own targets scored first (wave
//           w: the 16 targets of row group w as one MFMA column block, g = its diagonal); then the slice's candidates in
//           chunks of 64 (one 16-candidate column group per wave, rows straight from global into registers, the next
//           chunk's in flight), every accumulator register compared with its row's g, integer counts per lane; at the end a
//           16-lane sum, the four waves' sums through LDS, one integer atomic per (row, slice).
//
// Determinism: g and every s_p are the MFMA k-chain of retrieve.hip's rg_score_kernel (step j, element e and k-lane h cover
// dimension 16 j + 4 h + e; the chain's order depends on the dimension index alone), so s_y and g are the same bits and a
// (row, product) score is bit for bit the one the retrieval orders by.  The count is a sum of integers: it does not depend
// on the slices, on the order of the rows in a tile, or on the order of type_col inside a type.  No float atomics.
// The plan (count, scan, place), the slice plan and the order predicate are the family's (grouped_plan.h), the work-item
// decode and the query-tile load too (grouped_select.h).
#include "common.h"
#include "grouped_rank.h"          // rk_rank_body, rk_stream: the skeleton and the stream (nearest.hip's and where_rank.hip's too)

// rk_rank_body without a bias and without a predicate.
template <int D>
// three waves per SIMD at D = 128 and two at D = 256, as rg_score_kernel
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(D == 128 ? 3 : 2))) void rk_rank_kernel(
    const float* __restrict__ proj, const int32_t* __restrict__ targets, const int32_t* __restrict__ type_rowptr,
    const int32_t* __restrict__ type_col, const float* __restrict__ table, int n_types, int S, const int32_t* __restrict__ cnt,
    const int32_t* __restrict__ row_start, const int64_t* __restrict__ item_start, const int32_t* __restrict__ order,
    int32_t* __restrict__ rank_out) {
    rk_rank_body<D, false, false>(proj, targets, type_rowptr, type_col, table, nullptr, n_types, S, cnt, row_start, item_start,
                                  order, rank_out, pc_row_where{});
}

extern "C" size_t pc_rank_grouped_workspace_bytes(int rows, int n_types, int slices) {
    if (rows <= 0 || n_types <= 0 || slices < 0 || slices > RG_MAX_SLICES) return 0;
    return rg_ws_carve(nullptr, rows, n_types, 0, rg_slices(slices)).bytes;
}

extern "C" int pc_rank_grouped(const float* proj, const int32_t* types, const int32_t* targets, int rows,
                               const int32_t* type_rowptr, const int32_t* type_col, const float* table, int n_types,
                               int num_products, int dim, int slices, int32_t* rank_out, int32_t* bad_count, void* ws,
                               size_t ws_bytes, void* stream) {
    RkStart s;
    PC_TRY(rk_begin(s, proj && table, nullptr, types, targets, nullptr, rows, type_rowptr, type_col, n_types, num_products, nullptr,
                    nullptr, 0, nullptr, dim, slices, rank_out, bad_count, ws, ws_bytes, stream));
    const RgPlan& pl = s.w.plan;
    rk_dispatch(dim, false, [&](auto d, auto) {
        PC_LAUNCH(rk_rank_kernel<decltype(d)::value>, dim3(s.grid), dim3(256), 0, s.st, proj, targets, type_rowptr, type_col, table,
                  n_types, s.S, pl.cnt, pl.row_start, pl.item_start, pl.order, rank_out);
    });
    return pc_launch_status();
}
