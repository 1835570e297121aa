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
#include "grouped_select.h"        // the item decode, the tile load
#include "grouped_plan.h"          // rg_better
#include "rank_chain.h"
#include "where_rank.h"

// One work item's candidate stream for a tile of NG 16-row groups (nb_stream with the test in the count): accumulator register
// k of row group g holds query row g * 16 + 4 h + k; gs / ys / wq: the rows' target scores, targets and predicates.  b / pid /
// bs / a / f: the first chunk's rows, product ids, terms and attributes, pidn: the second chunk's ids (-1: a column past the
// slice's end; its b is product 0's row, its attributes are entry 0's, and nothing of it is counted).  Leaves the wave's counts
// in part[wv][row].
template <int D, int NG, bool BIAS>
__device__ __forceinline__ void wr_stream(const float* q, const float* gs, const int* ys, const WrRow* wq, int (*part)[8192 / D],
                                          const int32_t* __restrict__ type_col, const float* __restrict__ table,
                                          const float* __restrict__ bias, const pc_row_where& wh, int cb0, int ce,
                                          float4 (&b)[D / 16], int pid, int pidn, float bs, float a, int f, int wv, int c, int h) {
    int cn[NG][4];
#pragma unroll
    for (int g = 0; g < NG; g++)
#pragma unroll
        for (int k = 0; k < 4; k++) cn[g][k] = 0;
    for (int cb = cb0; cb < ce; cb += RG_CHUNK) {
        const int cc = cb + 2 * RG_CHUNK + wv * 16 + c;
        const int pidnn = cc < ce ? type_col[cc] : -1;
        // the next chunk's rows replace this one's step by step while it is scored
        const float4* next = reinterpret_cast<const float4*>(table + (size_t)max(pidn, 0) * D) + h;
        f32x4 acc[NG];
#pragma unroll
        for (int g = 0; g < NG; g++) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
        rk_chain<D, NG>(q, 0, b, next, acc, c, h);
        wr_count<NG, BIAS>(acc, bs, gs, cn, ys, wq, pid, a, f, h);
        // the next chunk's term and attributes, with its product id, a chunk ahead
        if constexpr (BIAS) bs = bias[max(pidn, 0)];
        a = wr_value(wh, pidn);
        f = wr_flags(wh, pidn);
        pid = pidn;
        pidn = pidnn;
    }
    wr_reduce<NG, 8192 / D>(cn, part, wv, c, h);
}

// Work item w = (type t, slice s, tile j) (rg_decode).  The four waves' counts meet in LDS: one integer atomic per (row, slice).
// Waves per SIMD as rk_rank_kernel / nb_rank_kernel: three at D = 128, two at D = 256.
template <int D, bool BIAS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(D == 128 ? 3 : 2))) void wr_rank_kernel(
    const float* __restrict__ proj, const int32_t* __restrict__ targets, const int32_t* __restrict__ type_rowptr,
    const int32_t* __restrict__ type_col, const float* __restrict__ table, const float* __restrict__ bias, int n_types, int S,
    const int32_t* __restrict__ cnt, const int32_t* __restrict__ row_start, const int64_t* __restrict__ item_start,
    const int32_t* __restrict__ order, int32_t* __restrict__ rank_out, pc_row_where wh) {
    constexpr int TM = 8192 / D;             // rows per tile: 64 (D = 128) or 32 (D = 256): a 32 KB query tile
    constexpr int RG = TM / 16;              // 16-row groups (at most one per wave)
    constexpr int QS = RK_QS(D);             // padded LDS row
    constexpr int NB = D / 16;               // float4 operands per lane per candidate
    __shared__ __attribute__((aligned(16))) float q[TM * QS];
    __shared__ __attribute__((aligned(16))) float gs[TM];            // the rows' target scores
    __shared__ __attribute__((aligned(16))) int ys[TM];              // the rows' targets
    __shared__ WrRow wq[TM];                                         // the rows' predicates
    __shared__ int part[4][TM];                                      // the waves' counts
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c = lane & 15, h = lane >> 4;
    const int64_t n_items = item_start[n_types];
    for (int64_t w = blockIdx.x; w < n_items; w += gridDim.x) {
        const RgItem it = rg_decode<TM>(w, item_start, cnt, row_start, type_rowptr, n_types, S);
        const int p0 = it.p0, valid = it.valid, rg = it.rg, cb0 = it.cb0, ce = it.ce;

        __syncthreads();                                  // the previous item's readers of q / wq / part are done
        rg_load_tile<D, QS>(q, proj, order, p0, valid, rg, tid);
        if (tid < TM) wq[tid] = wr_row(wh, tid < valid ? order[p0 + tid] : -1);

        auto load_pid = [&](int cb) { const int cc = cb + wv * 16 + c; return cc < ce ? type_col[cc] : -1; };
        // (a lane without a product reads product 0's row, term and attributes: no branch, and nothing of it is used)
        auto load_b = [&](float4* b, int pid) {
            const float4* f = reinterpret_cast<const float4*>(table + (size_t)max(pid, 0) * D) + h;
#pragma unroll
            for (int k = 0; k < NB; k++) b[k] = f[4 * k];
        };
        float4 b[NB];
        const int pid = load_pid(cb0);
        load_b(b, pid);
        float bs = 0.f;
        if constexpr (BIAS) bs = bias[max(pid, 0)];
        const float a = wr_value(wh, pid);
        const int f = wr_flags(wh, pid);
        const int pidn = load_pid(cb0 + RG_CHUNK);
        // wave wv: column c = the target of query row wv * 16 + c
        int ty = -1;
        if (wv < rg && wv * 16 + c < valid) ty = targets[order[p0 + wv * 16 + c]];
        __syncthreads();                                  // query tile in LDS
        if (wv < rg) {                                    // (wave-uniform)
            float4 bt[NB];
            load_b(bt, ty);
            float by = 0.f;
            if constexpr (BIAS) by = bias[max(ty, 0)];
            f32x4 ag[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};
            rk_chain<D, 1>(q, wv, bt, nullptr, ag, c, h);
            const f32x4 acc = ag[0];
            // C/D map of the 16x16 f32 MFMA: column lane & 15, row 4 (lane >> 4) + reg; the diagonal: row == column
            if ((c >> 2) == h) {
                const int k = c & 3;
                const float d = k == 0 ? acc[0] : k == 1 ? acc[1] : k == 2 ? acc[2] : acc[3];
                gs[wv * 16 + c] = BIAS ? d + by : d;
                ys[wv * 16 + c] = ty;
            }
        }
        __syncthreads();                                  // gs / ys / wq in LDS
        // the slice's candidates against the tile's NG row groups: straight-line code per NG
        if (rg == 1) wr_stream<D, 1, BIAS>(q, gs, ys, wq, part, type_col, table, bias, wh, cb0, ce, b, pid, pidn, bs, a, f, wv, c, h);
        else if (rg == 2) wr_stream<D, 2, BIAS>(q, gs, ys, wq, part, type_col, table, bias, wh, cb0, ce, b, pid, pidn, bs, a, f, wv, c, h);
        else if constexpr (RG == 4) {
            if (rg == 3) wr_stream<D, 3, BIAS>(q, gs, ys, wq, part, type_col, table, bias, wh, cb0, ce, b, pid, pidn, bs, a, f, wv, c, h);
            else wr_stream<D, 4, BIAS>(q, gs, ys, wq, part, type_col, table, bias, wh, cb0, ce, b, pid, pidn, bs, a, f, wv, c, h);
        }
        __syncthreads();
        if (tid < valid) {
            const int v = part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid];
            if (v) atomicAdd(&rank_out[order[p0 + tid]], v);
        }
    }
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
    constexpr int QS = RK_QS(D), NB = D / 16;
    __shared__ __attribute__((aligned(16))) float q[16 * QS];
    const int lane = threadIdx.x, c = lane & 15, h = lane >> 4;
    const int r = blockIdx.x;
    int key = -1;
    if (row_key) {
        key = row_key[r];
        if (key < -1 || key >= n_keys) {
            if (lane == 0) atomicAdd(bad_count, 1);
            key = -1;
        }
    }
    const int base = rank_out[r];
    if (base < 0) return;                                 // (wave-uniform, as every exit below) no type, or an id out of range
    const int t = types[r], y = targets[r];               // both inside their ranges: the plan counted the row
    const WrRow w = wr_row(wh, r);
    if ((row_key && cand_type[y] != t) || !wr_pass(w, wr_value(wh, y), wr_flags(wh, y))) {
        if (lane == 0) rank_out[r] = -1;
        return;
    }
    if (key < 0) return;
    const int elo = ex_rowptr[key], len = ex_rowptr[key + 1] - elo;
    if (len <= 0) return;
    for (int e = lane; e < 16 * (QS / 4); e += 64) {
        const int row = e / (QS / 4), d4 = e - row * (QS / 4);
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row == 0 && d4 < D / 4) x = reinterpret_cast<const float4*>(proj + (size_t)r * D)[d4];
        *reinterpret_cast<float4*>(&q[row * QS + 4 * d4]) = x;
    }
    __syncthreads();
    float g = 0.f;
    int dec = 0;
    bool hit = false;
    for (int v0 = 0; v0 <= len; v0 += 16) {               // column v: the target (v == 0), list entry v - 1
        const int v = v0 + c;
        int id = -1;
        if (v == 0) id = y;
        else if (v <= len) id = ex_col[elo + v - 1];
        if (id >= num_products) id = -1;
        float4 b[NB];
        const float4* f = reinterpret_cast<const float4*>(table + (size_t)max(id, 0) * D) + h;
#pragma unroll
        for (int k = 0; k < NB; k++) b[k] = f[4 * k];
        float bs = 0.f;
        if constexpr (BIAS) bs = bias[max(id, 0)];
        const bool ok = wr_pass(w, wr_value(wh, id), wr_flags(wh, id));
        f32x4 acc[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};
        rk_chain<D, 1>(q, 0, b, nullptr, acc, c, h);
        // C/D map of the 16x16 f32 MFMA: column lane & 15, row 4 (lane >> 4) + reg: row 0 is register 0 of lanes 0..15
        const float s = BIAS ? acc[0][0] + bs : acc[0][0];
        if (v0 == 0) g = __shfl(s, 0, 64);
        const bool mine = h == 0 && v > 0 && id >= 0;
        hit |= __any(mine && id == y);
        dec += __popcll(__ballot(mine && id != y && ok && cand_type[max(id, 0)] == t && rg_better(s, id, g, y)));
    }
    if (lane == 0) rank_out[r] = hit ? -1 : base - dec;
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
    if (!proj || !types || !targets || !type_rowptr || !type_col || !table || !rank_out || !bad_count || !ws) return PC_EINVAL;
    if (!wr_where_ok(where)) return PC_EINVAL;            // a null filter, or a half-given one
    if (rows <= 0 || n_types <= 0 || num_products <= 0) return PC_EINVAL;
    // the lists and the products' types: all or none
    if (!rg_lists_ok(row_key, ex_rowptr, ex_col, bad_count, n_keys) || !row_key != !cand_type) return PC_EINVAL;
    if ((dim != 128 && dim != 256) || slices < 0 || slices > RG_MAX_SLICES) return PC_ESHAPE;
    const int S = rg_slices(slices);
    hipStream_t st = (hipStream_t)stream;
    RgWs w;
    unsigned grid;
    PC_TRY(rg_begin(w, grid, ws, ws_bytes, types, targets, rows, type_rowptr, n_types, num_products, 0, S, 8192 / dim, rank_out,
                    bad_count, st));
    const RgPlan& pl = w.plan;
#define WR_RANK(D, BIAS)                                                                                                       \
    do {                                                                                                                       \
        PC_LAUNCH((wr_rank_kernel<D, BIAS>), dim3(grid), dim3(256), 0, st, proj, targets, type_rowptr, type_col, table, bias,  \
                  n_types, S, pl.cnt, pl.row_start, pl.item_start, pl.order, rank_out, *where);                                \
        PC_LAUNCH((wr_post_kernel<D, BIAS>), dim3(rows), dim3(64), 0, st, proj, types, targets, row_key, ex_rowptr, ex_col,    \
                  n_keys, cand_type, table, bias, num_products, *where, rank_out, bad_count);                                  \
    } while (0)
    if (dim == 128) {
        if (bias) WR_RANK(128, true); else WR_RANK(128, false);
    } else {
        if (bias) WR_RANK(256, true); else WR_RANK(256, false);
    }
#undef WR_RANK
    return pc_launch_status();
}
