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
#include "grouped_select.h"        // the item decode, the tile load

#include "rank_chain.h"           // RK_QS, rk_chain: THE k-chain (rank_exclude.hip scores through it too)

// One work item's candidate stream for a tile of NG 16-row groups (NG a template argument: the loop body is straight-line
// code).  Lane l of wave wv: column c = l & 15 (candidate wv * 16 + c of the chunk, query row g * 16 + c of the A operand),
// k-lane h = l >> 4; accumulator register k of row group g holds query row g * 16 + 4 h + k.  b / pid: the first chunk's
// rows and product ids, pidn: the second chunk's ids, all already in flight (-1: a column past the slice's end; its b is
// product 0's row and its scores are not counted).  Leaves the wave's counts in part[wv][row].
template <int D, int NG>
__device__ __forceinline__ void rk_stream(const float* q, const float* gs, const int* ys, int (*part)[8192 / D],
                                          const int32_t* __restrict__ type_col, const float* __restrict__ table, int cb0,
                                          int ce, float4 (&b)[D / 16], int pid, int pidn, int wv, int c, int h) {
    float gv[NG][4];
    int cn[NG][4];
#pragma unroll
    for (int g = 0; g < NG; g++) {
        const float4 x = *reinterpret_cast<const float4*>(&gs[g * 16 + 4 * h]);
        gv[g][0] = x.x; gv[g][1] = x.y; gv[g][2] = x.z; gv[g][3] = x.w;
#pragma unroll
        for (int k = 0; k < 4; k++) cn[g][k] = 0;
    }
    for (int cb = cb0; cb < ce; cb += RG_CHUNK) {
        const int cc = cb + 2 * RG_CHUNK + wv * 16 + c;
        const int pidnn = cc < ce ? type_col[cc] : -1;
        // the next chunk's rows replace this one's step by step while it is scored
        const float4* next = reinterpret_cast<const float4*>(table + (size_t)max(pidn, 0) * D) + h;
        f32x4 acc[NG];
#pragma unroll
        for (int g = 0; g < NG; g++) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
        rk_chain<D, NG>(q, 0, b, next, acc, c, h);
        // a score above g is counted.  Equal to g (the target itself, a copy of its row, or chance): the product index
        // decides -- rare, so the rows' targets stay in LDS and are read only where a lane meets such a score
        if (pid >= 0) {
            bool tie = false;
#pragma unroll
            for (int g = 0; g < NG; g++)
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    cn[g][k] += acc[g][k] > gv[g][k] ? 1 : 0;
                    tie |= acc[g][k] == gv[g][k];
                }
            if (tie) {
#pragma unroll
                for (int g = 0; g < NG; g++)
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        cn[g][k] += (acc[g][k] == gv[g][k] && pid < ys[g * 16 + 4 * h + k]) ? 1 : 0;
            }
        }
        pid = pidn;
        pidn = pidnn;
    }
    // the 16 columns of a (wave, k-lane) -> lane c == 0
#pragma unroll
    for (int g = 0; g < NG; g++)
#pragma unroll
        for (int k = 0; k < 4; k++) {
            int v = cn[g][k];
#pragma unroll
            for (int o = 8; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
            if (c == 0) part[wv][g * 16 + 4 * h + k] = v;
        }
}

// Work item w = (type t, slice s, tile j), items of one type ordered slice-major so that the tiles running side by side read
// the same candidates (L2).  The four waves' counts meet in LDS: one integer atomic per (row, slice).
template <int D>
// three waves per SIMD at D = 128 and two at D = 256, as rg_score_kernel
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(D == 128 ? 3 : 2))) void rk_rank_kernel(
    const float* __restrict__ proj, const int32_t* __restrict__ targets, const int32_t* __restrict__ type_rowptr,
    const int32_t* __restrict__ type_col, const float* __restrict__ table, int n_types, int S, const int32_t* __restrict__ cnt,
    const int32_t* __restrict__ row_start, const int64_t* __restrict__ item_start, const int32_t* __restrict__ order,
    int32_t* __restrict__ rank_out) {
    constexpr int TM = 8192 / D;             // rows per tile: 64 (D = 128) or 32 (D = 256): a 32 KB query tile
    constexpr int RG = TM / 16;              // 16-row groups (at most one per wave)
    constexpr int QS = RK_QS(D);             // padded LDS row
    constexpr int NB = D / 16;               // float4 operands per lane per candidate
    __shared__ __attribute__((aligned(16))) float q[TM * QS];
    __shared__ __attribute__((aligned(16))) float gs[TM];            // the rows' target scores
    __shared__ __attribute__((aligned(16))) int ys[TM];              // the rows' targets
    __shared__ int part[4][TM];                                      // the waves' counts
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c = lane & 15, h = lane >> 4;
    const int64_t n_items = item_start[n_types];
    for (int64_t w = blockIdx.x; w < n_items; w += gridDim.x) {
        const RgItem it = rg_decode<TM>(w, item_start, cnt, row_start, type_rowptr, n_types, S);
        const int p0 = it.p0, valid = it.valid, rg = it.rg, cb0 = it.cb0, ce = it.ce;

        __syncthreads();                                  // the previous item's readers of q / part are done
        rg_load_tile<D, QS>(q, proj, order, p0, valid, rg, tid);

        auto load_pid = [&](int cb) { const int cc = cb + wv * 16 + c; return cc < ce ? type_col[cc] : -1; };
        // (a lane without a product reads product 0's row: no branch, and nothing of it is used)
        auto load_b = [&](float4* b, int pid) {
            const float4* f = reinterpret_cast<const float4*>(table + (size_t)max(pid, 0) * D) + h;
#pragma unroll
            for (int k = 0; k < NB; k++) b[k] = f[4 * k];
        };
        float4 b[NB];
        const int pid = load_pid(cb0);
        load_b(b, pid);
        const int pidn = load_pid(cb0 + RG_CHUNK);
        // wave wv: column c = the target of query row wv * 16 + c
        int ty = -1;
        if (wv < rg && wv * 16 + c < valid) ty = targets[order[p0 + wv * 16 + c]];
        __syncthreads();                                  // query tile in LDS
        if (wv < rg) {                                    // (wave-uniform)
            float4 bt[NB];
            load_b(bt, ty);
            f32x4 ag[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};
            rk_chain<D, 1>(q, wv, bt, nullptr, ag, c, h);
            const f32x4 acc = ag[0];
            // C/D map of the 16x16 f32 MFMA: column lane & 15, row 4 (lane >> 4) + reg; the diagonal: row == column
            if ((c >> 2) == h) {
                const int k = c & 3;
                gs[wv * 16 + c] = k == 0 ? acc[0] : k == 1 ? acc[1] : k == 2 ? acc[2] : acc[3];
                ys[wv * 16 + c] = ty;
            }
        }
        __syncthreads();                                  // gs / ys in LDS
        // the slice's candidates against the tile's NG row groups: straight-line code per NG
        if (rg == 1) rk_stream<D, 1>(q, gs, ys, part, type_col, table, cb0, ce, b, pid, pidn, wv, c, h);
        else if (rg == 2) rk_stream<D, 2>(q, gs, ys, part, type_col, table, cb0, ce, b, pid, pidn, wv, c, h);
        else if constexpr (RG == 4) {
            if (rg == 3) rk_stream<D, 3>(q, gs, ys, part, type_col, table, cb0, ce, b, pid, pidn, wv, c, h);
            else rk_stream<D, 4>(q, gs, ys, part, type_col, table, cb0, ce, b, pid, pidn, wv, c, h);
        }
        __syncthreads();
        if (tid < valid) {
            const int v = part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid];
            if (v) atomicAdd(&rank_out[order[p0 + tid]], v);
        }
    }
}

extern "C" size_t pc_rank_grouped_workspace_bytes(int rows, int n_types, int slices) {
    if (rows <= 0 || n_types <= 0 || slices < 0 || slices > RG_MAX_SLICES) return 0;
    return rg_ws_carve(nullptr, rows, n_types, 0, rg_slices(slices)).bytes;
}

extern "C" int pc_rank_grouped(const float* proj, const int32_t* types, const int32_t* targets, int rows,
                               const int32_t* type_rowptr, const int32_t* type_col, const float* table, int n_types,
                               int num_products, int dim, int slices, int32_t* rank_out, int32_t* bad_count, void* ws,
                               size_t ws_bytes, void* stream) {
    if (!proj || !types || !targets || !type_rowptr || !type_col || !table || !rank_out || !bad_count || !ws) return PC_EINVAL;
    if (rows <= 0 || n_types <= 0 || num_products <= 0) return PC_EINVAL;
    if ((dim != 128 && dim != 256) || slices < 0 || slices > RG_MAX_SLICES) return PC_ESHAPE;
    const int S = rg_slices(slices);
    hipStream_t st = (hipStream_t)stream;
    RgWs w;
    unsigned grid;
    PC_TRY(rg_begin(w, grid, ws, ws_bytes, types, targets, rows, type_rowptr, n_types, num_products, 0, S, 8192 / dim, rank_out,
                    bad_count, st));
    const RgPlan& pl = w.plan;
    if (dim == 128)
        PC_LAUNCH(rk_rank_kernel<128>, dim3(grid), dim3(256), 0, st, proj, targets, type_rowptr, type_col, table, n_types, S,
                  pl.cnt, pl.row_start, pl.item_start, pl.order, rank_out);
    else
        PC_LAUNCH(rk_rank_kernel<256>, dim3(grid), dim3(256), 0, st, proj, targets, type_rowptr, type_col, table, n_types, S,
                  pl.cnt, pl.row_start, pl.item_start, pl.order, rank_out);
    return pc_launch_status();
}
