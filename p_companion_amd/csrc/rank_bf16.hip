// The rank of a known product among the products of its type over the bf16 copy of the catalogue alone
// (pc_rank_grouped_bf16; CompactInference.rank_targets / evaluate_catalogue and CompactSimilarProducts.rank_pairs in
// inference.py): for row r with type c = types[r] and target y = targets[r],
//   s_p = fl(d(r, p) + bias[p])  (bias null: s_p = d(r, p)),   g = s_y,
//   rank_out[r] = #{ p of type c, not in the row's list : s_p > g  or  (s_p == g and p < y) },
// the position y takes in the list pc_retrieve_list_grouped_bf16[_biased] serves for the row.  rank.hip's schedule and count
// under retrieve_bf16.hip's score chain: half the candidate bytes of the fp32 rank, and no fp32 table anywhere.
//
//   plan     grouped_plan.hip as it is (tiles of TM = 8192 / D rows); rank_out[r] = 0, or -1 for a row without a type or with
//            an id out of range (counted in *bad_count)
//   rank     rb_rank_kernel: grid-stride over the work items (type, slice, tile): the query tile is split ONCE by split3 into
//            three bf16 images in LDS; the tile's own targets scored first (wave w: the 16 targets of row group w as one MFMA
//            column block, g = its diagonal, plus bias[y]); then the slice's candidates in chunks of 64 (one 16-candidate column
//            group per wave, lane (c, h) holding the dimensions 32 k + 8 h .. + 7 of candidate c, the next chunk's rows in
//            flight), every accumulator register (plus bias[pid], gathered a chunk ahead) compared with its row's g, integer
//            counts per lane; at the end a 16-lane sum, the four waves' sums through LDS, one integer atomic per (row, slice)
//   exclude  rb_rank_exclude_kernel: rk_exclude_kernel's post-pass, one wave per row, through the same chain
//
// Determinism: d is rg_score_bf16_kernel's chain through rb_chain (rank_chain_bf16.h), the one text of the bf16 ranks: k-block 0 .. D / 32 - 1, inside
// a k-block the pieces p0, p1, p2, one v_mfma_f32_16x16x32_bf16 each into ONE accumulator per row group; an MFMA's output
// (row, column) depends on its A row and B column alone.  So a (row, product) score has the bits pc_retrieve_topk_grouped_bf16,
// pc_retrieve_list_grouped_bf16 and, with a bias, pc_retrieve_list_grouped_bf16_biased give it, s_y and g are the same bits,
// and the count is a sum of integers: it does not depend on the slices, on the order of the rows in a tile or on the order of
// type_col inside a type.  No float atomics.
#include "common.h"
#include "grouped_rank.h"          // rk_post: the row post-pass; rk_begin, rk_dispatch

// One work item's candidate stream for a tile of NG 16-row groups (NG a template argument: the loop body is straight-line
// code).  Lane l of wave wv: column c = l & 15 (candidate wv * 16 + c of the chunk), k-lane h = l >> 4; accumulator register k
// of row group g holds query row g * 16 + 4 h + k.  bn / pidn / bsn: the first chunk's rows, product ids and terms, pidnn: the
// second chunk's ids, all already in flight (-1: a column past the slice's end; its scores are not counted).  Leaves the
// wave's counts in part[wv][row].
template <int D, int NG, bool BIAS>
__device__ __forceinline__ void rb_stream(const bf16x8 (&q)[3][(D / 8) * (8192 / D)], const float* gs, const int* ys,
                                          int (*part)[8192 / D], const int32_t* __restrict__ type_col,
                                          const uint16_t* __restrict__ table, const float* __restrict__ bias, int cb0, int ce,
                                          bf16x8 (&bn)[D / 32], int pidn, int pidnn, float bsn, int wv, int c, int h) {
    constexpr int TM = 8192 / D, NB = D / 32;
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
        bf16x8 b[NB];
#pragma unroll
        for (int k = 0; k < NB; k++) b[k] = bn[k];
        const int pid = pidn;
        const float bs = bsn;
        pidn = pidnn;
        if (cb + RG_CHUNK < ce) rb_load_b<D>(bn, table, pidn, h);     // the next chunk's rows in flight while this one is scored
        if constexpr (BIAS) bsn = bias[max(pidn, 0)];                 // and its terms (a column without a product: bias[0], unused)
        const int cc = cb + 2 * RG_CHUNK + wv * 16 + c;
        pidnn = cc < ce ? type_col[cc] : -1;
        f32x4 acc[NG];
#pragma unroll
        for (int g = 0; g < NG; g++) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
        rb_chain<D, TM, NG>(q, 0, b, acc, c, h);
        // a score above g is counted.  Equal to g (the target itself, a copy of its row, or chance): the product index
        // decides -- rare, so the rows' targets stay in LDS and are read only where a lane meets such a score
        if (pid >= 0) {
            bool tie = false;
#pragma unroll
            for (int g = 0; g < NG; g++) {
                if constexpr (BIAS) acc[g] += bs;                     // the one addition: s = fl(d + bias[pid])
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    cn[g][k] += acc[g][k] > gv[g][k] ? 1 : 0;
                    tie |= acc[g][k] == gv[g][k];
                }
            }
            if (tie) {
#pragma unroll
                for (int g = 0; g < NG; g++)
#pragma unroll
                    for (int k = 0; k < 4; k++)
                        cn[g][k] += (acc[g][k] == gv[g][k] && pid < ys[g * 16 + 4 * h + k]) ? 1 : 0;
            }
        }
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

// Work item w = (type t, slice s, tile j) (rg_decode).  The four waves' counts meet in LDS: one integer atomic per (row, slice).
// amdgpu_waves_per_eu(2) as rg_score_bf16_kernel: at least two workgroups per CU.  The three query images take 48 KB; this
// kernel has no score tile, and gs / ys / part take 1.5 KB (D = 128) in its place, so the LDS has room for a third workgroup
// where the registers allow it.
template <int D, bool BIAS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void rb_rank_kernel(
    const float* __restrict__ proj, const int32_t* __restrict__ targets, const int32_t* __restrict__ type_rowptr,
    const int32_t* __restrict__ type_col, const uint16_t* __restrict__ table, const float* __restrict__ bias, int n_types, int S,
    const int32_t* __restrict__ cnt, const int32_t* __restrict__ row_start, const int64_t* __restrict__ item_start,
    const int32_t* __restrict__ order, int32_t* __restrict__ rank_out) {
    constexpr int TM = 8192 / D;             // rows per tile: 64 (D = 128) or 32 (D = 256)
    constexpr int RG = TM / 16;              // 16-row groups (at most one per wave)
    constexpr int NB = D / 32;               // k-blocks: 16-byte operands per lane per candidate
    __shared__ __attribute__((aligned(16))) bf16x8 q[3][(D / 8) * TM];   // the pieces p0, p1, p2 of the query tile
    __shared__ __attribute__((aligned(16))) float gs[TM];            // the rows' target scores
    __shared__ __attribute__((aligned(16))) int ys[TM];              // the rows' targets
    __shared__ int part[4][TM];                                      // the waves' counts
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c = lane & 15, h = lane >> 4;
    const int64_t n_items = item_start[n_types];
    for (int64_t w = blockIdx.x; w < n_items; w += gridDim.x) {
        const RgItem it = rg_decode<TM>(w, item_start, cnt, row_start, type_rowptr, n_types, S);
        const int p0 = it.p0, valid = it.valid, rg = it.rg, cb0 = it.cb0, ce = it.ce;

        __syncthreads();                                  // the previous item's readers of q / part are done
        for (int e = tid; e < rg * 16 * (D / 8); e += 256) {          // (rows past the last 16-row group are never read)
            const int d8 = e / (rg * 16), row = e - d8 * (rg * 16);   // (row fastest: a wave's 16-byte stores are contiguous)
            float4 x0 = make_float4(0.f, 0.f, 0.f, 0.f), x1 = x0;
            if (row < valid) {
                const float4* f = reinterpret_cast<const float4*>(proj + (size_t)order[p0 + row] * D) + 2 * d8;
                x0 = f[0];
                x1 = f[1];
            }
            const Split3 sp = split3(x0, x1);
            q[0][d8 * TM + row] = sp.p0;
            q[1][d8 * TM + row] = sp.p1;
            q[2][d8 * TM + row] = sp.p2;
        }

        auto load_pid = [&](int cb) { const int cc = cb + wv * 16 + c; return cc < ce ? type_col[cc] : -1; };
        bf16x8 bn[NB];
        const int pidn = load_pid(cb0);
        rb_load_b<D>(bn, table, pidn, h);
        float bsn = 0.f;
        if constexpr (BIAS) bsn = bias[max(pidn, 0)];
        const int pidnn = load_pid(cb0 + RG_CHUNK);
        // wave wv: column c = the target of query row wv * 16 + c
        int ty = -1;
        if (wv < rg && wv * 16 + c < valid) ty = targets[order[p0 + wv * 16 + c]];
        __syncthreads();                                  // query images in LDS
        if (wv < rg) {                                    // (wave-uniform)
            bf16x8 bt[NB];
            rb_load_b<D>(bt, table, ty, h);
            float by = 0.f;
            if constexpr (BIAS) by = bias[max(ty, 0)];
            f32x4 ag[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};
            rb_chain<D, TM, 1>(q, wv, bt, ag, c, h);
            const f32x4 acc = ag[0];
            // C/D map of the 16x16 MFMAs: column lane & 15, row 4 (lane >> 4) + reg; the diagonal: row == column
            if ((c >> 2) == h) {
                const int k = c & 3;
                const float d = k == 0 ? acc[0] : k == 1 ? acc[1] : k == 2 ? acc[2] : acc[3];
                gs[wv * 16 + c] = BIAS ? d + by : d;
                ys[wv * 16 + c] = ty;
            }
        }
        __syncthreads();                                  // gs / ys in LDS
        // the slice's candidates against the tile's NG row groups: straight-line code per NG
        if (rg == 1) rb_stream<D, 1, BIAS>(q, gs, ys, part, type_col, table, bias, cb0, ce, bn, pidn, pidnn, bsn, wv, c, h);
        else if (rg == 2) rb_stream<D, 2, BIAS>(q, gs, ys, part, type_col, table, bias, cb0, ce, bn, pidn, pidnn, bsn, wv, c, h);
        else if constexpr (RG == 4) {
            if (rg == 3) rb_stream<D, 3, BIAS>(q, gs, ys, part, type_col, table, bias, cb0, ce, bn, pidn, pidnn, bsn, wv, c, h);
            else rb_stream<D, 4, BIAS>(q, gs, ys, part, type_col, table, bias, cb0, ce, bn, pidn, pidnn, bsn, wv, c, h);
        }
        __syncthreads();
        if (tid < valid) {
            const int v = part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid];
            if (v) atomicAdd(&rank_out[order[p0 + tid]], v);
        }
    }
}

// rk_exclude_kernel's post-pass over the bf16 table (rk_post through rb_chain): rb_rank_kernel counted over the whole type; this
// takes the excluded products out again, and g and every s_e are the bits rb_rank_kernel compared.
template <int D, bool BIAS>
__global__ __launch_bounds__(64) void rb_rank_exclude_kernel(const float* __restrict__ proj, const int32_t* __restrict__ types,
                                                             const int32_t* __restrict__ targets,
                                                             const int32_t* __restrict__ row_key,
                                                             const int32_t* __restrict__ ex_rowptr,
                                                             const int32_t* __restrict__ ex_col, int n_keys,
                                                             const int32_t* __restrict__ cand_type,
                                                             const uint16_t* __restrict__ table, const float* __restrict__ bias,
                                                             int num_products, int32_t* __restrict__ rank_out,
                                                             int32_t* __restrict__ bad_count) {
    __shared__ __attribute__((aligned(16))) typename RkScoreBf16<D>::Image q;
    rk_post<D, RkScoreBf16<D>, BIAS, false>(q, proj, types, targets, row_key, ex_rowptr, ex_col, n_keys, cand_type, table, bias,
                                            num_products, pc_row_where{}, rank_out, bad_count);
}

extern "C" size_t pc_rank_grouped_bf16_workspace_bytes(int rows, int n_types, int slices) {
    return pc_rank_grouped_workspace_bytes(rows, n_types, slices);
}

extern "C" int pc_rank_grouped_bf16(const float* proj, const int32_t* types, const int32_t* targets, const int32_t* row_key,
                                    int rows, const int32_t* type_rowptr, const int32_t* type_col, const uint16_t* table_bf16,
                                    const float* bias, int n_types, int num_products, const int32_t* ex_rowptr,
                                    const int32_t* ex_col, int n_keys, const int32_t* cand_type, int dim, int slices,
                                    int32_t* rank_out, int32_t* bad_count, void* ws, size_t ws_bytes, void* stream) {
    RkStart s;
    PC_TRY(rk_begin(s, proj && table_bf16, table_bf16, types, targets, row_key, rows, type_rowptr, type_col, n_types, num_products,
                    ex_rowptr, ex_col, n_keys, cand_type, dim, slices, rank_out, bad_count, ws, ws_bytes, stream));
    const RgPlan& pl = s.w.plan;
    rk_dispatch(dim, bias != nullptr, [&](auto d, auto b) {
        constexpr int D = decltype(d)::value;
        constexpr bool BIAS = decltype(b)::value;
        PC_LAUNCH((rb_rank_kernel<D, BIAS>), dim3(s.grid), dim3(256), 0, s.st, proj, targets, type_rowptr, type_col, table_bf16, bias,
                  n_types, s.S, pl.cnt, pl.row_start, pl.item_start, pl.order, rank_out);
        if (row_key)
            PC_LAUNCH((rb_rank_exclude_kernel<D, BIAS>), dim3(rows), dim3(64), 0, s.st, proj, types, targets, row_key, ex_rowptr,
                      ex_col, n_keys, cand_type, table_bf16, bias, num_products, rank_out, bad_count);
    });
    return pc_launch_status();
}
