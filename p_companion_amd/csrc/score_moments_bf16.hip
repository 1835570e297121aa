// The first two moments of a row's scores over all candidates of its type, over the bf16 copy of the catalogue alone
// (pc_score_moments_grouped_bf16; ops.score_moments_grouped with a bf16 table, PCompanionInference.score_moments over a bf16
// catalogue or an ops.CompactCatalogue, CompactInference): score_moments.hip's contract --
//   s1 = sum_p fl(s_p - g),   s2 = sum_p fl(s_p - g)^2,   g = the score of the type's first candidate,
//   mean = g + s1 / n,   std = sqrt(max(s2 / n - (s1 / n)^2, 0)) --
// under rank_bf16.hip's score s_p = d(r, p): the unrounded query, split once into three bf16 pieces, against the ROUNDED rows.
// rank_bf16.hip's schedule with the sums in the count's place; half the candidate bytes, and no fp32 table anywhere.
//
//   plan     grouped_plan.hip as it is, without targets (tiles of TM = 8192 / D rows)
//   moments  smb_moments_kernel: rb_rank_kernel -- the query tile split ONCE by split3 into three bf16 images in LDS, the type's
//            first candidate scored first against every row group (the pivots = the diagonal), the slice's candidates in chunks
//            of 64 with the next chunk's rows in flight -- with sm_accum (score_moments.h) where the rank counts
//   finish   sm_finish_kernel (score_moments.hip)
//
// Determinism: d is rb_chain (rank_chain_bf16.h), so a (row, product) score has the bits pc_retrieve_list_grouped_bf16 and
// pc_rank_grouped_bf16 give it; the sums are score_moments.hip's, in its fixed order: bitwise reproducible for a given `slices`,
// last-bit differences across `slices`, none where the sums are exact.  No float atomics, no readback.
#include "common.h"
#include "grouped_select.h"        // the item decode
#include "rank_chain_bf16.h"
#include "score_moments.h"

// One work item's candidate stream for a tile of NG 16-row groups (rb_stream with the sums in the count's place).  bn / pidn:
// the first chunk's rows and product ids, pidnn: the second chunk's ids, all already in flight (-1: a column past the slice's
// end; nothing of it is added).  Leaves the wave's sums in part1 / part2[wv][row].
template <int D, int NG>
__device__ __forceinline__ void smb_stream(const bf16x8 (&q)[3][(D / 8) * (8192 / D)], const float* gs, float (*part1)[8192 / D],
                                           float (*part2)[8192 / D], const int32_t* __restrict__ type_col,
                                           const uint16_t* __restrict__ table, int cb0, int ce, bf16x8 (&bn)[D / 32], int pidn,
                                           int pidnn, int wv, int c, int h) {
    constexpr int TM = 8192 / D, NB = D / 32;
    float s1[NG][4], s2[NG][4];
#pragma unroll
    for (int g = 0; g < NG; g++)
#pragma unroll
        for (int k = 0; k < 4; k++) s1[g][k] = s2[g][k] = 0.f;
    for (int cb = cb0; cb < ce; cb += RG_CHUNK) {
        bf16x8 b[NB];
#pragma unroll
        for (int k = 0; k < NB; k++) b[k] = bn[k];
        const int pid = pidn;
        pidn = pidnn;
        if (cb + RG_CHUNK < ce) rb_load_b<D>(bn, table, pidn, h);     // the next chunk's rows in flight while this one is scored
        const int cc = cb + 2 * RG_CHUNK + wv * 16 + c;
        pidnn = cc < ce ? type_col[cc] : -1;
        f32x4 acc[NG];
#pragma unroll
        for (int g = 0; g < NG; g++) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
        rb_chain<D, TM, NG>(q, 0, b, acc, c, h);
        sm_accum<NG>(acc, gs, s1, s2, pid, h);
    }
    sm_reduce<NG, TM>(s1, part1, wv, c, h);
    sm_reduce<NG, TM>(s2, part2, wv, c, h);
}

// Work item w = (type t, slice s, tile j) (rg_decode).  Launch bounds and amdgpu_waves_per_eu(2) as rb_rank_kernel.
template <int D>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void smb_moments_kernel(
    const float* __restrict__ proj, const int32_t* __restrict__ types, const int32_t* __restrict__ type_rowptr,
    const int32_t* __restrict__ type_col, const uint16_t* __restrict__ table, int n_types, int S, const int32_t* __restrict__ cnt,
    const int32_t* __restrict__ row_start, const int64_t* __restrict__ item_start, const int32_t* __restrict__ order,
    float* __restrict__ p1, float* __restrict__ p2, float* __restrict__ pg) {
    constexpr int TM = 8192 / D;             // rows per tile: 64 (D = 128) or 32 (D = 256)
    constexpr int RG = TM / 16;              // 16-row groups (at most one per wave)
    constexpr int NB = D / 32;               // k-blocks: 16-byte operands per lane per candidate
    __shared__ __attribute__((aligned(16))) bf16x8 q[3][(D / 8) * TM];   // the pieces p0, p1, p2 of the query tile
    __shared__ __attribute__((aligned(16))) float gs[TM];            // the rows' pivots
    __shared__ float part1[4][TM], part2[4][TM];                     // the waves' sums
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c = lane & 15, h = lane >> 4;
    const int64_t n_items = item_start[n_types];
    for (int64_t w = blockIdx.x; w < n_items; w += gridDim.x) {
        const RgItem it = rg_decode<TM>(w, item_start, cnt, row_start, type_rowptr, n_types, S);
        const int p0 = it.p0, valid = it.valid, rg = it.rg, cb0 = it.cb0, ce = it.ce;

        __syncthreads();                                  // the previous item's readers of q / gs / part are done
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
        const int pidnn = load_pid(cb0 + RG_CHUNK);
        // the type's first candidate (an item exists only for a type with candidates and rows): every column of the block
        const int ty = type_col[type_rowptr[types[order[p0]]]];
        __syncthreads();                                  // query images in LDS
        if (wv < rg) {                                    // (wave-uniform)
            bf16x8 bt[NB];
            rb_load_b<D>(bt, table, ty, h);
            f32x4 ag[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};
            rb_chain<D, TM, 1>(q, wv, bt, ag, c, h);
            const f32x4 acc = ag[0];
            // C/D map of the 16x16 MFMAs: column lane & 15, row 4 (lane >> 4) + reg; the diagonal: row == column
            if ((c >> 2) == h) {
                const int k = c & 3;
                gs[wv * 16 + c] = k == 0 ? acc[0] : k == 1 ? acc[1] : k == 2 ? acc[2] : acc[3];
            }
        }
        __syncthreads();                                  // gs in LDS
        // the slice's candidates against the tile's NG row groups: straight-line code per NG
        if (rg == 1) smb_stream<D, 1>(q, gs, part1, part2, type_col, table, cb0, ce, bn, pidn, pidnn, wv, c, h);
        else if (rg == 2) smb_stream<D, 2>(q, gs, part1, part2, type_col, table, cb0, ce, bn, pidn, pidnn, wv, c, h);
        else if constexpr (RG == 4) {
            if (rg == 3) smb_stream<D, 3>(q, gs, part1, part2, type_col, table, cb0, ce, bn, pidn, pidnn, wv, c, h);
            else smb_stream<D, 4>(q, gs, part1, part2, type_col, table, cb0, ce, bn, pidn, pidnn, wv, c, h);
        }
        __syncthreads();
        sm_store<TM>(part1, part2, gs, tid, valid, p0, it.s, S, p1, p2, pg);
    }
}

extern "C" int pc_score_moments_grouped_bf16(const float* proj, const int32_t* types, int rows, const int32_t* type_rowptr,
                                             const int32_t* type_col, const uint16_t* table_bf16, int n_types, int dim,
                                             int slices, int32_t* count, float* pivot, float* s1, float* s2, float* mean,
                                             float* std_out, int32_t* bad_count, void* ws, size_t ws_bytes, void* stream) {
    const SmOut o{count, pivot, s1, s2, mean, std_out};
    PC_TRY(sm_check(proj, types, type_rowptr, type_col, table_bf16, o, bad_count, ws, rows, n_types, dim, slices));
    if ((uintptr_t)table_bf16 & 15) return PC_ESHAPE;     // a lane reads 16 bytes of a row at once
    const int S = rg_slices(slices);
    hipStream_t st = (hipStream_t)stream;
    SmWs w;
    unsigned grid;
    PC_TRY(sm_begin(w, grid, ws, ws_bytes, types, rows, type_rowptr, n_types, S, 8192 / dim, bad_count, st));
    const RgPlan& pl = w.plan;
    if (dim == 128)
        PC_LAUNCH(smb_moments_kernel<128>, dim3(grid), dim3(256), 0, st, proj, types, type_rowptr, type_col, table_bf16, n_types,
                  S, pl.cnt, pl.row_start, pl.item_start, pl.order, w.p1, w.p2, w.pg);
    else
        PC_LAUNCH(smb_moments_kernel<256>, dim3(grid), dim3(256), 0, st, proj, types, type_rowptr, type_col, table_bf16, n_types,
                  S, pl.cnt, pl.row_start, pl.item_start, pl.order, w.p1, w.p2, w.pg);
    sm_finish_launch(w, types, rows, type_rowptr, S, o, st);
    return pc_launch_status();
}
