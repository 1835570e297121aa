// The one-pass fold of the BatchNorm per-tile partial sums and the BatchNorm-backward finalize built on it, as device
// functions: ffn.hip's finalize kernels call them, and so do the rider workgroups of gemm_tn.hip's dW3 launch.
#pragma once
#include "common.h"

// partial[t][j] over 128-row tiles -> per-segment statistics: a workgroup owns FIN_COLS adjacent columns
#define FIN_COLS 32

#ifdef __HIPCC__
// All segments in ONE pass, 16-byte loads (round 6).  The per-segment folds of ffn.hip walk a segment's tiles with one dword load
// per lane and tile: a wave-load moves 256 B and the kernel is bound by the address pipe of its eight CUs, not by latency (5.6 us
// for 4 tiles, 8.8 for 352, 13.1 for 704 when run alone -- scripts/dev/bn_finalize_probe.sh -- and 12-14 us inside the step, four
// segments one after the other).  Here a thread owns FOUR adjacent columns (one float4 per tile and array), a workgroup is
// 8 column groups x 64 tile lanes (512 threads: 128 registers per thread would spill the 64 accumulator registers' neighbours),
// so a wave-load moves 1 KB (eight tile rows x 128 B) and a 352-tile fold is six loads per lane and array, all in flight
// before the first use.  A value is added to its segment's accumulator by predicate (tiles never
// straddle segments).  Lanes are reduced in a fixed order: xor-shuffles over the wave's eight tile lanes, then one LDS exchange
// over the eight waves.  Result: thread f < 128 holds the two sums of (segment f / 32, column f % 32 of the workgroup's 32).
// tid: the thread's index in its workgroup of FIN4_CG x FIN4_LANES (column group = tid % FIN4_CG, tile lane = tid / FIN4_CG).
#define FIN4_CG 8
#define FIN4_LANES 64
#define FIN4_WAVES (FIN4_CG * FIN4_LANES / 64)
#define FIN4_BATCH 6
__device__ __forceinline__ void fold_partials_all4(const float* __restrict__ p1, const float* __restrict__ p2, const SegInfo& si,
                                                   int col0, int tid, double (*red)[2][PC_MAX_SEG][FIN_COLS], double* o1, double* o2) {
    const int cg = tid % FIN4_CG, q = tid / FIN4_CG;
    const int wave = tid >> 6, lane = tid & 63;
    double a[PC_MAX_SEG][4], b[PC_MAX_SEG][4];
#pragma unroll
    for (int s = 0; s < PC_MAX_SEG; s++)
#pragma unroll
        for (int c = 0; c < 4; c++) { a[s][c] = 0.0; b[s][c] = 0.0; }
    const int t_end = si.tile0[si.nseg];
    const int b1 = si.nseg > 1 ? si.tile0[1] : t_end, b2 = si.nseg > 2 ? si.tile0[2] : t_end, b3 = si.nseg > 3 ? si.tile0[3] : t_end;
    const size_t c0 = (size_t)col0 + cg * 4;
    for (int t = si.tile0[0] + q; t < t_end; t += FIN4_BATCH * FIN4_LANES) {
        float4 x[FIN4_BATCH], y[FIN4_BATCH];
#pragma unroll
        for (int u = 0; u < FIN4_BATCH; u++) {
            const int tt = t + u * FIN4_LANES;
            const int tc = tt < t_end ? tt : t;                    // (a lane past the end re-reads its first tile: no branch, no use)
            x[u] = *reinterpret_cast<const float4*>(p1 + (size_t)tc * PC_H + c0);
            y[u] = *reinterpret_cast<const float4*>(p2 + (size_t)tc * PC_H + c0);
        }
#pragma unroll
        for (int u = 0; u < FIN4_BATCH; u++) {
            const int tt = t + u * FIN4_LANES;
            const int sg = tt < t_end ? (tt >= b1) + (tt >= b2) + (tt >= b3) : -1;
#pragma unroll
            for (int s = 0; s < PC_MAX_SEG; s++) {
                const bool on = sg == s;
                a[s][0] += on ? (double)x[u].x : 0.0; a[s][1] += on ? (double)x[u].y : 0.0;
                a[s][2] += on ? (double)x[u].z : 0.0; a[s][3] += on ? (double)x[u].w : 0.0;
                b[s][0] += on ? (double)y[u].x : 0.0; b[s][1] += on ? (double)y[u].y : 0.0;
                b[s][2] += on ? (double)y[u].z : 0.0; b[s][3] += on ? (double)y[u].w : 0.0;
            }
        }
    }
    // the wave's eight tile lanes (lane bits 3..5), fixed order
#pragma unroll
    for (int s = 0; s < PC_MAX_SEG; s++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
#pragma unroll
            for (int o = 8; o < 64; o <<= 1) { a[s][c] += __shfl_xor(a[s][c], o, 64); b[s][c] += __shfl_xor(b[s][c], o, 64); }
        }
    if (lane < FIN4_CG) {
#pragma unroll
        for (int s = 0; s < PC_MAX_SEG; s++)
#pragma unroll
            for (int c = 0; c < 4; c++) { red[wave][0][s][cg * 4 + c] = a[s][c]; red[wave][1][s][cg * 4 + c] = b[s][c]; }
    }
    __syncthreads();
    if (tid < PC_MAX_SEG * FIN_COLS) {
        const int s = tid / FIN_COLS, col = tid % FIN_COLS;
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int w = 0; w < FIN4_WAVES; w++) { s1 += red[w][0][s][col]; s2 += red[w][1][s][col]; }
        *o1 = s1; *o2 = s2;
    }
}
#endif

// per-tile (sum dz1, sum dz1*h0) -> dgamma, dbeta (+ per-segment means c1 = dbeta_s/n, c2 = dgamma_s/n), BatchNorm1d of
// product2vec.py:16.  lsum: NULL = fold this replica's per-tile partials here, else its folded sums; gsum: NULL or the
// all-reduced exchange buffer the means run over.
struct BnFinBwd {
    const float *psum, *pdot; const double *lsum, *gsum; const float *mean, *invstd;
    float *dgamma, *dbeta; int accumulate; float *c1, *c2;
};
// LDS scratch of one finalize workgroup
struct BnFinBwdScratch {
    double red[FIN4_WAVES][2][PC_MAX_SEG][FIN_COLS];
    double seg_g[PC_MAX_SEG][FIN_COLS], seg_b[PC_MAX_SEG][FIN_COLS];
};
#ifdef __HIPCC__
// One workgroup of FIN4_CG x FIN4_LANES threads finalizes columns [cb FIN_COLS, cb FIN_COLS + FIN_COLS), cb < PC_H / FIN_COLS;
// the whole workgroup calls (barriers inside).
__device__ __forceinline__ void bn_finalize_bwd_body(const BnFinBwd& f, const SegInfo& si, int cb, int tid, BnFinBwdScratch* sm) {
    double a = 0.0, b = 0.0;
    if (!f.lsum) fold_partials_all4(f.psum, f.pdot, si, cb * FIN_COLS, tid, sm->red, &a, &b);
    if (tid < PC_MAX_SEG * FIN_COLS) {
        const int s = tid / FIN_COLS, col = tid % FIN_COLS, j = cb * FIN_COLS + col;
        double tg = 0.0, tb = 0.0;
        if (s < si.nseg) {
            double n = si.count[s];                           // logical rows (a weighted row counts wmult times)
            if (f.lsum) { a = f.lsum[(2 * s) * PC_H + j]; b = f.lsum[(2 * s + 1) * PC_H + j]; }
            // the tiles carry the raw moment sum dz1*h0: sum dz1*xhat = invstd * (sum dz1*h0 - mean * sum dz1)
            const double is = (double)f.invstd[s * PC_H + j], mu = (double)f.mean[s * PC_H + j];
            b = is * (b - mu * a);
            tb = a;                                           // dbeta / dgamma: this replica's rows
            tg = b;
            double ga = a, gb = b;                            // the BN-backward means run over ALL replicas' rows
            if (f.gsum) {
                ga = f.gsum[(2 * s) * PC_H + j];
                gb = is * (f.gsum[(2 * s + 1) * PC_H + j] - mu * ga);
                n = f.gsum[2 * PC_MAX_SEG * PC_H + s];
            }
            f.c1[s * PC_H + j] = n > 0 ? (float)(ga / n) : 0.f;
            f.c2[s * PC_H + j] = n > 0 ? (float)(gb / n) : 0.f;
        }
        sm->seg_g[s][col] = tg;
        sm->seg_b[s][col] = tb;
    }
    __syncthreads();
    if (tid < FIN_COLS) {
        const int j = cb * FIN_COLS + tid;
        double tg = 0.0, tb = 0.0;
        for (int s = 0; s < si.nseg; s++) { tg += sm->seg_g[s][tid]; tb += sm->seg_b[s][tid]; }     // segment order, as before
        f.dgamma[j] = f.accumulate ? f.dgamma[j] + (float)tg : (float)tg;
        f.dbeta[j] = f.accumulate ? f.dbeta[j] + (float)tb : (float)tb;
    }
}
#endif

// The finalize as RIDERS of a weight-gradient launch (launch_gemm_tn_halves): workgroup block[i] of the launch's grid runs
// bn_finalize_bwd_body(fin, si, i, ...) and leaves (si: the segments once more -- the body indexes them by thread, which it
// can in an argument the kernel never modifies).  What the finalize reads (the dZ1 launch's
// per-tile sums, the forward's statistics) is complete before the host launch starts, and nothing it writes (c1 / c2,
// dgamma, dbeta) is touched by the host product.  n == 0: no riders.
#define PC_TN_RIDERS (PC_H / FIN_COLS)
struct TnRider { int n; int block[PC_TN_RIDERS]; BnFinBwd fin; SegInfo si; };
