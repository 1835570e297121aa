// The k-chain of the bf16 rank kernels (rank_bf16.hip: rb_rank_kernel, rb_rank_exclude_kernel; where_rank_bf16.hip: their
// twins under a per-row predicate) and a lane's load of a product's bf16 row.  One definition: a score formed by any of
// these kernels is the same bits.
#pragma once
#include "common.h"

// THE k-chain: NG row groups from g0 on of a query image with TM rows per operand column block against the 16 columns whose
// rows the lanes hold in b.  Image piece p, operand (d8, row) at q[p][d8 * TM + row] = the dimensions 8 d8 .. + 7 of the row's
// piece p (rg_score_bf16_kernel's layout: the 16 lanes of an LDS cycle read 16 consecutive operands, no padding).
// For one accumulator the MFMAs run k-block ascending and inside a k-block p0, p1, p2; unit u = (k-block u / (3 NG), piece
// (u / NG) % 3, group u % NG) is one MFMA on one ds_read_b128 of the image, read PD units ahead.  The fence after each unit
// keeps the scheduler from hoisting all 3 NG D / 32 image reads (4 registers each), which would push the rank kernel's
// registers into scratch (rk_chain's reason).
template <int D, int TM, int NG>
__device__ __forceinline__ void rb_chain(const bf16x8 (&q)[3][(D / 8) * TM], int g0, const bf16x8 (&b)[D / 32], f32x4 (&acc)[NG],
                                         int c, int h) {
    constexpr int U = (D / 32) * 3 * NG, PD = 4;
    auto load_a = [&](int u) { return q[(u / NG) % 3][(4 * (u / (3 * NG)) + h) * TM + (g0 + u % NG) * 16 + c]; };
    bf16x8 ar[PD + 1];
#pragma unroll
    for (int u = 0; u < PD && u < U; u++) ar[u] = load_a(u);
#pragma unroll
    for (int u = 0; u < U; u++) {
        if (u + PD < U) ar[(u + PD) % (PD + 1)] = load_a(u + PD);
        acc[u % NG] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ar[u % (PD + 1)], b[u / (3 * NG)], acc[u % NG], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// the 16 bytes h + 4 k of product pid's row for every k-block k (pid < 0: zeros, nothing is read)
template <int D>
__device__ __forceinline__ void rb_load_b(bf16x8 (&b)[D / 32], const uint16_t* __restrict__ table, int pid, int h) {
    if (pid >= 0) {
        const bf16x8* f = reinterpret_cast<const bf16x8*>(table + (size_t)pid * D) + h;
#pragma unroll
        for (int k = 0; k < D / 32; k++) b[k] = f[4 * k];
    } else {
#pragma unroll
        for (int k = 0; k < D / 32; k++) b[k] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
}
