// The k-chain of the rank kernels (rank.hip: rk_rank_kernel; rank_exclude.hip: rk_exclude_kernel) and the layout of the query
// tile it reads.  One definition: a score formed by either kernel is the same bits.
#pragma once
#include "common.h"

// LDS row of the query tile: D + 8 floats.  Lane (c, h) reads the 16 bytes at row c, float 16 k + 4 h, and ds_read_b128
// serves a wave in four groups of 16 lanes (lanes 0-3, 12-15, 20-27 | 4-11, 16-19, 28-31 | the same + 32) over 16 slots of
// 16 bytes: with a row stride of 2 slots mod 16 each group's 16 reads take 16 different slots.  (D + 4, one slot, puts
// lanes 12 and 27 of the first group on one slot: five LDS cycles per read instead of four.)
#define RK_QS(D) ((D) + 8)

// THE k-chain (rg_score_kernel's): NG row groups from g0 on against the 16 columns whose rows the lanes hold in b.  For one
// accumulator the MFMAs run in the order of the dimension index (step k, element x y z w); unit u = (k = u / NG, group
// u % NG) is four MFMAs on one ds_read_b128 of the query tile, read PD units ahead.  next != null: once step k's last unit
// has read b[k], the register takes the same 16 bytes of the lane's NEXT column (next + 4 k), so a whole chunk's time
// covers that load and one set of row registers serves both chunks.  The fence after each unit keeps the scheduler from
// hoisting all NB * NG query reads (4 registers each) and from sinking the refills, which would push the kernel's
// registers into scratch.
template <int D, int NG>
__device__ __forceinline__ void rk_chain(const float* q, int g0, float4 (&b)[D / 16], const float4* next, f32x4 (&acc)[NG],
                                         int c, int h) {
    constexpr int QS = RK_QS(D), NB = D / 16, U = NB * NG, PD = 3;
    auto load_a = [&](int u) {
        return *reinterpret_cast<const float4*>(&q[((g0 + u % NG) * 16 + c) * QS + 16 * (u / NG) + 4 * h]);
    };
    float4 ar[PD + 1];
#pragma unroll
    for (int u = 0; u < PD && u < U; u++) ar[u] = load_a(u);
#pragma unroll
    for (int u = 0; u < U; u++) {
        if (u + PD < U) ar[(u + PD) % (PD + 1)] = load_a(u + PD);
        const float4 a = ar[u % (PD + 1)];
        const int k = u / NG, g = u % NG;
        acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b[k].x, acc[g], 0, 0, 0);
        acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b[k].y, acc[g], 0, 0, 0);
        acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b[k].z, acc[g], 0, 0, 0);
        acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b[k].w, acc[g], 0, 0, 0);
        if (next && g == NG - 1) b[k] = next[4 * k];
        __builtin_amdgcn_sched_barrier(0);
    }
}
