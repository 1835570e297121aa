// The long-list family's bf16 score chain, shared by the units that score the bf16 copy of the catalogue:
// retrieve_list_bf16.hip and, under a per-product bias, nearest_list_bf16.hip.  One text, so a (row, product) pair has the same
// chain bits in both.
#pragma once
#include "grouped_list.h"

// retrieve_bf16.hip's chain (rg_score_bf16_kernel) at one 16-row group: the fp32 query tile is split ONCE per work item by
// split3 into the pieces p0, p1, p2, each an image of [D / 8][16] operands of 16 bytes (12 KB at D = 128, 24 KB at D = 256; with
// 16 rows the sixteen lanes c at one k-lane h read sixteen consecutive operands, so there is no padding); lane (c, h) holds the
// 8 dimensions 32 k + 8 h .. + 7 of candidate c for every k-block k.  LDS at NE = 8: 58 KB of buffers, 12 / 24 KB of images,
// 4 KB of scores.
template <int D_>
struct RlChainBf16 {
    static constexpr int D = D_, NB = D / 32;
    using Table = uint16_t;
    using B = bf16x8;
    using Q = bf16x8[3][(D / 8) * RL_TM];
    static __device__ __forceinline__ void load_tile(Q& q, const float* __restrict__ proj, const int32_t* __restrict__ order,
                                                     int p0, int valid, int tid) {
        for (int e = tid; e < RL_TM * (D / 8); e += 256) {
            const int d8 = e / RL_TM, row = e - d8 * RL_TM;           // (row fastest: a wave's 16-byte stores are contiguous)
            float4 x0 = make_float4(0.f, 0.f, 0.f, 0.f), x1 = x0;
            if (row < valid) {
                const float4* f = reinterpret_cast<const float4*>(proj + (size_t)order[p0 + row] * D) + 2 * d8;
                x0 = f[0];
                x1 = f[1];
            }
            const Split3 sp = split3(x0, x1);
            q[0][d8 * RL_TM + row] = sp.p0;
            q[1][d8 * RL_TM + row] = sp.p1;
            q[2][d8 * RL_TM + row] = sp.p2;
        }
    }
    static __device__ __forceinline__ B zero() { return bf16x8{0, 0, 0, 0, 0, 0, 0, 0}; }
    static __device__ __forceinline__ f32x4 score(const Q& q, const B* b, int c, int h) {
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < NB; k++) {
#pragma unroll
            for (int p = 0; p < 3; p++)
                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(q[p][(4 * k + h) * RL_TM + c], b[k], acc, 0, 0, 0);
        }
        return acc;
    }
};
