// The long-list family's fp32 score chain, shared by the units that score the fp32 table: retrieve_list.hip and, under a
// per-product bias, nearest_list.hip.  One text, so a (row, product) pair has the same chain bits in both.
#pragma once
#include "grouped_list.h"

// retrieve.hip's chain at one 16-row group: the query tile as padded fp32 rows; lane (c, h) holds the dimensions
// 16 k + 4 h .. + 3 of candidate c for every k, one 16x16x4 f32 MFMA per dimension.
template <int D_>
struct RlChainF32 {
    static constexpr int D = D_, QS = D + 4, NB = D / 16;
    using Table = float;
    using B = float4;
    using Q = float[RL_TM * QS];
    static __device__ __forceinline__ void load_tile(Q& q, const float* __restrict__ proj, const int32_t* __restrict__ order,
                                                     int p0, int valid, int tid) {
        for (int e = tid; e < RL_TM * (D / 4); e += 256) {
            const int row = e / (D / 4), d4 = e - row * (D / 4);
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row < valid) x = reinterpret_cast<const float4*>(proj + (size_t)order[p0 + row] * D)[d4];
            *reinterpret_cast<float4*>(&q[row * QS + 4 * d4]) = x;
        }
    }
    static __device__ __forceinline__ B zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
    static __device__ __forceinline__ f32x4 score(const Q& q, const B* b, int c, int h) {
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < NB; k++) {
            const float4 a = *reinterpret_cast<const float4*>(&q[c * QS + 16 * k + 4 * h]);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b[k].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b[k].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b[k].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b[k].w, acc, 0, 0, 0);
        }
        return acc;
    }
};
