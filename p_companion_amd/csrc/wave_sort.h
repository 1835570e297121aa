// One wave's bitonic network over 64 NE register slots under the total order of grouped_plan.h (rg_better: value descending,
// index ascending).  The long-list kernels (grouped_list.h) compact a row's candidate buffer with it; ingest.hip sorts a short neighbour bucket
// (all values equal: the order is the ascending index).
#pragma once
#include "grouped_plan.h"

// The value of lane (lane ^ M) for M = 1, 2: a quad permutation on the VALU (DPP), no trip through the LDS crossbar; other
// strides by shuffle.
template <int M>
__device__ __forceinline__ int rl_lane_xor(int x) {
    if constexpr (M == 1) return __builtin_amdgcn_update_dpp(x, x, 0xB1, 0xF, 0xF, false);       // quad_perm [1, 0, 3, 2]
    else if constexpr (M == 2) return __builtin_amdgcn_update_dpp(x, x, 0x4E, 0xF, 0xF, false);  // quad_perm [2, 3, 0, 1]
    else return __shfl_xor(x, M, 64);
}

// One stride of the network between lanes: slot pairs (i, i ^ j) with j = NE * M.
template <int NE, int M>
__device__ __forceinline__ void rl_cross(float (&v)[NE], int (&ix)[NE], int lane, int k) {
    const bool lower = (lane & M) == 0;
#pragma unroll
    for (int e = 0; e < NE; e++) {
        const bool up = ((lane * NE + e) & k) == 0;
        const float ov = __int_as_float(rl_lane_xor<M>(__float_as_int(v[e])));
        const int oi = rl_lane_xor<M>(ix[e]);
        const bool ob = rg_better(ov, oi, v[e], ix[e]);
        if (ob == (lower == up)) { v[e] = ov; ix[e] = oi; }      // the lower slot of an `up` pair keeps the better one
    }
}

// The bitonic network over 64 NE slots (slot i = NE * lane + e), best first under rg_better.  Padding slots hold
// (-inf, RG_NONE), which nothing real follows.  Strides below NE run between a lane's own registers, the others between
// lanes.  All loops unroll: every register index is a constant.
template <int NE>
__device__ __forceinline__ void rl_sort(float (&v)[NE], int (&ix)[NE], int lane) {
    constexpr int LOG = NE == 2 ? 7 : (NE == 4 ? 8 : 9);
    static_assert(64 * NE == 1 << LOG, "slots");
#pragma unroll
    for (int lk = 1; lk <= LOG; lk++) {
#pragma unroll
        for (int lj = lk - 1; lj >= 0; lj--) {
            const int k = 1 << lk, j = 1 << lj;
            if (j < NE) {
#pragma unroll
                for (int e = 0; e < NE; e++) {
                    if ((e & j) == 0) {                   // the pair (e, e | j) of this lane: e takes the better one if `up`
                        const bool up = ((lane * NE + e) & k) == 0;
                        const bool sw = rg_better(v[e | j], ix[e | j], v[e], ix[e]);
                        if (sw == up) {
                            const float tv = v[e]; const int ti = ix[e];
                            v[e] = v[e | j]; ix[e] = ix[e | j];
                            v[e | j] = tv; ix[e | j] = ti;
                        }
                    }
                }
            } else {
                switch (j / NE) {                         // (a constant once unrolled)
                    case 1: rl_cross<NE, 1>(v, ix, lane, k); break;
                    case 2: rl_cross<NE, 2>(v, ix, lane, k); break;
                    case 4: rl_cross<NE, 4>(v, ix, lane, k); break;
                    case 8: rl_cross<NE, 8>(v, ix, lane, k); break;
                    case 16: rl_cross<NE, 16>(v, ix, lane, k); break;
                    default: rl_cross<NE, 32>(v, ix, lane, k); break;
                }
            }
        }
    }
}
