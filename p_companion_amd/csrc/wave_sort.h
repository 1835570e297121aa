// One wave's bitonic network over 64 NE register slots under the total order of grouped_plan.h (rg_better: value descending,
// index ascending).  The long-list kernels (grouped_list.h) compact a row's candidate buffer with it; ingest.hip sorts a short neighbour bucket
// (all values equal: the order is the ascending index); fuse_lists.hip sorts a basket's pool of up to 1024 slots and carries
// each product's support through a second sort (rlw_sort, rlw_sort_with at the end of this file).
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

// ---- the same network for up to 16 slots per lane, with one int of payload per slot (fuse_lists.hip) --------------------
// At NE = 16 the network is too long for the optimizer's unrolling budget (the pragmas above are then dropped and the register
// indices become variables), so its strides are instantiated one by one; PAY: pay[] moves with its slot and is never compared
// (otherwise it is not touched).  The values are floats under rg_better or ints under the same rule (rlw_key: a float's bits
// as an int of the same order, in which +0.0 stands before -0.0 -- a strict order on the bits: an exchange between two lanes
// copies the better slot over an EQUAL one, so two slots that rg_better calls equal must be the same bits, or one of them is
// lost).  rl_sort above stays as it is: the kernels built on it keep their code.
__device__ __forceinline__ int rlw_key(float x) {
    const int b = __float_as_int(x);
    return b ^ ((b >> 31) & 0x7fffffff);                  // (its own inverse)
}
__device__ __forceinline__ float rlw_unkey(int k) { return __int_as_float(k ^ ((k >> 31) & 0x7fffffff)); }

__device__ __forceinline__ bool rlw_better(float x, int xi, float y, int yi) { return rg_better(x, xi, y, yi); }
__device__ __forceinline__ bool rlw_better(int x, int xi, int y, int yi) { return x > y || (x == y && xi < yi); }

template <int M>
__device__ __forceinline__ float rlw_lane_xor(float x) { return __int_as_float(rl_lane_xor<M>(__float_as_int(x))); }
template <int M>
__device__ __forceinline__ int rlw_lane_xor(int x) { return rl_lane_xor<M>(x); }

// One stride between lanes: slot pairs (i, i ^ j) with j = NE * M.
template <int NE, int M, bool PAY, typename T>
__device__ __forceinline__ void rlw_cross(T (&v)[NE], int (&ix)[NE], int (&pay)[NE], int lane, int k) {
    const bool lower = (lane & M) == 0;
#pragma unroll
    for (int e = 0; e < NE; e++) {
        const bool up = ((lane * NE + e) & k) == 0;
        const T ov = rlw_lane_xor<M>(v[e]);
        const int oi = rlw_lane_xor<M>(ix[e]);
        const bool take = rlw_better(ov, oi, v[e], ix[e]) == (lower == up);       // the lower slot of an `up` pair keeps the better one
        if constexpr (PAY) {
            const int op = rlw_lane_xor<M>(pay[e]);
            pay[e] = take ? op : pay[e];
        }
        if (take) { v[e] = ov; ix[e] = oi; }
    }
}

// One stride between a lane's own registers: the pairs (e, e | J), J < NE; e takes the better one if `up`.
template <int NE, int J, bool PAY, typename T>
__device__ __forceinline__ void rlw_within(T (&v)[NE], int (&ix)[NE], int (&pay)[NE], int lane, int k) {
#pragma unroll
    for (int e = 0; e < NE; e++) {
        if ((e & J) == 0) {
            const bool up = ((lane * NE + e) & k) == 0;
            const bool sw = rlw_better(v[e | J], ix[e | J], v[e], ix[e]);
            if (sw == up) {
                const T tv = v[e]; const int ti = ix[e];
                v[e] = v[e | J]; ix[e] = ix[e | J];
                v[e | J] = tv; ix[e | J] = ti;
                if constexpr (PAY) { const int tp = pay[e]; pay[e] = pay[e | J]; pay[e | J] = tp; }
            }
        }
    }
}

// The strides (LK, LJ), (LK, LJ - 1), ..., (LK, 0), (LK + 1, LK), ... up to LK = LOG: rl_sort's order of strides.
template <int NE, bool PAY, int LOG, int LK, int LJ, typename T>
__device__ __forceinline__ void rlw_strides(T (&v)[NE], int (&ix)[NE], int (&pay)[NE], int lane) {
    constexpr int k = 1 << LK, j = 1 << LJ;
    if constexpr (j < NE) rlw_within<NE, j, PAY>(v, ix, pay, lane, k);
    else rlw_cross<NE, j / NE, PAY>(v, ix, pay, lane, k);
    if constexpr (LJ > 0) rlw_strides<NE, PAY, LOG, LK, LJ - 1>(v, ix, pay, lane);
    else if constexpr (LK < LOG) rlw_strides<NE, PAY, LOG, LK + 1, LK>(v, ix, pay, lane);
}

// rl_sort for NE = 2, 4, 8, 16 over floats or keys: slot i = NE * lane + e, best first.
template <int NE, typename T>
__device__ __forceinline__ void rlw_sort(T (&v)[NE], int (&ix)[NE], int lane) {
    constexpr int LOG = NE == 2 ? 7 : (NE == 4 ? 8 : (NE == 8 ? 9 : 10));
    static_assert(64 * NE == 1 << LOG, "slots");
    rlw_strides<NE, false, LOG, 1, 0>(v, ix, ix, lane);   // (no payload: the third argument is not read)
}

// ... and with a payload.
template <int NE, typename T>
__device__ __forceinline__ void rlw_sort_with(T (&v)[NE], int (&ix)[NE], int (&pay)[NE], int lane) {
    constexpr int LOG = NE == 2 ? 7 : (NE == 4 ? 8 : (NE == 8 ? 9 : 10));
    static_assert(64 * NE == 1 << LOG, "slots");
    rlw_strides<NE, true, LOG, 1, 0>(v, ix, pay, lane);
}
