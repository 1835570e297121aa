// Four rows per wave-iteration, as the attention cores walk their key rows (attention.hip: attn_core_fwd4 / bwd4, the dK|dV
// rows; export.hip: the ragged core over the co-view CSR): lane = 16 g + l owns dims [DL l, DL l + DL) of row n0 + g
// (DL = D / 16: 8 or 16).  The lane's slice of a row, and the two transposing reductions over the heads.
#pragma once
#include "common.h"

template <int DL> struct LD { float v[DL]; };
template <int DL> __device__ __forceinline__ LD<DL> ld_load(const float* p) {
    LD<DL> r;
#pragma unroll
    for (int i = 0; i < DL / 4; i++) {
        const float4 t = *reinterpret_cast<const float4*>(p + 4 * i);
        r.v[4 * i] = t.x; r.v[4 * i + 1] = t.y; r.v[4 * i + 2] = t.z; r.v[4 * i + 3] = t.w;
    }
    return r;
}
template <int DL> __device__ __forceinline__ void ld_store(float* p, const LD<DL>& r) {
#pragma unroll
    for (int i = 0; i < DL / 4; i++) *reinterpret_cast<float4*>(p + 4 * i) = make_float4(r.v[4 * i], r.v[4 * i + 1], r.v[4 * i + 2], r.v[4 * i + 3]);
}
// four values per lane summed over the 16 lanes of a row group: afterwards lane l holds the total of value (l >> 2), the
// same bits in the four lanes of a head
__device__ __forceinline__ float heads_reduce16(float v0, float v1, float v2, float v3, int l) {
    const bool hi8 = (l & 8) != 0, hi4 = (l & 4) != 0;
    float a = hi8 ? v2 : v0, b = hi8 ? v3 : v1;
    const float sa = hi8 ? v0 : v2, sb = hi8 ? v1 : v3;
    a += __shfl_xor(sa, 8, 64);
    b += __shfl_xor(sb, 8, 64);
    float k = hi4 ? b : a;
    const float s = hi4 ? a : b;
    k += __shfl_xor(s, 4, 64);
    k += __shfl_xor(k, 2, 64);
    k += __shfl_xor(k, 1, 64);
    return k;
}
// fold the four row groups: per dim, the four head sums o0..o3 transpose-reduce over the groups (xor 32: keep two heads,
// xor 16: keep one) -- lane group g ends with head g.  The sums by value, and hi32 = (lane & 32) != 0, hi16 = (lane & 16) != 0
// formed by the caller: the caller's accumulators then stay scalars and its lane tests fold onto threadIdx before this is
// inlined, and the callers' instruction text is what it is with the fold written out in them.
template <int DL> __device__ __forceinline__ LD<DL> heads_fold4(LD<DL> o0, LD<DL> o1, LD<DL> o2, LD<DL> o3, bool hi32, bool hi16) {
    LD<DL> out;
#pragma unroll
    for (int d = 0; d < DL; d++) {
        float a = hi32 ? o2.v[d] : o0.v[d], bb = hi32 ? o3.v[d] : o1.v[d];
        const float sa = hi32 ? o0.v[d] : o2.v[d], sb = hi32 ? o1.v[d] : o3.v[d];
        a += __shfl_xor(sa, 32, 64);
        bb += __shfl_xor(sb, 32, 64);
        float k = hi16 ? bb : a;
        const float s2 = hi16 ? a : bb;
        k += __shfl_xor(s2, 16, 64);
        out.v[d] = k;
    }
    return out;
}
