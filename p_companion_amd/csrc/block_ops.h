// The block-level integer primitives of the data-preparation units (ingest.hip, events.hip, table_train.hip, generator.hip's
// scan): wave and workgroup sums, exclusive sums and predicate ranks, the inclusive scan of 1024 LDS partials, the pieces of a
// stable LSD radix sort over 8-bit digits.  Device inline functions in the manner of wave_sort.h: no kernels, no entry points,
// every LDS array the caller's; all threads of the wave (wave_*) or the workgroup (block_*, radix_*) call one together.
//
// Why the radix scatter is STABLE (so that the sparse Adam's fp32 sums and the co-view weights are functions of their inputs
// alone): elements of one digit are placed in source order, by three nested orders.
//   tiles   a range is walked in tiles of NT consecutive elements; base[d], where the next element of digit d goes, advances
//           by the tile's count of d after the whole tile is placed (a caller that splits a range into chunks, table_train.hip,
//           starts a chunk's base[d] behind the earlier chunks' elements of d)
//   waves   wave w holds the tile's elements 64 w .. 64 w + 63 and starts behind wcnt[q][d] summed over the waves q < w
//   lanes   lane l holds element 64 w + l; its rank is the number of LOWER lanes that agree with it in all eight digit bits
#pragma once
#include <type_traits>
#include "common.h"

// ---- sums and ranks ---------------------------------------------------------------------------------------------------
// The sum of v over the wave, in every lane (int, long long, unsigned long long; common.h has the float one).
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
    static_assert(std::is_integral_v<T>, "float: common.h's wave_sum");
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The sum of x over the lower lanes; total: the sum over the wave.
__device__ __forceinline__ int wave_exclusive_sum(int x, int lane, int& total) {
    int inc = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int y = __shfl_up(inc, d, 64); inc += lane >= d ? y : 0; }
    total = __shfl(inc, 63, 64);
    return inc - x;
}

// The sum of c over the NT-thread workgroup, in every thread.  wsum: NT / 64 LDS ints (unused at NT == 64: no barrier).
template <int NT>
__device__ __forceinline__ int block_sum(int c, int* wsum) {
    c = wave_sum(c);
    if constexpr (NT > 64) {
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = c;
        __syncthreads();
        c = 0;
#pragma unroll
        for (int i = 0; i < NT / 64; i++) c += wsum[i];
        __syncthreads();
    }
    return c;
}

// Position of a thread's element among the workgroup's elements with `pred`, in thread order, and their number.  wsum: NT / 64
// LDS ints (unused at NT == 64: no barrier).
template <int NT>
__device__ __forceinline__ int block_rank(bool pred, int* wsum, int& total) {
    const unsigned long long m = __ballot(pred);
    const int lane = threadIdx.x & 63;
    int r = __popcll(m & ((1ull << lane) - 1ull));
    total = __popcll(m);
    if constexpr (NT > 64) {
        const int w = threadIdx.x >> 6;
        if (lane == 0) wsum[w] = total;
        __syncthreads();
        int tot = 0;
#pragma unroll
        for (int i = 0; i < NT / 64; i++) { const int c = wsum[i]; r += i < w ? c : 0; tot += c; }
        total = tot;
        __syncthreads();
    }
    return r;
}

// Inclusive Hillis-Steele scan of one partial per thread of a 1024-thread workgroup through part[1024] (LDS): returns the sum
// over threads 0 .. threadIdx.x, and part[] holds every thread's on exit (part[1023]: the total).
template <typename T>
__device__ __forceinline__ T block_scan_1024(T x, T* part) {
    const int t = threadIdx.x;
    part[t] = x;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {
        const T v = t >= o ? part[t - o] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    return part[t];
}

// ---- the radix pass ---------------------------------------------------------------------------------------------------
// cnt[0, 256) (LDS) = the counts of the 8-bit digit at `shift` over key[lo, hi), a barrier behind them
template <int NT, typename K, typename I>
__device__ __forceinline__ void radix_hist(const K* key, I lo, I hi, int shift, int* cnt) {
    if (NT == 256 || threadIdx.x < 256) cnt[threadIdx.x] = 0;
    __syncthreads();
    for (I i = lo + (I)threadIdx.x; i < hi; i += NT) atomicAdd(&cnt[((uint32_t)key[i] >> shift) & 255u], 1);
    __syncthreads();
}

// The keys of a digit below d: thread d's offset among the digits.
__device__ __forceinline__ int radix_digit_offset(const int* cnt, int d) {
    int ex = 0;
    for (int e = 0; e < d; e++) ex += cnt[e];
    return ex;
}

// The number of lower lanes that are valid and hold digit d; same: the number of all such lanes, this one included.
__device__ __forceinline__ int wave_digit_rank(bool valid, uint32_t d, int lane, int& same) {
    unsigned long long m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; b++) {
        const bool bit = (d >> b) & 1u;
        const unsigned long long bm = __ballot(valid && bit);
        m &= bit ? bm : ~bm;
    }
    same = __popcll(m);
    return __popcll(m & ((1ull << lane) - 1ull));
}

// One stable scatter of skey[lo, hi) (HAS_VAL: and sval) by the 8-bit digit at `shift`, see the head of this file.  base[d]
// (256 LDS ints): where the next element of digit d goes, advanced by the range's counts on exit; wcnt: NT / 64 x 256 LDS ints.
// A position at or past `limit` is not written (never, when base[] scans this pass's digit counts below limit).
template <int NT, bool HAS_VAL, typename K, typename I>
__device__ __forceinline__ void radix_scatter(const K* skey, const uint32_t* sval, K* dkey, uint32_t* dval, I lo, I hi, I limit,
                                              int shift, int* base, int* wcnt) {
    static_assert(NT >= 256 && NT % 64 == 0, "threads 0 .. 255 own a digit each");
    constexpr int NW = NT / 64;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (I b0 = lo; b0 < hi; b0 += NT) {
#pragma unroll
        for (int j = 0; j < 4; j++) wcnt[j * NT + tid] = 0;   // (NW x 256 = 4 NT)
        __syncthreads();                                      // (orders base[] of the previous tile / the caller's scan as well)
        const I i = b0 + tid;
        const bool valid = i < hi;
        const uint32_t k = valid ? (uint32_t)skey[i] : 0u;
        uint32_t v = 0u;
        if constexpr (HAS_VAL) v = valid ? sval[i] : 0u;
        const uint32_t d = (k >> shift) & 255u;
        int same;
        const int r = wave_digit_rank(valid, d, lane, same);
        if (valid && r == 0) wcnt[w * 256 + d] = same;
        __syncthreads();
        if (valid) {
            I pos = (I)(base[d] + r);
            if constexpr (NW <= 4) {                          // (few waves: every slot read, the later ones selected to 0)
#pragma unroll
                for (int q = 0; q < NW; q++) pos += q < w ? (I)wcnt[q * 256 + d] : 0;
            } else {
                for (int q = 0; q < w; q++) pos += (I)wcnt[q * 256 + d];
            }
            if (pos < limit) {
                dkey[pos] = (K)k;
                if constexpr (HAS_VAL) dval[pos] = v;
            }
        }
        __syncthreads();
        if (NT == 256 || tid < 256) {
            int t = 0;
#pragma unroll
            for (int q = 0; q < NW; q++) t += wcnt[q * 256 + tid];
            base[tid] += t;
        }
        __syncthreads();
    }
}
