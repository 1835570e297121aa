// The device helpers the type-grouped catalogue kernels share (retrieve.hip with the merge, retrieve_bf16.hip, nearest.hip,
// retrieve_list.hip, rank.hip): the per-thread lists of up to 16 under rg_better, the dispatch on a tile's number of 16-row
// groups, the work-item decode, the fp32 query-tile load, a chunk's selection and the partial-list write.  One definition each: the bit-for-bit contracts between the entries (a zero
// bias is the unbiased entry, bf16 on integers is fp32, a short list is the 16-entry list) rest on the same selection.
#pragma once
#include <type_traits>
#include "grouped_plan.h"

#define RG_MAX_N 16

// insert (x, xi) into the descending list v / ix of length n (the caller has checked it beats the n-th entry)
__device__ __forceinline__ void rg_insert(float* v, int* ix, int n, float x, int xi) {
#pragma unroll
    for (int j = 0; j < RG_MAX_N; j++) {
        if (j < n && rg_better(x, xi, v[j], ix[j])) {
            const float tv = v[j]; const int ti = ix[j];
            v[j] = x; ix[j] = xi; x = tv; xi = ti;
        }
    }
}
__device__ __forceinline__ void rg_nth(const float* v, const int* ix, int n, float& tv, int& ti) {
#pragma unroll
    for (int j = 0; j < RG_MAX_N; j++)
        if (j == n - 1) { tv = v[j]; ti = ix[j]; }
}
__device__ __forceinline__ void rg_pop(float* v, int* ix) {
#pragma unroll
    for (int j = 0; j < RG_MAX_N - 1; j++) { v[j] = v[j + 1]; ix[j] = ix[j + 1]; }
    v[RG_MAX_N - 1] = -INFINITY; ix[RG_MAX_N - 1] = RG_NONE;
}

// f(integral_constant<R>) for the R in [1, RMAX] that equals rg: a score section written once per group count is straight-line
// code for every number of 16-row groups a tile can hold -- every loop bound a constant, no branch between an LDS read and
// its MFMA.
template <int RMAX, class F>
__device__ __forceinline__ void rg_dispatch_groups(int rg, F& f) {
    if (rg == RMAX) f(std::integral_constant<int, RMAX>{});
    else if constexpr (RMAX > 1) rg_dispatch_groups<RMAX - 1>(rg, f);
}

// Work item w = (type t, slice s, tile j), items of one type ordered slice-major so that the tiles running side by side read
// the same candidates (L2) -> the tile's rows order[p0 .. p0 + valid) in rg 16-row groups and the slice's candidates
// type_col[cb0 .. ce).
struct RgItem { int s, p0, valid, rg, cb0, ce; };
template <int TM>
__device__ __forceinline__ RgItem rg_decode(int64_t w, const int64_t* __restrict__ item_start, const int32_t* __restrict__ cnt,
                                            const int32_t* __restrict__ row_start, const int32_t* __restrict__ type_rowptr,
                                            int n_types, int S) {
    int lo = 0, hi = n_types - 1;                         // the largest t with item_start[t] <= w (< n_types: w < n_items)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (item_start[mid] <= w) lo = mid; else hi = mid - 1;
    }
    const int t = lo;
    const int rows_t = cnt[t];
    const int tiles = (rows_t + TM - 1) / TM;
    const int local = (int)(w - item_start[t]);
    RgItem it;
    it.s = local / tiles;
    const int j = local - it.s * tiles;
    it.p0 = row_start[t] + j * TM;
    it.valid = min(TM, rows_t - j * TM);
    it.rg = (it.valid + 15) >> 4;
    const int c0 = type_rowptr[t], C = type_rowptr[t + 1] - c0;
    int ns, L;
    rg_slice_plan(C, S, ns, L);
    it.cb0 = c0 + it.s * L;
    it.ce = c0 + min(C, (it.s + 1) * L);
    return it;
}

// One chunk's selection, the scores of the tile's rows against the chunk's RG_CHUNK candidates in sc and their product ids in
// cid (RG_NONE: no candidate).  Thread tid serves row rr = tid / TPR with the candidates qq + TPR k, qq = tid % TPR, and keeps
// a list v / ix of its best n; hv / hix is the row's threshold.  A candidate that does not beat the threshold -- the best of
// the TPR threads' n-th entries, so n products of the row beat it -- is out.  The test is cheap; the insertions then run as a
// loop over each lane's own survivors, so a wave pays for its busiest lane, not for every candidate some lane keeps.  EXCL: a
// survivor is searched in the row's exclusion list ex_col[elo, ehi) by bisection (the ids of a key are strictly ascending) and
// dropped BEFORE rg_insert, so an excluded product never enters a list and never moves a threshold: the threshold is still
// beaten by n kept products of the row, and the search is paid by the few survivors.  At the end the TPR threads of a row
// (adjacent lanes) agree on the row's new threshold.
template <int TM, bool EXCL>
__device__ __forceinline__ void rg_select_chunk(const float (*sc)[RG_CHUNK + 1], const int* cid, int rr, int qq, int valid, int n,
                                                float* v, int* ix, float& hv, int& hix, int elo, int ehi,
                                                const int32_t* __restrict__ ex_col) {
    constexpr int TPR = 256 / TM;            // threads per row
    constexpr int CPT = RG_CHUNK / TPR;      // candidates per thread per chunk
    unsigned keep = 0;
    if (rr < valid) {
#pragma unroll
        for (int k = 0; k < CPT; k++) {
            const int col = qq + TPR * k;
            const int xi = cid[col];
            if (xi != RG_NONE && rg_better(sc[rr][col], xi, hv, hix)) keep |= 1u << k;
        }
    }
    while (keep) {
        const int k = __builtin_ctz(keep);
        keep &= keep - 1;
        const int col = qq + TPR * k;
        const int xi = cid[col];
        const float x = sc[rr][col];
        if (rg_better(x, xi, hv, hix)) {
            if constexpr (EXCL) {
                int a = elo, b = ehi;                     // the first list entry >= xi
                while (a < b) {
                    const int mid = (a + b) >> 1;
                    if (ex_col[mid] < xi) a = mid + 1; else b = mid;
                }
                if (a < ehi && ex_col[a] == xi) continue;             // excluded: never inserted, the threshold stays
            }
            rg_insert(v, ix, n, x, xi);
            float tv = -INFINITY;                         // this thread's n-th entry
            int ti = RG_NONE;
            rg_nth(v, ix, n, tv, ti);
            if (rg_better(tv, ti, hv, hix)) { hv = tv; hix = ti; }
        }
    }
#pragma unroll
    for (int o = TPR / 2; o >= 1; o >>= 1) {
        const float ov = __shfl_xor(hv, o, 64);
        const int oi = __shfl_xor(hix, o, 64);
        if (rg_better(ov, oi, hv, hix)) { hv = ov; hix = oi; }
    }
}

// The TPR lists of a row (adjacent lanes) -> the top n of the row over the work item's slice, written as the partial list
// pv / pi[at .. at + n) by the row's writer (its first thread, where the row exists); at: the list's place in [rows][S][n], at
// the row's grouped position.
template <int TM>
__device__ __forceinline__ void rg_write_partial(float* v, int* ix, int n, bool writer, size_t at, float* __restrict__ pv,
                                                 int32_t* __restrict__ pi) {
    constexpr int TPR = 256 / TM;
    for (int k = 0; k < n; k++) {
        float bv = v[0];
        int bi = ix[0];
#pragma unroll
        for (int o = TPR / 2; o >= 1; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (rg_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        if (ix[0] == bi && bi != RG_NONE) rg_pop(v, ix);
        if (writer) {
            pv[at + k] = bv;
            pi[at + k] = bi;
        }
    }
}

// the rows order[p0 .. p0 + valid) of proj as the fp32 query tile in LDS (rows of QS floats; rows past `valid` of the last
// 16-row group are zero, rows past that group are never read)
template <int D, int QS>
__device__ __forceinline__ void rg_load_tile(float* q, const float* __restrict__ proj, const int32_t* __restrict__ order, int p0,
                                             int valid, int rg, int tid) {
    // (opaque to the optimiser: the addresses below are formed per work item and die with the load; hoisted out of the item loop
    // they live through the chunk loop, and the D = 128 kernels of nearest.hip then keep three of them in scratch)
    asm volatile("" : "+v"(tid));
    for (int e = tid; e < rg * 16 * (D / 4); e += 256) {
        const int row = e / (D / 4), d4 = e - row * (D / 4);
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < valid) x = reinterpret_cast<const float4*>(proj + (size_t)order[p0 + row] * D)[d4];
        *reinterpret_cast<float4*>(&q[row * QS + 4 * d4]) = x;
    }
}
