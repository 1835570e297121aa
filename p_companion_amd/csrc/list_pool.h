// What the list post-passes share: one wave owns one output row, its pool in NE register slots per lane.  Two forced-inline
// blocks: the ban-set pass that strikes slots out of the pool (fuse_sessions.hip), and the store tail that writes the kept slots
// and the padding behind them (cap_lists.hip, fuse_sessions.hip).  What makes a slot a candidate, the sorts and the walks
// between the two are the units' own.  fuse_lists.hip still carries both blocks written out: fl_fuse_kernel<16> runs at the
// edge of the register file, and with either block called from here its max walk came out 0.6 to 3.5 % slower in every helper
// form tried (HISTORY.md "Shared list post-pass blocks"); a change to one copy goes into the other.
#pragma once
#include "common.h"

#define LP_CHUNK 256               // ban ids per pass through LDS

typedef int lp_i32x4 __attribute__((ext_vector_type(4)));

// The ban set of one basket or session: its `count` sources src[0 .. count) -- product ids, -1 = no item -- and, with the CSR
// (ex_rowptr [num_products + 1], ex_col; both NULL: the sources alone), every id in the exclusion rows of those sources.  A
// slot e of any lane with a[e] equal to a ban id becomes (a_none, b_none).  COMPL: a[] holds ~id, so the ids are stored and
// matched complemented (~(-1) = 0, no candidate's value, which is negative); otherwise a[] holds the id and -1 matches nothing.
// A source outside [-1, num_products) is never used as an index, is counted (one integer atomic) and bans nothing.
// The sources go 64 at a time, one per lane, and behind them their exclusion rows as ONE flat list: a bisection over the
// lanes' scanned row lengths finds the row of a flat position.  The ids stream through lban, the wave's own LP_CHUNK-entry LDS
// chunk (16-byte aligned), which every lane walks as 16-byte broadcast reads against its own slots.  Wave-uniform control
// flow throughout; no workgroup barrier.
template <int NE, bool COMPL, typename B>
__device__ __forceinline__ void lp_ban_pass(const int32_t* src, int count, const int32_t* ex_rowptr, const int32_t* ex_col,
                                            int num_products, int32_t* bad_count, int* lban, int lane, int (&a)[NE], B (&b)[NE],
                                            int a_none, B b_none) {
    for (int s0 = 0; s0 < count; s0 += 64) {              // (int: count is at most the caller's row count, an int)
        int id = -1;
        if (s0 + lane < count) {
            id = src[s0 + lane];
            if (id < -1 || id >= num_products) {          // never used as an index; its row offered nothing at the load
                if (bad_count) atomicAdd(bad_count, 1);
                id = -1;
            }
        }
        int lo = 0, len = 0;
        if (ex_rowptr && id >= 0) {                       // (id < num_products: rowptr has num_products + 1 entries)
            lo = ex_rowptr[id];
            len = max(ex_rowptr[id + 1] - lo, 0);
        }
        int inc = len;                                    // the inclusive scan of the lanes' row lengths
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(inc, o, 64);
            if (lane >= o) inc += t;
        }
        const int total = __shfl(inc, 63, 64);
        for (int base = 0; base < 64 + total; base += LP_CHUNK) {                 // flat: 64 sources, then `total` row entries
#pragma unroll
            for (int k = 0; k < LP_CHUNK / 64; k++) {
                const int p = base + lane + 64 * k - 64;  // the flat position among the row entries
                int owner = 0;                            // the lanes whose rows end at or before p: the row that holds p
#pragma unroll
                for (int step = 32; step >= 1; step >>= 1)
                    if (__shfl(inc, owner + step - 1, 64) <= p) owner += step;    // (owner + step - 1 <= 63)
                const int o_inc = __shfl(inc, owner, 64), o_len = __shfl(len, owner, 64), o_lo = __shfl(lo, owner, 64);
                int x = -1;                               // equal to no candidate's id
                if (p < 0) x = id;                        // (base 0, k 0: the lane's own source)
                else if (p < total) x = ex_col[(size_t)o_lo + (p - (o_inc - o_len))];
                lban[lane + 64 * k] = COMPL ? ~x : x;
            }
            // Same-wave LDS instructions execute in order: the lanes' stores are in LDS before any lane's read-back.
            __builtin_amdgcn_wave_barrier();
            const int nq = (min(LP_CHUNK, 64 + total - base) + 3) >> 2;
            for (int q = 0; q < nq; q++) {
                const lp_i32x4 x = *reinterpret_cast<const lp_i32x4*>(&lban[4 * q]);            // (a broadcast)
#pragma unroll
                for (int t = 0; t < 4; t++)
#pragma unroll
                    for (int e = 0; e < NE; e++)
                        if (x[t] == a[e]) { a[e] = a_none; b[e] = b_none; }
            }
            __builtin_amdgcn_wave_barrier();              // the reads are done before the next chunk's stores
        }
    }
}

// The store tail of one output row: the wave's slots stand in serving order (slot NE * lane + e), keep[e] marks the ones to
// serve.  The kept flags are counted per lane, a shuffle scan over the wave gives each kept slot its place, places below n are
// stored at out[off + place] -- off = (size_t)row * n --, and the tail [kept, n) is filled with -1 / -inf (/ 0).  SUP: the row
// has a support column (sup, out_support); without it neither is read.
template <int NE, bool SUP>
__device__ __forceinline__ void lp_store_row(const bool (&keep)[NE], const int (&ix)[NE], const float (&v)[NE],
                                             const int (&sup)[NE], int lane, int n, size_t off, int32_t* out_idx,
                                             float* out_score, int32_t* out_support) {
    int mine = 0;
#pragma unroll
    for (int e = 0; e < NE; e++) mine += keep[e];
    int inc = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(inc, o, 64);
        if (lane >= o) inc += t;
    }
    const int kept = __shfl(inc, 63, 64);
    int pos = inc - mine;
#pragma unroll
    for (int e = 0; e < NE; e++) {
        if (keep[e]) {
            if (pos < n) {
                out_idx[off + pos] = ix[e];
                out_score[off + pos] = v[e];
                if constexpr (SUP) out_support[off + pos] = sup[e];
            }
            pos++;
        }
    }
    for (int k = kept + lane; k < n; k += 64) {
        out_idx[off + k] = -1;
        out_score[off + k] = -INFINITY;
        if constexpr (SUP) out_support[off + k] = 0;
    }
}
