// What the two ranks under a per-row predicate share (where_rank.hip over the fp32 table, where_rank_bf16.hip over the bf16
// copy): the pairing rule of a pc_row_where, a row's four words, the test, and the count of one chunk -- everything but the
// score chain, which is the table's own.  pc_row_where's predicate as grouped_list.h's WHERE hook tests it:
//   product p passes row r  iff  lo[r] <= value[p] && value[p] <= hi[r]                          (two fp32 compares, ends inclusive)
//                           and  (flags[p] & need[r]) == need[r] && (flags[p] & deny[r]) == 0    (32 bits, bit 31 among them)
// An absent array is a null pointer behind a wave-uniform branch and is never read: the word in its place passes everything
// (value 0 within [-inf, +inf]; flags 0 under need = deny = 0).
#pragma once
#include "common.h"

// RlWhere's pairing rule (grouped_list.h), and a null filter is refused
inline bool wr_where_ok(const pc_row_where* w) {
    return w && (w->value ? w->lo && w->hi : !w->lo && !w->hi) && (w->flags || (!w->need && !w->deny));
}

// A row's predicate: 16 bytes, so the lanes of one k-lane read a row's four words in one ds_read_b128 (a broadcast).
struct __attribute__((aligned(16))) WrRow {
    float lo, hi;
    int need, deny;
};

// row r's words (r < 0: no row -- the words that pass everything, as where a part is not given)
__device__ __forceinline__ WrRow wr_row(const pc_row_where& wh, int r) {
    WrRow w{-INFINITY, INFINITY, 0, 0};
    if (r >= 0) {
        if (wh.value) { w.lo = wh.lo[r]; w.hi = wh.hi[r]; }
        if (wh.need) w.need = wh.need[r];
        if (wh.deny) w.deny = wh.deny[r];
    }
    return w;
}

// product id's attributes (an absent array: the word that passes; id < 0 reads entry 0, and nothing of it is used)
__device__ __forceinline__ float wr_value(const pc_row_where& wh, int id) { return wh.value ? wh.value[max(id, 0)] : 0.f; }
__device__ __forceinline__ int wr_flags(const pc_row_where& wh, int id) { return wh.flags ? wh.flags[max(id, 0)] : 0; }

// two fp32 compares (a NaN passes nothing) and two masks
__device__ __forceinline__ bool wr_pass(const WrRow& w, float a, int f) {
    return w.lo <= a && a <= w.hi && (f & w.need) == w.need && (f & w.deny) == 0;
}

// One chunk's count for a lane: its column's product pid (attributes a / f, term bs) against the NG x 4 query rows
// g * 16 + 4 h + k whose scores the accumulators hold.  A score above the row's g is counted where the product passes THAT
// row's predicate: a 16-row group holds rows with different predicates, so the pass bit is per (row, candidate), from the
// row's words in LDS (wq) -- 16 bytes per row, read as the count goes, never held over the chain.  Equal to g (the target
// itself, a copy of its row, or chance): the product index decides, among passing products -- rare, so the rows' targets
// stay in LDS and are read only where a lane meets such a score.  The rows' g are read from LDS per row group too (one
// ds_read_b128 of gs), not held across the chain as the unfiltered kernels hold them: that gives back 4 NG registers, more
// than the attributes and the row's words take, so every variant stays inside its twin's registers.  The fence after each
// row group keeps the scheduler from hoisting all 4 NG reads of wq (4 registers each) above the compares.
template <int NG, bool BIAS>
__device__ __forceinline__ void wr_count(f32x4 (&acc)[NG], float bs, const float* gs, int (&cn)[NG][4], const int* ys,
                                         const WrRow* wq, int pid, float a, int f, int h) {
    if (pid < 0) return;
    bool tie = false;
#pragma unroll
    for (int g = 0; g < NG; g++) {
        if constexpr (BIAS) acc[g] += bs;                             // the one addition: s = fl(d + bias[pid])
        const float4 x = *reinterpret_cast<const float4*>(&gs[g * 16 + 4 * h]);
        const float gv[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const WrRow w = wq[g * 16 + 4 * h + k];
            cn[g][k] += (acc[g][k] > gv[k] && wr_pass(w, a, f)) ? 1 : 0;
            tie |= acc[g][k] == gv[k];
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    if (tie) {
#pragma unroll
        for (int g = 0; g < NG; g++)
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const int row = g * 16 + 4 * h + k;
                if (acc[g][k] == gs[row] && pid < ys[row] && wr_pass(wq[row], a, f)) cn[g][k]++;
            }
    }
}

// the 16 columns of a (wave, k-lane) -> lane c == 0 -> part[wv][row]
template <int NG, int TM>
__device__ __forceinline__ void wr_reduce(const int (&cn)[NG][4], int (*part)[TM], int wv, int c, int h) {
#pragma unroll
    for (int g = 0; g < NG; g++)
#pragma unroll
        for (int k = 0; k < 4; k++) {
            int v = cn[g][k];
#pragma unroll
            for (int o = 8; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
            if (c == 0) part[wv][g * 16 + 4 * h + k] = v;
        }
}
