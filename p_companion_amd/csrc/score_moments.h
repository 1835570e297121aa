// What the two score-moment kernels share (score_moments.hip over the fp32 table, score_moments_bf16.hip over the bf16 copy):
// the sums of one chunk, the reduction of a work item, the (row, slice) partials in the workspace and the finishing kernel's
// launch -- everything but the score chain, which is the table's own.  For row r of type t with n_t candidates and pivot
// g_r = the score of the type's first candidate type_col[type_rowptr[t]]:
//   d_p = fl(s_p - g_r),   S1 = sum_p d_p,   S2 = sum_p d_p^2   over the type's candidates,
// the first two moments of the row's scores about a point INSIDE their range: S2 then has no term of the size of mean^2, which a
// raw sum of s^2 loses to cancellation where |mean| >> std.
#pragma once
#include "common.h"
#include "grouped_plan.h"

// A moments entry's workspace: the plan, then the slices' partial sums p1 / p2 [rows][S] and the pivots pg [rows], all three at
// the rows' grouped positions.
struct SmWs {
    RgPlan plan;
    float *p1, *p2, *pg;
    size_t bytes;
};
inline SmWs sm_ws_carve(void* ws, int rows, int n_types, int S) {
    SmWs w;
    WsCarver cv(ws);
    w.plan = rg_plan_carve(cv, rows, n_types);
    w.p1 = (float*)cv.bytes((size_t)rows * S * 4);
    w.p2 = (float*)cv.bytes((size_t)rows * S * 4);
    w.pg = (float*)cv.bytes((size_t)rows * 4);
    w.bytes = cv.total;
    return w;
}

// The outputs of an entry, one value per row.
struct SmOut {
    int32_t* count;
    float *pivot, *s1, *s2, *mean, *std;
};

// What both entries check before anything is launched, in the rank entries' order (the table's alignment is the bf16 entry's).
inline int sm_check(const void* proj, const void* types, const void* type_rowptr, const void* type_col, const void* table,
                    const SmOut& o, const void* bad_count, const void* ws, int rows, int n_types, int dim, int slices) {
    if (!proj || !types || !type_rowptr || !type_col || !table || !o.count || !o.pivot || !o.s1 || !o.s2 || !o.mean || !o.std ||
        !bad_count || !ws)
        return PC_EINVAL;
    if (rows <= 0 || n_types <= 0) return PC_EINVAL;
    if ((dim != 128 && dim != 256) || slices < 0 || slices > RG_MAX_SLICES) return PC_ESHAPE;
    return PC_OK;
}

// Between an entry's checks and its hot kernel (rg_begin with this family's workspace): the workspace carved and checked, the
// plan launched without targets -- pos[r] = -1 for a row without a type or with a type >= n_types, the latter counted in
// *bad_count --, the hot kernel's grid.
inline int sm_begin(SmWs& w, unsigned& grid, void* ws, size_t ws_bytes, const int32_t* types, int rows,
                    const int32_t* type_rowptr, int n_types, int S, int TM, int32_t* bad_count, hipStream_t st) {
    w = sm_ws_carve(ws, rows, n_types, S);
    if (ws_bytes < w.bytes) return PC_EWORKSPACE;
    grid = rg_item_grid(rows, n_types, S, TM);
    return rg_plan_launch(w.plan, types, nullptr, rows, type_rowptr, n_types, 0, S, TM, nullptr, bad_count, st);
}

// sm_finish_kernel (score_moments.hip), one thread per row, after the hot kernel on the stream: the row's slices added in slice
// order, then count / pivot / s1 / s2 / mean / std; zeros for a row the plan left out and for an empty type.
void sm_finish_launch(const SmWs& w, const int32_t* types, int rows, const int32_t* type_rowptr, int S, const SmOut& o,
                      hipStream_t st);

// One chunk's sums for a lane: its column's scores against the NG x 4 query rows g * 16 + 4 h + k, which the accumulators hold.
// The rows' pivots are read from LDS per row group (one ds_read_b128 of gs), as where_rank.h's count reads them, not held over
// the chain: the two sums per accumulator register then take the registers the rank has for its pivots and its counts.  The
// fence after each row group keeps the scheduler from hoisting all NG reads above the arithmetic.  pid < 0: a column past the
// slice's end, which contributes nothing.
template <int NG>
__device__ __forceinline__ void sm_accum(const f32x4 (&acc)[NG], const float* gs, float (&s1)[NG][4], float (&s2)[NG][4], int pid,
                                         int h) {
    if (pid < 0) return;
#pragma unroll
    for (int g = 0; g < NG; g++) {
        const float4 x = *reinterpret_cast<const float4*>(&gs[g * 16 + 4 * h]);
        const float gv[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const float d = acc[g][k] - gv[k];
            s1[g][k] += d;
            s2[g][k] = __builtin_fmaf(d, d, s2[g][k]);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

// the 16 columns of a (wave, k-lane), a butterfly whose order is fixed -> lane c == 0 -> part[wv][row]
template <int NG, int TM>
__device__ __forceinline__ void sm_reduce(const float (&s)[NG][4], float (*part)[TM], int wv, int c, int h) {
#pragma unroll
    for (int g = 0; g < NG; g++)
#pragma unroll
        for (int k = 0; k < 4; k++) {
            float v = s[g][k];
#pragma unroll
            for (int o = 8; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
            if (c == 0) part[wv][g * 16 + 4 * h + k] = v;
        }
}

// The end of a work item (after the barrier behind sm_reduce): thread tid < valid adds the four waves' sums of tile row tid in
// wave order and stores the (row, slice) partials -- plain vector stores, every (row, slice) of a type with candidates written
// by exactly one thread --, slice 0 the row's pivot too.
template <int TM>
__device__ __forceinline__ void sm_store(const float (*part1)[TM], const float (*part2)[TM], const float* gs, int tid, int valid,
                                         int p0, int s, int S, float* __restrict__ p1, float* __restrict__ p2,
                                         float* __restrict__ pg) {
    if (tid < valid) {
        const size_t at = (size_t)(p0 + tid) * S + s;
        p1[at] = ((part1[0][tid] + part1[1][tid]) + part1[2][tid]) + part1[3][tid];
        p2[at] = ((part2[0][tid] + part2[1][tid]) + part2[2][tid]) + part2[3][tid];
        if (s == 0) pg[p0 + tid] = gs[tid];
    }
}
