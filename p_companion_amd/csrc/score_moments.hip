// The first two moments of a row's scores over ALL candidates of its type, over the fp32 table (pc_score_moments_grouped;
// ops.score_moments_grouped, PCompanionInference.score_moments and the normalise="zscore" keyword of the serving methods in
// inference.py): for row r with type t = types[r], n = type_rowptr[t + 1] - type_rowptr[t] candidates and pivot
// g = s_{type_col[type_rowptr[t]]},
//   s1 = sum_p fl(s_p - g),   s2 = sum_p fl(s_p - g)^2,   s_p = <proj[r], table[p]>   over the products p of type t,
//   mean = g + s1 / n,   std = sqrt(max(s2 / n - (s1 / n)^2, 0)),
// what a served score is standardised against -- z = (s - mean) / std says how exceptional a product is among everything that
// could have been served for the slot, so that the K lists of a query, whose projections differ in scale, can share a page.
// rank.hip's schedule with two fused multiply-adds where the rank has a compare and an integer add.
//
//   plan     grouped_plan.hip as it is, without targets (tiles of TM = 8192 / D rows): a row without a type, or with a type
//            >= n_types (counted in *bad_count), takes no part
//   moments  sm_moments_kernel: grid-stride over the work items (type, slice, tile): query tile -> LDS; the type's first
//            candidate scored first against the tile (wave w: 16 copies of it as one MFMA column block against row group w, the
//            pivots = its diagonal, exactly as rk_rank_kernel forms its targets' scores); then the slice's candidates in chunks
//            of 64, the next chunk's rows refilling the registers during the chain; per accumulator register d = s - g,
//            s1 += d, s2 = fma(d, d, s2) (sm_accum, score_moments.h); at the end a 16-lane sum, the four waves' sums through LDS,
//            one plain store per (row, slice) and sum into the workspace
//   finish   sm_finish_kernel, one thread per row: the slices added in slice order, the six outputs
//
// Determinism: every s_p and g is rk_chain (rank_chain.h), so a (row, product) score has the bits pc_retrieve_list_grouped and
// pc_rank_grouped give it, and g is the same bits in every slice and every tile.  The sums are fp32 in a fixed order -- a lane's
// chunks in stream order, the 16-lane butterfly, waves 0..3, slices 0..ns-1 -- so a call is bitwise reproducible for a given
// `slices`; another `slices`, or another order of type_col inside a type, moves candidates between lanes and may change the last
// bits (unlike the rank's integer count).  Where every term and partial sum is exactly representable the result is the same for
// every `slices` and order.  No float atomics, no readback.
#include "common.h"
#include "grouped_select.h"        // the item decode, the tile load
#include "rank_chain.h"
#include "score_moments.h"

// One work item's candidate stream for a tile of NG 16-row groups (rk_stream with the sums in the count's place): accumulator
// register k of row group g holds query row g * 16 + 4 h + k; gs: the rows' pivots.  b / pid: the first chunk's rows and
// product ids, pidn: the second chunk's ids (-1: a column past the slice's end; its b is product 0's row and nothing of it is
// added).  Leaves the wave's sums in part1 / part2[wv][row].
template <int D, int NG>
__device__ __forceinline__ void sm_stream(const float* q, const float* gs, float (*part1)[8192 / D], float (*part2)[8192 / D],
                                          const int32_t* __restrict__ type_col, const float* __restrict__ table, int cb0, int ce,
                                          float4 (&b)[D / 16], int pid, int pidn, int wv, int c, int h) {
    float s1[NG][4], s2[NG][4];
#pragma unroll
    for (int g = 0; g < NG; g++)
#pragma unroll
        for (int k = 0; k < 4; k++) s1[g][k] = s2[g][k] = 0.f;
    for (int cb = cb0; cb < ce; cb += RG_CHUNK) {
        const int cc = cb + 2 * RG_CHUNK + wv * 16 + c;
        const int pidnn = cc < ce ? type_col[cc] : -1;
        // the next chunk's rows replace this one's step by step while it is scored
        const float4* next = reinterpret_cast<const float4*>(table + (size_t)max(pidn, 0) * D) + h;
        f32x4 acc[NG];
#pragma unroll
        for (int g = 0; g < NG; g++) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
        rk_chain<D, NG>(q, 0, b, next, acc, c, h);
        sm_accum<NG>(acc, gs, s1, s2, pid, h);
        pid = pidn;
        pidn = pidnn;
    }
    sm_reduce<NG, 8192 / D>(s1, part1, wv, c, h);
    sm_reduce<NG, 8192 / D>(s2, part2, wv, c, h);
}

// Work item w = (type t, slice s, tile j) (rg_decode).  Launch bounds and waves per SIMD as rk_rank_kernel: three at D = 128,
// two at D = 256.
template <int D>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(D == 128 ? 3 : 2))) void sm_moments_kernel(
    const float* __restrict__ proj, const int32_t* __restrict__ types, const int32_t* __restrict__ type_rowptr,
    const int32_t* __restrict__ type_col, const float* __restrict__ table, int n_types, int S, const int32_t* __restrict__ cnt,
    const int32_t* __restrict__ row_start, const int64_t* __restrict__ item_start, const int32_t* __restrict__ order,
    float* __restrict__ p1, float* __restrict__ p2, float* __restrict__ pg) {
    constexpr int TM = 8192 / D;             // rows per tile: 64 (D = 128) or 32 (D = 256): a 32 KB query tile
    constexpr int RG = TM / 16;              // 16-row groups (at most one per wave)
    constexpr int QS = RK_QS(D);             // padded LDS row
    constexpr int NB = D / 16;               // float4 operands per lane per candidate
    __shared__ __attribute__((aligned(16))) float q[TM * QS];
    __shared__ __attribute__((aligned(16))) float gs[TM];            // the rows' pivots
    __shared__ float part1[4][TM], part2[4][TM];                     // the waves' sums
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c = lane & 15, h = lane >> 4;
    const int64_t n_items = item_start[n_types];
    for (int64_t w = blockIdx.x; w < n_items; w += gridDim.x) {
        const RgItem it = rg_decode<TM>(w, item_start, cnt, row_start, type_rowptr, n_types, S);
        const int p0 = it.p0, valid = it.valid, rg = it.rg, cb0 = it.cb0, ce = it.ce;

        __syncthreads();                                  // the previous item's readers of q / gs / part are done
        rg_load_tile<D, QS>(q, proj, order, p0, valid, rg, tid);

        auto load_pid = [&](int cb) { const int cc = cb + wv * 16 + c; return cc < ce ? type_col[cc] : -1; };
        // (a lane without a product reads product 0's row: no branch, and nothing of it is used)
        auto load_b = [&](float4* b, int pid) {
            const float4* f = reinterpret_cast<const float4*>(table + (size_t)max(pid, 0) * D) + h;
#pragma unroll
            for (int k = 0; k < NB; k++) b[k] = f[4 * k];
        };
        float4 b[NB];
        const int pid = load_pid(cb0);
        load_b(b, pid);
        const int pidn = load_pid(cb0 + RG_CHUNK);
        // the type's first candidate (an item exists only for a type with candidates and rows): every column of the block
        const int ty = type_col[type_rowptr[types[order[p0]]]];
        __syncthreads();                                  // query tile in LDS
        if (wv < rg) {                                    // (wave-uniform)
            float4 bt[NB];
            load_b(bt, ty);
            f32x4 ag[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};
            rk_chain<D, 1>(q, wv, bt, nullptr, ag, c, h);
            const f32x4 acc = ag[0];
            // C/D map of the 16x16 f32 MFMA: column lane & 15, row 4 (lane >> 4) + reg; the diagonal: row == column
            if ((c >> 2) == h) {
                const int k = c & 3;
                gs[wv * 16 + c] = k == 0 ? acc[0] : k == 1 ? acc[1] : k == 2 ? acc[2] : acc[3];
            }
        }
        __syncthreads();                                  // gs in LDS
        // the slice's candidates against the tile's NG row groups: straight-line code per NG
        if (rg == 1) sm_stream<D, 1>(q, gs, part1, part2, type_col, table, cb0, ce, b, pid, pidn, wv, c, h);
        else if (rg == 2) sm_stream<D, 2>(q, gs, part1, part2, type_col, table, cb0, ce, b, pid, pidn, wv, c, h);
        else if constexpr (RG == 4) {
            if (rg == 3) sm_stream<D, 3>(q, gs, part1, part2, type_col, table, cb0, ce, b, pid, pidn, wv, c, h);
            else sm_stream<D, 4>(q, gs, part1, part2, type_col, table, cb0, ce, b, pid, pidn, wv, c, h);
        }
        __syncthreads();
        sm_store<TM>(part1, part2, gs, tid, valid, p0, it.s, S, p1, p2, pg);
    }
}

// One thread per row, after the hot kernel on the stream.  A row the plan left out (pos < 0) and a row of an empty type: count
// 0 and zeros.  Otherwise the row's ns slices (rg_slice_plan: the hot kernel's own arithmetic) in slice order, and
//   mean = g + S1 / n,   std = sqrt(max(S2 / n - (S1 / n)^2, 0)):
// one IEEE rounding per operation in that order: the division and sqrtf are the correctly rounded ones (this build's default;
// the __f*_rn intrinsics are plain operators here and __fsqrt_rn the approximate root), and the pragma in the body keeps
// s2 / n - m1 * m1 from being contracted into a fused multiply-add.
__global__ __launch_bounds__(256) void sm_finish_kernel(const int32_t* __restrict__ types, int rows,
                                                        const int32_t* __restrict__ type_rowptr, int S,
                                                        const int32_t* __restrict__ pos, const int32_t* __restrict__ row_start,
                                                        const float* __restrict__ p1, const float* __restrict__ p2,
                                                        const float* __restrict__ pg, SmOut o) {
#pragma clang fp contract(off)
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    int n = 0;
    float g = 0.f, s1 = 0.f, s2 = 0.f, mean = 0.f, sd = 0.f;
    const int p = pos[r];
    if (p >= 0) {                                         // (then types[r] is inside [0, n_types))
        const int t = types[r];
        int ns, L;
        rg_slice_plan(type_rowptr[t + 1] - type_rowptr[t], S, ns, L);
        if (ns > 0) {
            n = type_rowptr[t + 1] - type_rowptr[t];
            const size_t at = (size_t)(row_start[t] + p);
            g = pg[at];
            for (int s = 0; s < ns; s++) {
                s1 += p1[at * S + s];
                s2 += p2[at * S + s];
            }
            const float fn = (float)n, m1 = s1 / fn, sq = m1 * m1;
            mean = g + m1;
            sd = sqrtf(fmaxf(s2 / fn - sq, 0.f));
        }
    }
    o.count[r] = n;
    o.pivot[r] = g;
    o.s1[r] = s1;
    o.s2[r] = s2;
    o.mean[r] = mean;
    o.std[r] = sd;
}

void sm_finish_launch(const SmWs& w, const int32_t* types, int rows, const int32_t* type_rowptr, int S, const SmOut& o,
                      hipStream_t st) {
    PC_LAUNCH(sm_finish_kernel, dim3((rows + 255) / 256), dim3(256), 0, st, types, rows, type_rowptr, S, w.plan.pos,
              w.plan.row_start, w.p1, w.p2, w.pg, o);
}

extern "C" size_t pc_score_moments_grouped_workspace_bytes(int rows, int n_types, int slices) {
    if (rows <= 0 || n_types <= 0 || slices < 0 || slices > RG_MAX_SLICES) return 0;
    return sm_ws_carve(nullptr, rows, n_types, rg_slices(slices)).bytes;
}

extern "C" int pc_score_moments_grouped(const float* proj, const int32_t* types, int rows, const int32_t* type_rowptr,
                                        const int32_t* type_col, const float* table, int n_types, int dim, int slices,
                                        int32_t* count, float* pivot, float* s1, float* s2, float* mean, float* std_out,
                                        int32_t* bad_count, void* ws, size_t ws_bytes, void* stream) {
    const SmOut o{count, pivot, s1, s2, mean, std_out};
    PC_TRY(sm_check(proj, types, type_rowptr, type_col, table, o, bad_count, ws, rows, n_types, dim, slices));
    const int S = rg_slices(slices);
    hipStream_t st = (hipStream_t)stream;
    SmWs w;
    unsigned grid;
    PC_TRY(sm_begin(w, grid, ws, ws_bytes, types, rows, type_rowptr, n_types, S, 8192 / dim, bad_count, st));
    const RgPlan& pl = w.plan;
    if (dim == 128)
        PC_LAUNCH(sm_moments_kernel<128>, dim3(grid), dim3(256), 0, st, proj, types, type_rowptr, type_col, table, n_types, S,
                  pl.cnt, pl.row_start, pl.item_start, pl.order, w.p1, w.p2, w.pg);
    else
        PC_LAUNCH(sm_moments_kernel<256>, dim3(grid), dim3(256), 0, st, proj, types, type_rowptr, type_col, table, n_types, S,
                  pl.cnt, pl.row_start, pl.item_start, pl.order, w.p1, w.p2, w.pg);
    sm_finish_launch(w, types, rows, type_rowptr, S, o, st);
    return pc_launch_status();
}
