// Long complement lists: the first n <= 256 products of a type per (query, type) row (PCompanionInference.recommend_batch
// above 16; pc_retrieve_list_grouped).  The contract, the plan, the work items, the chunks and the score chain are
// retrieve.hip's; what differs is the selection.  There every thread keeps a sorted list of 16 in registers; a list of 256
// per thread is out of reach of the register file, and indexed at run time it would live in scratch.  Here a ROW keeps an
// unsorted candidate buffer in LDS and a threshold:
//
//   plan    grouped_plan.hip as it is, with tiles of RL_TM = 16 rows (the buffers take the LDS the wider tile had)
//   score   work item (type, slice, tile): query tile -> LDS, candidates in chunks of 64 (one 16-candidate column group per
//           wave, the next chunk's rows in flight in registers), scores -> LDS.  The 16 threads of a row test 4 candidates
//           each against the row's threshold ((-inf, none) until the row has been compacted once); a survivor is looked up
//           in the row's exclusion list (when there is one) and appended to the row's buffer through an integer LDS counter.
//           A row whose buffer could overflow on the next chunk (more than CAP - 64 entries) is compacted, and every row
//           once more at the end of the item: one wave sorts the buffer under rg_better (a bitonic network over 64 NE
//           slots, slot i = NE lane + e: strides below NE between a lane's own registers, the others between lanes, all
//           register indices static), keeps the first n and sets the threshold to the n-th.  The partial lists
//           [rows][S][n] are written sorted.
//   merge   one wave per row: lane s holds a cursor into slice s's sorted list, n rounds of a wave-wide arg-max of the heads
//
// Determinism: a score is rg_score_kernel's MFMA k-chain (step j, element e, k-lane h cover dimension 16 j + 4 h + e), so a
// (row, product) pair has that kernel's bits.  The order in which survivors arrive in a buffer is decided by an LDS atomic
// and is free: every selection that follows is under the total order (score descending, product index ascending), and the
// threshold only ever drops candidates that n kept products of the row beat.  An excluded product never enters a buffer, so
// it never moves a threshold.  Hence the output does not depend on the slices, the rows' places, the order of type_col, or
// the arrival order; for n <= 16 it is pc_retrieve_topk_grouped[_excluding]'s bit for bit.  No float atomics, no readback.
#include "common.h"
#include "grouped_select.h"        // the item decode
#include "wave_sort.h"                 // rl_sort: the bitonic network (shared with ingest.hip)
#include "grouped_list.h"              // the RL_* sizes, rl_merge_launch (shared with retrieve_list_bf16.hip)

// Work item w = (type t, slice s, tile j) as in rg_score_kernel.  Lane l of wave wv: column c = l & 15 (candidate
// wv * 16 + c of the chunk, query row c of the A operand), k-lane h = l >> 4.  In the selection thread tid serves row
// rr = tid / 16 with candidates qq + 16 k, so the rows 4 wv .. 4 wv + 3 are appended to AND compacted by wave wv.
// NE = 2 / 4 / 8: 128 / 256 / RL_CAP buffer entries per row for n <= RL_N2 / RL_N4 / RL_MAX_N; the slack between n and
// CAP - 64 is what a compacted row can take before it is sorted again.  EX: with exclusion lists.
template <int D, int NE, bool EX>
__global__ __launch_bounds__(256) void rl_score_kernel(const float* __restrict__ proj, const int32_t* __restrict__ type_rowptr,
                                                       const int32_t* __restrict__ type_col, const float* __restrict__ table,
                                                       int n_types, int n, int S, const int32_t* __restrict__ cnt,
                                                       const int32_t* __restrict__ row_start,
                                                       const int64_t* __restrict__ item_start,
                                                       const int32_t* __restrict__ order, float* __restrict__ pv,
                                                       int32_t* __restrict__ pi, const int32_t* __restrict__ row_key, int rows,
                                                       const int32_t* __restrict__ ex_rowptr,
                                                       const int32_t* __restrict__ ex_col, int n_keys,
                                                       int32_t* __restrict__ bad_count) {
    constexpr int TM = RL_TM;
    constexpr int QS = D + 4;                // padded LDS row
    constexpr int TPR = 256 / TM;            // threads per row in the selection phase
    constexpr int CPT = RG_CHUNK / TPR;      // candidates per thread per chunk
    constexpr int NB = D / 16;               // float4 operands per lane per candidate
    constexpr int CAP = NE == 8 ? RL_CAP : 64 * NE;
    constexpr int BS = CAP + 4;              // buffer row stride: a lane's NE slots stay 16-byte aligned
    static_assert(CAP <= 64 * NE && CAP % NE == 0 && TM == 16 && TPR == 16, "buffer within the sort's slots; one MFMA row group");
    __shared__ __attribute__((aligned(16))) float q[TM * QS];
    __shared__ float sc[TM][RG_CHUNK + 1];
    __shared__ int cid[RG_CHUNK];
    __shared__ __attribute__((aligned(16))) float bv[TM][BS];        // the rows' candidate buffers, unsorted between compactions
    __shared__ __attribute__((aligned(16))) int bi[TM][BS];
    __shared__ int bcnt[TM];                 // entries in a row's buffer
    __shared__ float thv[TM];                // the row's threshold: its n-th entry at the last compaction
    __shared__ int thi[TM];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c = lane & 15, h = lane >> 4;
    const int rr = tid / TPR, qq = tid % TPR;
    const int64_t n_items = item_start[n_types];
    if (EX) {
        for (int r = blockIdx.x * 256 + tid; r < rows; r += gridDim.x * 256) {
            const int key = row_key[r];
            if (key < -1 || key >= n_keys) atomicAdd(bad_count, 1);
        }
    }
    for (int64_t w = blockIdx.x; w < n_items; w += gridDim.x) {
        const RgItem it = rg_decode<TM>(w, item_start, cnt, row_start, type_rowptr, n_types, S);
        const int s = it.s, p0 = it.p0, valid = it.valid, cb0 = it.cb0, ce = it.ce;

        __syncthreads();                                  // the previous item's readers of q and of the buffers are done
        for (int e = tid; e < TM * (D / 4); e += 256) {
            const int row = e / (D / 4), d4 = e - row * (D / 4);
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row < valid) x = reinterpret_cast<const float4*>(proj + (size_t)order[p0 + row] * D)[d4];
            *reinterpret_cast<float4*>(&q[row * QS + 4 * d4]) = x;
        }
        if (tid < TM) { bcnt[tid] = 0; thv[tid] = -INFINITY; thi[tid] = RG_NONE; }
        int elo = 0, ehi = 0;                             // this thread's row's list: ex_col[elo, ehi)
        if (EX && rr < valid) {
            const int key = row_key[order[p0 + rr]];
            if (key >= 0 && key < n_keys) { elo = ex_rowptr[key]; ehi = ex_rowptr[key + 1]; }
        }

        auto load_pid = [&](int cb) { const int cc = cb + wv * 16 + c; return cc < ce ? type_col[cc] : -1; };
        auto load_b = [&](float4* b, int pid) {
            if (pid >= 0) {
                const float4* f = reinterpret_cast<const float4*>(table + (size_t)pid * D) + h;
#pragma unroll
                for (int k = 0; k < NB; k++) b[k] = f[4 * k];
            } else {
#pragma unroll
                for (int k = 0; k < NB; k++) b[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        };
        float4 bn[NB];
        int pidn = load_pid(cb0);
        load_b(bn, pidn);
        int pidnn = load_pid(cb0 + RG_CHUNK);
        __syncthreads();                                  // query tile, counters and thresholds in LDS

        for (int cb = cb0;; cb += RG_CHUNK) {
            const bool fin = cb >= ce;                    // past the last chunk: the closing compaction only
            if (!fin) {
                float4 b[NB];
#pragma unroll
                for (int k = 0; k < NB; k++) b[k] = bn[k];
                const int pid = pidn;
                pidn = pidnn;
                if (cb + RG_CHUNK < ce) load_b(bn, pidn); // the next chunk's rows in flight while this one is scored
                pidnn = load_pid(cb + 2 * RG_CHUNK);
                f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int k = 0; k < NB; k++) {
                    const float4 a = *reinterpret_cast<const float4*>(&q[c * QS + 16 * k + 4 * h]);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b[k].x, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b[k].y, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b[k].z, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b[k].w, acc, 0, 0, 0);
                }
                // C/D map of the 16x16 f32 MFMA: column lane & 15 (the candidate), row 4 (lane >> 4) + reg (the query row)
#pragma unroll
                for (int k = 0; k < 4; k++) sc[4 * h + k][wv * 16 + c] = acc[k];
                if (h == 0) cid[wv * 16 + c] = pid < 0 ? RG_NONE : pid;
                __syncthreads();                          // (also: the last compaction's threshold and count are visible)
                if (rr < valid) {
                    const float hv = thv[rr];
                    const int hix = thi[rr];
#pragma unroll
                    for (int k = 0; k < CPT; k++) {
                        const int col = qq + TPR * k;
                        const int xi = cid[col];
                        const float x = sc[rr][col];
                        if (xi == RG_NONE || !rg_better(x, xi, hv, hix)) continue;
                        if (EX) {
                            int a = elo, e = ehi;         // the first list entry >= xi
                            while (a < e) {
                                const int mid = (a + e) >> 1;
                                if (ex_col[mid] < xi) a = mid + 1; else e = mid;
                            }
                            if (a < ehi && ex_col[a] == xi) continue;     // excluded: never buffered, the threshold stays
                        }
                        // at most CAP - 64 entries before the chunk (or the row was compacted to n <= CAP - 64) and at
                        // most 64 candidates of the row in a chunk: slot < CAP
                        const int slot = atomicAdd(&bcnt[rr], 1);
                        bv[rr][slot] = x;
                        bi[rr][slot] = xi;
                    }
                }
                __syncthreads();                          // the chunk's scores are read; the appends are visible
            }
            for (int k = 0; k < TM / 4; k++) {
                const int row = wv * (TM / 4) + k;
                const int cn = __builtin_amdgcn_readfirstlane(bcnt[row]);
                if (fin ? row >= valid : cn <= CAP - RG_CHUNK) continue;          // (wave-uniform)
                float v[NE];
                int ix[NE];
#pragma unroll
                for (int e = 0; e < NE; e++) { v[e] = -INFINITY; ix[e] = RG_NONE; }
                if (NE * lane < cn) {                     // (cn <= CAP, a multiple of NE: the lane's NE slots are inside the row)
#pragma unroll
                    for (int e = 0; e < NE; e++) {
                        const float x = bv[row][NE * lane + e];
                        const int xi = bi[row][NE * lane + e];
                        if (NE * lane + e < cn) { v[e] = x; ix[e] = xi; }
                    }
                }
                rl_sort<NE>(v, ix, lane);
                if (fin) {
                    const size_t o = ((size_t)(p0 + row) * S + s) * n;
#pragma unroll
                    for (int e = 0; e < NE; e++) {
                        const int slot = NE * lane + e;
                        if (slot < n) { pv[o + slot] = v[e]; pi[o + slot] = ix[e]; }
                    }
                } else {
                    float tv = -INFINITY;                 // slot n - 1: the n-th entry ((-inf, none) while the row holds fewer)
                    int ti = RG_NONE;
#pragma unroll
                    for (int e = 0; e < NE; e++) {
                        const int slot = NE * lane + e;
                        if (slot < n && slot < cn) { bv[row][slot] = v[e]; bi[row][slot] = ix[e]; }
                        if (e == (n - 1) % NE) { tv = v[e]; ti = ix[e]; }
                    }
                    tv = __shfl(tv, (n - 1) / NE, 64);
                    ti = __shfl(ti, (n - 1) / NE, 64);
                    if (lane == 0) { bcnt[row] = min(cn, n); thv[row] = tv; thi[row] = ti; }
                }
            }
            if (fin) break;
        }
    }
}

// One wave per row: lane s walks slice s's sorted partial list; every round the best head under rg_better is the next
// entry of the row, and its lane moves on.  Results are gathered 64 at a time and stored as a row of the wave.
__global__ __launch_bounds__(256) void rl_merge_kernel(const int32_t* __restrict__ types, int rows,
                                                       const int32_t* __restrict__ type_rowptr, int n_types, int n, int S,
                                                       const int32_t* __restrict__ rank, const int32_t* __restrict__ row_start,
                                                       const float* __restrict__ pv, const int32_t* __restrict__ pi,
                                                       int32_t* __restrict__ out_idx, float* __restrict__ out_score) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;                                // wave-uniform
    const int t = types[r];
    int ns = 0, L = 0, p = 0;
    if (t >= 0 && t < n_types) {
        rg_slice_plan(type_rowptr[t + 1] - type_rowptr[t], S, ns, L);
        if (ns > 0) p = row_start[t] + rank[r];
    }
    if (ns == 1) {                                        // one slice: its sorted list is the row's
        const size_t one = (size_t)p * S * n;
        for (int k = lane; k < n; k += 64) {
            const int xi = pi[one + k];
            out_idx[(size_t)r * n + k] = xi == RG_NONE ? -1 : xi;
            out_score[(size_t)r * n + k] = xi == RG_NONE ? -INFINITY : pv[one + k];
        }
        return;
    }
    const size_t mine = ((size_t)p * S + lane) * n;       // this lane's list (read only where lane < ns)
    int pos = 0;
    float hv = -INFINITY;
    int hi = RG_NONE;
    if (lane < ns) { hv = pv[mine]; hi = pi[mine]; }
    float rv = -INFINITY;
    int ri = RG_NONE;
    for (int k = 0; k < n; k++) {
        float bv = hv;
        int bi = hi;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (rg_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        if (hi == bi && bi != RG_NONE) {                  // (a product is in one slice: one lane)
            pos++;
            hv = -INFINITY; hi = RG_NONE;
            if (pos < n) { hv = pv[mine + pos]; hi = pi[mine + pos]; }
        }
        if (lane == (k & 63)) { rv = bv; ri = bi; }
        if ((k & 63) == 63 || k == n - 1) {
            const int o = (k & ~63) + lane;
            if (o <= k) {
                out_idx[(size_t)r * n + o] = ri == RG_NONE ? -1 : ri;
                out_score[(size_t)r * n + o] = ri == RG_NONE ? -INFINITY : rv;
            }
        }
    }
}

void rl_merge_launch(const RgWs& w, const int32_t* types, int rows, const int32_t* type_rowptr, int n_types, int n, int S,
                     int32_t* out_idx, float* out_score, hipStream_t st) {
    PC_LAUNCH(rl_merge_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, types, rows, type_rowptr, n_types, n, S, w.plan.pos,
              w.plan.row_start, w.pv, w.pi, out_idx, out_score);
}

namespace {
template <int D, int NE>
void rl_launch_score(dim3 grid, hipStream_t st, const float* proj, const int32_t* type_rowptr, const int32_t* type_col,
                     const float* table, int n_types, int n, int S, const RgWs& w, const int32_t* row_key, int rows,
                     const int32_t* ex_rowptr, const int32_t* ex_col, int n_keys, int32_t* bad_count) {
    const RgPlan& pl = w.plan;
    if (row_key)
        PC_LAUNCH((rl_score_kernel<D, NE, true>), grid, dim3(256), 0, st, proj, type_rowptr, type_col, table, n_types, n, S,
                  pl.cnt, pl.row_start, pl.item_start, pl.order, w.pv, w.pi, row_key, rows, ex_rowptr, ex_col, n_keys, bad_count);
    else
        PC_LAUNCH((rl_score_kernel<D, NE, false>), grid, dim3(256), 0, st, proj, type_rowptr, type_col, table, n_types, n, S,
                  pl.cnt, pl.row_start, pl.item_start, pl.order, w.pv, w.pi, row_key, rows, ex_rowptr, ex_col, n_keys, bad_count);
}
}  // namespace

extern "C" size_t pc_retrieve_list_grouped_workspace_bytes(int rows, int n_types, int n, int slices) {
    return rg_topn_workspace_bytes(rows, n_types, n, RL_MAX_N, slices);
}

extern "C" int pc_retrieve_list_grouped(const float* proj, const int32_t* types, const int32_t* row_key, int rows,
                                        const int32_t* type_rowptr, const int32_t* type_col, const float* table, int n_types,
                                        const int32_t* ex_rowptr, const int32_t* ex_col, int n_keys, int n, int dim, int slices,
                                        int32_t* out_idx, float* out_score, int32_t* bad_count, void* ws, size_t ws_bytes,
                                        void* stream) {
    // (this entry looks at its lists before its counts: a list without keys is a caller's slip)
    PC_TRY(rg_topn_check(proj && types && type_rowptr && type_col && table && out_idx && out_score && ws &&
                             rg_lists_ok(row_key, ex_rowptr, ex_col, bad_count, n_keys),
                         rows, n_types, true, n, RL_MAX_N, dim, slices));
    const int S = rg_slices(slices);
    hipStream_t st = (hipStream_t)stream;
    RgWs w;
    unsigned grid;
    PC_TRY(rg_begin(w, grid, ws, ws_bytes, types, nullptr, rows, type_rowptr, n_types, 0, n, S, RL_TM, nullptr, nullptr, st));
#define RL_SCORE(D, NE) \
    rl_launch_score<D, NE>(dim3(grid), st, proj, type_rowptr, type_col, table, n_types, n, S, w, row_key, rows, ex_rowptr, ex_col, n_keys, bad_count)
    if (dim == 128) {
        if (n <= RL_N2) RL_SCORE(128, 2);
        else if (n <= RL_N4) RL_SCORE(128, 4);
        else RL_SCORE(128, 8);
    } else {
        if (n <= RL_N2) RL_SCORE(256, 2);
        else if (n <= RL_N4) RL_SCORE(256, 4);
        else RL_SCORE(256, 8);
    }
#undef RL_SCORE
    rl_merge_launch(w, types, rows, type_rowptr, n_types, n, S, out_idx, out_score, st);
    return pc_launch_status();
}

