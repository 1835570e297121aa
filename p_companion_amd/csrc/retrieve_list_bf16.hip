// Long complement lists from the bf16 copy of the catalogue: the first n <= 256 products of a type per (query, type) row over
// a [P, D] bf16 table (pc_retrieve_list_grouped_bf16; PCompanionInference with an ops.CompactCatalogue, recommend_batch above
// 16).  Two existing units composed, nothing new in either half:
//
//   plan    grouped_plan.hip as it is, with tiles of RL_TM = 16 rows (retrieve_list.hip's)
//   score   retrieve_bf16.hip's chain (rg_score_bf16_kernel): the fp32 query tile is split ONCE per work item by split3 into
//           three bf16 images in LDS ([3][(D / 8) 16] operands of 16 B: 12 KB at D = 128, 24 KB at D = 256; with 16 rows the
//           sixteen lanes c at one k-lane h read sixteen consecutive operands, so there is no padding); candidates in chunks
//           of 64, one 16-candidate column group per wave, lane (c = lane & 15, h = lane >> 4) holds the 8 dimensions
//           32 k + 8 h .. + 7 of candidate c for every k-block k -- D / 32 loads of 16 B, the next chunk's in flight in
//           registers while this one is scored; scores -> LDS
//   select  retrieve_list.hip's selection (rl_score_kernel), RESTATED here -- that kernel's text is left alone, and the two
//           are to be unified behind an A/B of their own: per-row unsorted LDS buffers with the NE = 2 / 4 / 8 capacities
//           (n <= RL_N2 / RL_N4 / RL_MAX_N), the threshold test, the exclusion bisection before the append, rl_sort<NE>
//           compactions when a row could overflow and once at the end of the item, sorted partial lists [rows][S][n]
//   merge   rl_merge_kernel (retrieve_list.hip) through rl_merge_launch
//
// Determinism: the chain of a (row, product) pair is k-block 0 .. D / 32 - 1, inside a k-block the pieces p0, p1, p2, one
// v_mfma_f32_16x16x32_bf16 each into ONE accumulator, inside an MFMA k-lane h and element e cover dimension 32 k + 8 h + e: its
// order depends on the dimension index and the piece alone, so a (row, product) pair has the bits
// pc_retrieve_topk_grouped_bf16 gives it.  The order in which survivors arrive in a buffer is decided by an integer LDS
// atomic and is free: every selection that follows is under the total order (score descending, product index ascending), and
// the threshold only ever drops candidates that n kept products of the row beat.  An excluded product never enters a buffer,
// so it never moves a threshold.  Hence the output does not depend on the slices, the rows' places, the order of type_col or
// the arrival order; for n <= 16 it is pc_retrieve_topk_grouped_bf16's bit for bit.  No float atomics, nothing read back.
#include "common.h"
#include "grouped_select.h"        // the item decode
#include "wave_sort.h"                 // rl_sort: the bitonic network
#include "grouped_list.h"              // the RL_* sizes, rl_merge_launch

// Work item w = (type t, slice s, tile j) (rg_decode).  Lane l of wave wv: column c = l & 15 (candidate wv * 16 + c of the
// chunk, query row c of the A operand), k-lane h = l >> 4; the C/D map of the 16x16x32 bf16 MFMA is the 16x16x4 f32 one's
// (column lane & 15, row 4 (lane >> 4) + reg).  In the selection thread tid serves row rr = tid / 16 with candidates
// qq + 16 k, so the rows 4 wv .. 4 wv + 3 are appended to AND compacted by wave wv.  NE and EX as in rl_score_kernel.
// LDS at NE = 8: 58 KB of buffers, 12 / 24 KB of images, 4 KB of scores.
template <int D, int NE, bool EX>
__global__ __launch_bounds__(256) void rl_score_bf16_kernel(
    const float* __restrict__ proj, const int32_t* __restrict__ type_rowptr, const int32_t* __restrict__ type_col,
    const uint16_t* __restrict__ table, int n_types, int n, int S, const int32_t* __restrict__ cnt,
    const int32_t* __restrict__ row_start, const int64_t* __restrict__ item_start, const int32_t* __restrict__ order,
    float* __restrict__ pv, int32_t* __restrict__ pi, const int32_t* __restrict__ row_key, int rows,
    const int32_t* __restrict__ ex_rowptr, const int32_t* __restrict__ ex_col, int n_keys, int32_t* __restrict__ bad_count) {
    constexpr int TM = RL_TM;
    constexpr int TPR = 256 / TM;            // threads per row in the selection phase
    constexpr int CPT = RG_CHUNK / TPR;      // candidates per thread per chunk
    constexpr int NB = D / 32;               // k-blocks: 16-byte operands per lane per candidate
    constexpr int CAP = NE == 8 ? RL_CAP : 64 * NE;
    constexpr int BS = CAP + 4;              // buffer row stride: a lane's NE slots stay 16-byte aligned
    static_assert(CAP <= 64 * NE && CAP % NE == 0 && TM == 16 && TPR == 16, "buffer within the sort's slots; one MFMA row group");
    // the pieces p0, p1, p2 of the query tile, each as [D / 8][TM] operands of 16 bytes (rg_score_bf16_kernel's layout)
    __shared__ __attribute__((aligned(16))) bf16x8 q[3][(D / 8) * TM];
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
        for (int e = tid; e < TM * (D / 8); e += 256) {
            const int d8 = e / TM, row = e - d8 * TM;     // (row fastest: a wave's 16-byte stores are contiguous)
            float4 x0 = make_float4(0.f, 0.f, 0.f, 0.f), x1 = x0;
            if (row < valid) {
                const float4* f = reinterpret_cast<const float4*>(proj + (size_t)order[p0 + row] * D) + 2 * d8;
                x0 = f[0];
                x1 = f[1];
            }
            const Split3 sp = split3(x0, x1);
            q[0][d8 * TM + row] = sp.p0;
            q[1][d8 * TM + row] = sp.p1;
            q[2][d8 * TM + row] = sp.p2;
        }
        if (tid < TM) { bcnt[tid] = 0; thv[tid] = -INFINITY; thi[tid] = RG_NONE; }
        int elo = 0, ehi = 0;                             // this thread's row's list: ex_col[elo, ehi)
        if (EX && rr < valid) {
            const int key = row_key[order[p0 + rr]];
            if (key >= 0 && key < n_keys) { elo = ex_rowptr[key]; ehi = ex_rowptr[key + 1]; }
        }

        auto load_pid = [&](int cb) { const int cc = cb + wv * 16 + c; return cc < ce ? type_col[cc] : -1; };
        auto load_b = [&](bf16x8* b, int pid) {
            if (pid >= 0) {
                const bf16x8* f = reinterpret_cast<const bf16x8*>(table + (size_t)pid * D) + h;
#pragma unroll
                for (int k = 0; k < NB; k++) b[k] = f[4 * k];
            } else {
#pragma unroll
                for (int k = 0; k < NB; k++) b[k] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
            }
        };
        bf16x8 bn[NB];
        int pidn = load_pid(cb0);
        load_b(bn, pidn);
        int pidnn = load_pid(cb0 + RG_CHUNK);
        __syncthreads();                                  // query images, counters and thresholds in LDS

        for (int cb = cb0;; cb += RG_CHUNK) {
            const bool fin = cb >= ce;                    // past the last chunk: the closing compaction only
            if (!fin) {
                bf16x8 b[NB];
#pragma unroll
                for (int k = 0; k < NB; k++) b[k] = bn[k];
                const int pid = pidn;
                pidn = pidnn;
                if (cb + RG_CHUNK < ce) load_b(bn, pidn); // the next chunk's rows in flight while this one is scored
                pidnn = load_pid(cb + 2 * RG_CHUNK);
                // ---- the score chain: rg_score_bf16_kernel's, one 16-row group
                f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int k = 0; k < NB; k++) {
#pragma unroll
                    for (int p = 0; p < 3; p++)
                        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(q[p][(4 * k + h) * TM + c], b[k], acc, 0, 0, 0);
                }
                // C/D map: column lane & 15 (the candidate), row 4 (lane >> 4) + reg (the query row)
#pragma unroll
                for (int k = 0; k < 4; k++) sc[4 * h + k][wv * 16 + c] = acc[k];
                if (h == 0) cid[wv * 16 + c] = pid < 0 ? RG_NONE : pid;
                __syncthreads();                          // (also: the last compaction's threshold and count are visible)
                // ---- the selection: rl_score_kernel's (retrieve_list.hip), restated
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

namespace {
template <int D, int NE>
void rl_launch_score_bf16(dim3 grid, hipStream_t st, const float* proj, const int32_t* type_rowptr, const int32_t* type_col,
                          const uint16_t* table, int n_types, int n, int S, const RgWs& w, const int32_t* row_key, int rows,
                          const int32_t* ex_rowptr, const int32_t* ex_col, int n_keys, int32_t* bad_count) {
    const RgPlan& pl = w.plan;
    if (row_key)
        PC_LAUNCH((rl_score_bf16_kernel<D, NE, true>), grid, dim3(256), 0, st, proj, type_rowptr, type_col, table, n_types, n, S,
                  pl.cnt, pl.row_start, pl.item_start, pl.order, w.pv, w.pi, row_key, rows, ex_rowptr, ex_col, n_keys, bad_count);
    else
        PC_LAUNCH((rl_score_bf16_kernel<D, NE, false>), grid, dim3(256), 0, st, proj, type_rowptr, type_col, table, n_types, n, S,
                  pl.cnt, pl.row_start, pl.item_start, pl.order, w.pv, w.pi, row_key, rows, ex_rowptr, ex_col, n_keys, bad_count);
}
}  // namespace

extern "C" size_t pc_retrieve_list_grouped_bf16_workspace_bytes(int rows, int n_types, int n, int slices) {
    return rg_topn_workspace_bytes(rows, n_types, n, RL_MAX_N, slices);
}

extern "C" int pc_retrieve_list_grouped_bf16(const float* proj, const int32_t* types, const int32_t* row_key, int rows,
                                             const int32_t* type_rowptr, const int32_t* type_col, const uint16_t* table_bf16,
                                             int n_types, const int32_t* ex_rowptr, const int32_t* ex_col, int n_keys, int n,
                                             int dim, int slices, int32_t* out_idx, float* out_score, int32_t* bad_count,
                                             void* ws, size_t ws_bytes, void* stream) {
    // (pc_retrieve_list_grouped's checks in its order, then the alignment a lane's 16-byte reads of a row need)
    PC_TRY(rg_topn_check(proj && types && type_rowptr && type_col && table_bf16 && out_idx && out_score && ws &&
                             rg_lists_ok(row_key, ex_rowptr, ex_col, bad_count, n_keys),
                         rows, n_types, true, n, RL_MAX_N, dim, slices));
    if ((uintptr_t)table_bf16 & 15) return PC_ESHAPE;
    const int S = rg_slices(slices);
    hipStream_t st = (hipStream_t)stream;
    RgWs w;
    unsigned grid;
    PC_TRY(rg_begin(w, grid, ws, ws_bytes, types, nullptr, rows, type_rowptr, n_types, 0, n, S, RL_TM, nullptr, nullptr, st));
#define RL_SCORE(D, NE) \
    rl_launch_score_bf16<D, NE>(dim3(grid), st, proj, type_rowptr, type_col, table_bf16, n_types, n, S, w, row_key, rows, ex_rowptr, ex_col, n_keys, bad_count)
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
