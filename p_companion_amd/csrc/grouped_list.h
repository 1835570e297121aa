// The long-list family's header (retrieve_list.hip: the fp32 table; retrieve_list_bf16.hip: the bf16 copy; nearest_list.hip:
// the fp32 table under a per-product bias; nearest_list_bf16.hip: the bf16 copy under one; where_list.hip and
// where_list_bf16.hip: all four under a per-row predicate on per-product attributes), the way grouped_select.h is the
// 16-entry kernels': the list and buffer sizes, the score kernel's body and the host path, one text each.  A unit supplies its
// score chain (a policy, below), its kernels as one-line wrappers of rl_score_body and its entries.
//
// The kernel.  The contract, the plan, the work items and the chunks are retrieve.hip's; what differs is the selection.  There
// every thread keeps a sorted list of 16 in registers; a list of 256 per thread is out of reach of the register file, and
// indexed at run time it would live in scratch.  Here a ROW keeps an unsorted candidate buffer in LDS and a threshold:
//
//   plan    grouped_plan.hip as it is, with tiles of RL_TM = 16 rows (the buffers take the LDS the wider tile had)
//   score   work item (type, slice, tile): query tile -> LDS (the chain's image), candidates in chunks of 64 (one 16-candidate
//           column group per wave, the next chunk's rows in flight in registers), the chain's scores -> LDS.  The 16 threads of
//           a row test 4 candidates each against the row's threshold ((-inf, none) until the row has been compacted once); a
//           survivor is looked up in the row's exclusion list (when there is one) and appended to the row's buffer through an
//           integer LDS counter.  A row whose buffer could overflow on the next chunk (more than CAP - 64 entries) is
//           compacted, and every row once more at the end of the item: one wave sorts the buffer under rg_better (a bitonic
//           network over 64 NE slots, slot i = NE lane + e: strides below NE between a lane's own registers, the others
//           between lanes, all register indices static), keeps the first n and sets the threshold to the n-th.  The partial
//           lists [rows][S][n] are written sorted.
//   merge   rl_merge_kernel (retrieve_list.hip), one wave per row
#pragma once
#include <type_traits>
#include "grouped_select.h"        // the item decode
#include "wave_sort.h"             // rl_sort: the bitonic network (shared with ingest.hip)

#define RL_MAX_N 256
#define RL_N2 32                   // n up to here: 128 buffer entries per row (NE = 2); a compacted row has 32 entries of slack
#define RL_N4 96                   // n up to here: 256 entries (NE = 4), 96 of slack; above: RL_CAP (NE = 8), 128 at n = 256
#define RL_TM 16                   // rows per tile
#define RL_CAP 448                 // buffer entries per row of the long variant: n + three chunks at n = 256

// rl_merge_kernel (retrieve_list.hip), one wave per row: the first n <= RL_MAX_N of the row's slices' sorted partial lists
// w.pv / w.pi [rows][S][n] -> out_idx / out_score [rows][n] (-1 / -inf past the end of a short list).
void rl_merge_launch(const RgWs& w, const int32_t* types, int rows, const int32_t* type_rowptr, int n_types, int n, int S,
                     int32_t* out_idx, float* out_score, hipStream_t st);

// A score kernel's arguments, the table's element type T apart the same for both tables.
#define RL_SCORE_PARAMS(T)                                                                                                       \
    const float* __restrict__ proj, const int32_t* __restrict__ type_rowptr, const int32_t* __restrict__ type_col,               \
        const T* __restrict__ table, int n_types, int n, int S, const int32_t* __restrict__ cnt,                                 \
        const int32_t* __restrict__ row_start, const int64_t* __restrict__ item_start, const int32_t* __restrict__ order,        \
        float* __restrict__ pv, int32_t* __restrict__ pi, const int32_t* __restrict__ row_key, int rows,                         \
        const int32_t* __restrict__ ex_rowptr, const int32_t* __restrict__ ex_col, int n_keys, int32_t* __restrict__ bad_count
#define RL_SCORE_ARGS                                                                                                            \
    proj, type_rowptr, type_col, table, n_types, n, S, cnt, row_start, item_start, order, pv, pi, row_key, rows, ex_rowptr,      \
        ex_col, n_keys, bad_count

// Work item w = (type t, slice s, tile j) (rg_decode).  Lane l of wave wv: column c = l & 15 (candidate wv * 16 + c of the
// chunk, query row c of the A operand), k-lane h = l >> 4.  In the selection thread tid serves row rr = tid / 16 with
// candidates qq + 16 k, so the rows 4 wv .. 4 wv + 3 are appended to AND compacted by wave wv.
// NE = 2 / 4 / 8: 128 / 256 / RL_CAP buffer entries per row for n <= RL_N2 / RL_N4 / RL_MAX_N; the slack between n and
// CAP - 64 is what a compacted row can take before it is sorted again.  EX: with exclusion lists.
// Chain, the score chain of a table type at width D:
//   Q                                       the query tile's image in LDS (16-byte aligned)
//   load_tile(q, proj, order, p0, valid, tid)   the rows order[p0 .. p0 + valid) of proj -> q, rows past `valid` zero
//   B, NB, zero()                           a lane's operand of 16 bytes and how many a candidate row gives it: operand k
//                                           of lane (c, h) is the row's 16-byte piece h + 4 k; zero() where there is no row
//                                           (written out per type: B{} costs rl_score_kernel<128, 2, EX> a wave per SIMD)
//   score(q, b, c, h)                       the lane's part of the 16 x 16 scores of the tile against the wave's column
//                                           group in the C/D map of the 16-row MFMAs: column lane & 15 (the candidate), row
//                                           4 (lane >> 4) + reg (the query row)
// BIAS: the score is fl(chain + bias[pid]), ONE fp32 addition behind the chain (the accumulator starts at zero, as without):
// bias[pid] is a 4-byte gather per column, issued with the column's product id a chunk ahead (nb_score_kernel's scheme).  A
// column past the slice's end (pid -1) reads bias[0]; nothing of it is used: its id in LDS is RG_NONE.  Without BIAS the
// pointer is not read and the body is the text it was.
// WHERE: a per-row predicate on per-product attributes (RlWhere, below; where_list.hip, where_list_bf16.hip).  The h == 0 lanes
// gather value[pid] and flags[pid] with the column's product id a chunk ahead, as the bias is gathered, and stage them in LDS
// beside cid (wval / wflg, RG_CHUNK words each, the same lanes under the same barrier): 64 gathers a chunk whatever the
// selectivity.  A selection thread holds its row's lo / hi / need / deny in registers for the work item and tests a candidate
// that beat the threshold before the exclusion bisection; a candidate that fails is dropped as an excluded one is: never
// buffered, the threshold stays.  An absent array is a null pointer: the branch on it is wave-uniform, the array is never read,
// and the staged word / the row's bound is the one that passes everything (0 within [-inf, +inf]; need = deny = 0).  A column
// past the slice's end reads entry 0 and nothing of it is used.  The predicate reads no score: the score bits are the body's
// without it.  Without WHERE nothing of this is instantiated and the body is the text it was.
struct RlWhere : pc_row_where {
    // (rl_list_entry's required-pointer test of what travels behind bad_count: the pairing rule of the filter's parts)
    explicit operator bool() const { return (value ? lo && hi : !lo && !hi) && (flags || (!need && !deny)); }
};

template <class Chain, int NE, bool EX, bool BIAS = false, bool WHERE = false>
__device__ __forceinline__ void rl_score_body(RL_SCORE_PARAMS(typename Chain::Table), const float* __restrict__ bias = nullptr,
                                              RlWhere wh = RlWhere{}) {
    using B = typename Chain::B;
    constexpr int D = Chain::D, NB = Chain::NB;
    constexpr int TM = RL_TM;
    constexpr int TPR = 256 / TM;            // threads per row in the selection phase
    constexpr int CPT = RG_CHUNK / TPR;      // candidates per thread per chunk
    constexpr int CAP = NE == 8 ? RL_CAP : 64 * NE;
    constexpr int BS = CAP + 4;              // buffer row stride: a lane's NE slots stay 16-byte aligned
    static_assert(CAP <= 64 * NE && CAP % NE == 0 && TM == 16 && TPR == 16, "buffer within the sort's slots; one MFMA row group");
    static_assert(sizeof(B) == 16 && NB * 64 == D * (int)sizeof(typename Chain::Table), "four k-lanes of NB 16-byte operands are a row");
    __shared__ __attribute__((aligned(16))) typename Chain::Q q;
    __shared__ float sc[TM][RG_CHUNK + 1];
    __shared__ int cid[RG_CHUNK];
    __shared__ __attribute__((aligned(16))) float bv[TM][BS];        // the rows' candidate buffers, unsorted between compactions
    __shared__ __attribute__((aligned(16))) int bi[TM][BS];
    __shared__ int bcnt[TM];                 // entries in a row's buffer
    __shared__ float thv[TM];                // the row's threshold: its n-th entry at the last compaction
    __shared__ int thi[TM];
    float* wval = nullptr;                   // (WHERE) the chunk's columns' value / flags, beside cid
    int* wflg = nullptr;
    if constexpr (WHERE) {
        __shared__ float wval_[RG_CHUNK];
        __shared__ int wflg_[RG_CHUNK];
        wval = wval_;
        wflg = wflg_;
    }
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
        Chain::load_tile(q, proj, order, p0, valid, tid);
        if (tid < TM) { bcnt[tid] = 0; thv[tid] = -INFINITY; thi[tid] = RG_NONE; }
        int elo = 0, ehi = 0;                             // this thread's row's list: ex_col[elo, ehi)
        if (EX && rr < valid) {
            const int key = row_key[order[p0 + rr]];
            if (key >= 0 && key < n_keys) { elo = ex_rowptr[key]; ehi = ex_rowptr[key + 1]; }
        }
        float wlo = -INFINITY, whi = INFINITY;            // (WHERE) this thread's row's predicate
        int wneed = 0, wdeny = 0;
        if constexpr (WHERE) {
            if (rr < valid) {
                const int r = order[p0 + rr];
                if (wh.value) { wlo = wh.lo[r]; whi = wh.hi[r]; }
                if (wh.need) wneed = wh.need[r];
                if (wh.deny) wdeny = wh.deny[r];
            }
        }

        auto load_pid = [&](int cb) { const int cc = cb + wv * 16 + c; return cc < ce ? type_col[cc] : -1; };
        auto load_b = [&](B* b, int pid) {
            if (pid >= 0) {
                const B* f = reinterpret_cast<const B*>(table + (size_t)pid * D) + h;
#pragma unroll
                for (int k = 0; k < NB; k++) b[k] = f[4 * k];
            } else {
#pragma unroll
                for (int k = 0; k < NB; k++) b[k] = Chain::zero();
            }
        };
        B bn[NB];
        int pidn = load_pid(cb0);
        load_b(bn, pidn);
        int pidnn = load_pid(cb0 + RG_CHUNK);
        float bsn = 0.f;                                  // (BIAS) the term of the chunk in bn
        if constexpr (BIAS) bsn = bias[max(pidn, 0)];
        float wvn = 0.f;                                  // (WHERE) the attributes of the chunk in bn, in the h == 0 lanes
        int wfn = 0;
        if constexpr (WHERE) {
            if (h == 0 && wh.value) wvn = wh.value[max(pidn, 0)];
            if (h == 0 && wh.flags) wfn = wh.flags[max(pidn, 0)];
        }
        __syncthreads();                                  // query image, counters and thresholds in LDS

        for (int cb = cb0;; cb += RG_CHUNK) {
            const bool fin = cb >= ce;                    // past the last chunk: the closing compaction only
            if (!fin) {
                B b[NB];
#pragma unroll
                for (int k = 0; k < NB; k++) b[k] = bn[k];
                const int pid = pidn;
                const float bs = bsn;
                const float wvc = wvn;
                const int wfc = wfn;
                pidn = pidnn;
                if (cb + RG_CHUNK < ce) load_b(bn, pidn); // the next chunk's rows in flight while this one is scored
                pidnn = load_pid(cb + 2 * RG_CHUNK);
                f32x4 acc = Chain::score(q, b, c, h);
                if constexpr (BIAS) {
#pragma unroll
                    for (int k = 0; k < 4; k++) acc[k] = acc[k] + bs;     // the one addition: s = fl(d + bias[pid])
                    bsn = bias[max(pidn, 0)];             // the next chunk's term: in flight through this chunk's selection
                }
#pragma unroll
                for (int k = 0; k < 4; k++) sc[4 * h + k][wv * 16 + c] = acc[k];
                if (h == 0) cid[wv * 16 + c] = pid < 0 ? RG_NONE : pid;
                if constexpr (WHERE) {
                    if (h == 0) {
                        wval[wv * 16 + c] = wvc;
                        wflg[wv * 16 + c] = wfc;
                        if (wh.value) wvn = wh.value[max(pidn, 0)];       // the next chunk's: in flight through the selection
                        if (wh.flags) wfn = wh.flags[max(pidn, 0)];
                    }
                }
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
                        if constexpr (WHERE) {            // two fp32 compares (a NaN passes nothing) and two masks
                            const float a = wval[col];
                            const int f = wflg[col];
                            if (!(wlo <= a && a <= whi) || (f & wneed) != wneed || (f & wdeny) != 0) continue;
                        }
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

// The host path of an entry.  K names the unit's kernels: K::kernel<D, NE, EX>() is the score kernel over a table of T.
// The entry looks at its lists before its counts (a list without keys is a caller's slip), then -- the bf16 entry's refusal
// alone -- at the alignment a lane's 16-byte reads of a row need, then plans.  more: what the unit's kernels take behind
// bad_count (the biased unit's bias, the filtered units' RlWhere), required pointers of the entry like the table: each is
// tested as a bool.
template <class K, int D, int NE, class T, class... More>
void rl_launch_score(dim3 grid, hipStream_t st, const float* proj, const int32_t* type_rowptr, const int32_t* type_col,
                     const T* table, int n_types, int n, int S, const RgWs& w, const int32_t* row_key, int rows,
                     const int32_t* ex_rowptr, const int32_t* ex_col, int n_keys, int32_t* bad_count, More... more) {
    const RgPlan& pl = w.plan;
    if (row_key)
        PC_LAUNCH((K::template kernel<D, NE, true>()), grid, dim3(256), 0, st, proj, type_rowptr, type_col, table, n_types, n, S,
                  pl.cnt, pl.row_start, pl.item_start, pl.order, w.pv, w.pi, row_key, rows, ex_rowptr, ex_col, n_keys, bad_count, more...);
    else
        PC_LAUNCH((K::template kernel<D, NE, false>()), grid, dim3(256), 0, st, proj, type_rowptr, type_col, table, n_types, n, S,
                  pl.cnt, pl.row_start, pl.item_start, pl.order, w.pv, w.pi, row_key, rows, ex_rowptr, ex_col, n_keys, bad_count, more...);
}

template <class K, class T, class... More>
int rl_list_entry(const float* proj, const int32_t* types, const int32_t* row_key, int rows, const int32_t* type_rowptr,
                  const int32_t* type_col, const T* table, int n_types, const int32_t* ex_rowptr, const int32_t* ex_col, int n_keys,
                  int n, int dim, int slices, int32_t* out_idx, float* out_score, int32_t* bad_count, void* ws, size_t ws_bytes,
                  void* stream, More... more) {
    PC_TRY(rg_topn_check(proj && types && type_rowptr && type_col && table && (true && ... && more) && out_idx && out_score && ws &&
                             rg_lists_ok(row_key, ex_rowptr, ex_col, bad_count, n_keys),
                         rows, n_types, true, n, RL_MAX_N, dim, slices));
    if (std::is_same<T, uint16_t>::value && ((uintptr_t)table & 15)) return PC_ESHAPE;
    const int S = rg_slices(slices);
    hipStream_t st = (hipStream_t)stream;
    RgWs w;
    unsigned grid;
    PC_TRY(rg_begin(w, grid, ws, ws_bytes, types, nullptr, rows, type_rowptr, n_types, 0, n, S, RL_TM, nullptr, nullptr, st));
#define RL_SCORE(D, NE) \
    rl_launch_score<K, D, NE>(dim3(grid), st, proj, type_rowptr, type_col, table, n_types, n, S, w, row_key, rows, ex_rowptr, ex_col, n_keys, bad_count, more...)
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
