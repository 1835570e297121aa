// A device-resident BPG from behaviour edge lists (BehaviorProductGraph, src/data/bpg.py: the edge sets co_view,
// purchase_after_view and co_purchase) -- the ingestion counterpart of generator.hip.  Three unsorted, directed [E,2] int32
// lists with duplicates go in; the arrays of ops.generate_catalogue come out.  No global sort: an edge list is bucketed by
// source, and every row is then sorted on its own.
//
//   count     one thread per edge: ids checked against [0, P) BEFORE they index anything (an offender sets the list's bit in a
//             flag word and is skipped, here and in the scatter, so nothing downstream sees it), self-loops dropped,
//             cnt[source] += 1
//   scan      pc_exclusive_scan_i32 -> the raw row offsets
//   scatter   the target goes to its source's bucket through the row's integer cursor (arrival order arbitrary)
//   rows      per row: sort the bucket by id, run-length it into (id, weight = occurrences), and -- co_view only -- keep the
//             `cap` ids of greatest weight, equal weights the lower id.  The row stays IN its bucket as its distinct ids
//             ascending, bit 31 set on the kept ones (the full set answers "is this edge co-viewed", the kept ones are the
//             neighbour list).  Three row classes by RAW length n:
//               n <= ING_WAVE_ROW_MAX   one wave per row, wave_sort.h's bitonic network in registers
//               n <= ING_LDS_ROW_MAX    one workgroup per row, block_ops.h's LSD radix sort (8-bit digits) between two LDS buffers
//               longer                  one workgroup per row, the same radix sort between the bucket and a scratch buffer
//             The selection needs no second sort: the threshold weight w* (largest w with at least cap ids of weight >= w)
//             is bisected by counting, ids above it are kept, and of the ids AT it the first cap - #above in id order.
//   flag      set algebra, one wave per row: an entry is flagged when it is in the `need` set and in neither `forbid` set
//             (membership: bisection in the sorted row); the row's count of flagged entries is written
//   emit      after a scan of the counts: the flagged entries of every row in order -> CSR column / (s, t) pairs / pair degree
//
// Integer atomics only (counters, cursors, the flag word, a maximum), and they decide arrival order or nothing: every array
// written is a function of the lists as SETS (co_view: as a multiset), so a permuted input gives identical bits.
#include "block_ops.h"             // block_rank, block_sum and the radix pass
#include "wave_sort.h"

#define ING_WAVE_ROW_MAX 128
#define ING_LDS_ROW_MAX 4096
#define ING_CAP_MAX 64                 // generator.hip's GEN_CAP_MAX: the bound the device loaders are tested under
#define ING_FLAG 0x80000000u
#define ING_ID 0x7fffffffu
#define ING_LIST_GRID 2048             // workgroups that walk the list of long rows
#define ING_ROW_GRID (1u << 22)        // workgroups of the row-per-wave launches at most (they stride over the rows)

// ---- bucketing ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool ing_edge(const int32_t* __restrict__ edges, uint32_t e, uint32_t P, int list_bit, int32_t* bad,
                                         int& s, int& t) {
    const int2 st = reinterpret_cast<const int2*>(edges)[e];
    s = st.x; t = st.y;
    if ((uint32_t)s >= P || (uint32_t)t >= P) {
        if (bad) atomicOr(bad, list_bit);
        return false;
    }
    return s != t;
}

__global__ __launch_bounds__(256) void ing_count_kernel(const int32_t* __restrict__ edges, uint32_t E, uint32_t P, int list_bit,
                                                        int32_t* cnt, int32_t* bad) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    int s, t;
    if (e < E && ing_edge(edges, e, P, list_bit, bad, s, t)) atomicAdd(&cnt[s], 1);
}

// cursor[s] holds the row's count on entry and 0 on exit
__global__ __launch_bounds__(256) void ing_scatter_kernel(const int32_t* __restrict__ edges, uint32_t E, uint32_t P,
                                                          const int32_t* __restrict__ rowptr, int32_t* cursor, int32_t* bucket) {
    const uint32_t e = blockIdx.x * 256u + threadIdx.x;
    int s, t;
    if (e >= E || !ing_edge(edges, e, P, 0, nullptr, s, t)) return;
    const int lo = rowptr[s], n = rowptr[s + 1] - lo;
    const int k = atomicSub(&cursor[s], 1) - 1;
    if ((uint32_t)k < (uint32_t)n) bucket[(size_t)lo + k] = t;    // (always, when cursor is the count pass's output)
}

__global__ __launch_bounds__(256) void ing_classify_kernel(uint32_t P, const int32_t* __restrict__ rowptr, int32_t* list,
                                                           int32_t* nlist) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < P && rowptr[i + 1] - rowptr[i] > ING_WAVE_ROW_MAX) list[atomicAdd(nlist, 1)] = (int32_t)i;
}

// ---- the per-row pass -----------------------------------------------------------------------------------------------
// One stable pass of the LSD radix sort over the 8-bit digit at `shift`: src[0, n) -> dst[0, n) (block_ops.h: the digit
// histogram, the digit offsets, the tile scatter).  base: 256 LDS ints, wcnt: 4 x 256 LDS ints.
__device__ __forceinline__ void ing_radix_pass(const int32_t* src, int32_t* dst, int n, int shift, int* base, int* wcnt) {
    radix_hist<256>(src, 0, n, shift, base);
    const int ex = radix_digit_offset(base, threadIdx.x);
    __syncthreads();
    base[threadIdx.x] = ex;
    radix_scatter<256, false>(src, nullptr, dst, nullptr, 0, n, n, shift, base, wcnt);
}

// s[0, n): the row's raw targets sorted ascending; y[0, n): scratch.  Writes the row's D distinct ids ascending to dst[0, D)
// (dst may be s), bit 31 on the kept ones when cap > 0 (cap = 0: a plain set, no bits), D to full_cnt[row] and, when cap > 0,
// min(D, cap) to kept_cnt[row] and into the maximum *max_kept.  Every thread of the NT-thread workgroup calls it.
template <int NT>
__device__ __forceinline__ void ing_finish_row(int32_t* s, int32_t* y, int n, int cap, int32_t* dst, uint32_t row,
                                               int32_t* full_cnt, int32_t* kept_cnt, int32_t* max_kept, int* wsum) {
    const int tid = threadIdx.x;
    // run-length: distinct id p -> s[p], the index of its first occurrence -> y[p] (p <= index: s[i - 1] of a later tile is
    // either untouched or rewritten with its own value)
    int D = 0;
    for (int b0 = 0; b0 < n; b0 += NT) {
        const int i = b0 + tid;
        int v = 0;
        bool head = false;
        if (i < n) { v = s[i]; head = i == 0 || s[i - 1] != v; }
        __syncthreads();
        int tot;
        const int r = block_rank<NT>(head, wsum, tot);
        if (head) { s[D + r] = v; y[D + r] = i; }
        D += tot;
        __syncthreads();
    }
    // weight of distinct id p: y[p + 1] - y[p] (y[D] = n)
    int wstar = 0, at = 0;                                    // keep weight > wstar, and the first `at` ids of weight == wstar
    if (cap > 0 && D > cap) {
        int lo = 1, hi = n - D + 1;                           // count(weight >= lo) >= cap
        while (lo < hi) {
            const int mid = lo + (hi - lo + 1) / 2;
            int c = 0;
            for (int p = tid; p < D; p += NT) c += ((p + 1 < D ? y[p + 1] : n) - y[p]) >= mid ? 1 : 0;
            c = block_sum<NT>(c, wsum);
            if (c >= cap) lo = mid; else hi = mid - 1;
        }
        wstar = lo;
        int c = 0;
        for (int p = tid; p < D; p += NT) c += ((p + 1 < D ? y[p + 1] : n) - y[p]) > wstar ? 1 : 0;
        at = cap - block_sum<NT>(c, wsum);
    }
    int ties = 0;
    for (int b0 = 0; b0 < D; b0 += NT) {
        const int p = b0 + tid;
        int id = 0;
        bool keep = false, tie = false;
        if (p < D) {
            const int wgt = (p + 1 < D ? y[p + 1] : n) - y[p];
            id = s[p];
            keep = wgt > wstar;
            tie = wgt == wstar;
        }
        int tot;
        const int r = block_rank<NT>(tie, wsum, tot);
        if (p < D) {
            keep = keep || (tie && ties + r < at);
            dst[p] = (int32_t)((uint32_t)id | (cap > 0 && keep ? ING_FLAG : 0u));
        }
        ties += tot;
    }
    if (tid == 0) {
        full_cnt[row] = D;
        if (cap > 0) {
            const int k = D < cap ? D : cap;
            kept_cnt[row] = k;
            atomicMax(max_kept, k);
        }
    }
}

// rows of raw length <= ING_WAVE_ROW_MAX: one wave (= one workgroup) per row, slot i = 2 lane + e of the bitonic network
__global__ __launch_bounds__(64) void ing_rows_wave_kernel(uint32_t P, const int32_t* __restrict__ rowptr, int32_t* bucket, int cap,
                                                           int32_t* full_cnt, int32_t* kept_cnt, int32_t* max_kept) {
    __shared__ int32_t sh[2 * ING_WAVE_ROW_MAX + 1];
    const int lane = threadIdx.x;
    for (uint32_t row = blockIdx.x; row < P; row += gridDim.x) {
        const int lo = rowptr[row], n = rowptr[row + 1] - lo;
        if (n > ING_WAVE_ROW_MAX) continue;
        if (n <= 0) {
            if (lane == 0) { full_cnt[row] = 0; if (cap > 0) kept_cnt[row] = 0; }
            continue;
        }
        float v[2];
        int ix[2];
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const int i = 2 * lane + e;
            const bool real = i < n;
            v[e] = real ? 0.0f : -INFINITY;
            ix[e] = real ? bucket[(size_t)lo + i] : RG_NONE;
        }
        rl_sort<2>(v, ix, lane);
        sh[2 * lane] = ix[0];
        sh[2 * lane + 1] = ix[1];
        __syncthreads();
        ing_finish_row<64>(sh, sh + ING_WAVE_ROW_MAX, n, cap, bucket + (size_t)lo, row, full_cnt, kept_cnt, max_kept,
                           sh + 2 * ING_WAVE_ROW_MAX);
        __syncthreads();
    }
}

// the listed rows (raw length > ING_WAVE_ROW_MAX), one workgroup per row at a time.  IN_LDS: those up to ING_LDS_ROW_MAX,
// sorted between two LDS buffers; otherwise the longer ones, sorted between the bucket and scratch[lo, lo + n).  passes is
// even, so the sorted row ends where it started.
template <bool IN_LDS>
__global__ __launch_bounds__(256) void ing_rows_block_kernel(const int32_t* __restrict__ list, const int32_t* __restrict__ nlist,
                                                             const int32_t* __restrict__ rowptr, int32_t* bucket, int32_t* scratch,
                                                             int passes, int cap, int32_t* full_cnt, int32_t* kept_cnt,
                                                             int32_t* max_kept) {
    __shared__ int32_t sh[(IN_LDS ? 2 * ING_LDS_ROW_MAX : 0) + 256 + 4 * 256 + 4];
    int32_t* const base = sh + (IN_LDS ? 2 * ING_LDS_ROW_MAX : 0);
    int32_t* const wcnt = base + 256;
    int32_t* const wsum = wcnt + 4 * 256;
    const int nl = *nlist;
    for (int k = blockIdx.x; k < nl; k += gridDim.x) {
        const uint32_t row = (uint32_t)list[k];
        const int lo = rowptr[row], n = rowptr[row + 1] - lo;
        if ((n <= ING_LDS_ROW_MAX) != IN_LDS) continue;
        int32_t* a = IN_LDS ? sh : bucket + (size_t)lo;
        int32_t* b = IN_LDS ? sh + ING_LDS_ROW_MAX : scratch + (size_t)lo;
        if (IN_LDS) for (int i = threadIdx.x; i < n; i += 256) a[i] = bucket[(size_t)lo + i];
        __syncthreads();
        for (int p = 0; p < passes; p += 2) {
            ing_radix_pass(a, b, n, 8 * p, base, wcnt);
            __syncthreads();
            ing_radix_pass(b, a, n, 8 * p + 8, base, wcnt);
            __syncthreads();
        }
        ing_finish_row<256>(a, b, n, cap, bucket + (size_t)lo, row, full_cnt, kept_cnt, max_kept, wsum);
        __syncthreads();
    }
}

// ---- set algebra ----------------------------------------------------------------------------------------------------
// Row r of a set: buf[rowptr[r], rowptr[r] + cnt[r]) (cnt NULL: the whole CSR row), ids ascending, bit 31 ignored.
struct IngSet { const int32_t* buf; const int32_t* rowptr; const int32_t* cnt; };

__device__ __forceinline__ bool ing_member(const IngSet& a, uint32_t row, int t) {
    const int first = a.rowptr[row];
    const int n = a.cnt ? a.cnt[row] : a.rowptr[row + 1] - first;
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if ((int)((uint32_t)a.buf[(size_t)first + mid] & ING_ID) < t) lo = mid + 1; else hi = mid;
    }
    return lo < n && (int)((uint32_t)a.buf[(size_t)first + lo] & ING_ID) == t;
}

// one wave per source row: bit 31 of src's entry (r, t) := t in need (when given) and in neither forbid set; count[r] = their number
__global__ __launch_bounds__(256) void ing_flag_kernel(uint32_t P, int32_t* src, const int32_t* __restrict__ src_rowptr,
                                                       const int32_t* __restrict__ src_cnt, IngSet need, IngSet f1, IngSet f2,
                                                       int32_t* count) {
    const int lane = threadIdx.x & 63;
    for (uint64_t r64 = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); r64 < P; r64 += (uint64_t)gridDim.x * 4u) {
        const uint32_t row = (uint32_t)r64;
        const int first = src_rowptr[row];
        const int n = src_cnt ? src_cnt[row] : src_rowptr[row + 1] - first;
        int c = 0;
        for (int b0 = 0; b0 < n; b0 += 64) {
            const int i = b0 + lane;
            bool ok = false;
            if (i < n) {
                const int t = (int)((uint32_t)src[(size_t)first + i] & ING_ID);
                ok = !need.buf || ing_member(need, row, t);
                if (ok && f1.buf) ok = !ing_member(f1, row, t);
                if (ok && f2.buf) ok = !ing_member(f2, row, t);
                src[(size_t)first + i] = (int32_t)((uint32_t)t | (ok ? ING_FLAG : 0u));
            }
            c += __popcll(__ballot(ok));
        }
        if (lane == 0) count[row] = c;
    }
}

// one wave per source row: its flagged entries, in order, to position out_rowptr[r] onwards of out_col (ids), out_pairs ((r, id))
// and out_deg (deg_rowptr[r + 1] - deg_rowptr[r]); clear: the flags are removed from src on the way
__global__ __launch_bounds__(256) void ing_emit_kernel(uint32_t P, int32_t* src, const int32_t* __restrict__ src_rowptr,
                                                       const int32_t* __restrict__ src_cnt, const int32_t* __restrict__ out_rowptr,
                                                       int32_t* out_col, int32_t* out_pairs, int32_t* out_deg,
                                                       const int32_t* __restrict__ deg_rowptr, int clear) {
    const int lane = threadIdx.x & 63;
    for (uint64_t r64 = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6); r64 < P; r64 += (uint64_t)gridDim.x * 4u) {
        const uint32_t row = (uint32_t)r64;
        const int first = src_rowptr[row];
        const int n = src_cnt ? src_cnt[row] : src_rowptr[row + 1] - first;
        int o = out_rowptr[row];
        const int room = out_rowptr[row + 1];
        const int deg = out_deg ? deg_rowptr[row + 1] - deg_rowptr[row] : 0;
        for (int b0 = 0; b0 < n; b0 += 64) {
            const int i = b0 + lane;
            const uint32_t v = i < n ? (uint32_t)src[(size_t)first + i] : 0u;
            const bool f = (v & ING_FLAG) != 0;
            const unsigned long long m = __ballot(f);
            const int k = o + __popcll(m & ((1ull << lane) - 1ull));
            if (f && k < room) {                              // (k < room always, when out_rowptr scans this row's flag counts)
                const int32_t t = (int32_t)(v & ING_ID);
                if (out_col) out_col[k] = t;
                if (out_pairs) { out_pairs[2 * (size_t)k] = (int32_t)row; out_pairs[2 * (size_t)k + 1] = t; }
                if (out_deg) out_deg[k] = deg;
            }
            if (clear && f) src[(size_t)first + i] = (int32_t)(v & ING_ID);
            o += __popcll(m);
        }
    }
}

// ---- entries --------------------------------------------------------------------------------------------------------
static inline bool ing_sizes_ok(int64_t n_products, int64_t n_edges) {
    return n_products > 0 && n_products < (1ll << 31) && n_edges >= 0 && n_edges < (1ll << 31);
}

extern "C" int pc_ingest_row_limits(int* wave_row_max, int* lds_row_max) {
    if (!wave_row_max || !lds_row_max) return PC_EINVAL;
    *wave_row_max = ING_WAVE_ROW_MAX;
    *lds_row_max = ING_LDS_ROW_MAX;
    return 0;
}

extern "C" int pc_ingest_count(const int32_t* edges, int64_t n_edges, int64_t n_products, int list_bit, int32_t* cnt,
                               int32_t* bad, void* stream) {
    if (!ing_sizes_ok(n_products, n_edges) || !cnt || !bad || (n_edges > 0 && !edges) || list_bit <= 0) return PC_EINVAL;
    if (n_edges == 0) return 0;
    PC_LAUNCH(ing_count_kernel, dim3((unsigned)((n_edges + 255) / 256)), dim3(256), 0, (hipStream_t)stream, edges, (uint32_t)n_edges,
              (uint32_t)n_products, list_bit, cnt, bad);
    return pc_launch_status();
}

extern "C" int pc_ingest_scatter(const int32_t* edges, int64_t n_edges, int64_t n_products, const int32_t* rowptr,
                                 int32_t* cursor, int32_t* bucket, void* stream) {
    if (!ing_sizes_ok(n_products, n_edges) || !rowptr || !cursor || !bucket || (n_edges > 0 && !edges)) return PC_EINVAL;
    if (n_edges == 0) return 0;
    PC_LAUNCH(ing_scatter_kernel, dim3((unsigned)((n_edges + 255) / 256)), dim3(256), 0, (hipStream_t)stream, edges,
              (uint32_t)n_edges, (uint32_t)n_products, rowptr, cursor, bucket);
    return pc_launch_status();
}

extern "C" size_t pc_ingest_rows_workspace_bytes(int64_t n_products) {
    if (n_products <= 0 || n_products >= (1ll << 31)) return 0;
    return (size_t)(n_products + 64) * sizeof(int32_t);      // the counter (one 256-B line) and the list of long rows
}

extern "C" int pc_ingest_rows(int64_t n_products, const int32_t* rowptr, int32_t* bucket, int32_t* scratch, int degree_cap,
                              int32_t* full_cnt, int32_t* kept_cnt, int32_t* max_kept, void* ws, size_t ws_bytes,
                              void* stream) {
    if (n_products <= 0 || n_products >= (1ll << 31) || !rowptr || !bucket || !scratch || !full_cnt || !ws) return PC_EINVAL;
    if (degree_cap < 0 || degree_cap > ING_CAP_MAX) return PC_ESHAPE;
    if (degree_cap > 0 && (!kept_cnt || !max_kept)) return PC_EINVAL;
    if (ws_bytes < pc_ingest_rows_workspace_bytes(n_products)) return PC_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    int32_t* nlist = (int32_t*)ws;
    int32_t* list = nlist + 64;
    const uint32_t P = (uint32_t)n_products;
    const int passes = n_products <= 65536 ? 2 : 4;          // 8-bit digits covering ids below P
    PC_HIP_TRY(hipMemsetAsync(nlist, 0, sizeof(int32_t), st));
    PC_LAUNCH(ing_classify_kernel, dim3((P + 255u) / 256u), dim3(256), 0, st, P, rowptr, list, nlist);
    PC_LAUNCH(ing_rows_wave_kernel, dim3(P < ING_ROW_GRID ? P : ING_ROW_GRID), dim3(64), 0, st, P, rowptr, bucket, degree_cap, full_cnt, kept_cnt, max_kept);
    const unsigned grid = P < ING_LIST_GRID ? P : ING_LIST_GRID;
    PC_LAUNCH((ing_rows_block_kernel<true>), dim3(grid), dim3(256), 0, st, list, nlist, rowptr, bucket, scratch, passes, degree_cap,
              full_cnt, kept_cnt, max_kept);
    PC_LAUNCH((ing_rows_block_kernel<false>), dim3(grid), dim3(256), 0, st, list, nlist, rowptr, bucket, scratch, passes, degree_cap,
              full_cnt, kept_cnt, max_kept);
    return pc_launch_status();
}

static inline unsigned ing_wave_grid(uint32_t P) {         // four rows (waves) per workgroup
    const uint32_t g = (P + 3u) / 4u;
    return g < ING_ROW_GRID ? g : ING_ROW_GRID;
}
static inline bool ing_set_ok(const int32_t* buf, const int32_t* rowptr) { return !buf || rowptr; }

extern "C" int pc_ingest_flag(int64_t n_products, int32_t* src, const int32_t* src_rowptr, const int32_t* src_cnt,
                              const int32_t* need, const int32_t* need_rowptr, const int32_t* need_cnt,
                              const int32_t* forbid1, const int32_t* forbid1_rowptr, const int32_t* forbid1_cnt,
                              const int32_t* forbid2, const int32_t* forbid2_rowptr, const int32_t* forbid2_cnt,
                              int32_t* count, void* stream) {
    if (n_products <= 0 || n_products >= (1ll << 31) || !src || !src_rowptr || !count) return PC_EINVAL;
    if (!ing_set_ok(need, need_rowptr) || !ing_set_ok(forbid1, forbid1_rowptr) || !ing_set_ok(forbid2, forbid2_rowptr))
        return PC_EINVAL;
    const uint32_t P = (uint32_t)n_products;
    PC_LAUNCH(ing_flag_kernel, dim3(ing_wave_grid(P)), dim3(256), 0, (hipStream_t)stream, P, src, src_rowptr, src_cnt,
              IngSet{need, need_rowptr, need_cnt}, IngSet{forbid1, forbid1_rowptr, forbid1_cnt},
              IngSet{forbid2, forbid2_rowptr, forbid2_cnt}, count);
    return pc_launch_status();
}

extern "C" int pc_ingest_emit(int64_t n_products, int32_t* src, const int32_t* src_rowptr, const int32_t* src_cnt,
                              const int32_t* out_rowptr, int32_t* out_col, int32_t* out_pairs, int32_t* out_deg,
                              const int32_t* deg_rowptr, int clear, void* stream) {
    if (n_products <= 0 || n_products >= (1ll << 31) || !src || !src_rowptr || !out_rowptr) return PC_EINVAL;
    if ((!out_col && !out_pairs && !out_deg) || (out_deg && !deg_rowptr)) return PC_EINVAL;
    const uint32_t P = (uint32_t)n_products;
    PC_LAUNCH(ing_emit_kernel, dim3(ing_wave_grid(P)), dim3(256), 0, (hipStream_t)stream, P, src, src_rowptr, src_cnt, out_rowptr,
              out_col, out_pairs, out_deg, deg_rowptr, clear);
    return pc_launch_status();
}
