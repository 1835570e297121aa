// The three behaviour edge lists of ingest.hip derived from a raw shopper event log (ops.event_edges; data.event_edges_host is
// the host twin, equal bit for bit; DESIGN.md "Edge lists from shopper events" has the semantics).  events [N][4] int32, rows
// (session, product, kind, time) in any order, kind 0 = view, 1 = purchase.  A session with more than max_events raw rows is
// skipped whole; the items of a kept session are its distinct products, item x with fv(x) = its earliest view time (-1: never
// viewed) and lp(x) = its latest purchase time (-1: never purchased).  Per kept session and ordered pair of items a != b, with
// V(x) = fv(x) >= 0 and U(x) = lp(x) >= 0:
//     co_purchase           U(a) & U(b)
//     co_view               V(a) & V(b)                      [exclusive: & !(U(a) & U(b))]
//     purchase_after_view   V(a) & U(b) & fv(a) <= lp(b)     [exclusive: & !U(a)]
// Each list comes out as (a, b) rows ordered by (session, a, b); an edge appears once per session that shows it, so its
// multiplicity over the list -- the weight pc_ingest_rows reads -- is the number of such sessions.
//
//   count     one thread per row: every field is compared with its range BEFORE it indexes anything (an offender ORs its column's
//             bit into a flag word and is skipped, here and in the scatter), cnt[session] += 1
//   scan      pc_exclusive_scan_i32 -> the sessions' raw row offsets
//   scatter   (product, sort index) goes to its session's bucket through the session's integer cursor (arrival order arbitrary;
//             the rows of a session that will be skipped are not written).  sort index = (kind ^ 1) << 31 | time, as a signed
//             int: the views first (negative) in time order, then the purchases in time order
//   sessions  one wave per kept session, the bucket in NE = 2, 4, 8, 16 register slots per lane for up to 128, 256, 512, 1024
//             rows (every variant that max_events can reach is launched; a wave passes over a session of another class, the
//             smallest variant takes the empty and the skipped ones).  rlw_sort<NE> (wave_sort.h) under (product ascending, sort
//             index ascending): a run of equal products is one item, fv at its head if that is a view, lp at its tail if that is
//             a purchase.  The k-th head and the k-th tail belong to the same run, so one wave prefix sum over (heads, tails)
//             places both: the items go to LDS ascending by product, from there back into the bucket as (product, fv) and into
//             last_purchase, and the pair loop below COUNTS the session's rows of the three lists.  A reduction launch adds the
//             counts into 64-bit totals, which the host compares with its limit before any offset is scanned.
//   emit      after three scans of the per-session counts: one wave per session again, the items from the bucket into LDS, the
//             same pair loop WRITING (a, b) at the session's offsets.
//   pair loop the ordered pairs q = a m + b of a session of m items, 64 per step in ascending q -- (a, b) ascending --; a lane's
//             row of a list lands at the list's running offset plus the number of lower lanes with a row (a ballot).  a = q / m
//             is one multiply-high by floor(2^32 / m) + 1, exact for q < 2^20 and m <= 2^10.
// Integer atomics only (the counts, the cursors, the flag word, the totals); they decide the arrival order inside a bucket,
// which the sort removes, or sums.  No floats.  Every output is a function of the log as a multiset of rows.
#include <climits>

#include "block_ops.h"             // wave_sum, wave_exclusive_sum
#include "wave_sort.h"             // rlw_sort; grouped_plan.h: RG_NONE

#define EV_MAX_EVENTS 1024
#define EV_BAD_SESSION 1
#define EV_BAD_PRODUCT 2
#define EV_BAD_KIND 4
#define EV_BAD_TIME 8
#define EV_PAD INT_MIN                 // the sort value of a padding slot (~product of a real one is in [-2^31 + 1, -1])
#define EV_GRID (1u << 20)             // workgroups of the wave-per-session launches at most (they stride over the sessions)
#define EV_TOTALS 5                    // co_view, purchase_after_view, co_purchase rows; items; skipped sessions

// The variant that serves a session of n raw rows (sessions) or m items (emit).
__host__ __device__ __forceinline__ int ev_class(int n) { return n <= 128 ? 2 : (n <= 256 ? 4 : (n <= 512 ? 8 : 16)); }

// ---- bucketing by session ---------------------------------------------------------------------------------------------
__device__ __forceinline__ bool ev_row(const int32_t* __restrict__ events, uint32_t i, uint32_t S, uint32_t P, int32_t* bad, int& s,
                                       int& p, int& y) {
    const int4 r = reinterpret_cast<const int4*>(events)[i];
    const int f = ((uint32_t)r.x >= S ? EV_BAD_SESSION : 0) | ((uint32_t)r.y >= P ? EV_BAD_PRODUCT : 0) |
                  ((uint32_t)r.z > 1u ? EV_BAD_KIND : 0) | (r.w < 0 ? EV_BAD_TIME : 0);
    if (f) {
        if (bad) atomicOr(bad, f);
        return false;
    }
    s = r.x; p = r.y;
    y = (int)(((uint32_t)(r.z ^ 1) << 31) | (uint32_t)r.w);
    return true;
}

__global__ __launch_bounds__(256) void ev_count_kernel(const int32_t* __restrict__ events, uint32_t N, uint32_t S, uint32_t P,
                                                       int32_t* cnt, int32_t* bad) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    int s, p, y;
    if (i < N && ev_row(events, i, S, P, bad, s, p, y)) atomicAdd(&cnt[s], 1);
}

// cursor[s] holds the session's count on entry; on exit 0 for a kept session (a skipped one keeps its count)
__global__ __launch_bounds__(256) void ev_scatter_kernel(const int32_t* __restrict__ events, uint32_t N, uint32_t S, uint32_t P,
                                                         int max_events, const int32_t* __restrict__ rowptr, int32_t* cursor,
                                                         int2* bucket) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    int s, p, y;
    if (i >= N || !ev_row(events, i, S, P, nullptr, s, p, y)) return;
    const int lo = rowptr[s], n = rowptr[s + 1] - lo;
    if (n > max_events) return;
    const int k = atomicSub(&cursor[s], 1) - 1;
    if ((uint32_t)k < (uint32_t)n) bucket[(size_t)lo + k] = make_int2(p, y);   // (always, when cursor is the count pass's output)
}

// ---- the pair loop ----------------------------------------------------------------------------------------------------
// prod / fv / lp [m]: the session's items ascending by product (LDS).  o[3]: the running offsets of co_view,
// purchase_after_view, co_purchase -- on exit advanced by the session's rows.  EMIT: the rows are written to out[l] while they
// stay below room[l].  Every lane of the wave calls it.
template <bool EMIT>
__device__ __forceinline__ void ev_pairs(const int* prod, const int* fv, const int* lp, int m, int exclusive, int lane, int (&o)[3],
                                         const int (&room)[3], int2* const (&out)[3]) {
    if (m < 2) return;
    const uint32_t total = (uint32_t)m * (uint32_t)m;     // (m <= 1024)
    const uint32_t magic = 0xffffffffu / (uint32_t)m + 1u;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (uint32_t q0 = 0; q0 < total; q0 += 64u) {
        const uint32_t q = q0 + (uint32_t)lane;
        const uint32_t a = __umulhi(q, magic), b = q - a * (uint32_t)m;
        bool is[3] = {false, false, false};
        if (q < total && a != b) {
            const int fa = fv[a], la = lp[a], lb = lp[b];
            const bool va = fa >= 0, ua = la >= 0, vb = fv[b] >= 0, ub = lb >= 0;
            const bool both = ua && ub;
            is[0] = va && vb && !(exclusive && both);
            is[1] = va && ub && fa <= lb && !(exclusive && ua);
            is[2] = both;
        }
#pragma unroll
        for (int l = 0; l < 3; l++) {
            const unsigned long long mask = __ballot(is[l]);
            if constexpr (EMIT) {
                const int k = o[l] + __popcll(mask & below);
                if (is[l] && k < room[l]) out[l][k] = make_int2(prod[a], prod[b]);    // (k < room always, when room scans the counts)
            }
            o[l] += __popcll(mask);
        }
    }
}

// ---- sessions ---------------------------------------------------------------------------------------------------------
template <int NE>
__global__ __launch_bounds__(64) void ev_sessions_kernel(uint32_t S, const int32_t* __restrict__ rowptr, int2* bucket,
                                                         int32_t* last_purchase, int max_events, int exclusive, int32_t* n_items,
                                                         int32_t* count_cv, int32_t* count_pv, int32_t* count_cp) {
    __shared__ int s_prod[64 * NE], s_fv[64 * NE], s_lp[64 * NE];
    const int lane = threadIdx.x;
    for (uint32_t s = blockIdx.x; s < S; s += gridDim.x) {
        const int lo = rowptr[s], n = rowptr[s + 1] - lo;
        const bool kept = n > 0 && n <= max_events;
        if (ev_class(kept ? n : 0) != NE) continue;        // (uniform) another launch serves this session
        if (!kept) {
            if (lane == 0) {
                n_items[s] = 0; count_cv[s] = 0; count_pv[s] = 0; count_cp[s] = 0;
            }
            continue;
        }
        // ---- the bucket, lane-interleaved for the load (any order serves: the sort follows)
        int key[NE], ix[NE];
#pragma unroll
        for (int e = 0; e < NE; e++) {
            const int j = lane + 64 * e;
            key[e] = EV_PAD;
            ix[e] = RG_NONE;
            if (j < n) {
                const int2 r = bucket[(size_t)lo + j];
                key[e] = ~r.x;
                ix[e] = r.y;
            }
        }
        // slot NE * lane + e: product ascending, inside a product the views in time order, then the purchases; padding last
        rlw_sort<NE>(key, ix, lane);
        int before = __shfl_up(key[NE - 1], 1, 64), after = __shfl_down(key[0], 1, 64);
        if (lane == 0) before = EV_PAD;                    // (no real slot's value)
        if (lane == 63) after = EV_PAD;
        bool head[NE], tail[NE];
        int mine = 0;                                      // heads | tails << 16 of this lane (each at most 1024 over the wave)
#pragma unroll
        for (int e = 0; e < NE; e++) {
            const bool real = key[e] != EV_PAD;
            head[e] = real && key[e] != (e == 0 ? before : key[e == 0 ? 0 : e - 1]);
            tail[e] = real && key[e] != (e == NE - 1 ? after : key[e == NE - 1 ? e : e + 1]);
            mine += (head[e] ? 1 : 0) + (tail[e] ? 1 << 16 : 0);
        }
        int all;
        const int first = wave_exclusive_sum(mine, lane, all);
        const int m = all & 0xffff;                        // the session's items (= its tails)
        int h = first & 0xffff, t = first >> 16;
#pragma unroll
        for (int e = 0; e < NE; e++) {
            if (head[e]) {                                 // (h < m <= n <= 64 NE)
                s_prod[h] = ~key[e];
                s_fv[h] = ix[e] < 0 ? (ix[e] & 0x7fffffff) : -1;
                h++;
            }
            if (tail[e]) {
                s_lp[t] = ix[e] >= 0 ? ix[e] : -1;
                t++;
            }
        }
        __syncthreads();
        for (int i = lane; i < m; i += 64) {
            bucket[(size_t)lo + i] = make_int2(s_prod[i], s_fv[i]);
            last_purchase[(size_t)lo + i] = s_lp[i];
        }
        int o[3] = {0, 0, 0};
        const int room[3] = {0, 0, 0};
        int2* const out[3] = {nullptr, nullptr, nullptr};
        ev_pairs<false>(s_prod, s_fv, s_lp, m, exclusive, lane, o, room, out);
        if (lane == 0) {
            n_items[s] = m; count_cv[s] = o[0]; count_pv[s] = o[1]; count_cp[s] = o[2];
        }
        __syncthreads();                                   // the reads are done before the next session's stores
    }
}

// The 64-bit sums of the sessions pass over all sessions: one wave reduction and one integer atomic per quantity and wave.
__global__ __launch_bounds__(256) void ev_totals_kernel(uint32_t S, const int32_t* __restrict__ rowptr, int max_events,
                                                        const int32_t* __restrict__ n_items, const int32_t* __restrict__ count_cv,
                                                        const int32_t* __restrict__ count_pv, const int32_t* __restrict__ count_cp,
                                                        unsigned long long* totals) {
    unsigned long long t[EV_TOTALS] = {0ull, 0ull, 0ull, 0ull, 0ull};
    for (uint64_t s = (uint64_t)blockIdx.x * 256u + threadIdx.x; s < S; s += (uint64_t)gridDim.x * 256u) {
        t[0] += (unsigned long long)count_cv[s];
        t[1] += (unsigned long long)count_pv[s];
        t[2] += (unsigned long long)count_cp[s];
        t[3] += (unsigned long long)n_items[s];
        t[4] += rowptr[s + 1] - rowptr[s] > max_events ? 1ull : 0ull;
    }
#pragma unroll
    for (int k = 0; k < EV_TOTALS; k++) {
        const unsigned long long v = wave_sum(t[k]);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&totals[k], v);
    }
}

// ---- emit -------------------------------------------------------------------------------------------------------------
template <int NE>
__global__ __launch_bounds__(64) void ev_emit_kernel(uint32_t S, const int32_t* __restrict__ rowptr, const int2* __restrict__ bucket,
                                                     const int32_t* __restrict__ last_purchase, const int32_t* __restrict__ n_items,
                                                     int exclusive, const int32_t* __restrict__ off_cv,
                                                     const int32_t* __restrict__ off_pv, const int32_t* __restrict__ off_cp,
                                                     int2* out_cv, int2* out_pv, int2* out_cp) {
    __shared__ int s_prod[64 * NE], s_fv[64 * NE], s_lp[64 * NE];
    const int lane = threadIdx.x;
    for (uint32_t s = blockIdx.x; s < S; s += gridDim.x) {
        const int m = n_items[s];
        const int lo = rowptr[s], n = rowptr[s + 1] - lo;
        if (m < 2 || m > n || m > EV_MAX_EVENTS || ev_class(m) != NE) continue;     // (uniform; m <= n always)
        for (int i = lane; i < m; i += 64) {
            const int2 r = bucket[(size_t)lo + i];
            s_prod[i] = r.x;
            s_fv[i] = r.y;
            s_lp[i] = last_purchase[(size_t)lo + i];
        }
        __syncthreads();
        int o[3] = {off_cv[s], off_pv[s], off_cp[s]};
        const int room[3] = {off_cv[s + 1], off_pv[s + 1], off_cp[s + 1]};
        int2* const out[3] = {out_cv, out_pv, out_cp};
        ev_pairs<true>(s_prod, s_fv, s_lp, m, exclusive, lane, o, room, out);
        __syncthreads();
    }
}

// ---- entries ----------------------------------------------------------------------------------------------------------
static inline bool ev_sizes_ok(int64_t n_events, int64_t n_sessions, int64_t n_products) {
    return n_events >= 0 && n_events < (1ll << 31) && n_sessions > 0 && n_sessions < (1ll << 31) && n_products > 0 &&
           n_products < (1ll << 31);
}
static inline bool ev_max_ok(int max_events) { return max_events >= 2 && max_events <= EV_MAX_EVENTS; }
static inline unsigned ev_grid(int64_t n_sessions) { return (unsigned)(n_sessions < (int64_t)EV_GRID ? n_sessions : (int64_t)EV_GRID); }

extern "C" int pc_events_limits(int* max_events, int* n_totals) {
    if (!max_events || !n_totals) return PC_EINVAL;
    *max_events = EV_MAX_EVENTS;
    *n_totals = EV_TOTALS;
    return 0;
}

extern "C" int pc_events_count(const int32_t* events, int64_t n_events, int64_t n_sessions, int64_t n_products, int32_t* cnt,
                               int32_t* bad, void* stream) {
    if (!ev_sizes_ok(n_events, n_sessions, n_products) || !cnt || !bad || (n_events > 0 && !events)) return PC_EINVAL;
    if (((uintptr_t)events & 15u) != 0) return PC_ESHAPE;     // a row is read as one 16-byte word
    if (n_events == 0) return 0;
    PC_LAUNCH(ev_count_kernel, dim3((unsigned)((n_events + 255) / 256)), dim3(256), 0, (hipStream_t)stream, events, (uint32_t)n_events,
              (uint32_t)n_sessions, (uint32_t)n_products, cnt, bad);
    return pc_launch_status();
}

extern "C" int pc_events_scatter(const int32_t* events, int64_t n_events, int64_t n_sessions, int64_t n_products, int max_events,
                                 const int32_t* rowptr, int32_t* cursor, int32_t* bucket, void* stream) {
    if (!ev_sizes_ok(n_events, n_sessions, n_products) || !rowptr || !cursor || !bucket || (n_events > 0 && !events)) return PC_EINVAL;
    if (!ev_max_ok(max_events) || ((uintptr_t)events & 15u) != 0 || ((uintptr_t)bucket & 7u) != 0) return PC_ESHAPE;
    if (n_events == 0) return 0;
    PC_LAUNCH(ev_scatter_kernel, dim3((unsigned)((n_events + 255) / 256)), dim3(256), 0, (hipStream_t)stream, events,
              (uint32_t)n_events, (uint32_t)n_sessions, (uint32_t)n_products, max_events, rowptr, cursor, (int2*)bucket);
    return pc_launch_status();
}

extern "C" int pc_events_sessions(int64_t n_sessions, const int32_t* rowptr, int32_t* bucket, int32_t* last_purchase, int max_events,
                                  int exclusive, int32_t* n_items, int32_t* count_cv, int32_t* count_pv, int32_t* count_cp,
                                  int64_t* totals, void* stream) {
    if (n_sessions <= 0 || n_sessions >= (1ll << 31) || !rowptr || !bucket || !last_purchase || !n_items || !count_cv || !count_pv ||
        !count_cp || !totals)
        return PC_EINVAL;
    if (!ev_max_ok(max_events) || ((uintptr_t)bucket & 7u) != 0 || ((uintptr_t)totals & 7u) != 0) return PC_ESHAPE;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t S = (uint32_t)n_sessions;
    const dim3 grid(ev_grid(n_sessions)), block(64);
#define EV_GO(NE)                                                                                                           \
    PC_LAUNCH((ev_sessions_kernel<NE>), grid, block, 0, st, S, rowptr, (int2*)bucket, last_purchase, max_events, exclusive != 0, \
              n_items, count_cv, count_pv, count_cp)
    EV_GO(2);                                              // (the empty and the skipped sessions are here)
    if (max_events > 128) EV_GO(4);
    if (max_events > 256) EV_GO(8);
    if (max_events > 512) EV_GO(16);
#undef EV_GO
    const unsigned tgrid = (unsigned)((n_sessions + 255) / 256 < 1024 ? (n_sessions + 255) / 256 : 1024);
    PC_LAUNCH(ev_totals_kernel, dim3(tgrid), dim3(256), 0, st, S, rowptr, max_events, n_items, count_cv, count_pv, count_cp,
              (unsigned long long*)totals);
    return pc_launch_status();
}

extern "C" int pc_events_emit(int64_t n_sessions, const int32_t* rowptr, const int32_t* bucket, const int32_t* last_purchase,
                              const int32_t* n_items, int max_events, int exclusive, const int32_t* off_cv, const int32_t* off_pv,
                              const int32_t* off_cp, int32_t* out_cv, int32_t* out_pv, int32_t* out_cp, void* stream) {
    if (n_sessions <= 0 || n_sessions >= (1ll << 31) || !rowptr || !bucket || !last_purchase || !n_items || !off_cv || !off_pv ||
        !off_cp || !out_cv || !out_pv || !out_cp)
        return PC_EINVAL;
    if (!ev_max_ok(max_events) || ((uintptr_t)bucket & 7u) != 0 || ((uintptr_t)out_cv & 7u) != 0 || ((uintptr_t)out_pv & 7u) != 0 ||
        ((uintptr_t)out_cp & 7u) != 0)
        return PC_ESHAPE;
    hipStream_t st = (hipStream_t)stream;
    const uint32_t S = (uint32_t)n_sessions;
    const dim3 grid(ev_grid(n_sessions)), block(64);
#define EV_GO(NE)                                                                                                           \
    PC_LAUNCH((ev_emit_kernel<NE>), grid, block, 0, st, S, rowptr, (const int2*)bucket, last_purchase, n_items, exclusive != 0, \
              off_cv, off_pv, off_cp, (int2*)out_cv, (int2*)out_pv, (int2*)out_cp)
    EV_GO(2);
    if (max_events > 128) EV_GO(4);
    if (max_events > 256) EV_GO(8);
    if (max_events > 512) EV_GO(16);
#undef EV_GO
    return pc_launch_status();
}
