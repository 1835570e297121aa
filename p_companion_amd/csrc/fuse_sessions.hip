// Session recommendations: the lists of a session's items fused into one list, for ragged sessions with a weight per item
// (pc_fuse_sessions; ops.fuse_sessions, PCompanionInference.recommend_session_batch).  idx / score [rows][w]: row r is what a
// grouped retrieval returned for item r, its K type lists side by side, in any order, -1 ids and non-finite scores anywhere;
// optionally source [rows] (the item's product id, -1 = no item), weight [rows] (NULL: every weight is 1) and an exclusion CSR
// keyed by product id (ops.exclusion_csr: strictly ascending rows).  seg_rowptr [sessions + 1]: session b owns the rows
// [seg_rowptr[b], seg_rowptr[b + 1]).  The output is the first n products of the session under rg_better (fused score
// descending, product index ascending), each with its fused score and its support.
//
//   live rows    L = min(1024 / w, max_items if it is not 0).  Only the LAST L rows of a session -- its most recent items --
//                offer candidates; a session with more rows adds one to truncated_count.  Every row still bans.
//   offering row a live row whose source lies in [0, num_products) (without `source` every row qualifies) and whose weight is
//                finite and > 0.  A row with weight 0, a negative weight, NaN or +-inf offers nothing; its source still bans
//                ("already bought").
//   term         t = fl(weight[r] * score): ONE fp32 multiplication, rounded, formed before anything is added and never
//                contracted with an addition.  A slot is a candidate iff its row offers, its id lies in [0, num_products) and
//                t is finite: an overflowed term is no candidate.  Terms in the subnormal range are outside the contract.
//   ban set      the sources of ALL rows of the session, live or not, and, with the CSR, every id in the exclusion rows of
//                those sources.  A banned product is no candidate, whichever row offered it.
//   fusion       all candidate slots of a session with one product id are one product.  With its terms in descending order
//                t1 >= t2 >= ... (+0.0 before -0.0): sum: f = t1, f = fl(f + t2), ... -- sequential fp32, the largest first --;
//                max: f = t1.  support = the number of slots fused.  A sum that overflows is served as the infinity it became.
//   bad inputs   an id of a live row or a source of any row outside [-1, num_products) is never used as an index and is
//                counted (one integer atomic each; such a source's row offers nothing); the slots of rows that are not live
//                are not read.  A seg_rowptr entry outside [0, rows] or below its predecessor is counted once and clamped --
//                lo to [0, rows], hi to [lo, rows] --: nothing outside the arrays is read.
//   kernel       one wave per session, four sessions per workgroup, grid-stride over sessions; the waves of a workgroup never
//                meet (every wave has its own LDS rows).  The effective pool min(len, L) w of a session decides its variant,
//                NE = 2, 4, 8, 16 register slots per lane for pools <= 128, 256, 512, 1024; the host cannot know the pools
//                without reading them back, so it launches every variant that L w can reach on the one stream, and a wave
//                passes over, wave-uniformly, a session whose pool belongs to another variant (the smallest takes the empty
//                ones): every session is written by exactly one launch.  The live slots go into the registers lane-interleaved
//                (row of slot j: j / w), the term is formed there.  lp_ban_pass (list_pool.h) strikes the ban set out of them,
//                over all rows of the session.  rlw_sort<NE> (wave_sort.h) then sorts ints with the keys swapped -- value
//                ~id (INT_MIN for a non-candidate), index ~rlw_key(t) --: id ascending, then term
//                descending with +0.0 before -0.0, a strict order in which equal slots are equal bits, so a product's slots
//                are ADJACENT.  Ids and terms go to the wave's LDS rows; a slot is the head of its product iff it is a
//                candidate and its predecessor's id differs; each head walks forward while the id matches, adding in position
//                order -- the pinned one -- and counting its support.  The walk is bounded by the candidate count and costs the
//                longest run, not the pool.  A second sort (rlw_sort_with: the support travels as payload) puts the heads
//                under rg_better of their fused scores, and lp_store_row (list_pool.h) compacts and stores them with the
//                -1 / -inf / 0 tail.
// Both sorts run under strict orders, so the output bits do not depend on the variant.  Integer compares, float compares, one
// fp32 multiplication per slot and the fp32 additions above: no workspace, no float atomics (integer atomics for the two
// counters only), nothing read back; the result does not depend on the grid, the run, the variant, a permutation of a
// session's rows (with their sources and weights) among the rows of one truncation status, or of the slots inside rows.
#include <climits>

#include "common.h"
#include "list_pool.h"             // lp_ban_pass, lp_store_row, LP_CHUNK
#include "wave_sort.h"             // rlw_sort, rlw_sort_with, rlw_key; grouped_plan.h: rg_better, RG_NONE, RG_MAX_GRID

#define FUSE_SESSIONS_MAX_POOL 1024
#define FS_MAX_N 256
#define FS_WAVES 4                 // sessions per workgroup, one wave each
#define FS_OUT INT_MIN             // the sort value of a slot that is no candidate (~id of a candidate is in [-2^31 + 1, -1])

// The variant that serves a pool of m slots.
__host__ __device__ __forceinline__ int fs_class(int m) { return m <= 128 ? 2 : (m <= 256 ? 4 : (m <= 512 ? 8 : 16)); }

template <int NE>
__global__ __launch_bounds__(64 * FS_WAVES) void fs_fuse_kernel(
    const int32_t* __restrict__ idx, const float* __restrict__ score, const int32_t* __restrict__ source,
    const float* __restrict__ weight, const int32_t* __restrict__ seg_rowptr, const int32_t* __restrict__ ex_rowptr,
    const int32_t* __restrict__ ex_col, int rows, int sessions, int w, int live_max, int num_products, int n, int combine,
    int32_t* __restrict__ out_idx, float* __restrict__ out_score, int32_t* __restrict__ out_support,
    int32_t* __restrict__ bad_count, int32_t* __restrict__ truncated_count) {
    typedef int ivec __attribute__((ext_vector_type(NE)));
    typedef float fvec __attribute__((ext_vector_type(NE)));
    __shared__ __attribute__((aligned(16))) int lid_all[FS_WAVES][64 * NE];       // a wave's ~ids, equal ids adjacent
    __shared__ __attribute__((aligned(16))) float lsc_all[FS_WAVES][64 * NE];     // ... and their terms
    __shared__ __attribute__((aligned(16))) int lban_all[FS_WAVES][LP_CHUNK];     // a chunk of the session's ban ids
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int* lid = lid_all[wave];
    float* lsc = lsc_all[wave];
    int* lban = lban_all[wave];
    const int64_t stride = (int64_t)gridDim.x * FS_WAVES;
    for (int64_t b = (int64_t)blockIdx.x * FS_WAVES + wave; b < sessions; b += stride) {        // (wave-uniform)
        // ---- the session's rows [lo, hi), clamped into the arrays; its live rows [r0, hi); its variant
        const int lo_raw = seg_rowptr[b], hi_raw = seg_rowptr[b + 1];
        const int lo = min(max(lo_raw, 0), rows), hi = min(max(hi_raw, lo), rows);
        const int len = hi - lo, live = min(len, live_max);
        const int r0 = hi - live, m = live * w;           // (live <= 1024 / w: m <= 1024)
        if (fs_class(m) != NE) continue;                  // (uniform) another launch serves this session
        if (lane == 0) {
            // entry b + 1, and entry 0 with the first session: every entry is judged once, by the launch that serves the session
            const int bad_ends = (hi_raw < 0 || hi_raw > rows || hi_raw < lo_raw) + (b == 0 && (lo_raw < 0 || lo_raw > rows));
            if (bad_ends && bad_count) atomicAdd(bad_count, bad_ends);
            if (len > live && truncated_count) atomicAdd(truncated_count, 1);
        }
        // ---- the live slots, lane-interleaved for the load (any order serves: the sort follows); val = ~id, tk = ~key(term)
        int val[NE], tk[NE];
#pragma unroll
        for (int e = 0; e < NE; e++) {
            const int j = lane + 64 * e;
            val[e] = FS_OUT;
            tk[e] = RG_NONE;
            if (j < m) {
                const int r = r0 + j / w;                 // (r < hi <= rows)
                const int id = idx[(size_t)r0 * w + j];
                const float s = score[(size_t)r0 * w + j];
                const int src = source ? source[r] : 0;
                const float wt = weight ? weight[r] : 1.0f;
                const float t = __fmul_rn(wt, s);         // one rounded product, never contracted with an addition
                if (id < -1 || id >= num_products) {      // never used as an index
                    if (bad_count) atomicAdd(bad_count, 1);
                } else if (id >= 0 && src >= 0 && src < num_products && wt > 0.0f && __builtin_isfinite(wt) &&
                           __builtin_isfinite(t)) {
                    val[e] = ~id;
                    tk[e] = ~rlw_key(t);
                }
            }
        }
        // ---- the ban set: the sources of ALL rows and their exclusion rows (list_pool.h), matched as ~id
        if (source)                                       // (uniform)
            lp_ban_pass<NE, true>(source + (size_t)lo, len, ex_rowptr, ex_col, num_products, bad_count, lban, lane, val, tk,
                                  FS_OUT, RG_NONE);
        // slot NE * lane + e: id ascending, inside an id the term descending (+0.0 before -0.0), the non-candidates last
        rlw_sort<NE>(val, tk, lane);
        int cnt = 0;                                      // the candidates: the positions below cnt
#pragma unroll
        for (int e = 0; e < NE; e++) cnt += __popcll(__ballot(val[e] != FS_OUT));
        float v[NE];
        ivec wi;
        fvec ws;
#pragma unroll
        for (int e = 0; e < NE; e++) {
            v[e] = rlw_unkey(~tk[e]);
            wi[e] = val[e];
            ws[e] = v[e];
        }
        *reinterpret_cast<ivec*>(&lid[NE * lane]) = wi;
        *reinterpret_cast<fvec*>(&lsc[NE * lane]) = ws;
        __builtin_amdgcn_wave_barrier();
        // ---- heads and the walk: a head adds the run behind it in position order, which is descending
        int before = __shfl_up(val[NE - 1], 1, 64);       // the slot in front of the lane's first
        if (lane == 0) before = FS_OUT;                   // (no candidate's value: position 0 is a head if it is a candidate)
        int ix[NE], sup[NE];
#pragma unroll
        for (int e = 0; e < NE; e++) {
            const bool head = val[e] != FS_OUT && val[e] != (e == 0 ? before : val[e == 0 ? 0 : e - 1]);
            float f = v[e];
            int s = 0;
            if (head) {
                s = 1;
                for (int q = NE * lane + e + 1; q < cnt && lid[q] == val[e]; q++) {             // (q < cnt <= 64 NE)
                    if (combine == 0) f = __fadd_rn(f, lsc[q]);
                    s++;
                }
            }
            v[e] = head ? f : -INFINITY;
            ix[e] = head ? ~val[e] : RG_NONE;
            sup[e] = s;
        }
        __builtin_amdgcn_wave_barrier();                  // the reads are done before the next session's stores
        // the heads under rg_better of their fused scores (distinct ids: a strict order), each with its support
        rlw_sort_with<NE>(v, ix, sup, lane);
        // ---- compaction and store (list_pool.h): the heads' places, in serving order
        bool keep[NE];
#pragma unroll
        for (int e = 0; e < NE; e++) keep[e] = ix[e] != RG_NONE;
        lp_store_row<NE, true>(keep, ix, v, sup, lane, n, (size_t)b * n, out_idx, out_score, out_support);
    }
}

extern "C" int pc_fuse_sessions(const int32_t* idx, const float* score, const int32_t* source, const float* weight,
                                const int32_t* seg_rowptr, int rows, int sessions, int w, int max_items,
                                const int32_t* ex_rowptr, const int32_t* ex_col, int num_products, int n, int combine,
                                int32_t* out_idx, float* out_score, int32_t* out_support, int32_t* bad_count,
                                int32_t* truncated_count, void* stream) {
    if (rows < 0 || sessions < 0 || w < 1 || w > FUSE_SESSIONS_MAX_POOL || max_items < 0) return PC_ESHAPE;
    if (n < 1 || n > FS_MAX_N || num_products < 1 || (combine != 0 && combine != 1)) return PC_ESHAPE;
    if ((ex_rowptr != nullptr) != (ex_col != nullptr) || (ex_rowptr && !source)) return PC_ESHAPE;      // the rows are the sources'
    if (sessions == 0) return PC_OK;                                      // nothing to serve: no launch, no pointer is read
    if (!seg_rowptr || !out_idx || !out_score || !out_support || (rows > 0 && (!idx || !score))) return PC_ESHAPE;
    hipStream_t st = (hipStream_t)stream;
    int live_max = FUSE_SESSIONS_MAX_POOL / w;            // L: the rows of a session that offer
    if (max_items != 0) live_max = min(live_max, max_items);
    const int reach = min(live_max, rows) * w;            // the largest pool any session can have (<= 1024)
    const int wgs = sessions / FS_WAVES + (sessions % FS_WAVES != 0);
    const dim3 grid((unsigned)min(wgs, RG_MAX_GRID)), block(64 * FS_WAVES);
#define FS_GO(NE)                                                                                                            \
    PC_LAUNCH((fs_fuse_kernel<NE>), grid, block, 0, st, idx, score, source, weight, seg_rowptr, ex_rowptr, ex_col, rows,      \
              sessions, w, live_max, num_products, n, combine, out_idx, out_score, out_support, bad_count, truncated_count)
    FS_GO(2);                                             // (the empty sessions are here)
    if (reach > 128) FS_GO(4);
    if (reach > 256) FS_GO(8);
    if (reach > 512) FS_GO(16);
#undef FS_GO
    return pc_launch_status();
}
