// Basket recommendations: the lists of a basket's items fused into one list (pc_fuse_lists; ops.fuse_lists,
// PCompanionInference.recommend_basket_batch).  A basket has S source rows of w slots -- idx / score [B][S][w], each row what a
// grouped retrieval returned for one basket item, its K type lists side by side, in any order, -1 ids and non-finite scores
// anywhere --, optionally source [B][S] (the product id of the item behind each row, -1 = no item here) and an exclusion CSR
// keyed by product id (ops.exclusion_csr: strictly ascending rows).  The output is the first n products of the basket under
// rg_better (fused score descending, product index ascending), each with its fused score and its support.
//
//   candidate    a slot whose row's source is not -1 (without `source` every row counts), whose id lies in [0, num_products)
//                and whose score is finite.  An id outside [-1, num_products) is never used as an index and is counted (one
//                integer atomic), whatever its row; a source outside [-1, num_products) likewise, and its row is dropped.
//   ban set      the basket's own source ids and, with the CSR, every id in the exclusion rows of those sources.  A banned
//                product is no candidate, whichever row offered it.
//   fusion       all candidate slots of a basket with one product id are one product.  With its slot scores in descending
//                order s1 >= s2 >= ... (+0.0 before -0.0): sum: f = s1, f = fl(f + s2), ... -- sequential fp32, the largest
//                first: the pinned order makes the bits independent of the slot order --; max: f = s1.  support = the number of
//                slots fused.  A sum that overflows is served as the infinity it became, where rg_better puts it.
//   kernel       one wave per basket, four baskets per workgroup, grid-stride over baskets; the waves of a workgroup never meet
//                (every wave has its own LDS rows).  The slots go into NE registers per lane, non-candidates as
//                (-inf, RG_NONE).  The ban set is struck out of them by list_pool.h's lp_ban_pass, written out below (see
//                there; why this unit keeps its text: HISTORY.md "Shared list post-pass blocks").  rlw_sort<NE> sorts the
//                survivors under the strict order of (score bits, id) -- rg_better with +0.0 before -0.0 --, ids and scores go
//                to the wave's LDS rows, and every lane walks the candidates' part of them: for each of its slots it counts the
//                earlier slots of the same id (a slot with any is not the head of its product) and, for sum, adds the later
//                ones' scores to its own in slot order, which is already descending.  A second sort (rlw_sort_with: the support
//                travels as payload) puts the heads under rg_better of their fused scores, and list_pool.h's lp_store_row,
//                written out below as well, compacts and stores them with the -1 / -inf / 0 tail.
//   variants     NE = 2, 4, 8, 16 for S w <= 128, 256, 512, 1024.  Both sorts run under strict orders -- slots that compare
//                equal are the same bits --, so the output bits do not depend on the variant.
// Integer compares, float compares and the fp32 additions above: no workspace, no float atomics, nothing read back; the result
// does not depend on the grid, the run, or a permutation of a basket's rows (with their sources) or of the slots inside rows.
#include "common.h"
#include "wave_sort.h"             // rlw_sort, rlw_sort_with; grouped_plan.h: rg_better, RG_NONE, RG_MAX_GRID

#define FUSE_LISTS_MAX_POOL 1024
#define FL_MAX_N 256
#define FL_WAVES 4                 // baskets per workgroup, one wave each
#define FL_CHUNK 256               // ban ids per pass through LDS

typedef int fl_i32x4 __attribute__((ext_vector_type(4)));
typedef float fl_f32x4 __attribute__((ext_vector_type(4)));

// Every lane against the first `cnt` candidates of the wave's sorted rows (lid / lsc, position p = NE lane' + e'): c[e] = the
// earlier slots with the id of the lane's slot e; f[e] = its own score and (SUM) then the later ones' of that id, added in
// position order; sup[e] = 1 + the later ones.
template <int NE, bool SUM>
__device__ __forceinline__ void fl_walk(const int* lid, const float* lsc, int cnt, int lane, const int (&ix)[NE], int (&c)[NE],
                                        float (&f)[NE], int (&sup)[NE]) {
    const int nq = (cnt + 3) >> 2;                        // (<= 16 NE: inside the wave's rows, every entry of which is written)
    for (int q = 0; q < nq; q++) {
        const fl_i32x4 xi = *reinterpret_cast<const fl_i32x4*>(&lid[4 * q]);      // (one address per wave: a broadcast)
        fl_f32x4 xs = {0.0f, 0.0f, 0.0f, 0.0f};
        if constexpr (SUM) xs = *reinterpret_cast<const fl_f32x4*>(&lsc[4 * q]);
#pragma unroll
        for (int t = 0; t < 4; t++)
#pragma unroll
            for (int e = 0; e < NE; e++) {
                const bool same = xi[t] == ix[e];
                const bool later = same & (4 * q + t > NE * lane + e);
                c[e] += same & (4 * q + t < NE * lane + e);
                sup[e] += later;
                if constexpr (SUM) f[e] = later ? f[e] + xs[t] : f[e];
            }
    }
}

template <int NE>
__global__ __launch_bounds__(64 * FL_WAVES) void fl_fuse_kernel(const int32_t* __restrict__ idx, const float* __restrict__ score,
                                                                const int32_t* __restrict__ source,
                                                                const int32_t* __restrict__ ex_rowptr,
                                                                const int32_t* __restrict__ ex_col, int baskets, int S, int w,
                                                                int num_products, int n, int combine,
                                                                int32_t* __restrict__ out_idx, float* __restrict__ out_score,
                                                                int32_t* __restrict__ out_support,
                                                                int32_t* __restrict__ bad_count) {
    typedef int ivec __attribute__((ext_vector_type(NE)));
    typedef float fvec __attribute__((ext_vector_type(NE)));
    __shared__ __attribute__((aligned(16))) int lid_all[FL_WAVES][64 * NE];       // a wave's ids in serving order
    __shared__ __attribute__((aligned(16))) float lsc_all[FL_WAVES][64 * NE];     // ... and their scores
    __shared__ __attribute__((aligned(16))) int lban_all[FL_WAVES][FL_CHUNK];     // a chunk of the basket's ban ids
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int* lid = lid_all[wave];
    float* lsc = lsc_all[wave];
    int* lban = lban_all[wave];
    const int m = S * w;
    const int64_t stride = (int64_t)gridDim.x * FL_WAVES;
    for (int64_t b = (int64_t)blockIdx.x * FL_WAVES + wave; b < baskets; b += stride) {         // (wave-uniform)
        // ---- the basket's slots, lane-interleaved for the load (any order serves: the sort follows)
        float v[NE];
        int ix[NE];
#pragma unroll
        for (int e = 0; e < NE; e++) {
            const int j = lane + 64 * e;
            v[e] = -INFINITY;
            ix[e] = RG_NONE;
            if (j < m) {
                const int id = idx[(size_t)b * m + j];
                const float s = score[(size_t)b * m + j];
                const int src = source ? source[(size_t)b * S + j / w] : 0;       // (j / w < S)
                if (id < -1 || id >= num_products) {      // never used as an index
                    if (bad_count) atomicAdd(bad_count, 1);
                } else if (id >= 0 && __builtin_isfinite(s) && src >= 0 && src < num_products) {
                    v[e] = s;
                    ix[e] = id;
                }
            }
        }
        // ---- the ban set: the sources, 64 at a time, and behind them their exclusion rows as one flat list (lp_ban_pass's text)
        if (source) {                                     // (uniform)
            for (int s0 = 0; s0 < S; s0 += 64) {
                int src = -1;
                if (s0 + lane < S) {
                    src = source[(size_t)b * S + s0 + lane];
                    if (src < -1 || src >= num_products) { // never used as an index; its row was dropped above
                        if (bad_count) atomicAdd(bad_count, 1);
                        src = -1;
                    }
                }
                int lo = 0, len = 0;
                if (ex_rowptr && src >= 0) {              // (src < num_products: rowptr has num_products + 1 entries)
                    lo = ex_rowptr[src];
                    len = max(ex_rowptr[src + 1] - lo, 0);
                }
                int inc = len;                            // the inclusive scan of the lanes' row lengths
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const int t = __shfl_up(inc, o, 64);
                    if (lane >= o) inc += t;
                }
                const int total = __shfl(inc, 63, 64);
                for (int base = 0; base < 64 + total; base += FL_CHUNK) {         // flat: 64 sources, then `total` row entries
#pragma unroll
                    for (int k = 0; k < FL_CHUNK / 64; k++) {
                        const int p = base + lane + 64 * k - 64;                  // the flat position among the row entries
                        int owner = 0;                    // the lanes whose rows end at or before p: the row that holds p
#pragma unroll
                        for (int step = 32; step >= 1; step >>= 1)
                            if (__shfl(inc, owner + step - 1, 64) <= p) owner += step;          // (owner + step - 1 <= 63)
                        const int o_inc = __shfl(inc, owner, 64), o_len = __shfl(len, owner, 64), o_lo = __shfl(lo, owner, 64);
                        int val = -1;                     // equal to no candidate's id
                        if (p < 0) val = src;             // (base 0, k 0: the lane's own source)
                        else if (p < total) val = ex_col[(size_t)o_lo + (p - (o_inc - o_len))];
                        lban[lane + 64 * k] = val;
                    }
                    // Same-wave LDS instructions execute in order: the lanes' stores are in LDS before any lane's read-back.
                    __builtin_amdgcn_wave_barrier();
                    const int nq = (min(FL_CHUNK, 64 + total - base) + 3) >> 2;
                    for (int q = 0; q < nq; q++) {
                        const fl_i32x4 x = *reinterpret_cast<const fl_i32x4*>(&lban[4 * q]);    // (a broadcast)
#pragma unroll
                        for (int t = 0; t < 4; t++)
#pragma unroll
                            for (int e = 0; e < NE; e++)
                                if (x[t] == ix[e]) { v[e] = -INFINITY; ix[e] = RG_NONE; }       // (x: -1 or a product id)
                    }
                    __builtin_amdgcn_wave_barrier();      // the reads are done before the next chunk's stores
                }
            }
        }
        // slot NE * lane + e: best first, the non-candidates last -- under the strict order of the scores' bits (rlw_key: +0.0
        // before -0.0), in which the slots of one product stand in one fixed order whatever the order they came in
        int key[NE];
#pragma unroll
        for (int e = 0; e < NE; e++) key[e] = rlw_key(v[e]);
        rlw_sort<NE>(key, ix, lane);
#pragma unroll
        for (int e = 0; e < NE; e++) v[e] = rlw_unkey(key[e]);
        int cnt = 0;                                      // the candidates: the positions below cnt
#pragma unroll
        for (int e = 0; e < NE; e++) cnt += __popcll(__ballot(ix[e] != RG_NONE));
        ivec wi;
        fvec ws;
#pragma unroll
        for (int e = 0; e < NE; e++) { wi[e] = ix[e]; ws[e] = v[e]; }
        *reinterpret_cast<ivec*>(&lid[NE * lane]) = wi;
        *reinterpret_cast<fvec*>(&lsc[NE * lane]) = ws;
        __builtin_amdgcn_wave_barrier();
        int c[NE], sup[NE];
#pragma unroll
        for (int e = 0; e < NE; e++) { c[e] = 0; sup[e] = 1; }
        if (combine == 0) fl_walk<NE, true>(lid, lsc, cnt, lane, ix, c, v, sup);              // (uniform)
        else fl_walk<NE, false>(lid, lsc, cnt, lane, ix, c, v, sup);
        __builtin_amdgcn_wave_barrier();                  // the reads are done before the next basket's stores
#pragma unroll
        for (int e = 0; e < NE; e++)
            if (c[e] != 0) { v[e] = -INFINITY; ix[e] = RG_NONE; }                             // not the head of its product
        // the heads under rg_better of their fused scores (distinct ids: a strict order), each with its support
        rlw_sort_with<NE>(v, ix, sup, lane);
        // ---- compaction: the heads' places, in serving order (lp_store_row's text)
        bool keep[NE];
        int mine = 0;
#pragma unroll
        for (int e = 0; e < NE; e++) {
            keep[e] = ix[e] != RG_NONE;
            mine += keep[e];
        }
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
                    out_idx[(size_t)b * n + pos] = ix[e];
                    out_score[(size_t)b * n + pos] = v[e];
                    out_support[(size_t)b * n + pos] = sup[e];
                }
                pos++;
            }
        }
        for (int k = kept + lane; k < n; k += 64) {
            out_idx[(size_t)b * n + k] = -1;
            out_score[(size_t)b * n + k] = -INFINITY;
            out_support[(size_t)b * n + k] = 0;
        }
    }
}

extern "C" int pc_fuse_lists(const int32_t* idx, const float* score, const int32_t* source, int baskets, int sources, int w,
                             const int32_t* ex_rowptr, const int32_t* ex_col, int num_products, int n, int combine,
                             int32_t* out_idx, float* out_score, int32_t* out_support, int32_t* bad_count, void* stream) {
    if (baskets < 0 || sources < 1 || w < 1 || (int64_t)sources * w > FUSE_LISTS_MAX_POOL) return PC_ESHAPE;
    const int m = sources * w;
    if (n < 1 || n > min(m, FL_MAX_N) || num_products < 1 || (combine != 0 && combine != 1)) return PC_ESHAPE;
    if ((ex_rowptr != nullptr) != (ex_col != nullptr) || (ex_rowptr && !source)) return PC_ESHAPE;      // the rows are the sources'
    if (baskets == 0) return PC_OK;                                       // nothing to serve: no launch, no pointer is read
    if (!idx || !score || !out_idx || !out_score || !out_support) return PC_ESHAPE;
    hipStream_t st = (hipStream_t)stream;
    const int wgs = baskets / FL_WAVES + (baskets % FL_WAVES != 0);
    const dim3 grid((unsigned)min(wgs, RG_MAX_GRID)), block(64 * FL_WAVES);
#define FL_GO(NE)                                                                                                            \
    PC_LAUNCH((fl_fuse_kernel<NE>), grid, block, 0, st, idx, score, source, ex_rowptr, ex_col, baskets, sources, w, num_products, \
              n, combine, out_idx, out_score, out_support, bad_count)
    if (m <= 128) FL_GO(2);
    else if (m <= 256) FL_GO(4);
    else if (m <= 512) FL_GO(8);
    else FL_GO(16);
#undef FL_GO
    return pc_launch_status();
}
