// Group caps and the merged page: a post-pass over the served pools (pc_cap_lists; ops.cap_lists,
// PCompanionInference.recommend_capped_batch / recommend_page_batch, SimilarProducts.similar_capped_batch).  The pool of a row
// is what the grouped retrievals return -- idx / score [rows][m], m <= 256, in any order, -1 ids and non-finite scores
// anywhere --, or several such lists side by side.  The output is the first n <= m candidates under rg_better (score
// descending, product index ascending) of which no more than `cap` belong to one product group, each with its INPUT score bits.
//
//   candidate    a slot whose id lies in [0, num_products) and whose score is finite, and whose group is not the row's banned
//                group.  An id outside [-1, num_products) is never used as an index and is counted (one integer atomic).
//   rule         a grouped candidate is kept iff fewer than `cap` candidates of its group stand in front of it under the total
//                order; an ungrouped one (group[p] < 0, or no group array) always.
//   kernel       one wave per row, four rows per workgroup, grid-stride over rows; the waves of a workgroup never meet (no
//                workgroup barrier: every wave has its own LDS row).  The slots go into NE registers per lane, non-candidates
//                as (-inf, RG_NONE) so that a NaN never reaches a comparison, and through rl_sort<NE> (wave_sort.h): slot
//                NE lane + e is then in serving order.  group[id] is gathered for the real slots alone, the wave's groups go to
//                LDS, and every lane walks them as 16-byte broadcast reads, counting for each of its slots the earlier slots of
//                the same group: m / 4 reads and NE m integer compares per lane.  lp_store_row (list_pool.h) compacts and
//                stores the kept slots with the -1 / -inf tail.
//   variants     NE = 2 (m <= 128) and NE = 4 (m <= 256).  Both sort under one total order in which equal keys are equal slots
//                (same id, same score bits up to the sign of zero, see below), so the bits do not depend on the variant.
// Integer compares and float compares only: no workspace, no float atomics, nothing read back; the result does not depend on
// the grid or the run.  Two slots equal in (score, id) -- duplicate ids, outside the contract, or +0.0 / -0.0 under one id --
// are served in an unspecified order; with distinct ids every comparison is strict and every output bit is determined.
#include "common.h"
#include "list_pool.h"             // lp_store_row, lp_i32x4
#include "wave_sort.h"             // rl_sort; grouped_plan.h: rg_better, RG_NONE, RG_MAX_GRID

#define CL_MAX_POOL 256
#define CL_ROWS_PER_WG 4           // one wave each

template <int NE>
__global__ __launch_bounds__(64 * CL_ROWS_PER_WG) void cl_cap_kernel(const int32_t* __restrict__ idx,
                                                                     const float* __restrict__ score, int rows, int m,
                                                                     const int32_t* __restrict__ group,
                                                                     const int32_t* __restrict__ row_ban, int num_products,
                                                                     int n, int cap, int32_t* __restrict__ out_idx,
                                                                     float* __restrict__ out_score,
                                                                     int32_t* __restrict__ bad_count) {
    typedef int ivec __attribute__((ext_vector_type(NE)));
    __shared__ __attribute__((aligned(16))) int lg[CL_ROWS_PER_WG][64 * NE];     // a wave's groups in serving order
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int* wg = lg[wave];
    const int64_t stride = (int64_t)gridDim.x * CL_ROWS_PER_WG;
    for (int64_t r = (int64_t)blockIdx.x * CL_ROWS_PER_WG + wave; r < rows; r += stride) {      // (wave-uniform)
        // ---- the row's slots, lane-interleaved for the load (any order serves: the sort follows)
        float v[NE];
        int ix[NE];
#pragma unroll
        for (int e = 0; e < NE; e++) {
            const int j = lane + 64 * e;
            v[e] = -INFINITY;
            ix[e] = RG_NONE;
            if (j < m) {
                const int id = idx[(size_t)r * m + j];
                const float s = score[(size_t)r * m + j];
                if (id < -1 || id >= num_products) {      // never used as an index
                    if (bad_count) atomicAdd(bad_count, 1);
                } else if (id >= 0 && __builtin_isfinite(s)) {
                    v[e] = s;
                    ix[e] = id;
                }
            }
        }
        rl_sort<NE>(v, ix, lane);                         // slot NE * lane + e: best first, the non-candidates last
        bool keep[NE];
#pragma unroll
        for (int e = 0; e < NE; e++) keep[e] = ix[e] != RG_NONE;
        if (group) {                                      // (uniform)
            const int ban = row_ban ? row_ban[r] : -1;
            ivec g;                                       // -1: ungrouped, banned or no candidate -- equal to nothing below
#pragma unroll
            for (int e = 0; e < NE; e++) {
                g[e] = -1;
                if (keep[e]) {                            // (ix[e] is in [0, num_products): checked at the load)
                    const int x = group[ix[e]];
                    if (x >= 0 && x == ban) keep[e] = false;
                    else if (x >= 0) g[e] = x;
                }
            }
            // Same-wave LDS instructions execute in order: the lanes' stores are in LDS before any lane's read-back.
            *reinterpret_cast<ivec*>(&wg[NE * lane]) = g;
            __builtin_amdgcn_wave_barrier();
            int c[NE];
#pragma unroll
            for (int e = 0; e < NE; e++) c[e] = 0;
            const int nq = (m + 3) >> 2;                  // (<= 16 NE: inside the wave's row, every entry of which is written)
            for (int q = 0; q < nq; q++) {
                const lp_i32x4 x = *reinterpret_cast<const lp_i32x4*>(&wg[4 * q]);  // (one address per wave: a broadcast)
#pragma unroll
                for (int t = 0; t < 4; t++)
#pragma unroll
                    for (int e = 0; e < NE; e++) c[e] += (4 * q + t < NE * lane + e) & (x[t] == g[e]);
            }
            __builtin_amdgcn_wave_barrier();              // the reads are done before the next row's stores
#pragma unroll
            for (int e = 0; e < NE; e++)
                if (g[e] >= 0 && c[e] >= cap) keep[e] = false;
        }
        // ---- compaction and store (list_pool.h): the kept slots' places, in serving order; no support column (ix stands in)
        lp_store_row<NE, false>(keep, ix, v, ix, lane, n, (size_t)r * n, out_idx, out_score, nullptr);
    }
}

extern "C" int pc_cap_lists(const int32_t* idx, const float* score, int rows, int m, const int32_t* group, const int32_t* row_ban,
                            int num_products, int n, int cap, int32_t* out_idx, float* out_score, int32_t* bad_count,
                            void* stream) {
    if (rows < 0 || m < 1 || m > CL_MAX_POOL || n < 1 || n > m || cap < 1 || num_products < 1) return PC_ESHAPE;
    if (row_ban && !group) return PC_ESHAPE;                              // a ban names a group
    if (rows == 0) return PC_OK;                                          // nothing to serve: no launch, no pointer is read
    if (!idx || !score || !out_idx || !out_score) return PC_ESHAPE;
    hipStream_t st = (hipStream_t)stream;
    const int wgs = rows / CL_ROWS_PER_WG + (rows % CL_ROWS_PER_WG != 0);
    const dim3 grid((unsigned)min(wgs, RG_MAX_GRID));
    if (m <= 128)
        PC_LAUNCH((cl_cap_kernel<2>), grid, dim3(64 * CL_ROWS_PER_WG), 0, st, idx, score, rows, m, group, row_ban, num_products, n,
                  cap, out_idx, out_score, bad_count);
    else
        PC_LAUNCH((cl_cap_kernel<4>), grid, dim3(64 * CL_ROWS_PER_WG), 0, st, idx, score, rows, m, group, row_ban, num_products, n,
                  cap, out_idx, out_score, bad_count);
    return pc_launch_status();
}
