// The two kernels of the k-means cell index (ops.build_cell_index, inference.IndexedSimilarProducts) that the grouped retrieval
// does not already provide: the centroid update of a Lloyd iteration (pc_cell_means) and the merge of one row's probe lists
// (pc_merge_lists).  The assignment step and the search inside the probed cells are pc_retrieve_topk_grouped_biased as it is
// (nearest.hip): a cell is a "type", a centroid or a product a candidate.
//
//   means    cl_means_kernel: one workgroup per cell (grid-stride over the cells).  The 256 threads form G = 1024 / D groups of
//            D / 4 lanes; lane c of a group owns the float4 c of a row (16-byte loads), group g the members g, g + G, g + 2 G, ..
//            of the cell, added one after the other in that order into one fp32 float4, starting from zero.  The G sums meet in
//            LDS in a tree over the group distances G / 2, .., 1 (group g += group g + o), and group 0 divides by the count.
//   merge    cl_merge_kernel: rl_merge_kernel's loop (retrieve_list.hip) without the plan: one wave per row, lane l a cursor
//            into list l, n rounds of a wave-wide best head under rg_better.
//
// Determinism: the sum of a cell and dimension is a fixed expression of the members' positions in the cell -- which group adds
// a member, and when, depends on its position and on D alone, never on the grid, on the block that serves the cell or on other
// cells.  No atomics of any kind in the means; the merge is comparisons and copies.
#include "common.h"
#include "grouped_plan.h"          // rg_better, RG_NONE

#define CL_MAX_LISTS 64
#define CL_MAX_N 256
#define CL_MAX_GRID 65536

__device__ __forceinline__ float4 cl_add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// float4 c of product id's row, counted in m; +0 for an id out of range
template <int D>
__device__ __forceinline__ float4 cl_row(const float* __restrict__ table, int id, int num_products, int c, int& m) {
    const bool ok = id >= 0 && id < num_products;
    m += ok ? 1 : 0;
    return ok ? reinterpret_cast<const float4*>(table + (size_t)id * D)[c] : make_float4(0.f, 0.f, 0.f, 0.f);
}

// centroids[c] = (sum of table[cell_col[i]], i in [cell_rowptr[c], cell_rowptr[c + 1])) / m_c; m_c counts the ids inside
// [0, num_products) -- an id outside is passed over: not read, not summed, not counted.  m_c == 0: the centroid keeps its bits.
template <int D>
__global__ __launch_bounds__(256) void cl_means_kernel(const float* __restrict__ table, const int32_t* __restrict__ cell_rowptr,
                                                       const int32_t* __restrict__ cell_col, int n_cells, int num_products,
                                                       float* __restrict__ centroids) {
    constexpr int C4 = D / 4;                // float4s per row = lanes per group
    constexpr int G = 256 / C4;              // groups: 8 (D = 128) or 4 (D = 256)
    __shared__ float4 red[G][C4];
    __shared__ int cnt[G];
    const int tid = threadIdx.x, c = tid % C4, g = tid / C4;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    // member i's row, or +0 for an id out of range (acc + 0 keeps acc's bits: acc starts at +0 and a sum is -0 only where both
    // terms are, so acc is never -0); the count decides whether anything is written
    for (int cell = blockIdx.x; cell < n_cells; cell += gridDim.x) {
        const int lo = cell_rowptr[cell], hi = cell_rowptr[cell + 1];
        float4 acc = zero;
        int m = 0;
        int i = lo + g;
        // four members in flight; the additions stay in the order of i
        for (; (int64_t)i + 3 * G < hi; i += 4 * G) {
            int id[4];
            float4 x[4];
#pragma unroll
            for (int k = 0; k < 4; k++) id[k] = cell_col[i + k * G];
#pragma unroll
            for (int k = 0; k < 4; k++) x[k] = cl_row<D>(table, id[k], num_products, c, m);
#pragma unroll
            for (int k = 0; k < 4; k++) acc = cl_add(acc, x[k]);
        }
        for (; i < hi; i += G) acc = cl_add(acc, cl_row<D>(table, cell_col[i], num_products, c, m));
        __syncthreads();                                  // the previous cell's readers of red / cnt are done
        red[g][c] = acc;
        if (c == 0) cnt[g] = m;
        __syncthreads();
#pragma unroll
        for (int o = G / 2; o >= 1; o >>= 1) {
            if (g < o) red[g][c] = cl_add(red[g][c], red[g + o][c]);
            __syncthreads();
        }
        if (g == 0) {
            int total = 0;
#pragma unroll
            for (int k = 0; k < G; k++) total += cnt[k];
            if (total > 0) {
                const float4 s = red[0][c];
                const float mf = (float)total;
                reinterpret_cast<float4*>(centroids + (size_t)cell * D)[c] = make_float4(s.x / mf, s.y / mf, s.z / mf, s.w / mf);
            }
        }
    }
}

// One wave per row: lane l walks list l (idx / score [rows][L][n], sorted under rg_better, -1 / -inf behind its last entry);
// every round the best head is the next entry of the row and its lane moves on (the lists of a row hold disjoint products: one
// lane).  Results are gathered 64 at a time and stored as a row of the wave; -1 / -inf once every list is used up.
__global__ __launch_bounds__(256) void cl_merge_kernel(const int32_t* __restrict__ idx, const float* __restrict__ score, int rows,
                                                       int L, int n, int32_t* __restrict__ out_idx,
                                                       float* __restrict__ out_score) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;                                // wave-uniform
    const size_t mine = ((size_t)r * L + lane) * n;       // this lane's list (read only where lane < L)
    int pos = 0;
    float hv = -INFINITY;
    int hi = RG_NONE;
    auto head = [&]() {
        hv = -INFINITY; hi = RG_NONE;
        if (pos < n) {
            const int xi = idx[mine + pos];
            if (xi >= 0) { hi = xi; hv = score[mine + pos]; }
            else pos = n;                                 // the list's end
        }
    };
    if (lane < L) head();
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
        if (hi == bi && bi != RG_NONE) {
            pos++;
            head();
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

extern "C" int pc_cell_means(const float* table, const int32_t* cell_rowptr, const int32_t* cell_col, int n_cells,
                             int num_products, int dim, float* centroids, void* stream) {
    if (!table || !cell_rowptr || !cell_col || !centroids || n_cells <= 0 || num_products <= 0) return PC_EINVAL;
    if (dim != 128 && dim != 256) return PC_ESHAPE;
    if (((uintptr_t)table | (uintptr_t)centroids) & 15) return PC_ESHAPE;             // 16-byte loads and stores
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)min(n_cells, CL_MAX_GRID));
    if (dim == 128) PC_LAUNCH(cl_means_kernel<128>, grid, dim3(256), 0, st, table, cell_rowptr, cell_col, n_cells, num_products, centroids);
    else PC_LAUNCH(cl_means_kernel<256>, grid, dim3(256), 0, st, table, cell_rowptr, cell_col, n_cells, num_products, centroids);
    return pc_launch_status();
}

extern "C" int pc_merge_lists(const int32_t* idx, const float* score, int rows, int L, int n, int32_t* out_idx, float* out_score,
                              void* stream) {
    if (!idx || !score || !out_idx || !out_score || rows <= 0) return PC_EINVAL;
    if (L < 1 || L > CL_MAX_LISTS || n < 1 || n > CL_MAX_N) return PC_ESHAPE;
    PC_LAUNCH(cl_merge_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, idx, score, rows, L, n,
              out_idx, out_score);
    return pc_launch_status();
}
