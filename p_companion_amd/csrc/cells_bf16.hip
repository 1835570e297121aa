// The centroid update of a Lloyd iteration over the bf16 copy of the catalogue (pc_cell_means_bf16; ops.build_cell_index_bf16,
// inference.IndexedCompactSimilarProducts): cl_means_kernel (cells.hip) reading a [P, D] bf16 table.  A unit of its own, as
// nearest_list_bf16.hip: inside cells.hip the new kernels would move the existing ones.
//
//   means    cl_means_bf16_kernel: one workgroup per cell (grid-stride over the cells).  The 256 threads form G = 1024 / D groups
//            of D / 4 lanes; lane c of a group owns the columns 4 c .. 4 c + 3 of a row -- cl_means_kernel's ownership; here
//            ONE 8-byte load of four bf16 patterns, widened (exactly: the pattern in the high half of the word) to a float4.
//            Group g takes the members g, g + G, g + 2 G, .. of the cell, four in flight, added one after the other in that
//            order into one fp32 float4, starting from zero.  The G sums meet in LDS in a tree over the group distances G / 2,
//            .., 1 (group g += group g + o), and group 0 divides once by the count.
//
// Determinism and the fp32 kernel's bits: which lane owns a column, which group adds a member and when, the tree and the one
// division are cl_means_kernel's, and the widening is exact -- every addition is the same fp32 addition of the same operands.
// centroids are bit for bit pc_cell_means' on the widened table, which is never formed.  (16-byte loads of 8 columns per lane
// would halve the lanes of a group, double G and change the order of the sums.)  No atomics of any kind.
#include "common.h"

#define CLB_MAX_GRID 65536

__device__ __forceinline__ float4 clb_add(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// the columns 4 c .. 4 c + 3 of product id's row as a float4, counted in m; +0 for an id out of range (not read)
template <int D>
__device__ __forceinline__ float4 clb_row(const uint16_t* __restrict__ table, int id, int num_products, int c, int& m) {
    const bool ok = id >= 0 && id < num_products;
    m += ok ? 1 : 0;
    if (!ok) return make_float4(0.f, 0.f, 0.f, 0.f);
    const uint2 z = reinterpret_cast<const uint2*>(table + (size_t)id * D)[c];
    // (element 2 i of a 32-bit word is its low half: bf16 -> fp32 is the pattern in the high half)
    return make_float4(__builtin_bit_cast(float, z.x << 16), __builtin_bit_cast(float, z.x & 0xffff0000u),
                       __builtin_bit_cast(float, z.y << 16), __builtin_bit_cast(float, z.y & 0xffff0000u));
}

// centroids[c] = (sum of widened table[cell_col[i]], i in [cell_rowptr[c], cell_rowptr[c + 1])) / m_c; m_c counts the ids
// inside [0, num_products) -- an id outside is passed over: not read, not summed, not counted.  m_c == 0: the centroid keeps
// its bits.
template <int D>
__global__ __launch_bounds__(256) void cl_means_bf16_kernel(const uint16_t* __restrict__ table,
                                                            const int32_t* __restrict__ cell_rowptr,
                                                            const int32_t* __restrict__ cell_col, int n_cells, int num_products,
                                                            float* __restrict__ centroids) {
    constexpr int C4 = D / 4;                // four-column pieces per row = lanes per group
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
            for (int k = 0; k < 4; k++) x[k] = clb_row<D>(table, id[k], num_products, c, m);
#pragma unroll
            for (int k = 0; k < 4; k++) acc = clb_add(acc, x[k]);
        }
        for (; i < hi; i += G) acc = clb_add(acc, clb_row<D>(table, cell_col[i], num_products, c, m));
        __syncthreads();                                  // the previous cell's readers of red / cnt are done
        red[g][c] = acc;
        if (c == 0) cnt[g] = m;
        __syncthreads();
#pragma unroll
        for (int o = G / 2; o >= 1; o >>= 1) {
            if (g < o) red[g][c] = clb_add(red[g][c], red[g + o][c]);
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

extern "C" int pc_cell_means_bf16(const void* table, const int32_t* cell_rowptr, const int32_t* cell_col, int n_cells,
                                  int num_products, int dim, float* centroids, void* stream) {
    if (!table || !cell_rowptr || !cell_col || !centroids || n_cells <= 0 || num_products <= 0) return PC_EINVAL;
    if (dim != 128 && dim != 256) return PC_ESHAPE;
    if (((uintptr_t)table & 7) || ((uintptr_t)centroids & 15)) return PC_ESHAPE;      // 8-byte loads, 16-byte stores
    hipStream_t st = (hipStream_t)stream;
    const uint16_t* rows = (const uint16_t*)table;
    const dim3 grid((unsigned)min(n_cells, CLB_MAX_GRID));
    if (dim == 128) PC_LAUNCH(cl_means_bf16_kernel<128>, grid, dim3(256), 0, st, rows, cell_rowptr, cell_col, n_cells, num_products, centroids);
    else PC_LAUNCH(cl_means_bf16_kernel<256>, grid, dim3(256), 0, st, rows, cell_rowptr, cell_col, n_cells, num_products, centroids);
    return pc_launch_status();
}
