// Substitute lists from the bf16 copy of the catalogue alone: the first n <= 256 products of a type per (query, type) row over
// a [P, D] bf16 table under a per-product additive term on the score (pc_retrieve_list_grouped_bf16_biased;
// CompactSimilarProducts in inference.py), and the term that makes the order Euclidean over the stored rows
// (pc_half_sq_norm_bias_bf16):
//   s(r, p) = fl(d(r, p) + bias[p]),   d(r, p) = RlChainBf16 (grouped_list_bf16.h),
// pc_retrieve_list_grouped_bf16's contract with nearest_list.hip's score.  The kernel's body, the merge and the host path are
// grouped_list.h's and retrieve_list.hip's as they are: this unit is one more instantiation of the body, with its BIAS hook
// (bias[pid] gathered a chunk ahead, ONE fp32 addition behind the chain, the accumulator starts at zero).  The entry serves
// every n from 1: at n <= 16 the bf16 list kernel costs what the 16-entry bf16 kernel costs, so there is no 16-entry biased
// bf16 kernel.  A unit of its own, as nearest_list.hip: inside retrieve_list_bf16.hip the new kernels would move the existing
// ones.
//
// Determinism: d is rl_score_bf16_kernel's chain (k-block ascending, inside a k-block the pieces p0, p1, p2 of the query, one
// v_mfma_f32_16x16x32_bf16 each into one accumulator) and the bias is a function of the product: a (row, product) score has
// the same bits in any tile, slice or column, here and in both bf16 rank kernels (rank_bf16.hip).  The selection is the
// family's, under the total order (score descending, product index ascending): the output does not depend on the slices, the
// rows' places, the order of type_col or the arrival order in a buffer.  With a zero bias it is pc_retrieve_list_grouped_bf16's
// bit for bit, and pc_rank_grouped_bf16 (same bias, same lists) is < n exactly when the list holds the target at that position.
// No float atomics, no readback.
#include "common.h"
#include "grouped_list_bf16.h"

template <int D, int NE, bool EX>
__global__ __launch_bounds__(256) void nlb_score_kernel(RL_SCORE_PARAMS(uint16_t), const float* __restrict__ bias) {
    rl_score_body<RlChainBf16<D>, NE, EX, true>(RL_SCORE_ARGS, bias);
}

struct NlbKernels {
    template <int D, int NE, bool EX>
    static constexpr auto kernel() { return nlb_score_kernel<D, NE, EX>; }
};

extern "C" size_t pc_retrieve_list_grouped_bf16_biased_workspace_bytes(int rows, int n_types, int n, int slices) {
    return rg_topn_workspace_bytes(rows, n_types, n, RL_MAX_N, slices);
}

extern "C" int pc_retrieve_list_grouped_bf16_biased(const float* proj, const int32_t* types, const int32_t* row_key, int rows,
                                                    const int32_t* type_rowptr, const int32_t* type_col,
                                                    const uint16_t* table_bf16, const float* bias, int n_types,
                                                    const int32_t* ex_rowptr, const int32_t* ex_col, int n_keys, int n, int dim,
                                                    int slices, int32_t* out_idx, float* out_score, int32_t* bad_count, void* ws,
                                                    size_t ws_bytes, void* stream) {
    // (rl_list_entry: the bf16 entry's 16-byte alignment refusal goes with the table's element type)
    return rl_list_entry<NlbKernels>(proj, types, row_key, rows, type_rowptr, type_col, table_bf16, n_types, ex_rowptr, ex_col,
                                     n_keys, n, dim, slices, out_idx, out_score, bad_count, ws, ws_bytes, stream, bias);
}

// out[p] = -0.5f * sum_d e[p][d]^2 over the stored rows.  nb_half_sq_norm_kernel's sum (nearest.hip), restated: a group of 16
// lanes owns a row; lane l of the group adds, in this order, the squares of the dimensions 4 l + 64 j + e (j ascending, e
// ascending) into one fp32 sum by fused multiply-add, starting from zero; the 16 sums meet in a butterfly over the lane
// distances 8, 4, 2, 1.  The four dimensions are 8 bytes of bf16 patterns, widened (exactly) before the sum, so a row's value is
// bit for bit pc_half_sq_norm_bias's on the widened table -- which is never formed.  No atomics; a row's value does not depend
// on the grid.
template <int D>
__global__ __launch_bounds__(256) void nlb_half_sq_norm_kernel(const uint16_t* __restrict__ table, int rows,
                                                               float* __restrict__ out) {
    const int l = threadIdx.x & 15;
    const int64_t stride = (int64_t)gridDim.x * 16;
    for (int64_t p = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4); p < rows; p += stride) {
        const uint2* f = reinterpret_cast<const uint2*>(table + (size_t)p * D) + l;
        uint2 z[D / 64];
#pragma unroll
        for (int j = 0; j < D / 64; j++) z[j] = f[16 * j];
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < D / 64; j++) {
            // (element 2 i of a 32-bit word is its low half: bf16 -> fp32 is the pattern in the high half)
            const float x0 = __builtin_bit_cast(float, z[j].x << 16), x1 = __builtin_bit_cast(float, z[j].x & 0xffff0000u);
            const float x2 = __builtin_bit_cast(float, z[j].y << 16), x3 = __builtin_bit_cast(float, z[j].y & 0xffff0000u);
            s = __builtin_fmaf(x0, x0, s);
            s = __builtin_fmaf(x1, x1, s);
            s = __builtin_fmaf(x2, x2, s);
            s = __builtin_fmaf(x3, x3, s);
        }
        // (a group's 16 lanes run the same number of iterations: p depends on threadIdx.x >> 4 alone)
#pragma unroll
        for (int o = 8; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
        if (l == 0) out[p] = -0.5f * s;
    }
}

extern "C" int pc_half_sq_norm_bias_bf16(const uint16_t* table_bf16, int rows, int dim, float* out, void* stream) {
    if (!table_bf16 || !out || rows <= 0) return PC_EINVAL;
    if ((dim != 128 && dim != 256) || ((uintptr_t)table_bf16 & 7)) return PC_ESHAPE;      // a lane reads 8 bytes of a row at once
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)min((rows + 15) / 16, RG_MAX_GRID));        // 16 rows per workgroup and pass, grid-stride
    if (dim == 128) PC_LAUNCH(nlb_half_sq_norm_kernel<128>, grid, dim3(256), 0, st, table_bf16, rows, out);
    else PC_LAUNCH(nlb_half_sq_norm_kernel<256>, grid, dim3(256), 0, st, table_bf16, rows, out);
    return pc_launch_status();
}
