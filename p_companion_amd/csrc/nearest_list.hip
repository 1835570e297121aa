// Long substitute lists: the first n <= 256 products of a type per (query, type) row over the fp32 table under a per-product
// additive term on the score (pc_retrieve_list_grouped_biased; SimilarProducts.similar_list_batch in inference.py):
//   s(r, p) = fl(d(r, p) + bias[p]),   d(r, p) = RlChainF32 (grouped_list_f32.h),
// pc_retrieve_list_grouped's contract with nearest.hip's score.  The kernel's body -- plan, work items, chunks, the per-row
// LDS buffers with their threshold, the compactions --, the merge and the host path are grouped_list.h's and
// retrieve_list.hip's as they are; the body's BIAS hook gathers bias[pid] a chunk ahead and adds it to the lane's four
// accumulator registers before they go to LDS: ONE fp32 addition after the chain, the accumulator starts at zero, never at
// the bias.  A unit of its own, as nearest.hip: inside retrieve_list.hip the new kernels would move the existing ones.
//
// Determinism: d is rl_score_kernel's chain (step j, element e, k-lane h cover dimension 16 j + 4 h + e), which has rk_chain's
// bits, and the bias is a function of the product: a (row, product) score has the same bits in any tile, slice or column,
// here, in nb_score_kernel and in both biased rank kernels.  The selection is the family's, under the total order (score
// descending, product index ascending): the output does not depend on the slices, the rows' places, the order of type_col or
// the arrival order in a buffer.  For n <= 16 it is pc_retrieve_topk_grouped_biased's bit for bit, with a zero bias
// pc_retrieve_list_grouped's, and pc_rank_grouped_biased's rank < n exactly when the list holds the target at position rank.
// No float atomics, no readback.
#include "common.h"
#include "grouped_list_f32.h"

template <int D, int NE, bool EX>
__global__ __launch_bounds__(256) void nl_score_kernel(RL_SCORE_PARAMS(float), const float* __restrict__ bias) {
    rl_score_body<RlChainF32<D>, NE, EX, true>(RL_SCORE_ARGS, bias);
}

struct NlKernels {
    template <int D, int NE, bool EX>
    static constexpr auto kernel() { return nl_score_kernel<D, NE, EX>; }
};

extern "C" size_t pc_retrieve_list_grouped_biased_workspace_bytes(int rows, int n_types, int n, int slices) {
    return rg_topn_workspace_bytes(rows, n_types, n, RL_MAX_N, slices);
}

extern "C" int pc_retrieve_list_grouped_biased(const float* proj, const int32_t* types, const int32_t* row_key, int rows,
                                               const int32_t* type_rowptr, const int32_t* type_col, const float* table,
                                               const float* bias, int n_types, const int32_t* ex_rowptr, const int32_t* ex_col,
                                               int n_keys, int n, int dim, int slices, int32_t* out_idx, float* out_score,
                                               int32_t* bad_count, void* ws, size_t ws_bytes, void* stream) {
    return rl_list_entry<NlKernels>(proj, types, row_key, rows, type_rowptr, type_col, table, n_types, ex_rowptr, ex_col, n_keys, n,
                                    dim, slices, out_idx, out_score, bad_count, ws, ws_bytes, stream, bias);
}
