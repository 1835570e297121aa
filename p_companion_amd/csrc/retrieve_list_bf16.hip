// Long complement lists from the bf16 copy of the catalogue: the first n <= 256 products of a type per (query, type) row over
// a [P, D] bf16 table (pc_retrieve_list_grouped_bf16; PCompanionInference with an ops.CompactCatalogue, recommend_batch above
// 16).  The kernel's body and the host path are grouped_list.h's, the merge is rl_merge_kernel (retrieve_list.hip) through
// rl_merge_launch, the bf16 score chain grouped_list_bf16.h's; here are the kernels under their names and the entries.
//
// Determinism: the chain of a (row, product) pair is k-block 0 .. D / 32 - 1, inside a k-block the pieces p0, p1, p2, one
// v_mfma_f32_16x16x32_bf16 each into ONE accumulator, inside an MFMA k-lane h and element e cover dimension 32 k + 8 h + e: its
// order depends on the dimension index and the piece alone, so a (row, product) pair has the bits
// pc_retrieve_topk_grouped_bf16 gives it.  The order in which survivors arrive in a buffer is decided by an integer LDS
// atomic and is free: every selection that follows is under the total order (score descending, product index ascending), and
// the threshold only ever drops candidates that n kept products of the row beat.  An excluded product never enters a buffer,
// so it never moves a threshold.  Hence the output does not depend on the slices, the rows' places, the order of type_col or
// the arrival order; for n <= 16 it is pc_retrieve_topk_grouped_bf16's bit for bit.  No float atomics, nothing read back.
#include "common.h"
#include "grouped_list_bf16.h"     // RlChainBf16: the bf16 score chain (nearest_list_bf16.hip scores through it too)

template <int D, int NE, bool EX>
__global__ __launch_bounds__(256) void rl_score_bf16_kernel(RL_SCORE_PARAMS(uint16_t)) {
    rl_score_body<RlChainBf16<D>, NE, EX>(RL_SCORE_ARGS);
}

struct RlKernelsBf16 {
    template <int D, int NE, bool EX>
    static constexpr auto kernel() { return rl_score_bf16_kernel<D, NE, EX>; }
};

extern "C" size_t pc_retrieve_list_grouped_bf16_workspace_bytes(int rows, int n_types, int n, int slices) {
    return rg_topn_workspace_bytes(rows, n_types, n, RL_MAX_N, slices);
}

extern "C" int pc_retrieve_list_grouped_bf16(const float* proj, const int32_t* types, const int32_t* row_key, int rows,
                                             const int32_t* type_rowptr, const int32_t* type_col, const uint16_t* table_bf16,
                                             int n_types, const int32_t* ex_rowptr, const int32_t* ex_col, int n_keys, int n,
                                             int dim, int slices, int32_t* out_idx, float* out_score, int32_t* bad_count,
                                             void* ws, size_t ws_bytes, void* stream) {
    return rl_list_entry<RlKernelsBf16>(proj, types, row_key, rows, type_rowptr, type_col, table_bf16, n_types, ex_rowptr, ex_col,
                                        n_keys, n, dim, slices, out_idx, out_score, bad_count, ws, ws_bytes, stream);
}
