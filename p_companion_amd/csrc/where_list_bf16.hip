// Long lists under a per-query predicate on per-product attributes, from the bf16 copy of the catalogue:
// pc_retrieve_list_grouped_bf16_where and, under a per-product additive term on the score,
// pc_retrieve_list_grouped_bf16_biased_where -- where_list.hip's contract and predicate over a [P, D] bf16 table
// (PCompanionInference.recommend_where_batch with an ops.CompactCatalogue; CompactSimilarProducts.similar_where_batch).  The
// kernel's body, the merge and the host path are grouped_list.h's and retrieve_list.hip's as they are: this unit is two more
// instantiations of the body over grouped_list_bf16.h's chain, with its WHERE hook (value[pid] and flags[pid] staged in LDS per
// chunk column, the test between the threshold and the exclusion bisection).  A unit of its own, as nearest_list_bf16.hip.
//
// Determinism: the predicate reads no score: a (row, product) score has the bits of pc_retrieve_list_grouped_bf16 /
// pc_retrieve_list_grouped_bf16_biased, and a product that fails is dropped where an excluded product is dropped.  The output
// is the existing entry's over a CSR of the passing products, bit for bit, whatever the slices, the rows' places, the order of
// type_col or the arrival order in a buffer; with every array absent it is the existing entry's output.  No float atomics, no
// readback.
#include "common.h"
#include "grouped_list_bf16.h"

template <int D, int NE, bool EX>
__global__ __launch_bounds__(256) void wlb_score_kernel(RL_SCORE_PARAMS(uint16_t), RlWhere where) {
    rl_score_body<RlChainBf16<D>, NE, EX, false, true>(RL_SCORE_ARGS, nullptr, where);
}

template <int D, int NE, bool EX>
__global__ __launch_bounds__(256) void wlb_score_biased_kernel(RL_SCORE_PARAMS(uint16_t), const float* __restrict__ bias,
                                                               RlWhere where) {
    rl_score_body<RlChainBf16<D>, NE, EX, true, true>(RL_SCORE_ARGS, bias, where);
}

struct WlbKernels {
    template <int D, int NE, bool EX>
    static constexpr auto kernel() { return wlb_score_kernel<D, NE, EX>; }
};

struct WlbBiasedKernels {
    template <int D, int NE, bool EX>
    static constexpr auto kernel() { return wlb_score_biased_kernel<D, NE, EX>; }
};

extern "C" size_t pc_retrieve_list_grouped_bf16_where_workspace_bytes(int rows, int n_types, int n, int slices) {
    return rg_topn_workspace_bytes(rows, n_types, n, RL_MAX_N, slices);
}

extern "C" int pc_retrieve_list_grouped_bf16_where(const float* proj, const int32_t* types, const int32_t* row_key, int rows,
                                                   const int32_t* type_rowptr, const int32_t* type_col,
                                                   const uint16_t* table_bf16, int n_types, const int32_t* ex_rowptr,
                                                   const int32_t* ex_col, int n_keys, int n, int dim, int slices, int32_t* out_idx,
                                                   float* out_score, int32_t* bad_count, const pc_row_where* where, void* ws,
                                                   size_t ws_bytes, void* stream) {
    if (!where) return PC_EINVAL;
    // (rl_list_entry: the bf16 entry's 16-byte alignment refusal goes with the table's element type)
    return rl_list_entry<WlbKernels>(proj, types, row_key, rows, type_rowptr, type_col, table_bf16, n_types, ex_rowptr, ex_col,
                                     n_keys, n, dim, slices, out_idx, out_score, bad_count, ws, ws_bytes, stream, RlWhere{*where});
}

extern "C" size_t pc_retrieve_list_grouped_bf16_biased_where_workspace_bytes(int rows, int n_types, int n, int slices) {
    return rg_topn_workspace_bytes(rows, n_types, n, RL_MAX_N, slices);
}

extern "C" int pc_retrieve_list_grouped_bf16_biased_where(const float* proj, const int32_t* types, const int32_t* row_key,
                                                          int rows, const int32_t* type_rowptr, const int32_t* type_col,
                                                          const uint16_t* table_bf16, const float* bias, int n_types,
                                                          const int32_t* ex_rowptr, const int32_t* ex_col, int n_keys, int n,
                                                          int dim, int slices, int32_t* out_idx, float* out_score,
                                                          int32_t* bad_count, const pc_row_where* where, void* ws,
                                                          size_t ws_bytes, void* stream) {
    if (!where) return PC_EINVAL;
    return rl_list_entry<WlbBiasedKernels>(proj, types, row_key, rows, type_rowptr, type_col, table_bf16, n_types, ex_rowptr,
                                           ex_col, n_keys, n, dim, slices, out_idx, out_score, bad_count, ws, ws_bytes, stream,
                                           bias, RlWhere{*where});
}
