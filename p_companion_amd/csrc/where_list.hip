// Long lists under a per-query predicate on per-product attributes, over the fp32 table: the first n <= 256 products of a type
// per (query, type) row that pass the row's price band and flag masks (pc_retrieve_list_grouped_where and, under a per-product
// additive term on the score, pc_retrieve_list_grouped_biased_where; ops.retrieve_list_grouped_where,
// PCompanionInference.recommend_where_batch and SimilarProducts.similar_where_batch in inference.py):
//   product p passes row r  iff  lo[r] <= value[p] && value[p] <= hi[r]                          (two fp32 compares, ends inclusive)
//                           and  (flags[p] & need[r]) == need[r] && (flags[p] & deny[r]) == 0    (32 bits, bit 31 among them)
// with every part of pc_row_where optional.  The kernel's body -- plan, work items, chunks, the per-row LDS buffers with their
// threshold, the compactions --, the merge and the host path are grouped_list.h's and retrieve_list.hip's as they are; the body's
// WHERE hook stages value[pid] and flags[pid] in LDS per chunk column and tests a candidate that beat the row's threshold before
// the exclusion bisection.  The filter travels as rl_list_entry's trailing argument, by value.  A unit of its own, as
// nearest_list.hip: inside retrieve_list.hip or nearest_list.hip the new kernels would move the existing ones.
//
// Determinism: the predicate reads no score, so a (row, product) score has the bits of pc_retrieve_list_grouped /
// pc_retrieve_list_grouped_biased; a product that fails is dropped where an excluded product is dropped -- never buffered, the
// threshold does not move --, so a row's list is the unfiltered order (score descending, product index ascending) with the
// failing products taken out: the existing entry's output over a CSR of the passing products, bit for bit, and with every array
// absent the existing entry's output.  It does not depend on the slices, the rows' places, the order of type_col or the arrival
// order in a buffer.  No float atomics, no readback.
#include "common.h"
#include "grouped_list_f32.h"

// The row's predicate and the staged attributes cost about 12 vector registers.  Every instantiation keeps its workgroups per CU
// with them but <128, 2, EX> (n <= 32), which the unfiltered kernels run at 128 registers -- four waves per SIMD -- and which
// lands at 136 here: that variant alone is held to four waves (it fits without scratch: tests/test_abi.py gates the spills).
#define WL_WAVES(D, NE) __attribute__((amdgpu_waves_per_eu((D) == 128 && (NE) == 2 ? 4 : 1, 8)))

template <int D, int NE, bool EX>
__global__ __launch_bounds__(256) WL_WAVES(D, NE) void wl_score_kernel(RL_SCORE_PARAMS(float), RlWhere where) {
    rl_score_body<RlChainF32<D>, NE, EX, false, true>(RL_SCORE_ARGS, nullptr, where);
}

template <int D, int NE, bool EX>
__global__ __launch_bounds__(256) WL_WAVES(D, NE) void wl_score_biased_kernel(RL_SCORE_PARAMS(float),
                                                                               const float* __restrict__ bias, RlWhere where) {
    rl_score_body<RlChainF32<D>, NE, EX, true, true>(RL_SCORE_ARGS, bias, where);
}

struct WlKernels {
    template <int D, int NE, bool EX>
    static constexpr auto kernel() { return wl_score_kernel<D, NE, EX>; }
};

struct WlBiasedKernels {
    template <int D, int NE, bool EX>
    static constexpr auto kernel() { return wl_score_biased_kernel<D, NE, EX>; }
};

extern "C" size_t pc_retrieve_list_grouped_where_workspace_bytes(int rows, int n_types, int n, int slices) {
    return rg_topn_workspace_bytes(rows, n_types, n, RL_MAX_N, slices);
}

extern "C" int pc_retrieve_list_grouped_where(const float* proj, const int32_t* types, const int32_t* row_key, int rows,
                                              const int32_t* type_rowptr, const int32_t* type_col, const float* table, int n_types,
                                              const int32_t* ex_rowptr, const int32_t* ex_col, int n_keys, int n, int dim,
                                              int slices, int32_t* out_idx, float* out_score, int32_t* bad_count,
                                              const pc_row_where* where, void* ws, size_t ws_bytes, void* stream) {
    if (!where) return PC_EINVAL;
    return rl_list_entry<WlKernels>(proj, types, row_key, rows, type_rowptr, type_col, table, n_types, ex_rowptr, ex_col, n_keys, n,
                                    dim, slices, out_idx, out_score, bad_count, ws, ws_bytes, stream, RlWhere{*where});
}

extern "C" size_t pc_retrieve_list_grouped_biased_where_workspace_bytes(int rows, int n_types, int n, int slices) {
    return rg_topn_workspace_bytes(rows, n_types, n, RL_MAX_N, slices);
}

extern "C" int pc_retrieve_list_grouped_biased_where(const float* proj, const int32_t* types, const int32_t* row_key, int rows,
                                                     const int32_t* type_rowptr, const int32_t* type_col, const float* table,
                                                     const float* bias, int n_types, const int32_t* ex_rowptr,
                                                     const int32_t* ex_col, int n_keys, int n, int dim, int slices,
                                                     int32_t* out_idx, float* out_score, int32_t* bad_count,
                                                     const pc_row_where* where, void* ws, size_t ws_bytes, void* stream) {
    if (!where) return PC_EINVAL;
    return rl_list_entry<WlBiasedKernels>(proj, types, row_key, rows, type_rowptr, type_col, table, n_types, ex_rowptr, ex_col,
                                          n_keys, n, dim, slices, out_idx, out_score, bad_count, ws, ws_bytes, stream, bias,
                                          RlWhere{*where});
}
