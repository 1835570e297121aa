// The rank of a known product among the products of its type that the row's exclusion list leaves (PCompanionInference with
// set_exclusions / set_eligible: rank_targets, evaluate_catalogue).  A unit of its own: in rank.hip the new kernel changed the
// register allocation of rk_rank_kernel<128>, and the unfiltered path keeps its text.
#include "common.h"
#include "grouped_rank.h"          // rk_post: THE row post-pass

// rk_rank_kernel runs as it is and counts over the whole type; this post-pass (rk_post over the fp32 table, without a bias and
// without a predicate) takes the excluded products out again: g and every s_e are the bits rk_rank_kernel compared.
template <int D>
__global__ __launch_bounds__(64) void rk_exclude_kernel(const float* __restrict__ proj, const int32_t* __restrict__ types,
                                                        const int32_t* __restrict__ targets, const int32_t* __restrict__ row_key,
                                                        const int32_t* __restrict__ ex_rowptr, const int32_t* __restrict__ ex_col,
                                                        int n_keys, const int32_t* __restrict__ cand_type,
                                                        const float* __restrict__ table, int num_products,
                                                        int32_t* __restrict__ rank_out, int32_t* __restrict__ bad_count) {
    __shared__ __attribute__((aligned(16))) typename RkScoreF32<D>::Image q;
    rk_post<D, RkScoreF32<D>, false, false>(q, proj, types, targets, row_key, ex_rowptr, ex_col, n_keys, cand_type, table, nullptr,
                                            num_products, pc_row_where{}, rank_out, bad_count);
}

extern "C" int pc_rank_grouped_excluding(const float* proj, const int32_t* types, const int32_t* targets,
                                         const int32_t* row_key, int rows, const int32_t* type_rowptr,
                                         const int32_t* type_col, const float* table, int n_types, int num_products,
                                         const int32_t* ex_rowptr, const int32_t* ex_col, int n_keys, const int32_t* cand_type,
                                         int dim, int slices, int32_t* rank_out, int32_t* bad_count, void* ws, size_t ws_bytes,
                                         void* stream) {
    if (!row_key || !ex_rowptr || !ex_col || !cand_type || n_keys < 0) return PC_EINVAL;
    // every other check, the plan and rk_rank_kernel: the unfiltered entry as it is
    PC_TRY(pc_rank_grouped(proj, types, targets, rows, type_rowptr, type_col, table, n_types, num_products, dim, slices, rank_out,
                           bad_count, ws, ws_bytes, stream));
    rk_dispatch(dim, false, [&](auto d, auto) {
        PC_LAUNCH(rk_exclude_kernel<decltype(d)::value>, dim3(rows), dim3(64), 0, (hipStream_t)stream, proj, types, targets, row_key,
                  ex_rowptr, ex_col, n_keys, cand_type, table, num_products, rank_out, bad_count);
    });
    return pc_launch_status();
}
