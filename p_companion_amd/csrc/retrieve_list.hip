// Long complement lists: the first n <= 256 products of a type per (query, type) row over the fp32 table
// (PCompanionInference.recommend_batch above 16; pc_retrieve_list_grouped).  The kernel's body -- plan, work items, chunks, the
// per-row LDS buffers with their threshold, the compactions -- and the host path are grouped_list.h's, the fp32 score chain is
// grouped_list_f32.h's (shared with nearest_list.hip); here are the kernels under their names, the merge of the slices'
// partial lists (for every unit of the family) and the entries.
//
// Determinism: a score is rg_score_kernel's MFMA k-chain (step j, element e, k-lane h cover dimension 16 j + 4 h + e), so a
// (row, product) pair has that kernel's bits.  The order in which survivors arrive in a buffer is decided by an LDS atomic
// and is free: every selection that follows is under the total order (score descending, product index ascending), and the
// threshold only ever drops candidates that n kept products of the row beat.  An excluded product never enters a buffer, so
// it never moves a threshold.  Hence the output does not depend on the slices, the rows' places, the order of type_col, or
// the arrival order; for n <= 16 it is pc_retrieve_topk_grouped[_excluding]'s bit for bit.  No float atomics, no readback.
#include "common.h"
#include "grouped_list_f32.h"    // grouped_list.h and the fp32 score chain

template <int D, int NE, bool EX>
__global__ __launch_bounds__(256) void rl_score_kernel(RL_SCORE_PARAMS(float)) {
    rl_score_body<RlChainF32<D>, NE, EX>(RL_SCORE_ARGS);
}

// One wave per row: lane s walks slice s's sorted partial list; every round the best head under rg_better is the next
// entry of the row, and its lane moves on.  Results are gathered 64 at a time and stored as a row of the wave.
__global__ __launch_bounds__(256) void rl_merge_kernel(const int32_t* __restrict__ types, int rows,
                                                       const int32_t* __restrict__ type_rowptr, int n_types, int n, int S,
                                                       const int32_t* __restrict__ rank, const int32_t* __restrict__ row_start,
                                                       const float* __restrict__ pv, const int32_t* __restrict__ pi,
                                                       int32_t* __restrict__ out_idx, float* __restrict__ out_score) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;                                // wave-uniform
    const int t = types[r];
    int ns = 0, L = 0, p = 0;
    if (t >= 0 && t < n_types) {
        rg_slice_plan(type_rowptr[t + 1] - type_rowptr[t], S, ns, L);
        if (ns > 0) p = row_start[t] + rank[r];
    }
    if (ns == 1) {                                        // one slice: its sorted list is the row's
        const size_t one = (size_t)p * S * n;
        for (int k = lane; k < n; k += 64) {
            const int xi = pi[one + k];
            out_idx[(size_t)r * n + k] = xi == RG_NONE ? -1 : xi;
            out_score[(size_t)r * n + k] = xi == RG_NONE ? -INFINITY : pv[one + k];
        }
        return;
    }
    const size_t mine = ((size_t)p * S + lane) * n;       // this lane's list (read only where lane < ns)
    int pos = 0;
    float hv = -INFINITY;
    int hi = RG_NONE;
    if (lane < ns) { hv = pv[mine]; hi = pi[mine]; }
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
        if (hi == bi && bi != RG_NONE) {                  // (a product is in one slice: one lane)
            pos++;
            hv = -INFINITY; hi = RG_NONE;
            if (pos < n) { hv = pv[mine + pos]; hi = pi[mine + pos]; }
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

void rl_merge_launch(const RgWs& w, const int32_t* types, int rows, const int32_t* type_rowptr, int n_types, int n, int S,
                     int32_t* out_idx, float* out_score, hipStream_t st) {
    PC_LAUNCH(rl_merge_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, types, rows, type_rowptr, n_types, n, S, w.plan.pos,
              w.plan.row_start, w.pv, w.pi, out_idx, out_score);
}

struct RlKernelsF32 {
    template <int D, int NE, bool EX>
    static constexpr auto kernel() { return rl_score_kernel<D, NE, EX>; }
};

extern "C" size_t pc_retrieve_list_grouped_workspace_bytes(int rows, int n_types, int n, int slices) {
    return rg_topn_workspace_bytes(rows, n_types, n, RL_MAX_N, slices);
}

extern "C" int pc_retrieve_list_grouped(const float* proj, const int32_t* types, const int32_t* row_key, int rows,
                                        const int32_t* type_rowptr, const int32_t* type_col, const float* table, int n_types,
                                        const int32_t* ex_rowptr, const int32_t* ex_col, int n_keys, int n, int dim, int slices,
                                        int32_t* out_idx, float* out_score, int32_t* bad_count, void* ws, size_t ws_bytes,
                                        void* stream) {
    return rl_list_entry<RlKernelsF32>(proj, types, row_key, rows, type_rowptr, type_col, table, n_types, ex_rowptr, ex_col, n_keys,
                                       n, dim, slices, out_idx, out_score, bad_count, ws, ws_bytes, stream);
}
