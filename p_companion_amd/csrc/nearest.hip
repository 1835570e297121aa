// Grouped retrieval and grouped rank with a per-product additive term on the score (pc_retrieve_topk_grouped_biased,
// pc_rank_grouped_biased; SimilarProducts in inference.py), and the term that makes them Euclidean (pc_half_sq_norm_bias):
//   |q - e_p|^2 = |q|^2 - 2 (<q, e_p> - |e_p|^2 / 2),
// so the nearest product under L2 is the largest <q, e_p> + b_p with b_p = -|e_p|^2 / 2.  retrieve.hip's contract, plan, work
// items, chunks, selection and merge, and rank.hip's / rank_exclude.hip's counts; what differs is the score:
//   s(r, p) = fl(d(r, p) + bias[p]),   d(r, p) = rk_chain (rank_chain.h) over the fp32 table,
// ONE fp32 addition in the epilogue, after the chain -- the accumulator starts at zero, never at the bias -- so d is bit for bit
// what pc_retrieve_topk_grouped orders by and a zero bias gives that entry's output.  A unit of its own: inside retrieve.hip or
// rank.hip the new kernels move the register allocation of the existing ones.  The list helpers, the item decode, the tile
// load, the selection and the partial-list write are the family's (grouped_select.h), the merge is retrieve.hip's.
//
//   plan     grouped_plan.hip as it is (tiles of TM = 8192 / D rows)
//   score    nb_score_kernel: work item (type, slice, tile); query tile -> LDS in RK_QS rows; candidates in chunks of 64, one
//            16-candidate column group per wave; a lane holds ONE set of row registers, which rk_chain refills with the next
//            chunk's rows step by step (a tile of more than two 16-row groups in two passes of two accumulators); bias[pid] is
//            a 4-byte gather per column, issued with the column's product id a chunk ahead; biased scores -> LDS, then
//            rg_select_chunk (the threshold test, per-thread lists of 16, exclusion lists) and rg_write_partial
//   merge    rg_merge_kernel (retrieve.hip) through rg_merge_launch
//   rank     nb_rank_kernel: rk_rank_kernel with g = d(r, y) + bias[y] and every candidate compared as d + bias[pid] against g;
//            nb_rank_exclude_kernel: rk_exclude_kernel's post-pass with the same biased scores
//   bias     nb_half_sq_norm_kernel: out[p] = -0.5f * sum_d e[p][d]^2
//
// Determinism: the chain of a (row, product) pair runs in the order of the dimension index alone (step j, element e, k-lane h
// cover dimension 16 j + 4 h + e), and the bias is a function of the product, so a (row, product) score has the same bits
// wherever it is scored: in any tile, slice or column, in the retrieval and in both rank kernels.  Every selection is under the
// total order (score descending, product index ascending), so the output does not depend on the slices, on the order of the
// rows in a tile (the one thing the planning atomics decide) or on the order of type_col inside a type.  Counts are sums of
// integers, one integer atomic per (row, slice).  No float atomics.
#include "common.h"
#include "grouped_select.h"        // the item decode, the tile load, the dispatch on a tile's row groups, the selection, the write
#include "grouped_rank.h"          // rk_rank_body, rk_post: the rank skeleton and the row post-pass

// Lane l of wave wv: column c = l & 15 (candidate wv * 16 + c of the chunk, query row g * 16 + c of the A operand), k-lane
// h = l >> 4.  Partial lists: pv / pi [rows][S][n] at the row's grouped position.  EXCL: rg_score_excl_kernel's exclusion lists
// (bisection after the threshold test, before the insertion) and the count of keys outside [-1, n_keys) in *bad_count.
// A column past the slice's end (pid -1) reads product 0's row and bias[0]; nothing of it is used: its id in LDS is RG_NONE.
template <int D, bool EXCL>
// three waves per SIMD at D = 128 (the LDS allows three workgroups per CU) and two at D = 256, as rg_score_kernel
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(D == 128 ? 3 : 2))) void nb_score_kernel(
    const float* __restrict__ proj, const int32_t* __restrict__ type_rowptr, const int32_t* __restrict__ type_col,
    const float* __restrict__ table, const float* __restrict__ bias, int n_types, int n, int S, const int32_t* __restrict__ cnt,
    const int32_t* __restrict__ row_start, const int64_t* __restrict__ item_start, const int32_t* __restrict__ order,
    float* __restrict__ pv, int32_t* __restrict__ pi, const int32_t* __restrict__ row_key, int rows,
    const int32_t* __restrict__ ex_rowptr, const int32_t* __restrict__ ex_col, int n_keys, int32_t* __restrict__ bad_count) {
    constexpr int TM = 8192 / D;             // rows per tile: 64 (D = 128) or 32 (D = 256)
    constexpr int RG = TM / 16;              // 16-row groups
    constexpr int QS = RK_QS(D);             // padded LDS row
    constexpr int TPR = 256 / TM;            // threads per row in the selection phase
    constexpr int NB = D / 16;               // float4 operands per lane per candidate
    __shared__ __attribute__((aligned(16))) float q[TM * QS];
    __shared__ float sc[TM][RG_CHUNK + 1];
    __shared__ int cid[RG_CHUNK];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c = lane & 15, h = lane >> 4;
    const int rr = tid / TPR, qq = tid % TPR;
    const int64_t n_items = item_start[n_types];
    if constexpr (EXCL) {
        for (int r = blockIdx.x * 256 + tid; r < rows; r += gridDim.x * 256) {
            const int key = row_key[r];
            if (key < -1 || key >= n_keys) atomicAdd(bad_count, 1);
        }
    }
    for (int64_t w = blockIdx.x; w < n_items; w += gridDim.x) {
        const RgItem it = rg_decode<TM>(w, item_start, cnt, row_start, type_rowptr, n_types, S);
        const int p0 = it.p0, valid = it.valid, rg = it.rg, cb0 = it.cb0, ce = it.ce;

        __syncthreads();                                  // the previous item's readers of q are done
        rg_load_tile<D, QS>(q, proj, order, p0, valid, rg, tid);
        float v[RG_MAX_N];
        int ix[RG_MAX_N];
#pragma unroll
        for (int k = 0; k < RG_MAX_N; k++) { v[k] = -INFINITY; ix[k] = RG_NONE; }
        float hv = -INFINITY;                             // the row's threshold
        int hix = RG_NONE;
        int elo = 0, ehi = 0;                             // this thread's row's list: ex_col[elo, ehi)
        if constexpr (EXCL) {
            if (rr < valid) {
                const int key = row_key[order[p0 + rr]];
                if (key >= 0 && key < n_keys) { elo = ex_rowptr[key]; ehi = ex_rowptr[key + 1]; }
            }
        }

        auto load_pid = [&](int cb) { const int cc = cb + wv * 16 + c; return cc < ce ? type_col[cc] : -1; };
        float4 b[NB];
        int pid = load_pid(cb0);
        {
            const float4* f = reinterpret_cast<const float4*>(table + (size_t)max(pid, 0) * D) + h;
#pragma unroll
            for (int k = 0; k < NB; k++) b[k] = f[4 * k];
        }
        float bs = bias[max(pid, 0)];
        int pidn = load_pid(cb0 + RG_CHUNK);
        __syncthreads();                                  // query tile in LDS

        for (int cb = cb0; cb < ce; cb += RG_CHUNK) {
            const int pidnn = load_pid(cb + 2 * RG_CHUNK);
            // (the previous chunk's readers of cid are behind the barrier at the loop's end)
            if (h == 0) cid[wv * 16 + c] = pid < 0 ? RG_NONE : pid;
            // the next chunk's rows replace this one's step by step while it is scored
            const float4* next = reinterpret_cast<const float4*>(table + (size_t)max(pidn, 0) * D) + h;
            // A tile of more than two row groups is scored in two passes over the same row registers (the refill rides in the
            // last pass): two accumulators at a time keep the D = 128 kernel inside the registers of three waves per SIMD.  An
            // accumulator's chain is the same either way: the dimensions in index order.
            auto score = [&](auto groups) {
                constexpr int R = decltype(groups)::value, R1 = R > 2 ? 2 : R;
                // C/D map of the 16x16 f32 MFMA: column lane & 15 (the candidate), row 4 (lane >> 4) + reg (the query row);
                // the epilogue's one addition: s = fl(d + bias[pid])
                {
                    f32x4 acc[R1];
#pragma unroll
                    for (int g = 0; g < R1; g++) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
                    rk_chain<D, R1>(q, 0, b, R > 2 ? nullptr : next, acc, c, h);
#pragma unroll
                    for (int g = 0; g < R1; g++) {
#pragma unroll
                        for (int k = 0; k < 4; k++) sc[g * 16 + 4 * h + k][wv * 16 + c] = acc[g][k] + bs;
                    }
                }
                if constexpr (R > 2) {
                    f32x4 acc[R - 2];
#pragma unroll
                    for (int g = 0; g < R - 2; g++) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
                    rk_chain<D, R - 2>(q, 2, b, next, acc, c, h);
#pragma unroll
                    for (int g = 0; g < R - 2; g++) {
#pragma unroll
                        for (int k = 0; k < 4; k++) sc[(g + 2) * 16 + 4 * h + k][wv * 16 + c] = acc[g][k] + bs;
                    }
                }
            };
            rg_dispatch_groups<RG>(rg, score);
            // the next chunk's term, with its product id, a chunk ahead: in flight through this chunk's selection (issued
            // behind the chain, where a register is free for it)
            const float bsn = bias[max(pidn, 0)];
            __syncthreads();
            rg_select_chunk<TM, EXCL>(sc, cid, rr, qq, valid, n, v, ix, hv, hix, elo, ehi, ex_col);
            __syncthreads();
            pid = pidn;
            pidn = pidnn;
            bs = bsn;
        }
        rg_write_partial<TM>(v, ix, n, qq == 0 && rr < valid, ((size_t)(p0 + rr) * S + it.s) * n, pv, pi);
    }
}

// rk_rank_kernel with the biased score: rank_out[r] += #{ p of the slice : s_p > g or (s_p == g and p < y) }, one integer atomic
// per (row, slice).
template <int D>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(D == 128 ? 3 : 2))) void nb_rank_kernel(
    const float* __restrict__ proj, const int32_t* __restrict__ targets, const int32_t* __restrict__ type_rowptr,
    const int32_t* __restrict__ type_col, const float* __restrict__ table, const float* __restrict__ bias, int n_types, int S,
    const int32_t* __restrict__ cnt, const int32_t* __restrict__ row_start, const int64_t* __restrict__ item_start,
    const int32_t* __restrict__ order, int32_t* __restrict__ rank_out) {
    rk_rank_body<D, true, false>(proj, targets, type_rowptr, type_col, table, bias, n_types, S, cnt, row_start, item_start, order,
                                 rank_out, pc_row_where{});
}

// rk_exclude_kernel's post-pass with the biased score (rk_post): g and every s_e are the bits nb_rank_kernel compared.
template <int D>
__global__ __launch_bounds__(64) void nb_rank_exclude_kernel(const float* __restrict__ proj, const int32_t* __restrict__ types,
                                                             const int32_t* __restrict__ targets,
                                                             const int32_t* __restrict__ row_key,
                                                             const int32_t* __restrict__ ex_rowptr,
                                                             const int32_t* __restrict__ ex_col, int n_keys,
                                                             const int32_t* __restrict__ cand_type,
                                                             const float* __restrict__ table, const float* __restrict__ bias,
                                                             int num_products, int32_t* __restrict__ rank_out,
                                                             int32_t* __restrict__ bad_count) {
    __shared__ __attribute__((aligned(16))) typename RkScoreF32<D>::Image q;
    rk_post<D, RkScoreF32<D>, true, false>(q, proj, types, targets, row_key, ex_rowptr, ex_col, n_keys, cand_type, table, bias,
                                           num_products, pc_row_where{}, rank_out, bad_count);
}

// out[p] = -0.5f * sum_d e[p][d]^2.  ONE summation order per row, whatever the grid: a group of 16 lanes owns a row; lane l of
// the group adds, in this order, the squares of the elements x, y, z, w of the float4s l, l + 16, .. (dimensions 4 l + 64 j + e,
// j ascending, e ascending) into one fp32 sum by fused multiply-add, starting from zero; the 16 sums meet in a butterfly over
// the lane distances 8, 4, 2, 1 (a + b is commutative: every lane of the group holds the same bits).  No atomics; a row's value
// does not depend on which group, block or launch geometry computes it.
template <int D>
__global__ __launch_bounds__(256) void nb_half_sq_norm_kernel(const float* __restrict__ table, int rows, float* __restrict__ out) {
    const int l = threadIdx.x & 15;
    const int64_t stride = (int64_t)gridDim.x * 16;
    for (int64_t p = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4); p < rows; p += stride) {
        const float4* f = reinterpret_cast<const float4*>(table + (size_t)p * D) + l;
        float4 x[D / 64];
#pragma unroll
        for (int j = 0; j < D / 64; j++) x[j] = f[16 * j];
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < D / 64; j++) {
            s = __builtin_fmaf(x[j].x, x[j].x, s);
            s = __builtin_fmaf(x[j].y, x[j].y, s);
            s = __builtin_fmaf(x[j].z, x[j].z, s);
            s = __builtin_fmaf(x[j].w, x[j].w, s);
        }
        // (a group's 16 lanes run the same number of iterations: p depends on threadIdx.x >> 4 alone)
#pragma unroll
        for (int o = 8; o >= 1; o >>= 1) s += __shfl_xor(s, o, 64);
        if (l == 0) out[p] = -0.5f * s;
    }
}

extern "C" int pc_half_sq_norm_bias(const float* table, int rows, int dim, float* out, void* stream) {
    if (!table || !out || rows <= 0) return PC_EINVAL;
    if (dim != 128 && dim != 256) return PC_ESHAPE;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)min((rows + 15) / 16, RG_MAX_GRID));        // 16 rows per workgroup and pass, grid-stride
    if (dim == 128) PC_LAUNCH(nb_half_sq_norm_kernel<128>, grid, dim3(256), 0, st, table, rows, out);
    else PC_LAUNCH(nb_half_sq_norm_kernel<256>, grid, dim3(256), 0, st, table, rows, out);
    return pc_launch_status();
}

extern "C" size_t pc_retrieve_topk_grouped_biased_workspace_bytes(int rows, int n_types, int n, int slices) {
    return rg_topn_workspace_bytes(rows, n_types, n, RG_MAX_N, slices);
}

extern "C" int pc_retrieve_topk_grouped_biased(const float* proj, const int32_t* types, const int32_t* row_key, int rows,
                                               const int32_t* type_rowptr, const int32_t* type_col, const float* table,
                                               const float* bias, int n_types, const int32_t* ex_rowptr, const int32_t* ex_col,
                                               int n_keys, int n, int dim, int slices, int32_t* out_idx, float* out_score,
                                               int32_t* bad_count, void* ws, size_t ws_bytes, void* stream) {
    PC_TRY(rg_topn_check(proj && types && type_rowptr && type_col && table && bias && out_idx && out_score && ws, rows, n_types,
                         rg_lists_ok(row_key, ex_rowptr, ex_col, bad_count, n_keys), n, RG_MAX_N, dim, slices));
    const int S = rg_slices(slices);
    hipStream_t st = (hipStream_t)stream;
    RgWs w;
    unsigned grid;
    PC_TRY(rg_begin(w, grid, ws, ws_bytes, types, nullptr, rows, type_rowptr, n_types, 0, n, S, 8192 / dim, nullptr, nullptr, st));
    const RgPlan& pl = w.plan;
#define NB_SCORE(D, EXCL)                                                                                                       \
    PC_LAUNCH((nb_score_kernel<D, EXCL>), dim3(grid), dim3(256), 0, st, proj, type_rowptr, type_col, table, bias, n_types, n, S, \
              pl.cnt, pl.row_start, pl.item_start, pl.order, w.pv, w.pi, row_key, rows, ex_rowptr, ex_col, n_keys, bad_count)
    if (dim == 128) {
        if (row_key) NB_SCORE(128, true); else NB_SCORE(128, false);
    } else {
        if (row_key) NB_SCORE(256, true); else NB_SCORE(256, false);
    }
#undef NB_SCORE
    rg_merge_launch(w, types, rows, type_rowptr, n_types, n, S, out_idx, out_score, st);
    return pc_launch_status();
}

extern "C" size_t pc_rank_grouped_biased_workspace_bytes(int rows, int n_types, int slices) {
    return pc_rank_grouped_workspace_bytes(rows, n_types, slices);
}

extern "C" int pc_rank_grouped_biased(const float* proj, const int32_t* types, const int32_t* targets, const int32_t* row_key,
                                      int rows, const int32_t* type_rowptr, const int32_t* type_col, const float* table,
                                      const float* bias, int n_types, int num_products, const int32_t* ex_rowptr,
                                      const int32_t* ex_col, int n_keys, const int32_t* cand_type, int dim, int slices,
                                      int32_t* rank_out, int32_t* bad_count, void* ws, size_t ws_bytes, void* stream) {
    RkStart s;
    PC_TRY(rk_begin(s, proj && table && bias, nullptr, types, targets, row_key, rows, type_rowptr, type_col, n_types, num_products,
                    ex_rowptr, ex_col, n_keys, cand_type, dim, slices, rank_out, bad_count, ws, ws_bytes, stream));
    const RgPlan& pl = s.w.plan;
    rk_dispatch(dim, false, [&](auto d, auto) {
        constexpr int D = decltype(d)::value;
        PC_LAUNCH(nb_rank_kernel<D>, dim3(s.grid), dim3(256), 0, s.st, proj, targets, type_rowptr, type_col, table, bias, n_types,
                  s.S, pl.cnt, pl.row_start, pl.item_start, pl.order, rank_out);
        if (row_key)
            PC_LAUNCH(nb_rank_exclude_kernel<D>, dim3(rows), dim3(64), 0, s.st, proj, types, targets, row_key, ex_rowptr, ex_col,
                      n_keys, cand_type, table, bias, num_products, rank_out, bad_count);
    });
    return pc_launch_status();
}
