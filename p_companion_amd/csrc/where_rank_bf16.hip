// The rank of a known product among the products of its type that pass the row's predicate on per-product attributes, over
// the bf16 copy of the catalogue alone (pc_rank_grouped_bf16_where; ops.rank_grouped_where with a bf16 table,
// CompactInference.rank_targets_where / evaluate_catalogue_where and CompactSimilarProducts.rank_pairs_where /
// evaluate_pairs_where in inference.py): where_rank.hip's contract --
//   rank_out[r] = #{ p of type c : p passes w_r, p not in the row's list : s_p > g  or  (s_p == g and p < y) },
//   -1 where pc_rank_grouped_bf16 gives -1 or y itself fails w_r --
// under rank_bf16.hip's score s_p = fl(d(r, p) + bias[p]) (bias null: d), the position y takes in the list
// pc_retrieve_list_grouped_bf16_where / pc_retrieve_list_grouped_bf16_biased_where serves for the row.  rank_bf16.hip's schedule
// and count with the test inside the count; a unit of its own: inside rank_bf16.hip the new kernels would move the existing ones.
//
//   plan     grouped_plan.hip as it is (tiles of TM = 8192 / D rows)
//   rank     wrb_rank_kernel: rb_rank_kernel -- the query tile split ONCE by split3 into three bf16 images in LDS, the tile's
//            own targets scored first, the slice's candidates in chunks of 64 with the next chunk's rows in flight -- with the
//            rows' lo / hi / need / deny read through order[p0 + row] once per work item into LDS beside gs / ys, value[pid] /
//            flags[pid] gathered a chunk ahead with the product id as bias[pid] is, and wr_count (where_rank.h): a candidate is
//            counted where it beats (or ties and precedes) the row's g AND passes that row's predicate
//   post     wrb_post_kernel, one wave per row, in EVERY call: -1 for a target that fails its own predicate, after all slices'
//            atomics have landed; with lists rb_rank_exclude_kernel's post-pass, decrementing only for entries that pass
//
// Determinism: d is rb_chain (rank_chain_bf16.h), so a (row, product) score has the bits pc_retrieve_list_grouped_bf16[_biased]
// [_where] and pc_rank_grouped_bf16 give it; the predicate reads no score; the count is a sum of integers.  With every array of
// the filter absent: pc_rank_grouped_bf16's output.  No float atomics, no readback.
#include "common.h"
#include "grouped_rank.h"          // rk_post: the row post-pass; rk_begin, rk_dispatch

// One work item's candidate stream for a tile of NG 16-row groups (rb_stream with the test in the count).  bn / pidn / bsn / an /
// fn: the first chunk's rows, product ids, terms and attributes, pidnn: the second chunk's ids, all already in flight (-1: a
// column past the slice's end; its attributes are entry 0's and nothing of it is counted).  Leaves the wave's counts in
// part[wv][row].
template <int D, int NG, bool BIAS>
__device__ __forceinline__ void wrb_stream(const bf16x8 (&q)[3][(D / 8) * (8192 / D)], const float* gs, const int* ys,
                                           const WrRow* wq, int (*part)[8192 / D], const int32_t* __restrict__ type_col,
                                           const uint16_t* __restrict__ table, const float* __restrict__ bias,
                                           const pc_row_where& wh, int cb0, int ce, bf16x8 (&bn)[D / 32], int pidn, int pidnn,
                                           float bsn, float an, int fn, int wv, int c, int h) {
    constexpr int TM = 8192 / D, NB = D / 32;
    int cn[NG][4];
#pragma unroll
    for (int g = 0; g < NG; g++)
#pragma unroll
        for (int k = 0; k < 4; k++) cn[g][k] = 0;
    for (int cb = cb0; cb < ce; cb += RG_CHUNK) {
        bf16x8 b[NB];
#pragma unroll
        for (int k = 0; k < NB; k++) b[k] = bn[k];
        const int pid = pidn;
        const float bs = bsn, a = an;
        const int f = fn;
        pidn = pidnn;
        if (cb + RG_CHUNK < ce) rb_load_b<D>(bn, table, pidn, h);     // the next chunk's rows in flight while this one is scored
        if constexpr (BIAS) bsn = bias[max(pidn, 0)];                 // and its term and attributes (a column without a
        an = wr_value(wh, pidn);                                      // product: entry 0, unused)
        fn = wr_flags(wh, pidn);
        const int cc = cb + 2 * RG_CHUNK + wv * 16 + c;
        pidnn = cc < ce ? type_col[cc] : -1;
        f32x4 acc[NG];
#pragma unroll
        for (int g = 0; g < NG; g++) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
        rb_chain<D, TM, NG>(q, 0, b, acc, c, h);
        wr_count<NG, BIAS>(acc, bs, gs, cn, ys, wq, pid, a, f, h);
    }
    wr_reduce<NG, TM>(cn, part, wv, c, h);
}

// Work item w = (type t, slice s, tile j) (rg_decode).  amdgpu_waves_per_eu(2) as rb_rank_kernel -- but <256, BIAS>, which the
// compiler then takes to 170 registers, two waves per SIMD, where rb_rank_kernel<256, true> runs three at 166: that variant
// alone is held to three waves (168 registers, no scratch: tests/test_abi.py gates the spills) and keeps its twin's workgroups.
template <int D, bool BIAS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(D == 256 && BIAS ? 3 : 2))) void wrb_rank_kernel(
    const float* __restrict__ proj, const int32_t* __restrict__ targets, const int32_t* __restrict__ type_rowptr,
    const int32_t* __restrict__ type_col, const uint16_t* __restrict__ table, const float* __restrict__ bias, int n_types, int S,
    const int32_t* __restrict__ cnt, const int32_t* __restrict__ row_start, const int64_t* __restrict__ item_start,
    const int32_t* __restrict__ order, int32_t* __restrict__ rank_out, pc_row_where wh) {
    constexpr int TM = 8192 / D;             // rows per tile: 64 (D = 128) or 32 (D = 256)
    constexpr int RG = TM / 16;              // 16-row groups (at most one per wave)
    constexpr int NB = D / 32;               // k-blocks: 16-byte operands per lane per candidate
    __shared__ __attribute__((aligned(16))) bf16x8 q[3][(D / 8) * TM];   // the pieces p0, p1, p2 of the query tile
    __shared__ __attribute__((aligned(16))) float gs[TM];            // the rows' target scores
    __shared__ __attribute__((aligned(16))) int ys[TM];              // the rows' targets
    __shared__ WrRow wq[TM];                                         // the rows' predicates
    __shared__ int part[4][TM];                                      // the waves' counts
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c = lane & 15, h = lane >> 4;
    const int64_t n_items = item_start[n_types];
    for (int64_t w = blockIdx.x; w < n_items; w += gridDim.x) {
        const RgItem it = rg_decode<TM>(w, item_start, cnt, row_start, type_rowptr, n_types, S);
        const int p0 = it.p0, valid = it.valid, rg = it.rg, cb0 = it.cb0, ce = it.ce;

        __syncthreads();                                  // the previous item's readers of q / wq / part are done
        for (int e = tid; e < rg * 16 * (D / 8); e += 256) {          // (rows past the last 16-row group are never read)
            const int d8 = e / (rg * 16), row = e - d8 * (rg * 16);   // (row fastest: a wave's 16-byte stores are contiguous)
            float4 x0 = make_float4(0.f, 0.f, 0.f, 0.f), x1 = x0;
            if (row < valid) {
                const float4* f = reinterpret_cast<const float4*>(proj + (size_t)order[p0 + row] * D) + 2 * d8;
                x0 = f[0];
                x1 = f[1];
            }
            const Split3 sp = split3(x0, x1);
            q[0][d8 * TM + row] = sp.p0;
            q[1][d8 * TM + row] = sp.p1;
            q[2][d8 * TM + row] = sp.p2;
        }
        if (tid < TM) wq[tid] = wr_row(wh, tid < valid ? order[p0 + tid] : -1);

        auto load_pid = [&](int cb) { const int cc = cb + wv * 16 + c; return cc < ce ? type_col[cc] : -1; };
        bf16x8 bn[NB];
        const int pidn = load_pid(cb0);
        rb_load_b<D>(bn, table, pidn, h);
        float bsn = 0.f;
        if constexpr (BIAS) bsn = bias[max(pidn, 0)];
        const float an = wr_value(wh, pidn);
        const int fn = wr_flags(wh, pidn);
        const int pidnn = load_pid(cb0 + RG_CHUNK);
        // wave wv: column c = the target of query row wv * 16 + c
        int ty = -1;
        if (wv < rg && wv * 16 + c < valid) ty = targets[order[p0 + wv * 16 + c]];
        __syncthreads();                                  // query images in LDS
        if (wv < rg) {                                    // (wave-uniform)
            bf16x8 bt[NB];
            rb_load_b<D>(bt, table, ty, h);
            float by = 0.f;
            if constexpr (BIAS) by = bias[max(ty, 0)];
            f32x4 ag[1] = {f32x4{0.f, 0.f, 0.f, 0.f}};
            rb_chain<D, TM, 1>(q, wv, bt, ag, c, h);
            const f32x4 acc = ag[0];
            // C/D map of the 16x16 MFMAs: column lane & 15, row 4 (lane >> 4) + reg; the diagonal: row == column
            if ((c >> 2) == h) {
                const int k = c & 3;
                const float d = k == 0 ? acc[0] : k == 1 ? acc[1] : k == 2 ? acc[2] : acc[3];
                gs[wv * 16 + c] = BIAS ? d + by : d;
                ys[wv * 16 + c] = ty;
            }
        }
        __syncthreads();                                  // gs / ys / wq in LDS
        // the slice's candidates against the tile's NG row groups: straight-line code per NG
        if (rg == 1) wrb_stream<D, 1, BIAS>(q, gs, ys, wq, part, type_col, table, bias, wh, cb0, ce, bn, pidn, pidnn, bsn, an, fn, wv, c, h);
        else if (rg == 2) wrb_stream<D, 2, BIAS>(q, gs, ys, wq, part, type_col, table, bias, wh, cb0, ce, bn, pidn, pidnn, bsn, an, fn, wv, c, h);
        else if constexpr (RG == 4) {
            if (rg == 3) wrb_stream<D, 3, BIAS>(q, gs, ys, wq, part, type_col, table, bias, wh, cb0, ce, bn, pidn, pidnn, bsn, an, fn, wv, c, h);
            else wrb_stream<D, 4, BIAS>(q, gs, ys, wq, part, type_col, table, bias, wh, cb0, ce, bn, pidn, pidnn, bsn, an, fn, wv, c, h);
        }
        __syncthreads();
        if (tid < valid) {
            const int v = part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid];
            if (v) atomicAdd(&rank_out[order[p0 + tid]], v);
        }
    }
}

// where_rank.hip's row post-pass over the bf16 table, one wave per row, after wrb_rank_kernel on the stream: a row the plan left
// at -1 stays so; with lists (row_key != null; wave-uniform) a key outside [-1, n_keys) is no list and is counted in *bad_count
// and cand_type[y] != types[r] is rank -1; a target that fails its own row's predicate: rank -1.  Then rb_rank_exclude_kernel's
// pass through rb_chain (the row's split query is row 0 of a 16-row image): a list entry e with cand_type[e] == types[r] that
// passes the predicate and has rg_better(s_e, e, g, y) was counted: one off; e == y: rank -1.
template <int D, bool BIAS>
__global__ __launch_bounds__(64) void wrb_post_kernel(const float* __restrict__ proj, const int32_t* __restrict__ types,
                                                      const int32_t* __restrict__ targets, const int32_t* __restrict__ row_key,
                                                      const int32_t* __restrict__ ex_rowptr, const int32_t* __restrict__ ex_col,
                                                      int n_keys, const int32_t* __restrict__ cand_type,
                                                      const uint16_t* __restrict__ table, const float* __restrict__ bias,
                                                      int num_products, pc_row_where wh, int32_t* __restrict__ rank_out,
                                                      int32_t* __restrict__ bad_count) {
    __shared__ __attribute__((aligned(16))) typename RkScoreBf16<D>::Image q;
    rk_post<D, RkScoreBf16<D>, BIAS, true>(q, proj, types, targets, row_key, ex_rowptr, ex_col, n_keys, cand_type, table, bias,
                                           num_products, wh, rank_out, bad_count);
}

extern "C" size_t pc_rank_grouped_bf16_where_workspace_bytes(int rows, int n_types, int slices) {
    return pc_rank_grouped_workspace_bytes(rows, n_types, slices);
}

extern "C" int pc_rank_grouped_bf16_where(const float* proj, const int32_t* types, const int32_t* targets, const int32_t* row_key,
                                          int rows, const int32_t* type_rowptr, const int32_t* type_col,
                                          const uint16_t* table_bf16, const float* bias, int n_types, int num_products,
                                          const int32_t* ex_rowptr, const int32_t* ex_col, int n_keys, const int32_t* cand_type,
                                          int dim, int slices, int32_t* rank_out, int32_t* bad_count, const pc_row_where* where,
                                          void* ws, size_t ws_bytes, void* stream) {
    RkStart s;
    // (args_ok: a null filter, or a half-given one, too)
    PC_TRY(rk_begin(s, proj && table_bf16 && wr_where_ok(where), table_bf16, types, targets, row_key, rows, type_rowptr, type_col,
                    n_types, num_products, ex_rowptr, ex_col, n_keys, cand_type, dim, slices, rank_out, bad_count, ws, ws_bytes,
                    stream));
    const RgPlan& pl = s.w.plan;
    rk_dispatch(dim, bias != nullptr, [&](auto d, auto b) {
        constexpr int D = decltype(d)::value;
        constexpr bool BIAS = decltype(b)::value;
        PC_LAUNCH((wrb_rank_kernel<D, BIAS>), dim3(s.grid), dim3(256), 0, s.st, proj, targets, type_rowptr, type_col, table_bf16,
                  bias, n_types, s.S, pl.cnt, pl.row_start, pl.item_start, pl.order, rank_out, *where);
        PC_LAUNCH((wrb_post_kernel<D, BIAS>), dim3(rows), dim3(64), 0, s.st, proj, types, targets, row_key, ex_rowptr, ex_col,
                  n_keys, cand_type, table_bf16, bias, num_products, *where, rank_out, bad_count);
    });
    return pc_launch_status();
}
