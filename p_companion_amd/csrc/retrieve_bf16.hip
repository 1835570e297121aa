// Type-filtered top-n retrieval from a bf16 copy of the catalogue (pc_retrieve_topk_grouped_bf16; PCompanionInference with
// catalogue=): retrieve.hip's contract, plan, work items, chunks, selection and merge; what differs is the table -- [P, D]
// bf16, half the bytes per candidate row -- and the score chain.  The stored table is scored against the UNROUNDED query:
// the fp32 query row is split into three bf16 pieces q = p0 + p1 + p2 by truncation (split3, common.h: the residuals are
// exact, |q - (p0 + p1 + p2)| < 2^-24 |q|) and p0 . t, p1 . t, p2 . t run on v_mfma_f32_16x16x32_bf16.  A product of two
// bf16 values is exact in fp32, so the only rounding is the fp32 accumulation, as in rg_score_kernel: the score is the
// fp32-grade dot product of proj with the rounded table (oracle: float64 over the rounded table).
//
//   plan    grouped_plan.hip as it is (tiles of TM = 8192 / D rows)
//   score   work item (type, slice, tile): the query tile is split ONCE, into three bf16 images in LDS (3 TM D 2 B = 48 KB;
//           a split per chunk would make the VALU, not the matrix pipe, the bound); candidates in chunks of 64, one
//           16-candidate column group per wave: lane (c = lane & 15, h = lane >> 4) holds the 8 dimensions 32 k + 8 h .. + 7
//           of candidate c for every k-block k -- D / 32 loads of 16 B, the next chunk's in flight while this one is scored;
//           scores -> LDS, then the family's selection (grouped_select.h: rg_select_chunk, the threshold test, per-thread lists of
//           16 and (EXCL) exclusion lists) and partial-list write
//   merge   rg_merge_kernel (retrieve.hip) through rg_merge_launch: the one merge of the entries with lists of up to 16
//
// Determinism: the chain of a (row, product) pair is k-block 0 .. D / 32 - 1, inside a k-block the pieces p0, p1, p2, one
// MFMA each into ONE accumulator, inside an MFMA k-lane h and element e cover dimension 32 k + 8 h + e: its order depends on
// the dimension index and the piece alone, never on the tile, the slice or the candidate's position, so a (row, product) pair
// has the same bits wherever it is scored.  Every selection is under the total order (score descending, product index
// ascending), so the top n of the union does not depend on how the candidates were split, on the order of the rows in a tile
// (the one thing the planning atomics decide), or on the order of type_col inside a type.  No float atomics.
#include "common.h"
#include "grouped_select.h"        // the item decode, the dispatch on a tile's row groups, the selection, the partial-list write

// Work item w = (type t, slice s, tile j) (rg_decode).  Lane l of wave wv: column c = l & 15 (candidate
// wv * 16 + c of the chunk, query row g * 16 + c of the A operand), k-lane h = l >> 4.  The C/D map of the 16x16x32 bf16
// MFMA is the 16x16x4 f32 one's (column lane & 15, row 4 (lane >> 4) + reg), so the selection is rg_select_chunk as it is.
// EXCL: rg_score_excl_kernel's exclusion lists and key count.
// Two workgroups per CU: the three query images and the score tile take 66 KB (D = 128) / 58 KB (D = 256) of the 160 KB.
template <int D, bool EXCL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void rg_score_bf16_kernel(
    const float* __restrict__ proj, const int32_t* __restrict__ type_rowptr, const int32_t* __restrict__ type_col,
    const uint16_t* __restrict__ table, int n_types, int n, int S, const int32_t* __restrict__ cnt,
    const int32_t* __restrict__ row_start, const int64_t* __restrict__ item_start, const int32_t* __restrict__ order,
    float* __restrict__ pv, int32_t* __restrict__ pi, const int32_t* __restrict__ row_key, int rows,
    const int32_t* __restrict__ ex_rowptr, const int32_t* __restrict__ ex_col, int n_keys, int32_t* __restrict__ bad_count) {
    constexpr int TM = 8192 / D;             // rows per tile: 64 (D = 128) or 32 (D = 256)
    constexpr int RG = TM / 16;              // 16-row groups
    constexpr int TPR = 256 / TM;            // threads per row in the selection phase
    constexpr int NB = D / 32;               // k-blocks: 16-byte operands per lane per candidate
    // the pieces p0, p1, p2 of the query tile, each as [D / 8][TM] operands of 16 bytes: operand (d8, row) = the dimensions
    // 8 d8 .. 8 d8 + 7 of a row.  The 16 lanes of one LDS cycle of a ds_read_b128 (16 distinct columns c at one or two h) then
    // read 16 consecutive operands of one or two d8: 16 distinct 16-byte bank slots, no padding.
    __shared__ __attribute__((aligned(16))) bf16x8 q[3][(D / 8) * TM];
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
        auto load_b = [&](bf16x8* b, int pid) {
            if (pid >= 0) {
                const bf16x8* f = reinterpret_cast<const bf16x8*>(table + (size_t)pid * D) + h;
#pragma unroll
                for (int k = 0; k < NB; k++) b[k] = f[4 * k];
            } else {
#pragma unroll
                for (int k = 0; k < NB; k++) b[k] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
            }
        };
        bf16x8 bn[NB];
        int pidn = load_pid(cb0);
        load_b(bn, pidn);
        int pidnn = load_pid(cb0 + RG_CHUNK);
        __syncthreads();                                  // query images in LDS

        for (int cb = cb0; cb < ce; cb += RG_CHUNK) {
            bf16x8 b[NB];
#pragma unroll
            for (int k = 0; k < NB; k++) b[k] = bn[k];
            const int pid = pidn;
            pidn = pidnn;
            if (cb + RG_CHUNK < ce) load_b(bn, pidn);     // the next chunk's rows in flight while this one is scored
            pidnn = load_pid(cb + 2 * RG_CHUNK);
            auto score = [&](auto groups) {
                constexpr int R = decltype(groups)::value;
                f32x4 acc[R];
#pragma unroll
                for (int g = 0; g < R; g++) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int k = 0; k < NB; k++) {
#pragma unroll
                    for (int p = 0; p < 3; p++) {
#pragma unroll
                        for (int g = 0; g < R; g++)
                            acc[g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(q[p][(4 * k + h) * TM + g * 16 + c], b[k], acc[g], 0, 0, 0);
                    }
                }
                // C/D map: column lane & 15 (the candidate), row 4 (lane >> 4) + reg (the query row)
#pragma unroll
                for (int g = 0; g < R; g++) {
#pragma unroll
                    for (int k = 0; k < 4; k++) sc[g * 16 + 4 * h + k][wv * 16 + c] = acc[g][k];
                }
            };
            rg_dispatch_groups<RG>(rg, score);
            if (h == 0) cid[wv * 16 + c] = pid < 0 ? RG_NONE : pid;
            __syncthreads();
            rg_select_chunk<TM, EXCL>(sc, cid, rr, qq, valid, n, v, ix, hv, hix, elo, ehi, ex_col);
            __syncthreads();
        }
        rg_write_partial<TM>(v, ix, n, qq == 0 && rr < valid, ((size_t)(p0 + rr) * S + it.s) * n, pv, pi);
    }
}

extern "C" size_t pc_retrieve_topk_grouped_bf16_workspace_bytes(int rows, int n_types, int n, int slices) {
    return rg_topn_workspace_bytes(rows, n_types, n, RG_MAX_N, slices);
}

extern "C" int pc_retrieve_topk_grouped_bf16(const float* proj, const int32_t* types, const int32_t* row_key, int rows,
                                             const int32_t* type_rowptr, const int32_t* type_col, const uint16_t* table_bf16,
                                             int n_types, const int32_t* ex_rowptr, const int32_t* ex_col, int n_keys, int n,
                                             int dim, int slices, int32_t* out_idx, float* out_score, int32_t* bad_count,
                                             void* ws, size_t ws_bytes, void* stream) {
    PC_TRY(rg_topn_check(proj && types && type_rowptr && type_col && table_bf16 && out_idx && out_score && ws, rows, n_types,
                         rg_lists_ok(row_key, ex_rowptr, ex_col, bad_count, n_keys), n, RG_MAX_N, dim, slices));
    if ((uintptr_t)table_bf16 & 15) return PC_ESHAPE;     // a lane reads 16 bytes of a row at once
    const int S = rg_slices(slices);
    hipStream_t st = (hipStream_t)stream;
    RgWs w;
    unsigned grid;
    PC_TRY(rg_begin(w, grid, ws, ws_bytes, types, nullptr, rows, type_rowptr, n_types, 0, n, S, 8192 / dim, nullptr, nullptr, st));
    const RgPlan& pl = w.plan;
#define RB_SCORE(D, EXCL)                                                                                                   \
    PC_LAUNCH((rg_score_bf16_kernel<D, EXCL>), dim3(grid), dim3(256), 0, st, proj, type_rowptr, type_col, table_bf16, n_types, n, \
              S, pl.cnt, pl.row_start, pl.item_start, pl.order, w.pv, w.pi, row_key, rows, ex_rowptr, ex_col, n_keys, bad_count)
    if (dim == 128) {
        if (row_key) RB_SCORE(128, true); else RB_SCORE(128, false);
    } else {
        if (row_key) RB_SCORE(256, true); else RB_SCORE(256, false);
    }
#undef RB_SCORE
    rg_merge_launch(w, types, rows, type_rowptr, n_types, n, S, out_idx, out_score, st);
    return pc_launch_status();
}

