// Type-filtered top-n retrieval over a catalogue of any size (PCompanionInference.recommend, inference.py:90-118), grouped by
// type: the same contract as pc_retrieve_topk_dim (joint.hip), a different schedule.
//
// pc_retrieve_topk scores one (query, type) row per wave, so every row reads all candidate rows of its type again; at 10 M
// products / 100 types a 4096-query batch reads about 0.6 TB.  Here the rows of one type are gathered into tiles of TM
// rows (64 at D = 128, 32 at D = 256) and each tile scores its type's candidates as an fp32 GEMM on v_mfma_f32_16x16x4_f32:
// every candidate row is read once per tile, not once per row.  A large type's candidate range is split into up to S
// slices; every (tile, slice) work item keeps a running top-n per row and writes it as a partial list, and one wave per
// row merges the slices' lists.
//
//   plan    (grouped_plan.hip) count: rank[r] = atomic position of row r among the rows of its type, cnt[t] = rows of type
//           t; scan: row_start[t] = exclusive sum of cnt, item_start[t] = exclusive sum of tiles(t) * slices(t); place:
//           order[row_start[t] + rank[r]] = r
//   score   grid-stride over the work items (count read on the device): query tile -> LDS, candidates in chunks of 64
//           (one 16-candidate column group per wave, rows straight from global into registers, the next chunk's in
//           flight while this one is scored), scores -> LDS, a threshold test per (row, candidate), partial top-n per row
//   merge   one wave per row: the ns * n partial entries of its slices, n rounds of a wave-wide arg-max
//
// pc_retrieve_topk_grouped_excluding (PCompanionInference.set_exclusions): the same plan and merge around rg_score_excl_kernel,
// which drops the products of a per-row exclusion list before they enter a partial list (rg_score_body with EXCL).
//
// Determinism: a score is an MFMA k-chain whose order depends on the dimension index alone (step j, element e, k-lane h
// cover dimension 16 j + 4 h + e), never on the tile, the slice or the candidate's position, so a (row, product) pair has
// the same bits wherever it is scored.  Every selection is under the total order (score descending, product index
// ascending), so the top n of the union does not depend on how the candidates were split, on the order of the rows in a
// tile (the one thing the planning atomics decide), or on the order of type_col inside a type.  No float atomics.
#include "common.h"
#include "grouped_select.h"        // the lists of 16 (the decode, tile load, selection and write there are what the body writes out)

// The body of rg_score_kernel (EXCL false) and rg_score_excl_kernel (EXCL true).  Work item w = (type t, slice s, tile j),
// items of one type ordered slice-major so that the tiles running side by side read the same candidates (L2).  Lane l of
// wave wv: column c = l & 15 (candidate wv * 16 + c of the chunk, query row g * 16 + c of the A operand), k-lane h = l >> 4.
// Partial lists: pv / pi [rows][S][n] at the row's grouped position.
// EXCL, a per-row exclusion list (pc_retrieve_topk_grouped_excluding): a thread reads the bounds of its row's list once per
// work item (row_key -> ex_rowptr; a key outside [0, n_keys) is no list), and the selection drops a listed product before it
// enters a list.  The filter is a predicate of (row, product): the result does not depend on the slices, the rows' places or
// the order of type_col.  The prologue counts the keys outside [-1, n_keys) of ALL rows (grid-stride, one integer atomic each)
// in *bad_count.
template <int D, bool EXCL>
__device__ __forceinline__ void rg_score_body(const float* __restrict__ proj, const int32_t* __restrict__ type_rowptr,
                                              const int32_t* __restrict__ type_col, const float* __restrict__ table, int n_types,
                                              int n, int S, const int32_t* __restrict__ cnt, const int32_t* __restrict__ row_start,
                                              const int64_t* __restrict__ item_start, const int32_t* __restrict__ order,
                                              float* __restrict__ pv, int32_t* __restrict__ pi, const int32_t* __restrict__ row_key,
                                              int rows, const int32_t* __restrict__ ex_rowptr, const int32_t* __restrict__ ex_col,
                                              int n_keys, int32_t* __restrict__ bad_count) {
    constexpr int TM = 8192 / D;             // rows per tile: 64 (D = 128) or 32 (D = 256): a 32 KB query tile
    constexpr int RG = TM / 16;              // 16-row groups
    constexpr int QS = D + 4;                // padded LDS row
    constexpr int TPR = 256 / TM;            // threads per row in the selection phase
    constexpr int CPT = RG_CHUNK / TPR;      // candidates per thread per chunk
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
        // (rg_decode and rg_load_tile, written out)
        int lo = 0, hi = n_types - 1;                     // the largest t with item_start[t] <= w (< n_types: w < n_items)
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (item_start[mid] <= w) lo = mid; else hi = mid - 1;
        }
        const int t = lo;
        const int rows_t = cnt[t];
        const int tiles = (rows_t + TM - 1) / TM;
        const int local = (int)(w - item_start[t]);
        const int s = local / tiles, j = local - s * tiles;
        const int p0 = row_start[t] + j * TM;
        const int valid = min(TM, rows_t - j * TM);
        const int rg = (valid + 15) >> 4;
        const int c0 = type_rowptr[t], C = type_rowptr[t + 1] - c0;
        int ns, L;
        rg_slice_plan(C, S, ns, L);
        const int cb0 = c0 + s * L, ce = c0 + min(C, (s + 1) * L);

        __syncthreads();                                  // the previous item's readers of q are done
        for (int e = tid; e < rg * 16 * (D / 4); e += 256) {          // (rows past the last 16-row group are never read)
            const int row = e / (D / 4), d4 = e - row * (D / 4);
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row < valid) x = reinterpret_cast<const float4*>(proj + (size_t)order[p0 + row] * D)[d4];
            *reinterpret_cast<float4*>(&q[row * QS + 4 * d4]) = x;
        }
        float v[RG_MAX_N];
        int ix[RG_MAX_N];
#pragma unroll
        for (int k = 0; k < RG_MAX_N; k++) { v[k] = -INFINITY; ix[k] = RG_NONE; }
        float tv = -INFINITY, hv = -INFINITY;             // this thread's n-th entry; the row's threshold
        int ti = RG_NONE, hix = RG_NONE;
        int elo = 0, ehi = 0;                             // this thread's row's list: ex_col[elo, ehi)
        if constexpr (EXCL) {
            if (rr < valid) {
                const int key = row_key[order[p0 + rr]];
                if (key >= 0 && key < n_keys) { elo = ex_rowptr[key]; ehi = ex_rowptr[key + 1]; }
            }
        }

        auto load_pid = [&](int cb) { const int cc = cb + wv * 16 + c; return cc < ce ? type_col[cc] : -1; };
        auto load_b = [&](float4* b, int pid) {
            if (pid >= 0) {
                const float4* f = reinterpret_cast<const float4*>(table + (size_t)pid * D) + h;
#pragma unroll
                for (int k = 0; k < NB; k++) b[k] = f[4 * k];
            } else {
#pragma unroll
                for (int k = 0; k < NB; k++) b[k] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        };
        float4 bn[NB];
        int pidn = load_pid(cb0);
        load_b(bn, pidn);
        int pidnn = load_pid(cb0 + RG_CHUNK);
        __syncthreads();                                  // query tile in LDS

        for (int cb = cb0; cb < ce; cb += RG_CHUNK) {
            float4 b[NB];
#pragma unroll
            for (int k = 0; k < NB; k++) b[k] = bn[k];
            const int pid = pidn;
            pidn = pidnn;
            if (cb + RG_CHUNK < ce) load_b(bn, pidn);     // the next chunk's rows in flight while this one is scored
            pidnn = load_pid(cb + 2 * RG_CHUNK);
            f32x4 acc[RG];
#pragma unroll
            for (int g = 0; g < RG; g++) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < NB; k++) {
#pragma unroll
                for (int g = 0; g < RG; g++) {
                    if (g < rg) {
                        const float4 a = *reinterpret_cast<const float4*>(&q[(g * 16 + c) * QS + 16 * k + 4 * h]);
                        acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b[k].x, acc[g], 0, 0, 0);
                        acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b[k].y, acc[g], 0, 0, 0);
                        acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b[k].z, acc[g], 0, 0, 0);
                        acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b[k].w, acc[g], 0, 0, 0);
                    }
                }
            }
            // C/D map of the 16x16 f32 MFMA: column lane & 15 (the candidate), row 4 (lane >> 4) + reg (the query row)
#pragma unroll
            for (int g = 0; g < RG; g++)
                if (g < rg) {
#pragma unroll
                    for (int k = 0; k < 4; k++) sc[g * 16 + 4 * h + k][wv * 16 + c] = acc[g][k];
                }
            if (h == 0) cid[wv * 16 + c] = pid < 0 ? RG_NONE : pid;
            __syncthreads();
            // rg_select_chunk<TM, EXCL> (grouped_select.h: what the test and the loop do, and why), written out like the decode,
            // the tile load and the partial-list write: as a call the selection puts some 40 vector registers of the D = 128
            // kernels into scratch, and rg_decode or rg_load_tile cost rg_score_kernel<128> 1 % at 10 M products
            unsigned keep = 0;
            if (rr < valid) {
#pragma unroll
                for (int k = 0; k < CPT; k++) {
                    const int col = qq + TPR * k;
                    const int xi = cid[col];
                    if (xi != RG_NONE && rg_better(sc[rr][col], xi, hv, hix)) keep |= 1u << k;
                }
            }
            while (keep) {
                const int k = __builtin_ctz(keep);
                keep &= keep - 1;
                const int col = qq + TPR * k;
                const int xi = cid[col];
                const float x = sc[rr][col];
                if (rg_better(x, xi, hv, hix)) {
                    if constexpr (EXCL) {
                        int a = elo, b = ehi;                 // the first list entry >= xi
                        while (a < b) {
                            const int mid = (a + b) >> 1;
                            if (ex_col[mid] < xi) a = mid + 1; else b = mid;
                        }
                        if (a < ehi && ex_col[a] == xi) continue;         // excluded: never inserted, the threshold stays
                    }
                    rg_insert(v, ix, n, x, xi);
                    rg_nth(v, ix, n, tv, ti);
                    if (rg_better(tv, ti, hv, hix)) { hv = tv; hix = ti; }
                }
            }
#pragma unroll
            for (int o = TPR / 2; o >= 1; o >>= 1) {
                const float ov = __shfl_xor(hv, o, 64);
                const int oi = __shfl_xor(hix, o, 64);
                if (rg_better(ov, oi, hv, hix)) { hv = ov; hix = oi; }
            }
            __syncthreads();
        }
        for (int k = 0; k < n; k++) {
            float bv = v[0];
            int bi = ix[0];
#pragma unroll
            for (int o = TPR / 2; o >= 1; o >>= 1) {
                const float ov = __shfl_xor(bv, o, 64);
                const int oi = __shfl_xor(bi, o, 64);
                if (rg_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
            }
            if (ix[0] == bi && bi != RG_NONE) rg_pop(v, ix);
            if (qq == 0 && rr < valid) {
                const size_t o = ((size_t)(p0 + rr) * S + s) * n + k;
                pv[o] = bv;
                pi[o] = bi;
            }
        }
    }
}

// three waves per SIMD at D = 128 (the LDS allows three workgroups per CU); at D = 256 two, which it needs to keep its
// registers out of scratch
template <int D>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(D == 128 ? 3 : 2))) void rg_score_kernel(
    const float* __restrict__ proj, const int32_t* __restrict__ type_rowptr, const int32_t* __restrict__ type_col,
    const float* __restrict__ table, int n_types, int n, int S, const int32_t* __restrict__ cnt,
    const int32_t* __restrict__ row_start, const int64_t* __restrict__ item_start, const int32_t* __restrict__ order,
    float* __restrict__ pv, int32_t* __restrict__ pi) {
    rg_score_body<D, false>(proj, type_rowptr, type_col, table, n_types, n, S, cnt, row_start, item_start, order, pv, pi, nullptr, 0,
                            nullptr, nullptr, 0, nullptr);
}

template <int D>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(D == 128 ? 3 : 2))) void rg_score_excl_kernel(
    const float* __restrict__ proj, const int32_t* __restrict__ type_rowptr, const int32_t* __restrict__ type_col,
    const float* __restrict__ table, int n_types, int n, int S, const int32_t* __restrict__ cnt,
    const int32_t* __restrict__ row_start, const int64_t* __restrict__ item_start, const int32_t* __restrict__ order,
    float* __restrict__ pv, int32_t* __restrict__ pi, const int32_t* __restrict__ row_key, int rows,
    const int32_t* __restrict__ ex_rowptr, const int32_t* __restrict__ ex_col, int n_keys, int32_t* __restrict__ bad_count) {
    rg_score_body<D, true>(proj, type_rowptr, type_col, table, n_types, n, S, cnt, row_start, item_start, order, pv, pi, row_key,
                           rows, ex_rowptr, ex_col, n_keys, bad_count);
}

// One wave per row: the top n of its slices' partial lists (retrieve_topk_kernel's wave-wide arg-max pop).  THE merge of every
// entry with lists of up to 16 -- this unit's, retrieve_bf16.hip's and nearest.hip's -- through rg_merge_launch (grouped_plan.h).
// (Defined in this unit, as its last plain function: build.py's text digest of a kernel covers the padding behind it in the code
// object, and here the kernel keeps the digest it had before the three units shared it.)
__global__ __launch_bounds__(256) void rg_merge_kernel(const int32_t* __restrict__ types, int rows,
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
    float v[RG_MAX_N];
    int ix[RG_MAX_N];
#pragma unroll
    for (int k = 0; k < RG_MAX_N; k++) { v[k] = -INFINITY; ix[k] = RG_NONE; }
    const size_t base = (size_t)p * S * n;
    for (int e = lane; e < ns * n; e += 64) {
        const int xi = pi[base + e];
        if (xi != RG_NONE) rg_insert(v, ix, n, pv[base + e], xi);
    }
    for (int k = 0; k < n; k++) {
        float bv = v[0];
        int bi = ix[0];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const float ov = __shfl_xor(bv, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (rg_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
        }
        if (ix[0] == bi && bi != RG_NONE) rg_pop(v, ix);
        if (lane == 0) {
            out_idx[(size_t)r * n + k] = bi == RG_NONE ? -1 : bi;
            out_score[(size_t)r * n + k] = bi == RG_NONE ? -INFINITY : bv;
        }
    }
}

void rg_merge_launch(const RgWs& w, const int32_t* types, int rows, const int32_t* type_rowptr, int n_types, int n, int S,
                     int32_t* out_idx, float* out_score, hipStream_t st) {
    PC_LAUNCH(rg_merge_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, types, rows, type_rowptr, n_types, n, S, w.plan.pos,
              w.plan.row_start, w.pv, w.pi, out_idx, out_score);
}

extern "C" size_t pc_retrieve_topk_grouped_workspace_bytes(int rows, int n_types, int n, int slices) {
    return rg_topn_workspace_bytes(rows, n_types, n, RG_MAX_N, slices);
}

extern "C" int pc_retrieve_topk_grouped(const float* proj, const int32_t* types, int rows, const int32_t* type_rowptr,
                                        const int32_t* type_col, const float* table, int n_types, int n, int dim, int slices,
                                        int32_t* out_idx, float* out_score, void* ws, size_t ws_bytes, void* stream) {
    PC_TRY(rg_topn_check(proj && types && type_rowptr && type_col && table && out_idx && out_score && ws, rows, n_types, true, n,
                         RG_MAX_N, dim, slices));
    const int S = rg_slices(slices);
    hipStream_t st = (hipStream_t)stream;
    RgWs w;
    unsigned grid;
    PC_TRY(rg_begin(w, grid, ws, ws_bytes, types, nullptr, rows, type_rowptr, n_types, 0, n, S, 8192 / dim, nullptr, nullptr, st));
    const RgPlan& pl = w.plan;
    if (dim == 128)
        PC_LAUNCH(rg_score_kernel<128>, dim3(grid), dim3(256), 0, st, proj, type_rowptr, type_col, table, n_types, n, S, pl.cnt,
                  pl.row_start, pl.item_start, pl.order, w.pv, w.pi);
    else
        PC_LAUNCH(rg_score_kernel<256>, dim3(grid), dim3(256), 0, st, proj, type_rowptr, type_col, table, n_types, n, S, pl.cnt,
                  pl.row_start, pl.item_start, pl.order, w.pv, w.pi);
    rg_merge_launch(w, types, rows, type_rowptr, n_types, n, S, out_idx, out_score, st);
    return pc_launch_status();
}

extern "C" size_t pc_retrieve_topk_grouped_excluding_workspace_bytes(int rows, int n_types, int n, int slices) {
    return pc_retrieve_topk_grouped_workspace_bytes(rows, n_types, n, slices);
}

extern "C" int pc_retrieve_topk_grouped_excluding(const float* proj, const int32_t* types, const int32_t* row_key, int rows,
                                                  const int32_t* type_rowptr, const int32_t* type_col, const float* table,
                                                  int n_types, const int32_t* ex_rowptr, const int32_t* ex_col, int n_keys,
                                                  int n, int dim, int slices, int32_t* out_idx, float* out_score,
                                                  int32_t* bad_count, void* ws, size_t ws_bytes, void* stream) {
    PC_TRY(rg_topn_check(proj && types && row_key && type_rowptr && type_col && table && ex_rowptr && ex_col && out_idx &&
                             out_score && bad_count && ws,
                         rows, n_types, n_keys >= 0, n, RG_MAX_N, dim, slices));
    const int S = rg_slices(slices);
    hipStream_t st = (hipStream_t)stream;
    RgWs w;
    unsigned grid;
    PC_TRY(rg_begin(w, grid, ws, ws_bytes, types, nullptr, rows, type_rowptr, n_types, 0, n, S, 8192 / dim, nullptr, nullptr, st));
    const RgPlan& pl = w.plan;
    if (dim == 128)
        PC_LAUNCH(rg_score_excl_kernel<128>, dim3(grid), dim3(256), 0, st, proj, type_rowptr, type_col, table, n_types, n, S,
                  pl.cnt, pl.row_start, pl.item_start, pl.order, w.pv, w.pi, row_key, rows, ex_rowptr, ex_col, n_keys, bad_count);
    else
        PC_LAUNCH(rg_score_excl_kernel<256>, dim3(grid), dim3(256), 0, st, proj, type_rowptr, type_col, table, n_types, n, S,
                  pl.cnt, pl.row_start, pl.item_start, pl.order, w.pv, w.pi, row_key, rows, ex_rowptr, ex_col, n_keys, bad_count);
    rg_merge_launch(w, types, rows, type_rowptr, n_types, n, S, out_idx, out_score, st);
    return pc_launch_status();
}

