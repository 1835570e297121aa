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
// which drops the products of a per-row exclusion list before they enter a partial list (see that kernel).
//
// Determinism: a score is an MFMA k-chain whose order depends on the dimension index alone (step j, element e, k-lane h
// cover dimension 16 j + 4 h + e), never on the tile, the slice or the candidate's position, so a (row, product) pair has
// the same bits wherever it is scored.  Every selection is under the total order (score descending, product index
// ascending), so the top n of the union does not depend on how the candidates were split, on the order of the rows in a
// tile (the one thing the planning atomics decide), or on the order of type_col inside a type.  No float atomics.
#include "common.h"
#include "grouped_plan.h"          // the constants, the plan, rg_better, the item decode and tile load (shared with rank.hip)

#define RG_MAX_N 16

// insert (x, xi) into the descending list v / ix of length n (the caller has checked it beats the n-th entry)
__device__ __forceinline__ void rg_insert(float* v, int* ix, int n, float x, int xi) {
#pragma unroll
    for (int j = 0; j < RG_MAX_N; j++) {
        if (j < n && rg_better(x, xi, v[j], ix[j])) {
            const float tv = v[j]; const int ti = ix[j];
            v[j] = x; ix[j] = xi; x = tv; xi = ti;
        }
    }
}
__device__ __forceinline__ void rg_nth(const float* v, const int* ix, int n, float& tv, int& ti) {
#pragma unroll
    for (int j = 0; j < RG_MAX_N; j++)
        if (j == n - 1) { tv = v[j]; ti = ix[j]; }
}
__device__ __forceinline__ void rg_pop(float* v, int* ix) {
#pragma unroll
    for (int j = 0; j < RG_MAX_N - 1; j++) { v[j] = v[j + 1]; ix[j] = ix[j + 1]; }
    v[RG_MAX_N - 1] = -INFINITY; ix[RG_MAX_N - 1] = RG_NONE;
}

// Work item w = (type t, slice s, tile j), items of one type ordered slice-major so that the tiles running side by side read
// the same candidates (L2).  Lane l of wave wv: column c = l & 15 (candidate wv * 16 + c of the chunk, query row g * 16 + c
// of the A operand), k-lane h = l >> 4.  Partial lists: pv / pi [rows][S][n] at the row's grouped position.
template <int D>
// three waves per SIMD at D = 128 (the LDS allows three workgroups per CU); at D = 256 two, which it needs to keep its
// registers out of scratch
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(D == 128 ? 3 : 2))) void rg_score_kernel(const float* __restrict__ proj, const int32_t* __restrict__ type_rowptr,
                                                       const int32_t* __restrict__ type_col, const float* __restrict__ table,
                                                       int n_types, int n, int S, const int32_t* __restrict__ cnt,
                                                       const int32_t* __restrict__ row_start,
                                                       const int64_t* __restrict__ item_start,
                                                       const int32_t* __restrict__ order, float* __restrict__ pv,
                                                       int32_t* __restrict__ pi) {
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
    for (int64_t w = blockIdx.x; w < n_items; w += gridDim.x) {
        // (this decode and the tile load below are rank.hip's rk_rank_kernel; as a shared function they move both kernels' code)
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
            // a candidate that does not beat the row's threshold -- the best of the TPR threads' n-th entries, so n products
            // of the row beat it -- is out.  The test is cheap; the insertions then run as a loop over each lane's own
            // survivors, so a wave pays for its busiest lane, not for every candidate some lane keeps.
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
        // the TPR lists of a row (adjacent lanes) -> the slice's top n of the row
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

// rg_score_kernel with a per-row exclusion list (pc_retrieve_topk_grouped_excluding): the same tiling, chunking, register
// prefetch and score chain, written out again and not shared -- a body shared with rg_score_kernel moves that kernel's
// instructions, and the unfiltered path keeps its text.  What is added: a thread reads the bounds of its row's list once per
// work item (row_key -> ex_rowptr; a key outside [0, n_keys) is no list); a candidate that has passed the threshold test is
// searched in the list by bisection (the ids of a key are strictly ascending) and dropped BEFORE rg_insert, so an excluded
// product never enters a list and never moves a threshold: the threshold is still beaten by n kept products of the row.
// Most candidates fail the threshold test after the first chunks, so the search is paid by the few survivors.  The filter is
// a predicate of (row, product): the result does not depend on the slices, the rows' places or the order of type_col.
// The prologue counts the keys outside [-1, n_keys) of ALL rows (grid-stride, one integer atomic each) in *bad_count.
template <int D>
// three waves per SIMD at D = 128 (the LDS allows three workgroups per CU); at D = 256 two, which it needs to keep its
// registers out of scratch
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(D == 128 ? 3 : 2))) void rg_score_excl_kernel(const float* __restrict__ proj, const int32_t* __restrict__ type_rowptr,
                                                       const int32_t* __restrict__ type_col, const float* __restrict__ table,
                                                       int n_types, int n, int S, const int32_t* __restrict__ cnt,
                                                       const int32_t* __restrict__ row_start,
                                                       const int64_t* __restrict__ item_start,
                                                       const int32_t* __restrict__ order, float* __restrict__ pv,
                                                       int32_t* __restrict__ pi, const int32_t* __restrict__ row_key,
                                                       int rows, const int32_t* __restrict__ ex_rowptr,
                                                       const int32_t* __restrict__ ex_col, int n_keys,
                                                       int32_t* __restrict__ bad_count) {
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
    for (int r = blockIdx.x * 256 + tid; r < rows; r += gridDim.x * 256) {
        const int key = row_key[r];
        if (key < -1 || key >= n_keys) atomicAdd(bad_count, 1);
    }
    for (int64_t w = blockIdx.x; w < n_items; w += gridDim.x) {
        // (rg_score_kernel's decode and tile load)
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
        if (rr < valid) {
            const int key = row_key[order[p0 + rr]];
            if (key >= 0 && key < n_keys) { elo = ex_rowptr[key]; ehi = ex_rowptr[key + 1]; }
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
            // a candidate that does not beat the row's threshold -- the best of the TPR threads' n-th entries, so n products
            // of the row beat it -- is out.  The test is cheap; the insertions then run as a loop over each lane's own
            // survivors, so a wave pays for its busiest lane, not for every candidate some lane keeps.
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
                    int a = elo, b = ehi;                 // the first list entry >= xi
                    while (a < b) {
                        const int mid = (a + b) >> 1;
                        if (ex_col[mid] < xi) a = mid + 1; else b = mid;
                    }
                    if (a < ehi && ex_col[a] == xi) continue;         // excluded: never inserted, the threshold stays
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
        // the TPR lists of a row (adjacent lanes) -> the slice's top n of the row
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

// Instantiated here, by name: an implicit instantiation is emitted after every other kernel of the unit and would then follow
// rg_score_kernel<256> in the code object's text, whose end (and with it that kernel's instruction-text digest) it changes.
#define RG_EXCL_INSTANCE(D)                                                                                                    \
    template __global__ void rg_score_excl_kernel<D>(const float*, const int32_t*, const int32_t*, const float*, int, int, int, \
                                                     const int32_t*, const int32_t*, const int64_t*, const int32_t*, float*,   \
                                                     int32_t*, const int32_t*, int, const int32_t*, const int32_t*, int, int32_t*)
RG_EXCL_INSTANCE(128);
RG_EXCL_INSTANCE(256);

// One wave per row: the top n of its slices' partial lists (retrieve_topk_kernel's wave-wide arg-max pop).
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

namespace {
struct RgWs {
    RgPlan plan;
    float* pv;                             // the partial lists [rows][S][n]
    int32_t* pi;
    size_t bytes;
};
RgWs rg_layout(void* ws, int rows, int n_types, int n, int S) {
    RgWs w;
    WsCarver cv(ws);
    w.plan = rg_plan_carve(cv, rows, n_types);
    w.pv = (float*)cv.bytes((size_t)rows * S * n * 4);
    w.pi = (int32_t*)cv.bytes((size_t)rows * S * n * 4);
    w.bytes = cv.total;
    return w;
}
}  // namespace

extern "C" size_t pc_retrieve_topk_grouped_workspace_bytes(int rows, int n_types, int n, int slices) {
    if (rows <= 0 || n_types <= 0 || n < 1 || n > RG_MAX_N || slices < 0 || slices > RG_MAX_SLICES) return 0;
    return rg_layout(nullptr, rows, n_types, n, rg_slices(slices)).bytes;
}

extern "C" int pc_retrieve_topk_grouped(const float* proj, const int32_t* types, int rows, const int32_t* type_rowptr,
                                        const int32_t* type_col, const float* table, int n_types, int n, int dim, int slices,
                                        int32_t* out_idx, float* out_score, void* ws, size_t ws_bytes, void* stream) {
    if (!proj || !types || !type_rowptr || !type_col || !table || !out_idx || !out_score || !ws) return PC_EINVAL;
    if (rows <= 0 || n_types <= 0) return PC_EINVAL;
    if (n < 1 || n > RG_MAX_N || (dim != 128 && dim != 256) || slices < 0 || slices > RG_MAX_SLICES) return PC_ESHAPE;
    const int S = rg_slices(slices);
    const RgWs w = rg_layout(ws, rows, n_types, n, S);
    if (ws_bytes < w.bytes) return PC_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int TM = 8192 / dim;
    const RgPlan& pl = w.plan;
    PC_TRY(rg_plan_launch(pl, types, nullptr, rows, type_rowptr, n_types, 0, S, TM, nullptr, nullptr, st));
    const dim3 sgrid(rg_item_grid(rows, n_types, S, TM));
    if (dim == 128)
        PC_LAUNCH(rg_score_kernel<128>, sgrid, dim3(256), 0, st, proj, type_rowptr, type_col, table, n_types, n, S, pl.cnt,
                  pl.row_start, pl.item_start, pl.order, w.pv, w.pi);
    else
        PC_LAUNCH(rg_score_kernel<256>, sgrid, dim3(256), 0, st, proj, type_rowptr, type_col, table, n_types, n, S, pl.cnt,
                  pl.row_start, pl.item_start, pl.order, w.pv, w.pi);
    PC_LAUNCH(rg_merge_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, types, rows, type_rowptr, n_types, n, S, pl.pos,
              pl.row_start, w.pv, w.pi, out_idx, out_score);
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
    if (!proj || !types || !row_key || !type_rowptr || !type_col || !table || !ex_rowptr || !ex_col || !out_idx || !out_score ||
        !bad_count || !ws)
        return PC_EINVAL;
    if (rows <= 0 || n_types <= 0 || n_keys < 0) return PC_EINVAL;
    if (n < 1 || n > RG_MAX_N || (dim != 128 && dim != 256) || slices < 0 || slices > RG_MAX_SLICES) return PC_ESHAPE;
    const int S = rg_slices(slices);
    const RgWs w = rg_layout(ws, rows, n_types, n, S);
    if (ws_bytes < w.bytes) return PC_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const int TM = 8192 / dim;
    const RgPlan& pl = w.plan;
    PC_TRY(rg_plan_launch(pl, types, nullptr, rows, type_rowptr, n_types, 0, S, TM, nullptr, nullptr, st));
    const dim3 sgrid(rg_item_grid(rows, n_types, S, TM));
    if (dim == 128)
        PC_LAUNCH(rg_score_excl_kernel<128>, sgrid, dim3(256), 0, st, proj, type_rowptr, type_col, table, n_types, n, S, pl.cnt,
                  pl.row_start, pl.item_start, pl.order, w.pv, w.pi, row_key, rows, ex_rowptr, ex_col, n_keys, bad_count);
    else
        PC_LAUNCH(rg_score_excl_kernel<256>, sgrid, dim3(256), 0, st, proj, type_rowptr, type_col, table, n_types, n, S, pl.cnt,
                  pl.row_start, pl.item_start, pl.order, w.pv, w.pi, row_key, rows, ex_rowptr, ex_col, n_keys, bad_count);
    PC_LAUNCH(rg_merge_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, types, rows, type_rowptr, n_types, n, S, pl.pos,
              pl.row_start, w.pv, w.pi, out_idx, out_score);
    return pc_launch_status();
}
