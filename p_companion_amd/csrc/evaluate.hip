// Metrics.evaluate_model (src/utils/metrics.py:62-117) over a device-resident validation split as ONE call
// (pc_joint_eval_epoch), and its per-batch statistics for tensors the caller holds (pc_eval_batch_stats).
//
// In eval mode a sample's similarity row and its top-K are a function of its query TYPE alone, and the weights do not change
// during an evaluation.  So:
//
//   plan    once per evaluation, over row chunks of EV_PLAN_ROWS types (the launches of joint_forward_impl with rows = types):
//           topk_table[t, :K] = top-K of dec(relu(enc(E_q[t]))) . E_c^T, tp_table[t, k, :] = type_projection(E_c[topk_table[t, k]]).
//           The [rows, T] similarity chunk is the only scratch that depends on T; it is linear in T.
//   per batch of B labelled pairs (query, target, label):
//     prep    ids from the pair list, clamped and counted into *bad_count; beat[] and the column mask cleared
//     pi      item_projection(E_prod[query])                     (the shared NT GEMM with a row gather)
//     rows    one group of D/4 lanes per sample: proj[b,k,:] = pi[b] * tp_table[type(query_b), k, :] (only the eligible rows
//             r = b K + k < B reach memory), cos[b,k] against the positive row -- features[target] for label +1, the loader's
//             filler row for label -1, formed here with pc_filler_chunk: the builder's bits -- and the pairs of columns of
//             complementary_types [B,K] that differ in some row (an integer OR)
//     count   the B x B x D product proj_r . y_c of the eligible rows against y_c = features[target_c] on
//             v_mfma_f32_16x16x4_f32, work item = (tile of TM rows, column slice): the row tile in LDS, candidate rows straight
//             into registers with the next chunk in flight (retrieve.hip's schedule); the epilogue is a compare against
//             g_r = proj_r . y_r and an integer count, beat[r] += #{c: s_rc > g_r or (s_rc == g_r and c < r)}: nothing of
//             size B x B is written (the reference's [B K, B] score matrix, metrics.py:95-100; its rows r >= B can never hit)
//     finish  hits_k = #{r < B: beat_r < min(k, B)} for k = 1, 3, min(10, B); cos summed in a fixed order; the distinct columns
//   final   one workgroup: the five metrics as metrics.py forms them, written as double[5]
//
// Determinism: a score is an MFMA k-chain whose order depends on the dimension index alone (step j, element e, k-lane h cover
// dimension 16 j + 4 h + e), never on the tile, the slice or the column's position.  Every work item first scores its row tile
// against the tile's OWN columns through that same chain and keeps the diagonal: g_r and s_rr are the same bits, so a row never
// counts itself, and a pair (r, c) compares the same two numbers whichever slice holds c.  The counts are integer sums (integer
// atomics), the cosine sum has a fixed order: no float atomics, results bitwise repeatable.
#include "common.h"

#define EV_MAX_K 8
#define EV_CHUNK 64                // columns per chunk: four waves x 16
#define EV_PLAN_ROWS 1024          // types per chunk of the plan
#define EV_ITEMS 512               // work items the count launch aims for (256 CUs, two workgroups each)
#ifndef EV_ROW_PAD
#define EV_ROW_PAD 4               // floats of padding behind a row of the LDS tile (developer A/B builds: -DEV_ROW_PAD=...)
#endif
#define EV_MIN_ROWS 10             // a batch of fewer rows makes metrics.py:103's key min(10, cols) a new one

struct EvalWs {
    int32_t* topk_table;           // [T, K]        (FIRST: tests and probes read the plan's types back from ws)
    float* tp_table;               // [T, K, D]
    float *h, *c, *sims;           // plan scratch: [PR, L/2], [PR, L], [PR, T]
    int32_t *qidx, *tgt, *qtype;   // [B] each
    int32_t* beat;                 // [B]
    int32_t* diffmask;             // [1]
    float *pi, *proj, *cos;        // [B, D], [B, D] (the eligible rows), [B K]
    size_t total;
};

static EvalWs eval_ws_layout(void* base, int B, int T, int K, int D) {
    EvalWs w;
    WsCarver cv(base);
    auto take = [&](size_t bytes) { return cv.bytes(bytes); };
    const size_t pr = T < EV_PLAN_ROWS ? T : EV_PLAN_ROWS;
    w.topk_table = (int32_t*)take((size_t)T * K * 4);
    w.tp_table = (float*)take((size_t)T * K * D * 4);
    w.h = (float*)take(pr * (PC_L / 2) * 4);
    w.c = (float*)take(pr * PC_L * 4);
    w.sims = (float*)take(pr * (size_t)T * 4);
    w.qidx = (int32_t*)take((size_t)B * 4);
    w.tgt = (int32_t*)take((size_t)B * 4);
    w.qtype = (int32_t*)take((size_t)B * 4);
    w.beat = (int32_t*)take((size_t)B * 4);
    w.diffmask = (int32_t*)take(4);
    w.pi = (float*)take((size_t)B * D * 4);
    w.proj = (float*)take((size_t)B * D * 4);
    w.cos = (float*)take((size_t)B * K * 4);
    w.total = cv.total;
    return w;
}

extern "C" size_t pc_joint_eval_workspace_bytes(int batch, int num_types, int k, int dim) {
    if (batch <= 0 || num_types <= 0 || k < 1 || k > EV_MAX_K || (dim != 128 && dim != 256)) return 0;
    return eval_ws_layout(nullptr, batch, num_types, k, dim).total;
}

// Column slices of a batch of B columns: ns slices of L columns (L a multiple of the chunk, the last slice shorter), none empty.
static inline void ev_slice_plan(int B, int TM, int& ns, int& L) {
    const int tiles = (B + TM - 1) / TM;
    int want = (EV_ITEMS + tiles - 1) / tiles;
    const int chunks = (B + EV_CHUNK - 1) / EV_CHUNK;
    if (want > chunks) want = chunks;
    if (want < 1) want = 1;
    const int per = (B + want - 1) / want;
    L = (per + EV_CHUNK - 1) / EV_CHUNK * EV_CHUNK;
    ns = (B + L - 1) / L;
}

// ---- prep: the batch's ids from the pair list; anything outside its table is clamped and counted, never dereferenced
__global__ __launch_bounds__(256) void eval_prep_kernel(const int32_t* __restrict__ pairs, int B, const int32_t* __restrict__ type_idx,
                                                        int num_products, int num_types, int32_t* __restrict__ qidx,
                                                        int32_t* __restrict__ tgt, int32_t* __restrict__ qtype,
                                                        int32_t* __restrict__ beat, int32_t* __restrict__ diffmask,
                                                        int32_t* __restrict__ bad_count) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b == 0) *diffmask = 0;
    if (b >= B) return;
    int q = pairs[3 * b], tg = pairs[3 * b + 1], bad = 0;
    if ((unsigned)q >= (unsigned)num_products) { q = 0; bad++; }
    if ((unsigned)tg >= (unsigned)num_products) { tg = 0; bad++; }
    int qt = type_idx[q];
    if ((unsigned)qt >= (unsigned)num_types) { qt = 0; bad++; }
    qidx[b] = q; tgt[b] = tg; qtype[b] = qt;
    beat[b] = 0;
    if (bad && bad_count) atomicAdd(bad_count, bad);
}

// ---- rows: projected rows, cosines and the column-difference mask, one group of D / 4 lanes per sample
struct EvalRowsArgs {
    int B, K;
    // tensors the caller holds (pc_eval_batch_stats)
    const float* proj; const float* pos; const int32_t* types;
    // the epoch's batch
    const float* pi; const float* tp_table; const int32_t* topk_table;
    const int32_t *qtype, *tgt, *pairs; const float* features;
    uint64_t seed, step;
    float* proj_out;               // rows r < B of the flat [B K, D] projection
    float* cos; int32_t* diffmask;
};

template <int G>
__device__ __forceinline__ float ev_group_sum(float v) {
#pragma unroll
    for (int o = G / 2; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

template <int D, bool EPOCH>
__global__ __launch_bounds__(256) void eval_rows_kernel(EvalRowsArgs a) {
    constexpr int G = D / 4, SPB = 256 / G;
    const int l = threadIdx.x % G;
    const int bx = blockIdx.x * SPB + threadIdx.x / G;
    const bool live = bx < a.B;
    const int b = live ? bx : 0;
    float4 y;
    int qt = 0;
    if (EPOCH) {
        qt = a.qtype[b];
        const bool pos = a.pairs[3 * b + 2] == 1;
        const float4 f = *reinterpret_cast<const float4*>(a.features + (size_t)a.tgt[b] * D + 4 * l);
        const float4 fill = pc_filler_chunk(a.seed, a.step, (uint32_t)(b * G + l));
        // (component-wise selects: `pos ? f : fill` on the structs becomes an indexed stack array)
        y = make_float4(pos ? f.x : fill.x, pos ? f.y : fill.y, pos ? f.z : fill.z, pos ? f.w : fill.w);
    } else {
        y = *reinterpret_cast<const float4*>(a.pos + (size_t)b * D + 4 * l);
    }
    const float nb = sqrtf(ev_group_sum<G>(y.x * y.x + y.y * y.y + y.z * y.z + y.w * y.w));
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    if (EPOCH) p = *reinterpret_cast<const float4*>(a.pi + (size_t)b * D + 4 * l);
    int ty[EV_MAX_K];
#pragma unroll
    for (int k = 0; k < EV_MAX_K; k++) {
        ty[k] = 0;
        if (k < a.K) {
            float4 x;
            if (EPOCH) {
                ty[k] = a.topk_table[(size_t)qt * a.K + k];              // (only compared below, never an address)
                const float4 t = *reinterpret_cast<const float4*>(a.tp_table + ((size_t)qt * a.K + k) * D + 4 * l);
                x = make_float4(p.x * t.x, p.y * t.y, p.z * t.z, p.w * t.w);            // item_prediction.py:38
                const int r = b * a.K + k;
                if (live && r < a.B) *reinterpret_cast<float4*>(a.proj_out + (size_t)r * D + 4 * l) = x;
            } else {
                ty[k] = a.types[(size_t)b * a.K + k];
                x = *reinterpret_cast<const float4*>(a.proj + ((size_t)b * a.K + k) * D + 4 * l);
            }
            const float dot = ev_group_sum<G>(x.x * y.x + x.y * y.y + x.z * y.z + x.w * y.w);
            const float na = sqrtf(ev_group_sum<G>(x.x * x.x + x.y * x.y + x.z * x.z + x.w * x.w));
            // torch.cosine_similarity's eps (metrics.py:44-60), as cosine_rows_kernel
            if (live && l == 0) a.cos[(size_t)b * a.K + k] = dot / (fmaxf(na, 1e-8f) * fmaxf(nb, 1e-8f));
        }
    }
    // metrics.py:29-42 unique(dim=1): bit (i, j), i < j, is set when columns i and j differ in some row
    if (live && l == 0) {
        unsigned m = 0;
        int bit = 0;
#pragma unroll
        for (int j = 1; j < EV_MAX_K; j++)
#pragma unroll
            for (int i = 0; i < j; i++, bit++)
                if (j < a.K && ty[i] != ty[j]) m |= 1u << bit;
        if (m) atomicOr(a.diffmask, (int)m);
    }
}

// ---- count: work item blockIdx.x = (slice s, row tile j), slice-major so that the tiles running side by side read the same
// columns (L2).  Lane l of wave wv: column c = l & 15 (column wv * 16 + c of the chunk, row g * 16 + c of the A operand),
// k-lane h = l >> 4.
template <int D>
__global__ __launch_bounds__(256) void eval_count_kernel(const float* __restrict__ proj, const float* __restrict__ Y,
                                                         const int32_t* __restrict__ yidx, int B, int L,
                                                         int32_t* __restrict__ beat) {
    constexpr int TM = 8192 / D;             // rows per tile: 64 (D = 128) or 32 (D = 256): a 32 KB row tile
    constexpr int RG = TM / 16;              // 16-row groups
    constexpr int QS = D + EV_ROW_PAD;       // padded LDS row
    constexpr int NB = D / 16;               // float4 operands per lane per column
    __shared__ __attribute__((aligned(16))) float q[TM * QS];
    __shared__ float gs[TM];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, c = lane & 15, h = lane >> 4;
    const int tiles = (B + TM - 1) / TM;
    const int s = blockIdx.x / tiles, j = blockIdx.x - s * tiles;
    const int r0 = j * TM;
    const int valid = min(TM, B - r0);
    const int rg = (valid + 15) >> 4;
    const int cb0 = s * L, ce = min(B, (s + 1) * L);

    for (int e = tid; e < rg * 16 * (D / 4); e += 256) {              // (rows past the last 16-row group are never read)
        const int row = e / (D / 4), d4 = e - row * (D / 4);
        float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < valid) x = reinterpret_cast<const float4*>(proj + (size_t)(r0 + row) * D)[d4];
        *reinterpret_cast<float4*>(&q[row * QS + 4 * d4]) = x;
    }
    // column `col` of the batch: y_col = Y[yidx ? yidx[col] : col]; past `end`: zeros (never counted)
    auto load_b = [&](float4* b, int col, int end) {
        if (col < end) {
            const size_t row = yidx ? (size_t)yidx[col] : (size_t)col;
            const float4* f = reinterpret_cast<const float4*>(Y + row * D) + h;
#pragma unroll
            for (int k = 0; k < NB; k++) b[k] = f[4 * k];
        } else {
#pragma unroll
            for (int k = 0; k < NB; k++) b[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    // the ONE score chain: dimension 16 k + 4 h + e at step (k, e), for every (row, column) wherever it is formed
    auto score = [&](const float4* b, f32x4* acc) {
#pragma unroll
        for (int g = 0; g < RG; g++) acc[g] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < NB; k++) {
#pragma unroll
            for (int g = 0; g < RG; g++) {
                if (g < rg) {
                    const float4 x = *reinterpret_cast<const float4*>(&q[(g * 16 + c) * QS + 16 * k + 4 * h]);
                    acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.x, b[k].x, acc[g], 0, 0, 0);
                    acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.y, b[k].y, acc[g], 0, 0, 0);
                    acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.z, b[k].z, acc[g], 0, 0, 0);
                    acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.w, b[k].w, acc[g], 0, 0, 0);
                }
            }
        }
    };
    float4 bn[NB];
    load_b(bn, cb0 + wv * 16 + c, ce);                    // the slice's first chunk: in flight under the diagonal pass
    __syncthreads();                                      // row tile in LDS

    // ---- g_r = proj_r . y_r: the tile's own columns through the same chain; the diagonal stays
    // C/D map of the 16x16 f32 MFMA: column lane & 15, row 4 (lane >> 4) + reg
    for (int cb = r0; cb < r0 + valid; cb += EV_CHUNK) {
        float4 b[NB];
        const int col = cb + wv * 16 + c;
        load_b(b, col, r0 + valid);
        f32x4 acc[RG];
        score(b, acc);
#pragma unroll
        for (int g = 0; g < RG; g++)
            if (g < rg) {
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int row = r0 + g * 16 + 4 * h + k;
                    if (row == col && row < r0 + valid) gs[row - r0] = acc[g][k];
                }
            }
    }
    __syncthreads();
    float gv[RG][4];
    int cnt[RG][4];
#pragma unroll
    for (int g = 0; g < RG; g++)
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int row = g * 16 + 4 * h + k;
            gv[g][k] = row < valid ? gs[row] : 0.f;
            cnt[g][k] = 0;
        }

    // ---- the slice's columns: compare and count
    for (int cb = cb0; cb < ce; cb += EV_CHUNK) {
        float4 b[NB];
#pragma unroll
        for (int k = 0; k < NB; k++) b[k] = bn[k];
        if (cb + EV_CHUNK < ce) load_b(bn, cb + EV_CHUNK + wv * 16 + c, ce);      // the next chunk's rows in flight
        f32x4 acc[RG];
        score(b, acc);
        const int col = cb + wv * 16 + c;
        const bool cv = col < ce;
#pragma unroll
        for (int g = 0; g < RG; g++)
            if (g < rg) {
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int row = r0 + g * 16 + 4 * h + k;
                    const float v = acc[g][k], gr = gv[g][k];
                    cnt[g][k] += (cv && (v > gr || (v == gr && col < row))) ? 1 : 0;      // ties -> the lower index (hit_rank_kernel)
                }
            }
    }
    // the 16 column lanes of a k-lane group -> one integer per row and wave
#pragma unroll
    for (int g = 0; g < RG; g++)
#pragma unroll
        for (int k = 0; k < 4; k++) {
            int v = cnt[g][k];
#pragma unroll
            for (int o = 8; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
            const int row = g * 16 + 4 * h + k;
            if (c == 0 && row < valid && v) atomicAdd(&beat[r0 + row], v);
        }
}

// ---- finish (one workgroup): the batch's five integers and its cosine sum
__global__ __launch_bounds__(256) void eval_finish_kernel(const int32_t* __restrict__ beat, const float* __restrict__ cos,
                                                          const int32_t* __restrict__ diffmask, int B, int K,
                                                          int32_t* __restrict__ stats, float* __restrict__ cos_sum) {
    __shared__ int hi[3][256];
    __shared__ float cs[256];
    const int t = threadIdx.x;
    const int k1 = min(1, B), k3 = min(3, B), k10 = min(10, B);
    int h1 = 0, h3 = 0, h10 = 0;
    for (int r = t; r < B; r += 256) {
        const int v = beat[r];
        h1 += v < k1; h3 += v < k3; h10 += v < k10;
    }
    float sum = 0.f;
    for (int r = t; r < B * K; r += 256) sum += cos[r];               // fixed order: thread t adds rows t, t + 256, ...
    hi[0][t] = h1; hi[1][t] = h3; hi[2][t] = h10; cs[t] = sum;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {                              // ... and a fixed tree over the threads
        if (t < o) { hi[0][t] += hi[0][t + o]; hi[1][t] += hi[1][t + o]; hi[2][t] += hi[2][t + o]; cs[t] += cs[t + o]; }
        __syncthreads();
    }
    if (t == 0) {
        const unsigned m = (unsigned)*diffmask;
        int distinct = 0, bit = 0;
        for (int j = 0; j < K; j++) {                                 // column j is new iff it differs from every earlier column
            bool fresh = true;
            for (int i = 0; i < j; i++, bit++) fresh = fresh && ((m >> bit) & 1u);
            distinct += fresh ? 1 : 0;
        }
        stats[0] = hi[0][0]; stats[1] = hi[1][0]; stats[2] = hi[2][0]; stats[3] = distinct; stats[4] = B;
        *cos_sum = cs[0];
    }
}

// ---- final (one workgroup): metrics.py:101-117.  Per batch the three hit rates and the relevance are fp32 means over B K rows
// (torch's .float().mean()), the diversity a Python float division (metrics.py:42); the sum over the batches and the division
// by their number are Python floats: fp64, in batch order.  out = {hit@1, hit@3, hit@10, type_diversity, mean_relevance}.
__global__ __launch_bounds__(64) void eval_final_kernel(const int32_t* __restrict__ stats, const float* __restrict__ cos_sum,
                                                        int64_t n_batches, int K, double* __restrict__ out) {
    const int m = threadIdx.x;
    if (m >= 5) return;
    double acc = 0.0;
    for (int64_t i = 0; i < n_batches; i++) {
        const int32_t* s = stats + 5 * i;
        const float rows = (float)(s[4] * K);
        double v;
        if (m < 3) v = (double)((float)s[m] / rows);
        else if (m == 3) v = (double)s[3] / (double)K;
        else v = (double)(cos_sum[i] / rows);
        acc += v;
    }
    out[m] = acc / (double)(n_batches > 0 ? n_batches : 1);
}

template <bool EPOCH>
static void launch_rows(const EvalRowsArgs& a, int dim, hipStream_t st) {
    if (dim == 128) PC_LAUNCH((eval_rows_kernel<128, EPOCH>), dim3((a.B + 7) / 8), dim3(256), 0, st, a);
    else PC_LAUNCH((eval_rows_kernel<256, EPOCH>), dim3((a.B + 3) / 4), dim3(256), 0, st, a);
}

static void launch_count(const float* proj, const float* Y, const int32_t* yidx, int B, int dim, int32_t* beat, hipStream_t st) {
    const int TM = 8192 / dim;
    int ns, L;
    ev_slice_plan(B, TM, ns, L);
    const int tiles = (B + TM - 1) / TM;
    if (dim == 128) PC_LAUNCH(eval_count_kernel<128>, dim3(tiles * ns), dim3(256), 0, st, proj, Y, yidx, B, L, beat);
    else PC_LAUNCH(eval_count_kernel<256>, dim3(tiles * ns), dim3(256), 0, st, proj, Y, yidx, B, L, beat);
}

extern "C" int pc_eval_batch_stats(const float* proj, const float* targets, const float* pos_items, const int32_t* types,
                                   int batch, int k, int dim, int32_t* stats, float* cos_sum, void* ws, size_t ws_bytes,
                                   void* stream) {
    if (!proj || !targets || !pos_items || !types || !stats || !cos_sum || !ws || batch <= 0 || k <= 0) return PC_EINVAL;
    if ((dim != 128 && dim != 256) || k > EV_MAX_K) return PC_ESHAPE;
    if ((int64_t)batch * k * (dim / 4) >= (1ll << 31)) return PC_EINVAL;
    const EvalWs w = eval_ws_layout(ws, batch, 1, k, dim);
    if (ws_bytes < w.total) return PC_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    PC_HIP_TRY(hipMemsetAsync(w.beat, 0, (size_t)batch * 4, st));
    PC_HIP_TRY(hipMemsetAsync(w.diffmask, 0, 4, st));
    EvalRowsArgs a = {};
    a.B = batch; a.K = k; a.proj = proj; a.pos = pos_items; a.types = types; a.cos = w.cos; a.diffmask = w.diffmask;
    launch_rows<false>(a, dim, st);
    launch_count(proj, targets, nullptr, batch, dim, w.beat, st);
    PC_LAUNCH(eval_finish_kernel, dim3(1), dim3(256), 0, st, w.beat, w.cos, w.diffmask, batch, k, stats, cos_sum);
    return pc_launch_status();
}

extern "C" int pc_joint_eval_epoch(const pc_joint_tensors* p, const int32_t* pairs, int64_t n_pairs, const float* features,
                                   const int32_t* type_idx, int n_types, int dim, uint64_t seed, uint64_t first_step, int batch,
                                   int num_types, int k, int num_products, int32_t* stats_out, float* cos_sum_out,
                                   double* metrics_out, int32_t* bad_count, void* ws, size_t ws_bytes, void* stream) {
    if (!joint_tensors_ok(p, true)) return PC_EINVAL;
    if (!pairs || !features || !type_idx || !stats_out || !cos_sum_out || !metrics_out || !ws) return PC_EINVAL;
    if (n_pairs <= 0 || batch <= 0 || num_types <= 0 || n_types <= 0 || num_products <= 0) return PC_EINVAL;
    if (dim != 128 && dim != 256) return PC_ESHAPE;
    if (k < 1 || k > EV_MAX_K || k > num_types) return PC_ESHAPE;
    if ((int64_t)batch * k * (dim / 4) >= (1ll << 31)) return PC_EINVAL;
    const int64_t full = n_pairs / batch;
    const int rest = (int)(n_pairs % batch);
    // metrics.py:103: a batch of fewer than 10 rows has no 'hit@10' of its own (the reference raises KeyError or adds into
    // hit@1 / hit@3 twice): refused here, the caller's loop reproduces it
    if ((rest > 0 && rest < EV_MIN_ROWS) || (full > 0 && batch < EV_MIN_ROWS)) return PC_ESHAPE;
    const int T = num_types, K = k;
    const EvalWs w = eval_ws_layout(ws, batch, T, K, dim);
    if (ws_bytes < w.total) return PC_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;

    // ---- the type plan (p_companion.py:56-65 with rows = types; type_transition.py:17-19 in eval mode: no dropout)
    for (int t0 = 0; t0 < T; t0 += EV_PLAN_ROWS) {
        const int n = T - t0 < EV_PLAN_ROWS ? T - t0 : EV_PLAN_ROWS;
        PC_TRY(pc_linear_forward(p->query_types + (size_t)t0 * PC_L, nullptr, n, PC_L, p->enc_w, p->enc_b, PC_L / 2, 2, w.h, stream));
        PC_TRY(pc_linear_forward(w.h, nullptr, n, PC_L / 2, p->dec_w, p->dec_b, PC_L, 0, w.c, stream));
        PC_TRY(pc_linear_forward(w.c, nullptr, n, PC_L, p->comp_types, nullptr, T, 0, w.sims, stream));
        PC_TRY(pc_topk_rows(w.sims, n, T, K, w.topk_table + (size_t)t0 * K, nullptr, stream));
        PC_TRY(pc_linear_forward(p->comp_types, w.topk_table + (size_t)t0 * K, n * K, PC_L, p->typ_w, p->typ_b, dim, 0,
                                 w.tp_table + (size_t)t0 * K * dim, stream));
    }
    // ---- the batches, in loader order: full ones, then the ragged rest
    const int64_t n_batches = full + (rest ? 1 : 0);
    for (int64_t i = 0; i < n_batches; i++) {
        const int B = i < full ? batch : rest;
        const int32_t* pr = pairs + 3 * i * (int64_t)batch;
        PC_LAUNCH(eval_prep_kernel, dim3((B + 255) / 256), dim3(256), 0, st, pr, B, type_idx, num_products, T, w.qidx, w.tgt,
                  w.qtype, w.beat, w.diffmask, bad_count);
        // pi = item_projection(E_prod[query])                 item_prediction.py:31, p_companion.py:51
        PC_TRY(pc_linear_forward(p->product_table, w.qidx, B, dim, p->itm_w, p->itm_b, dim, 0, w.pi, stream));
        EvalRowsArgs a = {};
        a.B = B; a.K = K; a.pi = w.pi; a.tp_table = w.tp_table; a.topk_table = w.topk_table;
        a.qtype = w.qtype; a.tgt = w.tgt; a.pairs = pr; a.features = features; a.seed = seed; a.step = first_step + (uint64_t)i;
        a.proj_out = w.proj; a.cos = w.cos; a.diffmask = w.diffmask;
        launch_rows<true>(a, dim, st);
        launch_count(w.proj, features, w.tgt, B, dim, w.beat, st);
        PC_LAUNCH(eval_finish_kernel, dim3(1), dim3(256), 0, st, w.beat, w.cos, w.diffmask, B, K, stats_out + 5 * i,
                  cos_sum_out + i);
    }
    PC_LAUNCH(eval_final_kernel, dim3(1), dim3(64), 0, st, stats_out, cos_sum_out, n_batches, K, metrics_out);
    return pc_launch_status();
}
