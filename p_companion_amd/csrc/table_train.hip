// A trainable product table in the joint step (a labelled extension; one device, world = 1).
//
// In the reference's batch layout only the QUERY row reaches the product table (q_b = E_prod[query_idx[b]],
// p_companion.py:51; positive_items / negative_items are feature rows of the batch), so the rows with a gradient are exactly
// query_idx, and the only path is the item hinge through item_projection.  Two entries:
//
//   pc_joint_query_grad   dq[b] = W_item^T sum_k dx_bk * tp_bk for the K predicted types of the step that just ran.  The two
//                         [B, D] x [D, D] products and the type projection go through the library's NT GEMM; the row-wise
//                         pass between them (x = pi * tp, both norms, the hinge, dpi) is one wave per sample -- the item half
//                         of joint_rowwise_kernel, same expressions, for D = 128 and 256.
//   pc_sparse_adam_rows   torch.optim.SparseAdam over the rows named by idx [R] (duplicates expected): block_ops.h's LSD radix sort
//                         of (id, r) by id, stable -- so the sources of a row stay in ascending r -- then one wave per
//                         distinct row sums its sources in that order and updates the row's parameter and both moments.
//                         No float atomics: the result is a function of the inputs alone.
//
// Integer atomics only (the `bad` counter, LDS digit counts), and none of them decides a value that is written.
#include "block_ops.h"

#define TT_NT 1024                     // threads of the sorting workgroups
#define TT_CHUNK 4096                  // keys per workgroup and pass of the multi-workgroup sort
#define TT_SMALL_R 8192                // up to here ONE workgroup sorts (one launch); above: histogram / scan / scatter per pass
#define TT_MAX_R (1 << 20)
#define TT_INVALID 0xffffffffu

// ---- row-sparse Adam: the sort ---------------------------------------------------------------------------------------
// key of source r: its id, or P for a source that is skipped (-1: padding; anything else outside [0, P): counted in *bad).
// P < 2^31 sorts behind every valid id, and the digits cover bit_length(P) bits.
__device__ __forceinline__ void tt_init_range(const int32_t* __restrict__ idx, uint32_t lo, uint32_t hi, uint32_t P, uint32_t* key,
                                              uint32_t* val, int32_t* bad) {
    int nbad = 0;
    for (uint32_t r = lo + threadIdx.x; r < hi; r += TT_NT) {
        const int32_t id = idx[r];
        const bool ok = (uint32_t)id < P;
        nbad += (!ok && id != -1) ? 1 : 0;
        key[r] = ok ? (uint32_t)id : P;
        val[r] = r;
    }
    nbad = wave_sum(nbad);
    if ((threadIdx.x & 63) == 0 && nbad) atomicAdd(bad, nbad);
}

// R <= TT_SMALL_R: keys, every pass and nothing else, by one workgroup.  The sorted arrays end in buffer (passes & 1).
__global__ __launch_bounds__(TT_NT) void tt_sort_small_kernel(const int32_t* __restrict__ idx, uint32_t R, uint32_t P, int passes,
                                                             uint32_t* key0, uint32_t* val0, uint32_t* key1, uint32_t* val1,
                                                             int32_t* bad) {
    __shared__ int base[256], cnt[256], wcnt[(TT_NT / 64) * 256];
    tt_init_range(idx, 0, R, P, key0, val0, bad);
    __syncthreads();
    for (int p = 0; p < passes; p++) {
        const uint32_t* sk = (p & 1) ? key1 : key0; const uint32_t* sv = (p & 1) ? val1 : val0;
        uint32_t* dk = (p & 1) ? key0 : key1; uint32_t* dv = (p & 1) ? val0 : val1;
        radix_hist<TT_NT>(sk, 0u, R, 8 * p, cnt);
        if (threadIdx.x < 256) base[threadIdx.x] = radix_digit_offset(cnt, threadIdx.x);
        __syncthreads();
        radix_scatter<TT_NT, true>(sk, sv, dk, dv, 0u, R, R, 8 * p, base, wcnt);
        __syncthreads();
    }
}

__global__ __launch_bounds__(TT_NT) void tt_init_kernel(const int32_t* __restrict__ idx, uint32_t R, uint32_t P, uint32_t* key,
                                                       uint32_t* val, int32_t* bad) {
    const uint32_t lo = blockIdx.x * (uint32_t)TT_CHUNK, hi = min(R, lo + (uint32_t)TT_CHUNK);
    tt_init_range(idx, lo, hi, P, key, val, bad);
}

// counts[d * nblk + j] = keys of digit d in chunk j
__global__ __launch_bounds__(TT_NT) void tt_hist_kernel(const uint32_t* __restrict__ key, uint32_t R, int shift, int nblk,
                                                       int32_t* counts) {
    __shared__ int cnt[256];
    const uint32_t lo = blockIdx.x * (uint32_t)TT_CHUNK, hi = min(R, lo + (uint32_t)TT_CHUNK);
    radix_hist<TT_NT>(key, lo, hi, shift, cnt);
    if (threadIdx.x < 256) counts[threadIdx.x * nblk + blockIdx.x] = cnt[threadIdx.x];
}

// counts -> exclusive offsets in (digit, chunk) order, in place: one workgroup, thread d walks the nblk <= 256 chunks of digit d
__global__ __launch_bounds__(256) void tt_scan_kernel(int nblk, int32_t* counts) {
    __shared__ int tot[256];
    const int d = threadIdx.x;
    int s = 0;
    for (int j = 0; j < nblk; j++) s += counts[d * nblk + j];
    tot[d] = s;
    __syncthreads();
    int ex = radix_digit_offset(tot, d);
    for (int j = 0; j < nblk; j++) {
        const int c = counts[d * nblk + j];
        counts[d * nblk + j] = ex;
        ex += c;
    }
}

__global__ __launch_bounds__(TT_NT) void tt_scatter_kernel(const uint32_t* __restrict__ skey, const uint32_t* __restrict__ sval,
                                                          uint32_t* dkey, uint32_t* dval, uint32_t R, int shift, int nblk,
                                                          const int32_t* __restrict__ offsets) {
    __shared__ int base[256], wcnt[(TT_NT / 64) * 256];
    if (threadIdx.x < 256) base[threadIdx.x] = offsets[threadIdx.x * nblk + blockIdx.x];
    __syncthreads();
    const uint32_t lo = blockIdx.x * (uint32_t)TT_CHUNK, hi = min(R, lo + (uint32_t)TT_CHUNK);
    radix_scatter<TT_NT, true>(skey, sval, dkey, dval, lo, hi, R, shift, base, wcnt);
}

// ---- row-sparse Adam: the update -------------------------------------------------------------------------------------
// torch.optim.SparseAdam's update of one element; every operation is one fp32 rounding (contraction off), division and square
// root correctly rounded.  neg_s = fl32(-lr sqrt(1 - beta2^t) / (1 - beta1^t)), formed in fp64 on the host.
__device__ __forceinline__ void tt_sparse_adam(float& p, float& m, float& v, float g, float omb1, float omb2, float eps,
                                               float neg_s) {
#pragma clang fp contract(off)
    const float um = (g - m) * omb1;
    m = m + um;
    const float uv = (g * g - v) * omb2;
    v = v + uv;
    const float den = sqrtf(v) + eps;               // (sqrtf and / are the correctly rounded forms in this build; __fsqrt_rn is
    p = p + neg_s * (m / den);                      //  the 1-ulp native instruction here)
}

// One wave per 64 sorted positions: every position that starts a run of one valid id is a distinct row; the wave walks the
// run (past its own 64 positions where it goes on), sums grad[r] over the run's sources in order -- eight rows in flight, added
// one after the other -- and updates row id.  A lane owns dims (2 lane, 2 lane + 1) of every 128-dim chunk.
template <int NCH>
__global__ __launch_bounds__(256) void tt_sparse_adam_kernel(const uint32_t* __restrict__ key, const uint32_t* __restrict__ val,
                                                             uint32_t R, uint32_t P, const float* __restrict__ grad, float* table,
                                                             float* exp_avg, float* exp_avg_sq, float omb1, float omb2, float eps,
                                                             float neg_s) {
    constexpr int D = 128 * NCH;
    const int lane = threadIdx.x & 63;
    const uint32_t i0 = (blockIdx.x * 4u + (threadIdx.x >> 6)) * 64u;
    if (i0 >= R) return;
    const uint32_t i = i0 + lane;
    const uint32_t k = i < R ? key[i] : TT_INVALID;
    const uint32_t kprev = (i > 0 && i < R) ? key[i - 1] : TT_INVALID;
    unsigned long long heads = __ballot(i < R && k < P && (i == 0 || kprev != k));
    while (heads) {
        const int hl = __ffsll((long long)heads) - 1;
        heads &= heads - 1;
        const uint32_t h = i0 + hl;
        const uint32_t u = (uint32_t)__shfl((int)k, hl, 64);
        // the run's end: the first later position of another key (positions past R hold TT_INVALID)
        const unsigned long long later = __ballot(lane > hl && k != u);
        uint32_t e;
        if (later) {
            e = i0 + (__ffsll((long long)later) - 1);
        } else {
            e = i0 + 64u;
            for (;;) {
                const uint32_t kk = e + lane < R ? key[e + lane] : TT_INVALID;
                const unsigned long long df = __ballot(kk != u);
                if (df) { e += __ffsll((long long)df) - 1; break; }
                e += 64u;
            }
        }
        float2 g[NCH];
        {
            const uint32_t r = val[h];
            if (r >= R) continue;                                     // (never: the values are a permutation of [0, R))
#pragma unroll
            for (int ch = 0; ch < NCH; ch++) g[ch] = *reinterpret_cast<const float2*>(grad + (size_t)r * D + 128 * ch + 2 * lane);
        }
        for (uint32_t j = h + 1; j < e; j += 8) {
            float2 x[8][NCH];
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const uint32_t r = j + q < e ? val[j + q] : TT_INVALID;
#pragma unroll
                for (int ch = 0; ch < NCH; ch++)
                    x[q][ch] = r < R ? *reinterpret_cast<const float2*>(grad + (size_t)r * D + 128 * ch + 2 * lane) : make_float2(0.f, 0.f);
            }
#pragma unroll
            for (int q = 0; q < 8; q++)
                if (j + q < e) {
#pragma unroll
                    for (int ch = 0; ch < NCH; ch++) { g[ch].x += x[q][ch].x; g[ch].y += x[q][ch].y; }
                }
        }
#pragma unroll
        for (int ch = 0; ch < NCH; ch++) {
            const size_t o = (size_t)u * D + 128 * ch + 2 * lane;
            float2 p = *reinterpret_cast<float2*>(table + o);
            float2 m = *reinterpret_cast<float2*>(exp_avg + o);
            float2 v = *reinterpret_cast<float2*>(exp_avg_sq + o);
            tt_sparse_adam(p.x, m.x, v.x, g[ch].x, omb1, omb2, eps, neg_s);
            tt_sparse_adam(p.y, m.y, v.y, g[ch].y, omb1, omb2, eps, neg_s);
            *reinterpret_cast<float2*>(table + o) = p;
            *reinterpret_cast<float2*>(exp_avg + o) = m;
            *reinterpret_cast<float2*>(exp_avg_sq + o) = v;
        }
    }
}

struct SparseAdamWs { uint32_t *key[2], *val[2]; int32_t* counts; int nblk; size_t total; };

static SparseAdamWs sparse_adam_ws_layout(void* base, int R) {
    SparseAdamWs w;
    WsCarver cv(base);
    for (int i = 0; i < 2; i++) {
        w.key[i] = static_cast<uint32_t*>(cv.bytes((size_t)R * 4));
        w.val[i] = static_cast<uint32_t*>(cv.bytes((size_t)R * 4));
    }
    w.nblk = (R + TT_CHUNK - 1) / TT_CHUNK;
    w.counts = static_cast<int32_t*>(cv.bytes((size_t)256 * w.nblk * 4));
    w.total = cv.total;
    return w;
}

extern "C" size_t pc_sparse_adam_rows_workspace_bytes(int R) {
    if (R < 1 || R > TT_MAX_R) return 0;
    return sparse_adam_ws_layout(nullptr, R).total;
}

extern "C" int pc_sparse_adam_rows(float* table, float* exp_avg, float* exp_avg_sq, int64_t P, int dim, const int32_t* idx,
                                   const float* grad, int R, int64_t t, double lr, double beta1, double beta2, double eps,
                                   int32_t* bad, void* ws, size_t ws_bytes, void* stream) {
    if (!table || !exp_avg || !exp_avg_sq || !idx || !grad || !bad || !ws) return PC_EINVAL;
    if (P < 1 || P >= (1ll << 31) || R < 1 || R > TT_MAX_R || t < 1) return PC_EINVAL;
    if (dim != 128 && dim != 256) return PC_ESHAPE;
    if (((uintptr_t)table | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq | (uintptr_t)grad | (uintptr_t)ws) & 15) return PC_ESHAPE;
    if (((uintptr_t)idx | (uintptr_t)bad) & 3) return PC_ESHAPE;
    if (ws_bytes < pc_sparse_adam_rows_workspace_bytes(R)) return PC_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const SparseAdamWs w = sparse_adam_ws_layout(ws, R);
    int bits = 0;
    while ((P >> bits) != 0) bits++;                                   // bit_length(P): the keys lie in [0, P]
    const int passes = (bits + 7) / 8;
    const uint32_t Ru = (uint32_t)R, Pu = (uint32_t)P;
    if (R <= TT_SMALL_R) {
        PC_LAUNCH(tt_sort_small_kernel, dim3(1), dim3(TT_NT), 0, st, idx, Ru, Pu, passes, w.key[0], w.val[0], w.key[1], w.val[1], bad);
    } else {
        PC_LAUNCH(tt_init_kernel, dim3(w.nblk), dim3(TT_NT), 0, st, idx, Ru, Pu, w.key[0], w.val[0], bad);
        for (int p = 0; p < passes; p++) {
            const int s = p & 1;
            PC_LAUNCH(tt_hist_kernel, dim3(w.nblk), dim3(TT_NT), 0, st, w.key[s], Ru, 8 * p, w.nblk, w.counts);
            PC_LAUNCH(tt_scan_kernel, dim3(1), dim3(256), 0, st, w.nblk, w.counts);
            PC_LAUNCH(tt_scatter_kernel, dim3(w.nblk), dim3(TT_NT), 0, st, w.key[s], w.val[s], w.key[s ^ 1], w.val[s ^ 1], Ru, 8 * p,
                      w.nblk, w.counts);
        }
    }
    PC_TRY(pc_launch_status());
    const int s = passes & 1;
    // the bias corrections in fp64, as adam_at_kernel forms them; one fp32 rounding of the step size
    const double bc1 = 1.0 - pow(beta1, (double)t), bc2 = 1.0 - pow(beta2, (double)t);
    const float neg_s = -(float)(lr * sqrt(bc2) / bc1);
    const float omb1 = (float)(1.0 - beta1), omb2 = (float)(1.0 - beta2), epsf = (float)eps;
    const dim3 grid((unsigned)((R + 255) / 256)), block(256);
    if (dim == 128) PC_LAUNCH(tt_sparse_adam_kernel<1>, grid, block, 0, st, w.key[s], w.val[s], Ru, Pu, grad, table, exp_avg, exp_avg_sq,
                              omb1, omb2, epsf, neg_s);
    else PC_LAUNCH(tt_sparse_adam_kernel<2>, grid, block, 0, st, w.key[s], w.val[s], Ru, Pu, grad, table, exp_avg, exp_avg_sq,
                   omb1, omb2, epsf, neg_s);
    return pc_launch_status();
}

// ---- the query rows' gradient ----------------------------------------------------------------------------------------
// ids that must not index anything: qsafe[b] = query_idx[b] or -1 (the GEMM loaders read a -1 row as zeros), ksafe likewise
// for the B K predicted types; zero[b] = 1 when sample b holds any such id (its dq row is then zero); every offender counts.
__global__ __launch_bounds__(256) void tt_query_ids_kernel(const int32_t* __restrict__ query_idx, const int32_t* __restrict__ topk,
                                                          int B, int K, uint32_t P, uint32_t T, int32_t* qsafe, int32_t* ksafe,
                                                          int32_t* zero, int32_t* bad) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    int nbad = 0;
    if (b < B) {
        const int32_t q = query_idx[b];
        const bool qok = (uint32_t)q < P;
        nbad += qok ? 0 : 1;
        qsafe[b] = qok ? q : -1;
        for (int k = 0; k < K; k++) {
            const int32_t c = topk[(size_t)b * K + k];
            const bool ok = (uint32_t)c < T;
            nbad += ok ? 0 : 1;
            ksafe[(size_t)b * K + k] = ok ? c : -1;
        }
        zero[b] = nbad ? 1 : 0;
    }
    nbad = wave_sum(nbad);
    if ((threadIdx.x & 63) == 0 && nbad) atomicAdd(bad, nbad);
}

// dpi[b] = sum_k dx_bk * tp_bk, one wave per sample: joint_rowwise_kernel's item half (x = pi * tp, torch.norm without eps,
// the strict hinge, subgradient 0 at a zero norm), the gradient scale alpha / (B K) a constant.
template <int NCH>
__global__ __launch_bounds__(256) void tt_query_rowwise_kernel(const float* __restrict__ pi, const float* __restrict__ tp,
                                                              const float* __restrict__ pos_items, const float* __restrict__ neg_items,
                                                              const int32_t* __restrict__ zero, int B, int K, float margin, float alpha,
                                                              float* dpi) {
    constexpr int D = 128 * NCH;
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    float2 a[NCH], pp[NCH], nn[NCH], acc[NCH];
#pragma unroll
    for (int ch = 0; ch < NCH; ch++) {
        const size_t o = (size_t)b * D + 128 * ch + 2 * lane;
        a[ch] = *reinterpret_cast<const float2*>(pi + o);
        pp[ch] = *reinterpret_cast<const float2*>(pos_items + o);
        nn[ch] = *reinterpret_cast<const float2*>(neg_items + o);
        acc[ch] = make_float2(0.f, 0.f);
    }
    const bool live = zero[b] == 0;
    for (int k = 0; k < K && live; k++) {
        float2 t[NCH], dp[NCH], dn[NCH];
        float sp_ = 0.f, sn_ = 0.f;
#pragma unroll
        for (int ch = 0; ch < NCH; ch++) {
            t[ch] = *reinterpret_cast<const float2*>(tp + ((size_t)b * K + k) * D + 128 * ch + 2 * lane);
            const float2 x = make_float2(a[ch].x * t[ch].x, a[ch].y * t[ch].y);
            dp[ch] = make_float2(x.x - pp[ch].x, x.y - pp[ch].y); dn[ch] = make_float2(x.x - nn[ch].x, x.y - nn[ch].y);
            sp_ += dp[ch].x * dp[ch].x + dp[ch].y * dp[ch].y; sn_ += dn[ch].x * dn[ch].x + dn[ch].y * dn[ch].y;
        }
        const float np_ = sqrtf(wave_sum(sp_));
        const float nn_ = sqrtf(wave_sum(sn_));
        const float l = margin - np_ + nn_;
        const float g = l > 0.f ? alpha / ((float)B * (float)K) : 0.f;
        const float ip = np_ > 0.f ? g / np_ : 0.f, in = nn_ > 0.f ? g / nn_ : 0.f;   // torch.norm: subgradient 0 at 0
#pragma unroll
        for (int ch = 0; ch < NCH; ch++) {
            const float2 d = make_float2(-dp[ch].x * ip + dn[ch].x * in, -dp[ch].y * ip + dn[ch].y * in);
            acc[ch].x += d.x * t[ch].x; acc[ch].y += d.y * t[ch].y;
        }
    }
#pragma unroll
    for (int ch = 0; ch < NCH; ch++) *reinterpret_cast<float2*>(dpi + (size_t)b * D + 128 * ch + 2 * lane) = acc[ch];
}

struct QueryGradWs { int32_t *qsafe, *ksafe, *zero; float *pi, *tp, *dpi, *wt; size_t total; };

static QueryGradWs query_grad_ws_layout(void* base, int B, int K, int D) {
    QueryGradWs w;
    WsCarver cv(base);
    w.qsafe = static_cast<int32_t*>(cv.bytes((size_t)B * 4));
    w.ksafe = static_cast<int32_t*>(cv.bytes((size_t)B * K * 4));
    w.zero = static_cast<int32_t*>(cv.bytes((size_t)B * 4));
    w.pi = cv.floats((size_t)B * D);
    w.tp = cv.floats((size_t)B * K * D);
    w.dpi = cv.floats((size_t)B * D);
    w.wt = cv.floats((size_t)D * D);
    w.total = cv.total;
    return w;
}

extern "C" size_t pc_joint_query_grad_workspace_bytes(int B, int K, int dim) {
    if (B <= 0 || K < 1 || K > 8 || (dim != 128 && dim != 256) || (int64_t)B * K >= (1ll << 31) / 256) return 0;
    return query_grad_ws_layout(nullptr, B, K, dim).total;
}

extern "C" int pc_joint_query_grad(const pc_joint_tensors* p, const int32_t* query_idx, const int32_t* topk, const float* pos_items,
                                   const float* neg_items, int B, int64_t P, int T, int K, int dim, float margin, float alpha,
                                   float* dq, int32_t* bad, void* ws, size_t ws_bytes, void* stream) {
    if (!p || !p->product_table || !p->itm_w || !p->itm_b || !p->typ_w || !p->typ_b || !p->comp_types) return PC_EINVAL;
    if (!query_idx || !topk || !pos_items || !neg_items || !dq || !bad || !ws) return PC_EINVAL;
    if (B <= 0 || T <= 0 || P < 1 || P >= (1ll << 31)) return PC_EINVAL;
    if (K < 1 || K > 8 || K > T || (dim != 128 && dim != 256)) return PC_ESHAPE;
    if (((uintptr_t)pos_items | (uintptr_t)neg_items | (uintptr_t)dq | (uintptr_t)ws) & 15) return PC_ESHAPE;
    const size_t need = pc_joint_query_grad_workspace_bytes(B, K, dim);
    if (need == 0) return PC_EINVAL;
    if (ws_bytes < need) return PC_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    const QueryGradWs w = query_grad_ws_layout(ws, B, K, dim);
    PC_LAUNCH(tt_query_ids_kernel, dim3((B + 255) / 256), dim3(256), 0, st, query_idx, topk, B, K, (uint32_t)P, (uint32_t)T, w.qsafe,
              w.ksafe, w.zero, bad);
    PC_TRY(pc_launch_status());
    // pi = item_projection(E_prod[query_idx]), tp = type_projection(E_c[topk])       item_prediction.py:31-35
    NtArgs ip = nt_plain(p->product_table, dim, p->itm_w, dim, p->itm_b, w.pi, dim, B, dim, dim);
    ip.gather = w.qsafe;
    PC_TRY(launch_gemm_nt(ip, st));
    NtArgs tpj = nt_plain(p->comp_types, PC_L, p->typ_w, PC_L, p->typ_b, w.tp, dim, B * K, dim, PC_L);
    tpj.gather = w.ksafe;
    PC_TRY(launch_gemm_nt(tpj, st));
    PC_TRY(launch_transpose(p->itm_w, dim, dim, w.wt, st));
    if (dim == 128) PC_LAUNCH(tt_query_rowwise_kernel<1>, dim3((B + 3) / 4), dim3(256), 0, st, w.pi, w.tp, pos_items, neg_items, w.zero,
                              B, K, margin, alpha, w.dpi);
    else PC_LAUNCH(tt_query_rowwise_kernel<2>, dim3((B + 3) / 4), dim3(256), 0, st, w.pi, w.tp, pos_items, neg_items, w.zero, B, K,
                   margin, alpha, w.dpi);
    PC_TRY(pc_launch_status());
    // dq = dpi W_item
    return launch_gemm_nt(nt_plain(w.dpi, dim, w.wt, dim, nullptr, dq, dim, B, dim, dim), st);
}
