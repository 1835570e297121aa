// Small HBM-bound kernels of the hot path: the triplet loss of Product2Vec.train_model
// (forward + backward in one pass), dense Adam, row gather / row scatter-add.
#include "common.h"

// ---------------------------------------------------------------------------------------
// P9 (product2vec.py:137-154): one wavefront per sample, lane l owns dims (2l, 2l+1).
//   d+ = ||a - p + eps||, d-_j = ||a - n_j + eps||, d- = mean_j d-_j, l = relu(margin - d+ + d-)
#define LOSS_MAX_K 8
#define PAIR_EPS 1e-6f

// lane l owns dims [VW l, VW l + VW), VW = D / 64 (2 at D = 128, 4 at D = 256)
template <int VW>
__global__ __launch_bounds__(256) void triplet_loss_kernel(const float* a, const float* p, const float* n, int B,
                                                           int K, float margin, float* d_pos, float* d_neg,
                                                           float* da, float* dp, float* dn) {
    constexpr int D = 64 * VW;
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    float av[VW], dpv[VW];
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < VW; c++) {
        av[c] = a[(size_t)b * D + VW * lane + c];
        dpv[c] = av[c] - p[(size_t)b * D + VW * lane + c] + PAIR_EPS;
        s += dpv[c] * dpv[c];
    }
    const float dpos = sqrtf(wave_sum(s));
    float dnv[LOSS_MAX_K][VW];
    float dn_j[LOSS_MAX_K];
    float dneg = 0.f;
#pragma unroll
    for (int j = 0; j < LOSS_MAX_K; j++) {
        if (j < K) {
            float t = 0.f;
#pragma unroll
            for (int c = 0; c < VW; c++) {
                dnv[j][c] = av[c] - n[((size_t)b * K + j) * D + VW * lane + c] + PAIR_EPS;
                t += dnv[j][c] * dnv[j][c];
            }
            dn_j[j] = sqrtf(wave_sum(t));
            dneg += dn_j[j];
        }
    }
    dneg /= (float)K;
    if (lane == 0) { d_pos[b] = dpos; d_neg[b] = dneg; }
    if (!da) return;
    const bool active = (margin - dpos + dneg) > 0.f;      // relu'(0) = 0 as in torch
    const float gs = active ? 1.0f / (float)B : 0.f;        // d(mean)/d(l_b)
    // d l / d d+ = -1 ; d l / d d-_j = 1/K; a distance of exactly 0 sends nothing (torch's norm: subgradient 0 at 0)
    const float ip = dpos > 0.f ? gs / dpos : 0.f;
    float ga[VW];
#pragma unroll
    for (int c = 0; c < VW; c++) {
        ga[c] = -dpv[c] * ip;
        dp[(size_t)b * D + VW * lane + c] = dpv[c] * ip;
    }
#pragma unroll
    for (int j = 0; j < LOSS_MAX_K; j++) {
        if (j < K) {
            const float in = dn_j[j] > 0.f ? gs / ((float)K * dn_j[j]) : 0.f;
#pragma unroll
            for (int c = 0; c < VW; c++) {
                ga[c] += dnv[j][c] * in;
                dn[((size_t)b * K + j) * D + VW * lane + c] = -dnv[j][c] * in;
            }
        }
    }
#pragma unroll
    for (int c = 0; c < VW; c++) da[(size_t)b * D + VW * lane + c] = ga[c];
}

// loss = mean_b relu(margin - d+ + d-): single block, fixed summation order
__global__ void hinge_mean_kernel(HingeMeanJob j) {
    __shared__ float red[256];
    hinge_mean_body(j, red);
}

// PRODUCT_EMB_DIM = 128: a 16-lane group per sample, sixteen samples per workgroup (triplet_sample16, common.h: the definition the
// fused step's loss prologue shares)
__global__ __launch_bounds__(256) void triplet_loss16_kernel(const float* a, const float* p, const float* n, int B, int K, float margin,
                                                             float* d_pos, float* d_neg, float* da, float* dp, float* dn) {
    const int l16 = threadIdx.x & 15;
    const int b = blockIdx.x * 16 + (threadIdx.x >> 4);
    const bool live = b < B;
    float ga[8];
    triplet_sample16(a, p, n, b, B, K, margin, live, d_pos, d_neg, dp, dn, da != nullptr, l16, ga);
    if (da && live) {
        *reinterpret_cast<float4*>(da + (size_t)b * 128 + 8 * l16) = make_float4(ga[0], ga[1], ga[2], ga[3]);
        *reinterpret_cast<float4*>(da + (size_t)b * 128 + 8 * l16 + 4) = make_float4(ga[4], ga[5], ga[6], ga[7]);
    }
}

// with_mean == 0: the caller folds the mean into a later launch (HingeMeanJob rider of launch_gemm_nt_chain)
int triplet_loss_launch(const float* a, const float* p, const float* n, int batch, int k_neg, int dim, float margin,
                        float* loss, float* d_pos, float* d_neg, float* da, float* dp, float* dn, void* stream, int with_mean) {
    if (!a || !p || !n || !loss || !d_pos || !d_neg || batch <= 0) return PC_EINVAL;
    if (k_neg < 1 || k_neg > LOSS_MAX_K || (dim != 128 && dim != 256)) return PC_ESHAPE;
    if (da && (!dp || !dn)) return PC_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (dim == 128) PC_LAUNCH(triplet_loss16_kernel, dim3((batch + 15) / 16), dim3(256), 0, st, a, p, n, batch, k_neg, margin,
                              d_pos, d_neg, da, dp, dn);
    else PC_LAUNCH(triplet_loss_kernel<4>, dim3((batch + 3) / 4), dim3(256), 0, st, a, p, n, batch, k_neg, margin,
                   d_pos, d_neg, da, dp, dn);
    PC_TRY(pc_launch_status());
    if (!with_mean) return PC_OK;
    const HingeMeanJob j = {d_pos, d_neg, batch, margin, loss};
    PC_LAUNCH(hinge_mean_kernel, dim3(1), dim3(256), 0, st, j);
    return pc_launch_status();
}

extern "C" int pc_p2v_triplet_loss_dim(const float* a, const float* p, const float* n, int batch, int k_neg, int dim,
                                       float margin, float* loss, float* d_pos, float* d_neg, float* da, float* dp,
                                       float* dn, void* stream) {
    return triplet_loss_launch(a, p, n, batch, k_neg, dim, margin, loss, d_pos, d_neg, da, dp, dn, stream, 1);
}

extern "C" int pc_p2v_triplet_loss(const float* a, const float* p, const float* n, int batch, int k_neg,
                                   float margin, float* loss, float* d_pos, float* d_neg, float* da, float* dp,
                                   float* dn, void* stream) {
    return pc_p2v_triplet_loss_dim(a, p, n, batch, k_neg, PC_D, margin, loss, d_pos, d_neg, da, dp, dn, stream);
}

// ---------------------------------------------------------------------------------------
// P10: torch.optim.Adam (defaults) over a flat fp32 range.  Scalars follow torch's
// single-tensor path: bias corrections and step size in fp64, rounded to fp32 at use.
__global__ void adam_prep_kernel(int64_t* step_count, double lr, double beta1, double beta2, float* scal) {
    const int64_t t = *step_count + 1;
    *step_count = t;
    const double bc1 = 1.0 - pow(beta1, (double)t);
    const double bc2 = 1.0 - pow(beta2, (double)t);
    scal[0] = (float)(lr / bc1);              // step_size
    scal[1] = (float)sqrt(bc2);               // bias_correction2_sqrt
}

__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                            float* __restrict__ v, size_t n, const float* scal, float omb1, float beta2,
                            float omb2, float eps) {
    const float step_size = scal[0], bc2s = scal[1];
    const size_t i4 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i4 + 3 < n) {
        float4 pv = *reinterpret_cast<float4*>(p + i4);
        const float4 gv = *reinterpret_cast<const float4*>(g + i4);
        float4 mv = *reinterpret_cast<float4*>(m + i4);
        float4 vv = *reinterpret_cast<float4*>(v + i4);
        if (pc_adam_dead(gv, mv, vv)) return;              // (g = m = v = 0: the update changes nothing -- nothing is written)
#define ADAM1(c) pc_adam_update(pv.c, mv.c, vv.c, gv.c, step_size, bc2s, omb1, beta2, omb2, eps);
        ADAM1(x) ADAM1(y) ADAM1(z) ADAM1(w)
#undef ADAM1
        *reinterpret_cast<float4*>(p + i4) = pv;
        *reinterpret_cast<float4*>(m + i4) = mv;
        *reinterpret_cast<float4*>(v + i4) = vv;
    } else {
        for (size_t i = i4; i < n; i++) {
            float pp = p[i], mm = m[i], vv = v[i];
            pc_adam_update(pp, mm, vv, g[i], step_size, bc2s, omb1, beta2, omb2, eps);
            p[i] = pp;
            m[i] = mm;
            v[i] = vv;
        }
    }
}

// The same update with the step number t known to the HOST (an optimizer that owns every increment of its counter): the
// scalars are formed per workgroup by the same fp64 expressions as adam_prep_kernel (same bits), nothing reads the device
// counter, so one launch does what pc_adam_step needs two for; block 0 leaves *step_count = t for whoever reads it later.
__global__ void adam_at_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                               float* __restrict__ v, size_t n, int64_t* step_count, long long t, double lr, double beta1,
                               double beta2, float omb1, float beta2f, float omb2, float eps) {
    __shared__ float sc[2];
    if (threadIdx.x == 0) {
        const double bc1 = 1.0 - pow(beta1, (double)t);
        const double bc2 = 1.0 - pow(beta2, (double)t);
        sc[0] = (float)(lr / bc1);
        sc[1] = (float)sqrt(bc2);
        if (blockIdx.x == 0 && step_count) *step_count = t;
    }
    __syncthreads();
    const float step_size = sc[0], bc2s = sc[1];
    const size_t i4 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i4 + 3 < n) {
        float4 pv = *reinterpret_cast<float4*>(p + i4);
        const float4 gv = *reinterpret_cast<const float4*>(g + i4);
        float4 mv = *reinterpret_cast<float4*>(m + i4);
        float4 vv = *reinterpret_cast<float4*>(v + i4);
        if (pc_adam_dead(gv, mv, vv)) return;              // (g = m = v = 0: the update changes nothing -- nothing is written)
#define ADAM1(c) pc_adam_update(pv.c, mv.c, vv.c, gv.c, step_size, bc2s, omb1, beta2f, omb2, eps);
        ADAM1(x) ADAM1(y) ADAM1(z) ADAM1(w)
#undef ADAM1
        *reinterpret_cast<float4*>(p + i4) = pv;
        *reinterpret_cast<float4*>(m + i4) = mv;
        *reinterpret_cast<float4*>(v + i4) = vv;
    } else {
        for (size_t i = i4; i < n; i++) {
            float pp = p[i], mm = m[i], vv = v[i];
            pc_adam_update(pp, mm, vv, g[i], step_size, bc2s, omb1, beta2f, omb2, eps);
            p[i] = pp;
            m[i] = mm;
            v[i] = vv;
        }
    }
}

extern "C" int pc_adam_step_at(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n,
                               int64_t* step_count, int64_t t, double lr, double beta1, double beta2, double eps,
                               void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || n == 0 || t < 1) return PC_EINVAL;
    if (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) return PC_ESHAPE;
    const size_t threads = (n + 3) / 4;
    PC_LAUNCH(adam_at_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg,
              exp_avg_sq, n, step_count, (long long)t, lr, beta1, beta2, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2),
              (float)eps);
    return pc_launch_status();
}

extern "C" int pc_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n,
                            int64_t* step_count, float* scalars, double lr, double beta1, double beta2,
                            double eps, void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || !step_count || !scalars || n == 0) return PC_EINVAL;
    if (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) return PC_ESHAPE;
    hipStream_t st = (hipStream_t)stream;
    PC_LAUNCH(adam_prep_kernel, dim3(1), dim3(1), 0, st, step_count, lr, beta1, beta2, scalars);
    PC_TRY(pc_launch_status());
    const size_t threads = (n + 3) / 4;
    PC_LAUNCH(adam_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, param, grad, exp_avg,
                       exp_avg_sq, n, scalars, (float)(1.0 - beta1), (float)beta2, (float)(1.0 - beta2), (float)eps);
    return pc_launch_status();
}

// ---------------------------------------------------------------------------------------
// out[r] = idx[r] >= 0 ? table[idx[r]] : 0 ; one 16-B chunk per thread, rows coalesced
__global__ void gather_rows_kernel(const float* table, const int32_t* idx, int rows, int w4, float* out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)rows * w4;
    if (t >= total) return;
    const int r = (int)(t / w4), c = (int)(t % w4);
    const int src = idx ? idx[r] : r;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (src >= 0) v = *reinterpret_cast<const float4*>(table + ((size_t)src * w4 + c) * 4);
    *reinterpret_cast<float4*>(out + t * 4) = v;
}

extern "C" int pc_gather_rows(const float* table, const int32_t* idx, int rows, int width, float* out,
                              void* stream) {
    if (!table || !out || rows <= 0 || width <= 0) return PC_EINVAL;
    if (width % 4) return PC_ESHAPE;
    const size_t total = (size_t)rows * (width / 4);
    PC_LAUNCH(gather_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       table, idx, rows, width / 4, out);
    return pc_launch_status();
}

// table[idx[r]] += src[r] : one wave-instruction adds 64 consecutive floats of one row
// (256 contiguous bytes per atomic instruction = the full-rate shape on gfx950)
__global__ void scatter_add_rows_kernel(float* table, const int32_t* idx, int rows, int width, const float* src) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)rows * width;
    if (t >= total) return;
    const int r = (int)(t / width), c = (int)(t % width);
    const int dst = idx[r];
    if (dst >= 0) unsafeAtomicAdd(table + (size_t)dst * width + c, src[t]);
}

// Small tables (the [T,64] type tables at T ~ 100: thousands of source rows collide on a few
// destination rows): each workgroup first accumulates its slice of source rows into a private LDS
// copy of the table (LDS atomics), then adds the copy to HBM once -> global atomic traffic and
// same-address contention drop by the number of source rows per workgroup.
__global__ __launch_bounds__(256) void scatter_add_rows_lds_kernel(float* table, const int32_t* idx, int rows,
                                                                   int width, int table_rows, const float* src,
                                                                   int rows_per_block) {
    extern __shared__ float priv[];
    const int n = table_rows * width;
    for (int i = threadIdx.x; i < n; i += blockDim.x) priv[i] = 0.f;
    __syncthreads();
    const int r0 = blockIdx.x * rows_per_block, r1 = min(rows, r0 + rows_per_block);
    const int end = r1 * width;
    for (int base = r0 * width + threadIdx.x; base < end; base += 8 * blockDim.x) {    // (loads first: see the slab kernel)
        int d[8];
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int t = base + u * blockDim.x;
            const bool ok = t < end;
            d[u] = ok ? idx[t / width] : -1;
            v[u] = ok ? src[t] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int t = base + u * blockDim.x;
            if (d[u] >= 0) unsafeAtomicAdd(&priv[d[u] * width + t % width], v[u]);      // ds_add_f32 (plain atomicAdd would compile to a CAS loop)
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const float v = priv[i];
        if (v != 0.f) unsafeAtomicAdd(table + i, v);
    }
}

// Deterministic form for callers with a workspace (the fused joint step): every workgroup writes its private
// table to its own slab; the caller sums the slabs in fixed order (tn_reduce) -- no global atomics at all
// (the flush above is 600 k same-address float atomics for a [100,64] table and 12 k source rows: 19 us).
__global__ __launch_bounds__(1024) void scatter_add_rows_slab_kernel(const int32_t* idx, int rows, int width,
                                                                    int table_rows, const float* src,
                                                                    int rows_per_block, float* slabs) {
    extern __shared__ float priv[];
    const int n = table_rows * width;
    for (int i = threadIdx.x; i < n; i += blockDim.x) priv[i] = 0.f;
    __syncthreads();
    const int r0 = blockIdx.x * rows_per_block, r1 = min(rows, r0 + rows_per_block);
    // eight (index, value) pairs are requested before the first LDS atomic: one dependent load chain per element
    // made this loop pure memory latency (32 round trips per thread: 18 us for 12 k rows)
    const int end = r1 * width;
    for (int base = r0 * width + threadIdx.x; base < end; base += 8 * blockDim.x) {
        int d[8];
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int t = base + u * blockDim.x;
            const bool ok = t < end;
            d[u] = ok ? idx[t / width] : -1;
            v[u] = ok ? src[t] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int t = base + u * blockDim.x;
            if (d[u] >= 0) unsafeAtomicAdd(&priv[d[u] * width + t % width], v[u]);
        }
    }
    __syncthreads();
    float* out = slabs + (size_t)blockIdx.x * n;
    for (int i = threadIdx.x * 4; i < n; i += blockDim.x * 4)                 // n is a multiple of 4 (checked by the launcher)
        *reinterpret_cast<float4*>(out + i) = *reinterpret_cast<const float4*>(priv + i);
}

// slabs needed by launch_scatter_add_slabs (0: table too large for the LDS form)
int scatter_add_slab_blocks(int table_rows, int rows, int width) {
    if ((size_t)table_rows * width * sizeof(float) > 65536 || (table_rows * width) % 4) return 0;
    int blocks = (rows + 127) / 128;
    return blocks > 256 ? 256 : blocks;
}

int launch_scatter_add_slabs(const int32_t* idx, int rows, int width, int table_rows, const float* src, float* slabs,
                             hipStream_t st) {
    const int blocks = scatter_add_slab_blocks(table_rows, rows, width);
    if (blocks <= 0 || !idx || !src || !slabs) return PC_EINVAL;
    const int rpb = (rows + blocks - 1) / blocks;
    // 1024 threads: 128 rows x 64 floats = one pass of 8 elements per thread (the kernel is a chain of memory latencies)
    PC_LAUNCH(scatter_add_rows_slab_kernel, dim3(blocks), dim3(1024), (size_t)table_rows * width * sizeof(float), st, idx,
              rows, width, table_rows, src, rpb, slabs);
    return pc_launch_status();
}

extern "C" int pc_scatter_add_rows(float* table, const int32_t* idx, int rows, int width, const float* src,
                                   void* stream) {
    if (!table || !idx || !src || rows <= 0 || width <= 0) return PC_EINVAL;
    const size_t total = (size_t)rows * width;
    PC_LAUNCH(scatter_add_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
              table, idx, rows, width, src);
    return pc_launch_status();
}

// same, when the caller knows the destination table is small (table_rows * width * 4 <= 64 KB)
extern "C" int pc_scatter_add_rows_small(float* table, int table_rows, const int32_t* idx, int rows, int width,
                                         const float* src, void* stream) {
    if (!table || !idx || !src || rows <= 0 || width <= 0 || table_rows <= 0) return PC_EINVAL;
    const size_t bytes = (size_t)table_rows * width * sizeof(float);
    if (bytes > 65536) return pc_scatter_add_rows(table, idx, rows, width, src, stream);
    int blocks = (rows + 127) / 128;
    if (blocks > 256) blocks = 256;
    const int rpb = (rows + blocks - 1) / blocks;
    PC_LAUNCH(scatter_add_rows_lds_kernel, dim3(blocks), dim3(256), bytes, (hipStream_t)stream, table, idx, rows, width,
              table_rows, src, rpb);
    return pc_launch_status();
}

// out[idx[r]] = src[r]  (row assignment; idx < 0 skipped; duplicate targets: last writer wins)
__global__ void scatter_rows_kernel(float* out, const int32_t* idx, int rows, int w4, const float* src) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)rows * w4) return;
    const int r = (int)(t / w4), c = (int)(t % w4);
    const int dst = idx[r];
    if (dst >= 0) *reinterpret_cast<float4*>(out + ((size_t)dst * w4 + c) * 4) = *reinterpret_cast<const float4*>(src + t * 4);
}

extern "C" int pc_scatter_rows(float* out, const int32_t* idx, int rows, int width, const float* src,
                               void* stream) {
    if (!out || !idx || !src || rows <= 0 || width <= 0) return PC_EINVAL;
    if (width % 4) return PC_ESHAPE;
    const size_t total = (size_t)rows * (width / 4);
    PC_LAUNCH(scatter_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       out, idx, rows, width / 4, src);
    return pc_launch_status();
}

// dx = dy * act'(y): act 1 tanh (1 - y^2), 2 relu (y > 0)
__global__ void act_backward_kernel(const float* dy, const float* y, size_t n, int act, float* dx) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = y[i];
    dx[i] = act == 1 ? dy[i] * (1.f - v * v) : (v > 0.f ? dy[i] : 0.f);
}

extern "C" int pc_act_backward(const float* dy, const float* y, size_t n, int act, float* dx, void* stream) {
    if (!dy || !y || !dx || n == 0) return PC_EINVAL;
    if (act != 1 && act != 2) return PC_EINVAL;
    PC_LAUNCH(act_backward_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, dy,
                       y, n, act, dx);
    return pc_launch_status();
}

// ---------------------------------------------------------------------------------------
// Row-sharded feature table: product r lives on rank r % G as local row r / G.  One launch turns
// the id arrays of a batch into (a) per-owner request lists of FIXED capacity C -- send_ids[G][C], local row indices,
// unused slots stay -1 -- and (b) the batch's indices over the table the exchange will deliver, row = owner * C + slot
// of the [G][C][D] receive buffer.  Everything stays on the device: no counts travel to the host, the two all-to-all
// rounds have constant shapes.  Slots are handed out by wave-aggregated integer atomics (one per wave and owner): the
// slot ORDER varies run to run, the rows the indices resolve to do not.  A bucket that would exceed C sets *overflow
// and maps the id to -1 (the caller checks the flag when it synchronises anyway and enlarges C).
struct ShardJobs { const int32_t* ids[4]; int32_t* out[4]; int n[4]; const int32_t* n_dev[4]; int n_dev_add[4]; int count; };
// HOT SET (round 6; BASELINE configs[4]: Zipf-skewed negatives): the H most popular products are REPLICATED on every rank behind
// the exchange buffer -- rows [G*C, G*C + H) of the table the step reads -- and an id that belongs to the set is served from
// there instead of taking a request slot (with Zipf(1) negatives over 100 M products the 1 024 most popular are 37 % of all
// negative draws; under a row-sharded table 7/8 of those would cross the wire at G = 8).  hot_ids: the set, ascending (binary
// search; NULL = the ids [0, H): popularity rank = product id, the default of the Zipf sampler); hot slot = position in the set.
__device__ __forceinline__ int hot_slot(const int32_t* hot_ids, int H, int id) {
    if (H <= 0 || id < 0) return -1;
    if (!hot_ids) return id < H ? id : -1;
    int lo = 0, hi = H;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (hot_ids[mid] < id) lo = mid + 1; else hi = mid;
    }
    return (lo < H && hot_ids[lo] == id) ? lo : -1;
}

__global__ __launch_bounds__(256) void shard_bucket_kernel(ShardJobs j, int G, int C, const int32_t* hot_ids, int H, int32_t* counts,
                                                           int32_t* send_ids, int32_t* overflow, int32_t* hot_served) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    // which array and position (the arrays are walked as one virtual concatenation of their CAPACITIES)
    int a = 0, pos = t;
#pragma unroll
    for (int i = 0; i < 3; i++)
        if (a == i && i + 1 < j.count && pos >= j.n[i]) { pos -= j.n[i]; a = i + 1; }
    const bool inside = a < j.count && pos < j.n[a];
    int id = -1;
    if (inside) {
        const int live = j.n_dev[a] ? min(j.n[a], *j.n_dev[a] + j.n_dev_add[a]) : j.n[a];     // entries past it are scratch
        if (pos < live) id = j.ids[a][pos];
    }
    const int hs = hot_slot(hot_ids, H, id);
    if (H > 0 && hot_served) {                             // (wave-uniform branch; one atomic per wave)
        const unsigned long long hm = __ballot(hs >= 0);
        if (hm != 0ull && lane == __ffsll((long long)hm) - 1) atomicAdd(hot_served, __popcll(hm));
    }
    const int owner = (id >= 0 && hs < 0) ? id % G : -1;
    int slot = -1;
    for (int o = 0; o < G; o++) {                          // wave-uniform loop: one atomic per wave and owner
        const unsigned long long m = __ballot(owner == o);
        if (m == 0ull) continue;
        const int leader = __ffsll((long long)m) - 1;
        int base = 0;
        if (lane == leader) base = atomicAdd(&counts[o], __popcll(m));
        base = __shfl(base, leader, 64);
        if (owner == o) slot = base + __popcll(m & ((1ull << lane) - 1ull));
    }
    if (!inside) return;
    int r = -1;
    if (hs >= 0) {
        r = G * C + hs;                                    // the local replica behind the exchange buffer
    } else if (id >= 0) {
        if (slot < C) { send_ids[(size_t)owner * C + slot] = id / G; r = owner * C + slot; }
        else atomicAdd(overflow, 1);
    }
    j.out[a][pos] = r;
}

extern "C" int pc_shard_bucket_hot(const int32_t* const* ids, const int* n, const int32_t* const* n_dev, const int* n_dev_add,
                                   int32_t* const* remap_out, int count, int world, int capacity, const int32_t* hot_ids,
                                   int hot_rows, int32_t* counts, int32_t* send_ids, int32_t* overflow, int32_t* hot_served,
                                   void* stream) {
    if (!ids || !n || !remap_out || !counts || !send_ids || !overflow || count < 1 || count > 4 || world < 1 || capacity < 1 ||
        hot_rows < 0)
        return PC_EINVAL;
    if ((long)world * capacity + hot_rows > 2147483647L) return PC_ESHAPE;
    ShardJobs j = {};
    long total = 0;
    for (int a = 0; a < count; a++) {
        if (!ids[a] || !remap_out[a] || n[a] <= 0) return PC_EINVAL;
        j.ids[a] = ids[a]; j.out[a] = remap_out[a]; j.n[a] = n[a];
        j.n_dev[a] = n_dev ? n_dev[a] : nullptr; j.n_dev_add[a] = n_dev_add ? n_dev_add[a] : 0;
        total += n[a];
    }
    j.count = count;
    hipStream_t st = (hipStream_t)stream;
    PC_HIP_TRY(hipMemsetAsync(counts, 0, (size_t)world * sizeof(int32_t), st));
    PC_HIP_TRY(hipMemsetAsync(send_ids, 0xff, (size_t)world * capacity * sizeof(int32_t), st));       // -1 = no request
    PC_LAUNCH(shard_bucket_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, j, world, capacity, hot_ids, hot_rows,
              counts, send_ids, overflow, hot_served);
    return pc_launch_status();
}

extern "C" int pc_shard_bucket(const int32_t* const* ids, const int* n, const int32_t* const* n_dev, const int* n_dev_add,
                               int32_t* const* remap_out, int count, int world, int capacity, int32_t* counts,
                               int32_t* send_ids, int32_t* overflow, void* stream) {
    return pc_shard_bucket_hot(ids, n, n_dev, n_dev_add, remap_out, count, world, capacity, nullptr, 0, counts, send_ids, overflow,
                               nullptr, stream);
}

// ---------------------------------------------------------------------------------------
// nn.Dropout (type_transition.py:13,17) on a flat fp32 tensor: y[e] = x[e] * m[e], m = the counter-based mask of
// common.h (0 or 1/(1-p)).  Its own backward (dx = dy * m with the same seed / offset).  One 16-B group per thread.
__global__ void dropout_kernel(const float* x, size_t n4, DropCfg drop, unsigned stream, float* y) {
    const size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n4) return;
    float m[4];
    pc_dropout_keep4(drop, (unsigned)g, stream, m);
    const float4 v = *reinterpret_cast<const float4*>(x + 4 * g);
    *reinterpret_cast<float4*>(y + 4 * g) = make_float4(v.x * m[0], v.y * m[1], v.z * m[2], v.w * m[3]);
}

int launch_dropout(const float* x, size_t n, const pc_dropout& d, unsigned stream_id, float* y, hipStream_t st) {
    if (!x || !y || n == 0 || n % 4 || d.p <= 0.f || d.p >= 1.f) return PC_EINVAL;
    PC_LAUNCH(dropout_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, st, x, n / 4, make_dropcfg(d), stream_id, y);
    return pc_launch_status();
}

extern "C" int pc_dropout_hidden(const float* x, size_t n, const pc_dropout* d, float* y, void* stream) {
    if (!d) return PC_EINVAL;
    return launch_dropout(x, n, *d, PC_DROP_STREAM_HIDDEN, y, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------
// Index validation (the reference's nn.Embedding / dict lookups raise IndexError / KeyError for an id outside the
// table, p_companion.py:48-54): up to four index arrays against their table sizes in ONE launch; the number of bad
// entries is ADDED to *bad (a device counter the caller reads when it chooses to synchronise).  Entries of -1 are
// legal where allow_pad is set (the zero-row sentinel of the collate padding).
struct IdxJobs { const int32_t* idx[4]; int n[4], hi[4], allow_pad[4], count; };
__global__ void check_indices_kernel(IdxJobs j, int32_t* bad) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    int wrong = 0;
#pragma unroll
    for (int a = 0; a < 4; a++)
        if (a < j.count && t < j.n[a]) {
            const int v = j.idx[a][t];
            if (v >= j.hi[a] || v < (j.allow_pad[a] ? -1 : 0)) wrong++;
        }
    if (wrong) atomicAdd(bad, wrong);
}

extern "C" int pc_check_indices(const int32_t* const* idx, const int* n, const int* hi, const int* allow_pad, int count,
                                int32_t* bad, void* stream) {
    if (!idx || !n || !hi || !bad || count < 1 || count > 4) return PC_EINVAL;
    IdxJobs j = {};
    int mx = 0;
    for (int a = 0; a < count; a++) {
        if (!idx[a] || n[a] <= 0 || hi[a] <= 0) return PC_EINVAL;
        j.idx[a] = idx[a]; j.n[a] = n[a]; j.hi[a] = hi[a]; j.allow_pad[a] = allow_pad ? allow_pad[a] : 0;
        mx = n[a] > mx ? n[a] : mx;
    }
    j.count = count;
    PC_LAUNCH(check_indices_kernel, dim3((mx + 255) / 256), dim3(256), 0, (hipStream_t)stream, j, bad);
    return pc_launch_status();
}

extern "C" int pc_abi_version(void) { return PC_ABI_VERSION; }

// Developer knobs compiled into THIS translation unit's build (build.py passes PC_EXTRA_HIPCC_FLAGS to every file, so
// one unit sees them all).  The PC_EXP_* defines remove a part of a GEMM loop to price it -- such a build computes
// WRONG numbers by design -- and the *_TIMING defines add clock reads and atomics.  A production build returns 0;
// tests/test_abi.py and __graft_entry__.build() assert it, so a knob build can never be tested or benchmarked as the
// product.
extern "C" unsigned pc_build_flags(void) {
    unsigned f = 0;
#ifdef PC_EXP_NO_MFMA
    f |= PC_FLAG_EXP_NO_MFMA;
#endif
#ifdef PC_EXP_NO_SPLIT
    f |= PC_FLAG_EXP_NO_SPLIT;
#endif
#ifdef PC_EXP_NO_LDSREAD
    f |= PC_FLAG_EXP_NO_LDSREAD;
#endif
#ifdef PC_EXP_NO_DMA
    f |= PC_FLAG_EXP_NO_DMA;
#endif
#ifdef PC_EXP_NO_SLAB
    f |= PC_FLAG_EXP_NO_SLAB;
#endif
#ifdef PC_EXP_STAGGER
    f |= PC_FLAG_EXP_STAGGER;
#endif
#ifdef PC_EXP_DMA_L2
    f |= PC_FLAG_EXP_DMA_L2;
#endif
#ifdef PC_EXP_NO_BARRIER
    f |= PC_FLAG_EXP_NO_BARRIER;
#endif
#ifdef PC_EXP_NO_VMWAIT
    f |= PC_FLAG_EXP_NO_VMWAIT;
#endif
#ifdef PC_NT_TIMING
    f |= PC_FLAG_NT_TIMING;
#endif
#ifdef PC_JOINT_TIMING
    f |= PC_FLAG_JOINT_TIMING;
#endif
#ifdef PC_CHAIN_TIMING
    f |= PC_FLAG_CHAIN_TIMING;
#endif
    return f;
}
