// P11 over a device CSR: Product2Vec.generate_all_embeddings (product2vec.py:83-111), eval mode, with the co-view graph
// resident in HBM and the products processed in chunks of bounded size.
//
//   e1  = ffn(x)                                                for every product
//   out = e1                                                    products without co-view out-neighbours
//   out = attn(query = ffn(e1[i]), keys = e1[cv_col[rowptr[i] : rowptr[i+1]]])   the others (exact list, no padding)
//
// The attention is the absorbed-projection form of attention.hip (attn_core_fwd4_kernel): qt = Wk_h^T q_h by the chain
// GEMM, a core that forms c[h] = sum_n p_{n,h} y_n and sp[h] = sum_n p_{n,h}, then ctx / out by the second chain.  What
// differs here: the number of keys varies per node and comes from the CSR, keys are read through cv_col, there are no
// saved probabilities (eval only), and the scores are RECOMPUTED instead of kept in LDS -- pass 1 takes the maximum,
// pass 2 the exp-sum, pass 3 the weighted sums -- so any degree works (the key rows are L2 hits after the first pass).
#include "common.h"
#include "wave_rows.h"        // LD<DL>, ld_load / ld_store, heads_reduce16, heads_fold4 (the lane layout of attn_core_fwd4_kernel)

// One wave per node of the chunk [first, first + rows).  qt [rows,HEADS,D] (unscaled Wk_h^T q_h) in; c [rows,HEADS,D],
// sp [rows,HEADS] out (zeros for a node without neighbours: the select kernel replaces its row afterwards).
// Neighbour ids are trusted (as in pc_gather_rows); row offsets are size_t (100 M x 128 overflows int32).
template <int DL>
__global__ __launch_bounds__(256) void export_attn_core_kernel(const float* __restrict__ qt, const float* __restrict__ e1,
                                                               const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                               int64_t first, int rows, float* __restrict__ c,
                                                               float* __restrict__ sp) {
    constexpr int D = 16 * DL;
    constexpr int UF = DL == 8 ? 4 : 2;                  // row groups of four per trip (loads in flight before the first use)
    constexpr int TRIP = 4 * UF;
    const int lane = threadIdx.x & 63, g = lane >> 4, l = lane & 15;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= rows) return;                               // wave-uniform
    const int64_t node = first + b;
    const int lo = rowptr[node], N = rowptr[node + 1] - lo;
    if (N <= 0) {
        const LD<DL> z = {};
        ld_store<DL>(c + ((size_t)b * PC_HEADS + g) * D + DL * l, z);
        if (lane < PC_HEADS) sp[(size_t)b * PC_HEADS + lane] = 0.f;
        return;
    }
    const int32_t* ids = col + lo;
    const float scale = DL == 8 ? 0.17677669529663687f : 0.125f;       // 1/sqrt(head dim)
    LD<DL> qv[PC_HEADS];
#pragma unroll
    for (int hh = 0; hh < PC_HEADS; hh++) {
        qv[hh] = ld_load<DL>(qt + ((size_t)b * PC_HEADS + hh) * D + DL * l);
#pragma unroll
        for (int d = 0; d < DL; d++) qv[hh].v[d] *= scale;
    }
    // one trip: the rows n0 + 4u + g (u < UF) and, in lane l, the score of head l >> 2 of each.  The node's ids are read 64
    // at a time into a register and handed out by shuffles; a dead slot loads the node's first row and is masked afterwards.
    int idreg = 0;
    auto trip = [&](int n0, LD<DL>* yu, float* s) {
        if ((n0 & 63) == 0) idreg = n0 + lane < N ? ids[n0 + lane] : ids[0];
#pragma unroll
        for (int u = 0; u < UF; u++) {
            const int n = n0 + 4 * u + g;
            const int row = __shfl(idreg, (n & 63), 64);
            yu[u] = ld_load<DL>(e1 + (size_t)row * D + DL * l);
        }
#pragma unroll
        for (int u = 0; u < UF; u++) {
            float p[PC_HEADS];
#pragma unroll
            for (int hh = 0; hh < PC_HEADS; hh++) {
                float t = 0.f;
#pragma unroll
                for (int d = 0; d < DL; d++) t += qv[hh].v[d] * yu[u].v[d];
                p[hh] = t;
            }
            s[u] = heads_reduce16(p[0], p[1], p[2], p[3], l);
        }
    };
    // pass 1: maximum of head l >> 2
    float m = -INFINITY;
    for (int n0 = 0; n0 < N; n0 += TRIP) {
        LD<DL> yu[UF];
        float s[UF];
        trip(n0, yu, s);
#pragma unroll
        for (int u = 0; u < UF; u++)
            if (n0 + 4 * u + g < N) m = fmaxf(m, s[u]);
    }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    // pass 2: exp-sum of head l >> 2 (the recomputed scores are the same bits as in pass 1)
    float sum = 0.f;
    for (int n0 = 0; n0 < N; n0 += TRIP) {
        LD<DL> yu[UF];
        float s[UF];
        trip(n0, yu, s);
#pragma unroll
        for (int u = 0; u < UF; u++)
            if (n0 + 4 * u + g < N) sum += expf(s[u] - m);
    }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.0f / sum;
    // pass 3: c[h] = sum_n p_{n,h} y_n over this lane's dims for all four heads (head hh's probability of the group's row
    // comes from lane 4 hh of the group), sp of head l >> 2
    LD<DL> o[PC_HEADS];
#pragma unroll
    for (int hh = 0; hh < PC_HEADS; hh++)
#pragma unroll
        for (int d = 0; d < DL; d++) o[hh].v[d] = 0.f;
    float spa = 0.f;
    for (int n0 = 0; n0 < N; n0 += TRIP) {
        LD<DL> yu[UF];
        float s[UF];
        trip(n0, yu, s);
#pragma unroll
        for (int u = 0; u < UF; u++) {
            const bool valid = n0 + 4 * u + g < N;
            const float pr = valid ? expf(s[u] - m) * inv : 0.f;
            spa += pr;
#pragma unroll
            for (int hh = 0; hh < PC_HEADS; hh++) {
                const float ph = __shfl(pr, 16 * g + 4 * hh, 64);
#pragma unroll
                for (int d = 0; d < DL; d++) o[hh].v[d] += ph * yu[u].v[d];
            }
        }
    }
    spa += __shfl_xor(spa, 16, 64);
    spa += __shfl_xor(spa, 32, 64);
    if (lane < 16 && (l & 3) == 0) sp[(size_t)b * PC_HEADS + (l >> 2)] = spa;
    // the four row groups fold: lane group g ends with head g
    const LD<DL> out = heads_fold4<DL>(o[0], o[1], o[2], o[3], (lane & 32) != 0, (lane & 16) != 0);
    ld_store<DL>(c + ((size_t)b * PC_HEADS + g) * D + DL * l, out);
}

// out[first + r] = e1[first + r] for the chunk's nodes without co-view out-neighbours (one float4 per thread)
__global__ __launch_bounds__(256) void export_select_kernel(const int32_t* __restrict__ rowptr, int64_t first, int rows, int d4,
                                                            const float* __restrict__ e1, float* __restrict__ out) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)rows * d4) return;
    const int64_t node = first + (int64_t)(t / d4);
    if (rowptr[node + 1] != rowptr[node]) return;
    const size_t at = (size_t)node * d4 + t % d4;
    reinterpret_cast<float4*>(out)[at] = reinterpret_cast<const float4*>(e1)[at];
}

// ---------------------------------------------------------------------------------------
struct ExportWs {
    void* ffn; size_t ffn_bytes;           // pc_p2v_ffn_forward_eval's own workspace for `chunk` rows
    float *e2, *q, *qt, *c, *sp, *ctx;     // [C,D], [C,D], [C,HEADS,D], [C,HEADS,D], [C,HEADS], [C,D]
    float *wkvt;                           // [D,2D]: [Wk;Wv]^T
    size_t total;
};

static ExportWs export_ws_layout(void* base, int chunk, int D) {
    ExportWs w;
    WsCarver cv(base);
    auto takef = [&](size_t floats) { return cv.floats(floats); };
    w.ffn_bytes = pc_p2v_ffn_workspace_bytes(chunk);
    w.ffn = cv.bytes(w.ffn_bytes);
    w.e2 = takef((size_t)chunk * D);
    w.q = takef((size_t)chunk * D);
    w.qt = takef((size_t)chunk * PC_HEADS * D);
    w.c = takef((size_t)chunk * PC_HEADS * D);
    w.sp = takef((size_t)chunk * PC_HEADS);
    w.ctx = takef((size_t)chunk * D);
    w.wkvt = takef((size_t)2 * D * D);
    w.total = cv.total;
    return w;
}

#define PC_EXPORT_MAX_CHUNK (1 << 20)     // (keeps chunk_rows x HEADS x D inside the GEMMs' int offsets)

extern "C" size_t pc_p2v_export_workspace_bytes(int chunk_rows, int dim) {
    if (chunk_rows <= 0 || chunk_rows > PC_EXPORT_MAX_CHUNK || (dim != 128 && dim != 256)) return 0;
    return export_ws_layout(nullptr, chunk_rows, dim).total;
}

extern "C" int pc_p2v_export_embeddings(const pc_p2v_tensors* p, const float* features, int64_t n_products,
                                        const int32_t* cv_rowptr, const int32_t* cv_col, float* e1, float* out,
                                        int chunk_rows, void* ws, size_t ws_bytes, void* stream) {
    if (!p || !features || n_products <= 0 || !cv_rowptr || !cv_col || !e1 || !out || chunk_rows <= 0 || !ws) return PC_EINVAL;
    if (!p2v_dim_ok(p)) return PC_ESHAPE;
    if (!p->w0 || !p->b0 || !p->gamma || !p->beta || !p->w3 || !p->b3 || !p->w5 || !p->b5 || !p->running_mean ||
        !p->running_var || !p->in_proj_w || !p->in_proj_b || !p->out_proj_w || !p->out_proj_b) return PC_EINVAL;
    if (n_products > INT32_MAX || chunk_rows > PC_EXPORT_MAX_CHUNK) return PC_ESHAPE;    // (node ids are int32)
    const int D = p->dim == 256 ? 256 : PC_D;
    if (ws_bytes < pc_p2v_export_workspace_bytes(chunk_rows, D)) return PC_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    ExportWs w = export_ws_layout(ws, chunk_rows, D);
    TransposeBatch tb = {};
    tb.job[0] = {p->in_proj_w + (size_t)D * D, w.wkvt, 2 * D, D};       // [Wk;Wv] [2D,D] -> [D,2D]
    tb.n = 1;
    PC_TRY(launch_transpose_batch(tb, st));
    // pass 1: e1 = ffn(x) for every product (every neighbour's key row must exist before any attention reads it)
    for (int64_t first = 0; first < n_products; first += chunk_rows) {
        const int rows = (int)(n_products - first < chunk_rows ? n_products - first : chunk_rows);
        PC_TRY(pc_p2v_ffn_forward_eval(p, features + (size_t)first * D, nullptr, rows, e1 + (size_t)first * D, w.ffn,
                                       w.ffn_bytes, stream));
    }
    // pass 2, per chunk: e2 = ffn(e1), q / qt, the ragged core, ctx / out straight into the table's rows, then the
    // degree-0 rows back to e1
    const float* bv = p->in_proj_b + 2 * D;
    for (int64_t first = 0; first < n_products; first += chunk_rows) {
        const int rows = (int)(n_products - first < chunk_rows ? n_products - first : chunk_rows);
        const float* e1c = e1 + (size_t)first * D;
        float* outc = out + (size_t)first * D;
        PC_TRY(pc_p2v_ffn_forward_eval(p, e1c, nullptr, rows, w.e2, w.ffn, w.ffn_bytes, stream));
        // in_proj rows [0,D) = Wq, [D,2D) = Wk, [2D,3D) = Wv; qt[r][h][:] = q[r][h hd : (h+1) hd] Wk[h hd : (h+1) hd][:]
        const NtArgs qch[2] = {nt_plain(w.e2, D, p->in_proj_w, D, p->in_proj_b, w.q, D, rows, D, D),
                               nt_plain(w.q, D, w.wkvt, 2 * D, nullptr, w.qt, PC_HEADS * D, rows, PC_HEADS * D, D)};
        const int qmodes[2] = {NT_MODE_PLAIN, NT_MODE_KHEAD};
        PC_TRY(launch_gemm_nt_chain(qch, qmodes, 2, st));
        if (D == 128) PC_LAUNCH(export_attn_core_kernel<8>, dim3((rows + 3) / 4), dim3(256), 0, st, w.qt, e1, cv_rowptr, cv_col,
                                first, rows, w.c, w.sp);
        else PC_LAUNCH(export_attn_core_kernel<16>, dim3((rows + 3) / 4), dim3(256), 0, st, w.qt, e1, cv_rowptr, cv_col,
                       first, rows, w.c, w.sp);
        PC_TRY(pc_launch_status());
        // ctx[:, head h] = c[:,h,:] Wv_h^T + bv_h sp[:,h];  out = ctx Wo^T + bo
        NtArgs c0 = nt_plain(w.c, PC_HEADS * D, p->in_proj_w + (size_t)2 * D * D, D, bv, w.ctx, D, rows, D, PC_HEADS * D);
        c0.brs = w.sp; c0.ldbrs = PC_HEADS;
        const NtArgs och[2] = {c0, nt_plain(w.ctx, D, p->out_proj_w, D, p->out_proj_b, outc, D, rows, D, D)};
        const int omodes[2] = {NT_MODE_AHEAD, NT_MODE_PLAIN};
        PC_TRY(launch_gemm_nt_chain(och, omodes, 2, st));
        const size_t threads = (size_t)rows * (D / 4);
        PC_LAUNCH(export_select_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, cv_rowptr, first, rows, D / 4,
                  e1, out);
        PC_TRY(pc_launch_status());
    }
    return PC_OK;
}
