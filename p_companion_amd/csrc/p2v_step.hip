// One iteration of Product2Vec.train_model's loop body (product2vec.py:126-159) in index
// form: the four FFN calls of :132-134 run as ONE segmented launch sequence over the
// concatenated rows [anchor | neighbours | positive | negatives] (BatchNorm statistics stay
// per call), then attention, loss and the whole backward.  Gradients overwrite `g`
// (= optimizer.zero_grad() + loss.backward()); the optimizer step is pc_adam_step.
#include "common.h"

struct StepWs {
    int32_t* idx_all;
    float *y, *h0, *a2, *a1, *bn;     // bn: mean, invstd, scale, shift  [4][MAX_SEG][H]
    float *q, *qt, *probs, *c, *sp, *ctx, *emb;
    float *dy, *demb, *dpos_tmp, *dneg_tmp;
    void* ffn_ws; size_t ffn_bytes;
    void* attn_ws; size_t attn_bytes;
    size_t total;
};

static StepWs step_ws_layout(void* base, int B, int N, int K, int D) {
    StepWs w;
    const size_t R = (size_t)B * (2 + N + K) + 1;          // +1: the shared padding row of the compact layout
    WsCarver cv(base);
    auto take = [&](size_t bytes) { return cv.bytes(bytes); };
    w.idx_all = (int32_t*)take(R * 4);
    w.y = (float*)take(R * D * 4);
    w.h0 = (float*)take(R * PC_H * 4);
    w.a2 = (float*)take(R * PC_H * 4);
    w.a1 = (float*)take(R * PC_H * 4);
    w.bn = (float*)take(4 * PC_MAX_SEG * PC_H * 4);
    w.q = (float*)take((size_t)B * D * 4);
    w.qt = (float*)take((size_t)B * PC_HEADS * D * 4);
    w.c = (float*)take((size_t)B * PC_HEADS * D * 4);
    w.sp = (float*)take((size_t)B * PC_HEADS * 4);
    w.probs = (float*)take((size_t)B * PC_HEADS * (N > 0 ? N : 1) * 4);
    w.ctx = (float*)take((size_t)B * D * 4);
    w.emb = (float*)take((size_t)B * D * 4);
    w.dy = (float*)take(R * D * 4);
    w.demb = (float*)take((size_t)B * D * 4);
    w.dpos_tmp = (float*)take((size_t)B * 4);
    w.dneg_tmp = (float*)take((size_t)B * 4);
    w.ffn_bytes = pc_p2v_ffn_workspace_bytes((int)R);
    w.ffn_ws = take(w.ffn_bytes);
    w.attn_bytes = N > 0 ? pc_p2v_attention_workspace_bytes_dim(B, N, D) : 0;
    w.attn_ws = take(w.attn_bytes);
    w.total = cv.total;
    return w;
}

extern "C" size_t pc_p2v_train_step_workspace_bytes_dim(int batch, int n_nbr, int k_neg, int dim) {
    if (batch <= 0 || n_nbr < 0 || k_neg <= 0 || (dim != 128 && dim != 256)) return 0;
    return step_ws_layout(nullptr, batch, n_nbr, k_neg, dim).total;
}
extern "C" size_t pc_p2v_train_step_workspace_bytes(int batch, int n_nbr, int k_neg) {
    return pc_p2v_train_step_workspace_bytes_dim(batch, n_nbr, k_neg, PC_D);
}
__device__ __forceinline__ void concat_idx_body(const int32_t* a, int na, const int32_t* b, int nb, const int32_t* c, int nc,
                                                const int32_t* d, int nd, int32_t* out, int i) {
    if (i < na) out[i] = a[i];
    else if (i < na + nb) out[i] = b[i - na];
    else if (i < na + nb + nc) out[i] = c[i - na - nb];
    else if (i < na + nb + nc + nd) out[i] = d[i - na - nb - nc];
}
__global__ void concat_idx_kernel(const int32_t* a, int na, const int32_t* b, int nb, const int32_t* c, int nc,
                                  const int32_t* d, int nd, int32_t* out) {
    concat_idx_body(a, na, b, nb, c, nc, d, nd, out, blockIdx.x * blockDim.x + threadIdx.x);
}

// The loader's side of the unsplit step's first launch (round 6): the same concatenation, queued behind the batch builder on
// ITS stream, with the neighbour row count read from the device (the host learns it a step later).
__global__ void concat_rows_dev_kernel(const int32_t* a, int na, const int32_t* b, const int32_t* nb_dev, int nb_cap, const int32_t* c,
                                       int nc, const int32_t* d, int nd, int32_t* out) {
    int nb = *nb_dev + 1;                                    // the distinct neighbours and the -1 row
    nb = nb < 1 ? 1 : (nb > nb_cap ? nb_cap : nb);
    concat_idx_body(a, na, b, nb, c, nc, d, nd, out, blockIdx.x * blockDim.x + threadIdx.x);
}

extern "C" int pc_p2v_concat_step_rows(const int32_t* anchor_idx, const int32_t* positive_idx, const int32_t* negative_idx,
                                       const int32_t* nb_rows, const int32_t* n_unique_dev, int nb_capacity, int B, int K,
                                       int32_t* rows_out, int rows_capacity, void* stream) {
    if (!anchor_idx || !positive_idx || !negative_idx || !nb_rows || !n_unique_dev || !rows_out) return PC_EINVAL;
    if (B <= 0 || K <= 0 || nb_capacity < 1) return PC_EINVAL;
    const long long most = (long long)B * (2 + K) + nb_capacity;
    if (most > rows_capacity) return PC_ESHAPE;
    PC_LAUNCH(concat_rows_dev_kernel, dim3((unsigned)((most + 255) / 256)), dim3(256), 0, (hipStream_t)stream, anchor_idx, B, nb_rows,
              n_unique_dev, nb_capacity, positive_idx, B, negative_idx, B * K, rows_out);
    return pc_launch_status();
}

// The step's first launch: the row-index concatenation AND every transposed weight of the step (workgroups
// [0, concat_blocks) concatenate, the rest are 32 x 32 transpose tiles, tiles_x x tiles_y per job) -- the two were separate
// launches of ~5 us each, i.e. of pure launch latency.
__global__ __launch_bounds__(256) void p2v_prologue_kernel(const int32_t* a, int na, const int32_t* b, int nb, const int32_t* c, int nc,
                                                           const int32_t* d, int nd, int32_t* out, int concat_blocks,
                                                           TransposeBatch tb, int tiles_x, int tiles_y) {
    __shared__ float t[32][33];
    if ((int)blockIdx.x < concat_blocks) {
        concat_idx_body(a, na, b, nb, c, nc, d, nd, out, blockIdx.x * 256 + threadIdx.x);
        return;
    }
    transpose_tile_body<256>(tb, (int)blockIdx.x - concat_blocks, tiles_x, tiles_y, t, threadIdx.x);
}

// One call of the step, by name.  nb_idx: neighbour rows of the step, nbc of them.  Dense layout: nbc = B*N slots in slot
// order (slot_row NULL).  Compact layout: the M real neighbours then one -1 row (nbc = M + 1), slot_row[B*N] maps every slot
// to its row and the -1 row carries the weight of all padding slots.
struct P2VStepCall {
    const pc_p2v_tensors *p = nullptr, *g = nullptr;
    const float* table = nullptr;
    const int32_t *anchor_idx = nullptr, *positive_idx = nullptr, *negative_idx = nullptr, *nb_idx = nullptr;
    int nbc = 0;
    const int32_t* slot_row = nullptr;
    // (unique-neighbour layout) multiplicity of each of the nbc neighbour rows (its last entry = the number of padding
    // slots): replaces the single weighted row of the compact layout; ref_off / ref_slot: row -> slots
    const float* nb_weight = nullptr;
    const int32_t *ref_off = nullptr, *ref_slot = nullptr;
    // [anchor | neighbour rows | positive | negatives] as the loader concatenated them (pc_p2v_concat_step_rows).  The step
    // then has no launch of its own in front of Linear0: the transposed weights, which nothing needs before the attention,
    // ride in the BatchNorm finalize launch of the FFN forward.
    const int32_t* rows_ready = nullptr;
    int B = 0, N = 0, K = 0;
    float margin = 0.f;
    float *loss = nullptr, *d_pos = nullptr, *d_neg = nullptr, *anchor_emb = nullptr;
    void* ws = nullptr;
    size_t ws_bytes = 0;
    // -1: the whole step with this replica's BatchNorm statistics; 0/1/2: see pc_p2v_train_step_compact_sync
    int phase = -1;
    double *fwd_sums = nullptr, *bwd_local = nullptr;
    const double* bwd_global = nullptr;
    const pc_adam_fused* adam = nullptr;     // the optimizer rides in the unsplit step's last launch only
    void* profile = nullptr;
    void* stream = nullptr;
    // The key-padding mask (a labelled deviation from the reference, off by default; compact and unique layouts, unsplit step):
    // the slots mapped to the padding row are no keys of the attention, and the neighbour call's BatchNorm spans the
    // n_real_slots real slots -- the padding row weighs 0 whatever nb_weight's last entry says (the caller's array is not written:
    // one batch serves both modes).
    bool masked = false;
    int n_real_slots = 0;
};

// the compact and unique layouts: n_real real neighbour rows in front of the padding row, every slot mapped (and a slot count
// that an int holds: the step indexes slots with one)
static bool nb_layout_ok(const int32_t* slot_row, const int32_t* nb_rows, int n_real, int B, int N) {
    const long long slots = (long long)B * N;
    return slot_row && nb_rows && N > 0 && n_real >= 0 && n_real <= slots && slots < INT32_MAX;
}

static int p2v_step_impl(const P2VStepCall& c) {
    const pc_p2v_tensors *p = c.p, *g = c.g;
    const int32_t *slot_row = c.slot_row, *rows_ready = c.rows_ready;
    const int B = c.B, N = c.N, K = c.K, nbc = c.nbc, phase = c.phase;
    void* const stream = c.stream;
    const bool p0 = phase <= 0, p1 = phase == -1 || phase == 1, p2 = phase == -1 || phase == 2;
    if ((c.adam || rows_ready) && phase != -1) return PC_EINVAL;
    if (c.adam && g) {
        // the gradient tensors must be views of the flat buffer the optimizer updates
        const float* gt[4] = {g->w0, g->w3, g->w5, g->out_proj_w};
        for (const float* x : gt)
            if (!x || x < c.adam->grad || x >= c.adam->grad + c.adam->n) return PC_EINVAL;
    }
    ProfileScope prof_scope((pc_profile*)c.profile);
    if (!p || !g || !c.table || !c.anchor_idx || !c.positive_idx || !c.negative_idx || !c.loss || !c.ws) return PC_EINVAL;
    if (B <= 0 || N < 0 || K <= 0 || (N > 0 && !c.nb_idx) || nbc < 0 || nbc > B * N + 1) return PC_EINVAL;
    // the anchor and positive calls are [B,128] BatchNorm inputs: the reference raises for a single row in training
    // mode (torch/nn/functional.py _verify_batch_size); so does a [1,5,128] negative block when K = 1
    if (B == 1) return PC_EBATCHNORM;
    if (c.masked) {
        if (phase != -1) return PC_EINVAL;                       // (cross-replica masked statistics: not built)
        if (!slot_row || N <= 0 || nbc < 1) return PC_EINVAL;
        // every real row holds at least one real slot
        if (c.n_real_slots < nbc - 1 || (long long)c.n_real_slots > (long long)B * N) return PC_EINVAL;
        if (!c.nb_weight && c.n_real_slots != nbc - 1) return PC_EINVAL;      // (compact layout: one row per real slot)
        if (c.n_real_slots == 1) return PC_EBATCHNORM;           // a neighbour call of one row, as B == 1 above
    }
    if (!p2v_dim_ok(p)) return PC_ESHAPE;
    const int D = p2v_dim(p);
    if (c.ws_bytes < pc_p2v_train_step_workspace_bytes_dim(B, N, K, D)) return PC_EWORKSPACE;
    hipStream_t st = (hipStream_t)stream;
    StepWs w = step_ws_layout(c.ws, B, N, K, D);
    const int32_t* rows = rows_ready ? rows_ready : w.idx_all;
    const int R = 2 * B + nbc + B * K;
    const int rA = 0, rN = B, rP = B + nbc, rG = rP + B;

    // call order of product2vec.py:132-134: anchor (:73), neighbours (:78), positive, negative
    pc_segments seg = {};
    seg.weighted_row = -1;
    seg.weight = 1.f;
    if (c.masked && c.n_real_slots == 0) {
        // a batch of padding alone: the neighbour call did not happen.  Its one (padding) row is carried at the end of the
        // anchor call's segment with weight 0 -- it enters no statistic and no gradient, and what the FFN makes of it is finite --
        // so three BatchNorm calls update the running statistics and num_batches_tracked, and nothing is divided by 0.
        seg.nseg = 3; seg.start[0] = rA; seg.start[1] = rP; seg.start[2] = rG; seg.start[3] = R; seg.start[4] = R;
        seg.count[0] = B;
        seg.weighted_row = rN; seg.weight = 0.f;
    } else if (c.masked) {
        seg.nseg = 4; seg.start[0] = rA; seg.start[1] = rN; seg.start[2] = rP; seg.start[3] = rG; seg.start[4] = R;
        seg.count[1] = c.n_real_slots;                         // BatchNorm sees the real slots only
        seg.weighted_row = rN + nbc - 1; seg.weight = 0.f;     // (looked up for rows outside row_weight's range: common.h row_multiplicity)
        if (c.nb_weight) { seg.row_weight = c.nb_weight; seg.row_weight_start = rN; seg.row_weight_rows = nbc - 1; }
    } else if (N > 0) {
        seg.nseg = 4; seg.start[0] = rA; seg.start[1] = rN; seg.start[2] = rP; seg.start[3] = rG; seg.start[4] = R;
        seg.count[1] = B * N;                                  // BatchNorm sees every padded slot
        if (c.nb_weight) { seg.row_weight = c.nb_weight; seg.row_weight_start = rN; seg.row_weight_rows = nbc; }
        else if (slot_row) { seg.weighted_row = rN + nbc - 1; seg.weight = (float)(B * N - (nbc - 1)); }
    } else {
        seg.nseg = 3; seg.start[0] = rA; seg.start[1] = rP; seg.start[2] = rG; seg.start[3] = R; seg.start[4] = R;
    }

    pc_ffn_saved sv;
    sv.h0 = w.h0; sv.a2 = w.a2; sv.a1 = w.a1;
    sv.bn_mean = w.bn; sv.bn_invstd = w.bn + PC_MAX_SEG * PC_H; sv.bn_scale = w.bn + 2 * PC_MAX_SEG * PC_H;
    sv.bn_shift = w.bn + 3 * PC_MAX_SEG * PC_H;
    // the FFN's call block: its four parts differ in the fields set in front of each (the sums are set in the split phases
    // alone, and each of those returns before another part could read them)
    FfnCall fc;
    fc.p = p; fc.g = g; fc.table = c.table; fc.idx = rows; fc.rows = R; fc.seg = &seg; fc.sv = &sv;
    fc.ws = w.ffn_ws; fc.ws_bytes = w.ffn_bytes; fc.stream = stream;
    // every transposed weight of the step (attention: Wo^T, Wq^T, [Wk;Wv]^T; FFN backward: W5^T, W3^T): one launch, which also
    // clears the key-bias gradient (exactly 0, see attention.hip); in the unsplit step it is the SAME launch as the row-index
    // concatenation
    TransposeBatch tb = {};
    if (p1) {
        PC_TRY(ffn_transposes(p, w.ffn_ws, R, 0, &tb));
        if (N > 0) PC_TRY(attention_transposes(p, w.attn_ws, B, N, slot_row ? nbc : B * N, &tb, g->in_proj_b + D));
    }
    if (p0) {
        if (rows_ready) {
            // (nothing to launch)
        } else if (phase == -1) {
            int tiles_x, tiles_y;
            transpose_batch_tiles(tb, &tiles_x, &tiles_y);
            const int cb = (R + 255) / 256;
            PC_LAUNCH(p2v_prologue_kernel, dim3(cb + tiles_x * tiles_y * tb.n), dim3(256), 0, st, c.anchor_idx, B, c.nb_idx, nbc,
                      c.positive_idx, B, c.negative_idx, B * K, w.idx_all, cb, tb, tiles_x, tiles_y);
        } else {
            PC_LAUNCH(concat_idx_kernel, dim3((R + 255) / 256), dim3(256), 0, st, c.anchor_idx, B, c.nb_idx, nbc, c.positive_idx, B,
                      c.negative_idx, B * K, w.idx_all);
        }
        PC_TRY(pc_launch_status());
        fc.local_sums = phase == 0 ? c.fwd_sums : nullptr;
        PC_TRY(ffn_forward_part1(fc));
        if (phase == 0) return PC_OK;
    }
    if (p2 && !p1) {
        fc.local_sums = c.bwd_local; fc.global_sums = c.bwd_global;
        return ffn_backward_part2(fc);
    }
    if (phase == 1) PC_TRY(launch_transpose_batch(tb, st));      // (the split step: phase 0 ran the concatenation alone)
    fc.update_running = 1; fc.y = w.y; fc.global_sums = phase == 1 ? c.fwd_sums : nullptr;
    fc.ride = rows_ready ? &tb : nullptr;
    PC_TRY(ffn_forward_part2(fc));

    pc_attn_saved as;
    as.q = w.q; as.qt = w.qt; as.probs = w.probs; as.c = w.c; as.sp = w.sp; as.ctx = w.ctx;
    const float* emb = w.y;                     // anchor embedding = FFN output when there are no neighbours
    // (D = 128 with neighbours, the hinge riding: the forward's out-projection chain is deferred into the backward's first launch)
    const bool out_chain_rides = N > 0 && D == 128 && K <= 8 && pc_opt_fused_loss() && pc_opt_fused_out_chain();
    NtArgs fwd_out_chain[2];
    // the attention block's call block, forward and backward
    AttnCall ac;
    ac.p = p; ac.query = w.y + (size_t)rA * D; ac.keys = w.y + (size_t)rN * D; ac.B = B; ac.N = N; ac.key_rows = nbc;
    ac.slot_row = slot_row; ac.sv = &as; ac.ws = w.attn_ws; ac.ws_bytes = w.attn_bytes; ac.stream = stream;
    ac.transposed = true; ac.masked = c.masked;
    if (N > 0) {
        ac.out = w.emb; ac.defer_out_chain = out_chain_rides ? fwd_out_chain : nullptr;
        PC_TRY(attention_forward_impl(ac));
        emb = w.emb;
    }

    float* dp_out = c.d_pos ? c.d_pos : w.dpos_tmp;
    float* dn_out = c.d_neg ? c.d_neg : w.dneg_tmp;
    float* demb = N > 0 ? w.demb : w.dy + (size_t)rA * D;
    // the hinge mean rides on the first launch of the attention backward (D = 128 with neighbours); nothing in the step reads it
    const bool mean_rides = N > 0 && D == 128;
    // ... and so does the hinge itself (round 6): the prologue of the attention backward's first chain (LossPro, common.h) --
    // pc_set_option(PC_OPT_FUSED_LOSS, 0) keeps its own launch
    const bool loss_rides = mean_rides && K <= 8 && pc_opt_fused_loss();
    const LossPro lp = {emb, w.y + (size_t)rP * D, w.y + (size_t)rG * D, B, K, c.margin, dp_out, dn_out,
                        w.dy + (size_t)rP * D, w.dy + (size_t)rG * D, w.demb};
    if (!loss_rides)
        PC_TRY(triplet_loss_launch(emb, w.y + (size_t)rP * D, w.y + (size_t)rG * D, B, K, D, c.margin, c.loss, dp_out,
                                   dn_out, demb, w.dy + (size_t)rP * D, w.dy + (size_t)rG * D, stream, mean_rides ? 0 : 1));
    const HingeMeanJob hm = {dp_out, dn_out, B, c.margin, c.loss};
    if (c.anchor_emb && !out_chain_rides)
        PC_HIP_TRY(hipMemcpyAsync(c.anchor_emb, emb, (size_t)B * D * 4, hipMemcpyDeviceToDevice, st));

    // the slab sums of ALL weight gradients of the step (attention: 10 few-row products, FFN: dW5, dW3 x 2, dW0) fold in
    // one launch at the end of the call
    TnDefer df;
    tn_defer_init(&df);
    if (phase == -1) df.fork = pc_fork_get(st);              // (the unsplit step: two small launches leave the main queue, common.h PcFork)
    df.adam = c.adam;                                          // torch.optim.Adam inside the final slab reduce (pc_p2v_train_step_unique_adam)
    // an error return below must not leave work on the side queue that nothing orders before the caller's next use (or
    // free) of the workspace and gradient buffers: join it into the main queue on the way out (a no-op after the normal
    // end of the step, whose reduce launch has joined already)
    struct ForkGuard {
        PcFork* f; hipStream_t st;
        ~ForkGuard() { if (f && f->pending) (void)pc_fork_join(f, 1, st); }
    } fork_guard{df.fork, st};
    if (N > 0) {
        ac.g = g; ac.pad_row = slot_row ? nbc - 1 : -1; ac.dout = w.demb;
        ac.dquery = w.dy + (size_t)rA * D; ac.dkeys = w.dy + (size_t)rN * D; ac.ref_off = c.ref_off; ac.ref_slot = c.ref_slot;
        ac.defer = &df; ac.rider = mean_rides ? &hm : nullptr; ac.loss = loss_rides ? &lp : nullptr;
        ac.fwd_out_chain = out_chain_rides ? fwd_out_chain : nullptr;
        PC_TRY(attention_backward_impl(ac));
        if (c.anchor_emb && out_chain_rides)                    // (the embedding exists once the backward's first launch has run)
            PC_HIP_TRY(hipMemcpyAsync(c.anchor_emb, emb, (size_t)B * D * 4, hipMemcpyDeviceToDevice, st));
    } else {
        PC_HIP_TRY(hipMemsetAsync(g->in_proj_w, 0, 3 * D * D * 4, st));
        PC_HIP_TRY(hipMemsetAsync(g->in_proj_b, 0, 3 * D * 4, st));
        PC_HIP_TRY(hipMemsetAsync(g->out_proj_w, 0, D * D * 4, st));
        PC_HIP_TRY(hipMemsetAsync(g->out_proj_b, 0, D * 4, st));
    }
    fc.dy = w.dy; fc.transposed = 1; fc.defer = &df; fc.local_sums = phase == 1 ? c.bwd_local : nullptr;
    PC_TRY(ffn_backward_part1(fc));
    if (phase == 1) return launch_tn_reduce_deferred(&df, st);
    PC_TRY(ffn_backward_part2(fc));
    return launch_tn_reduce_deferred(&df, st);
}

// what every entry point passes through unchanged
#define P2V_STEP_COMMON(c)                                                                              \
    c.p = p; c.g = g; c.table = table; c.B = B; c.N = N; c.K = K; c.margin = margin;                    \
    c.loss = loss; c.d_pos = d_pos; c.d_neg = d_neg; c.anchor_emb = anchor_emb;                         \
    c.ws = ws; c.ws_bytes = ws_bytes; c.stream = stream
#define P2V_STEP_TRIPLET(c) c.anchor_idx = anchor_idx; c.positive_idx = positive_idx; c.negative_idx = negative_idx

extern "C" int pc_p2v_train_step(const pc_p2v_tensors* p, const pc_p2v_tensors* g, const float* table,
                                 const int32_t* anchor_idx, const int32_t* positive_idx,
                                 const int32_t* negative_idx, const int32_t* neighbor_idx, int B, int N, int K,
                                 float margin, float* loss, float* d_pos, float* d_neg, float* anchor_emb,
                                 void* profile, void* ws, size_t ws_bytes, void* stream) {
    P2VStepCall c;
    P2V_STEP_COMMON(c); P2V_STEP_TRIPLET(c);
    c.nb_idx = neighbor_idx; c.nbc = B * N; c.profile = profile;
    return p2v_step_impl(c);
}

extern "C" int pc_p2v_train_step_compact(const pc_p2v_tensors* p, const pc_p2v_tensors* g, const float* table,
                                         const int32_t* anchor_idx, const int32_t* positive_idx,
                                         const int32_t* negative_idx, const int32_t* nb_rows, int n_real,
                                         const int32_t* slot_row, int B, int N, int K, float margin, float* loss,
                                         float* d_pos, float* d_neg, float* anchor_emb, void* profile, void* ws,
                                         size_t ws_bytes, void* stream) {
    if (!nb_layout_ok(slot_row, nb_rows, n_real, B, N)) return PC_EINVAL;
    P2VStepCall c;
    P2V_STEP_COMMON(c); P2V_STEP_TRIPLET(c);
    c.nb_idx = nb_rows; c.nbc = n_real + 1; c.slot_row = slot_row; c.profile = profile;
    return p2v_step_impl(c);
}

extern "C" int pc_p2v_train_step_compact_sync(const pc_p2v_tensors* p, const pc_p2v_tensors* g, const float* table,
                                              const int32_t* anchor_idx, const int32_t* positive_idx,
                                              const int32_t* negative_idx, const int32_t* nb_rows, int n_real,
                                              const int32_t* slot_row, int B, int N, int K, float margin, float* loss,
                                              float* d_pos, float* d_neg, float* anchor_emb, int phase,
                                              double* fwd_sums, double* bwd_local, const double* bwd_global, void* ws,
                                              size_t ws_bytes, void* stream) {
    if (!nb_layout_ok(slot_row, nb_rows, n_real, B, N)) return PC_EINVAL;
    if (phase < 0 || phase > 2 || !fwd_sums || !bwd_local || (phase == 2 && !bwd_global)) return PC_EINVAL;
    if ((((uintptr_t)fwd_sums | (uintptr_t)bwd_local | (uintptr_t)bwd_global) & 7)) return PC_ESHAPE;
    P2VStepCall c;
    P2V_STEP_COMMON(c); P2V_STEP_TRIPLET(c);
    c.nb_idx = nb_rows; c.nbc = n_real + 1; c.slot_row = slot_row;
    c.phase = phase; c.fwd_sums = fwd_sums; c.bwd_local = bwd_local; c.bwd_global = bwd_global;
    return p2v_step_impl(c);
}

// Unique-neighbour layout (see pcompanion_hip.h): nb_rows[n_unique + 1] distinct neighbour products then -1,
// nb_weight[n_unique + 1] their multiplicities then the number of padding slots, slot_row[B*N] slot -> row,
// ref_off / ref_slot row -> slots.
#define P2V_UNIQUE_OK (nb_layout_ok(slot_row, nb_rows, n_unique, B, N) && nb_weight && ref_off && ref_slot)
#define P2V_STEP_UNIQUE(c)                                                                              \
    c.nb_idx = nb_rows; c.nbc = n_unique + 1; c.slot_row = slot_row; c.nb_weight = nb_weight;           \
    c.ref_off = ref_off; c.ref_slot = ref_slot; c.profile = profile

extern "C" int pc_p2v_train_step_unique(const pc_p2v_tensors* p, const pc_p2v_tensors* g, const float* table,
                                        const int32_t* anchor_idx, const int32_t* positive_idx,
                                        const int32_t* negative_idx, const int32_t* nb_rows, const float* nb_weight,
                                        int n_unique, const int32_t* slot_row, const int32_t* ref_off,
                                        const int32_t* ref_slot, int B, int N, int K, float margin,
                                        float* loss, float* d_pos, float* d_neg, float* anchor_emb, void* profile,
                                        int phase, double* fwd_sums, double* bwd_local, const double* bwd_global,
                                        void* ws, size_t ws_bytes, void* stream) {
    if (!P2V_UNIQUE_OK) return PC_EINVAL;
    P2VStepCall c;
    P2V_STEP_UNIQUE(c);
    if (phase < -1 || phase > 2) return PC_EINVAL;
    if (phase >= 0 && (!fwd_sums || !bwd_local || (phase == 2 && !bwd_global))) return PC_EINVAL;
    P2V_STEP_COMMON(c); P2V_STEP_TRIPLET(c);
    c.phase = phase; c.fwd_sums = fwd_sums; c.bwd_local = bwd_local; c.bwd_global = bwd_global;
    return p2v_step_impl(c);
}

extern "C" int pc_p2v_train_step_unique_adam(const pc_p2v_tensors* p, const pc_p2v_tensors* g, const float* table,
                                             const int32_t* anchor_idx, const int32_t* positive_idx,
                                             const int32_t* negative_idx, const int32_t* nb_rows, const float* nb_weight,
                                             int n_unique, const int32_t* slot_row, const int32_t* ref_off,
                                             const int32_t* ref_slot, int B, int N, int K, float margin, float* loss,
                                             float* d_pos, float* d_neg, float* anchor_emb, void* profile, void* ws,
                                             size_t ws_bytes, const pc_adam_fused* adam, void* stream) {
    if (!P2V_UNIQUE_OK) return PC_EINVAL;
    P2VStepCall c;
    P2V_STEP_UNIQUE(c);
    P2V_STEP_COMMON(c); P2V_STEP_TRIPLET(c);
    c.adam = adam;
    return p2v_step_impl(c);
}

// ... with the step's row indices [anchor | nb_rows[0 .. n_unique] | positive | negatives] already concatenated
// (pc_p2v_concat_step_rows behind the loader's builder): the step's first launch is Linear0
extern "C" int pc_p2v_train_step_unique_rows(const pc_p2v_tensors* p, const pc_p2v_tensors* g, const float* table,
                                             const int32_t* step_rows, const int32_t* nb_rows, const float* nb_weight, int n_unique,
                                             const int32_t* slot_row, const int32_t* ref_off, const int32_t* ref_slot, int B, int N,
                                             int K, float margin, float* loss, float* d_pos, float* d_neg, float* anchor_emb,
                                             void* profile, void* ws, size_t ws_bytes, const pc_adam_fused* adam, void* stream) {
    if (!step_rows || B <= 0) return PC_EINVAL;
    if (!P2V_UNIQUE_OK) return PC_EINVAL;
    P2VStepCall c;
    P2V_STEP_UNIQUE(c);
    P2V_STEP_COMMON(c);
    c.anchor_idx = step_rows; c.positive_idx = step_rows + B + n_unique + 1; c.negative_idx = step_rows + 2 * B + n_unique + 1;
    c.adam = adam; c.rows_ready = step_rows;
    return p2v_step_impl(c);
}

// The masked mode of the compact and unique steps (see P2VStepCall::masked; pcompanion_hip.h has the semantics).
extern "C" int pc_p2v_train_step_compact_masked(const pc_p2v_tensors* p, const pc_p2v_tensors* g, const float* table,
                                                const int32_t* anchor_idx, const int32_t* positive_idx,
                                                const int32_t* negative_idx, const int32_t* nb_rows, int n_real,
                                                const int32_t* slot_row, int B, int N, int K, float margin, float* loss,
                                                float* d_pos, float* d_neg, float* anchor_emb, void* profile, void* ws,
                                                size_t ws_bytes, void* stream) {
    if (!nb_layout_ok(slot_row, nb_rows, n_real, B, N)) return PC_EINVAL;
    P2VStepCall c;
    P2V_STEP_COMMON(c); P2V_STEP_TRIPLET(c);
    c.nb_idx = nb_rows; c.nbc = n_real + 1; c.slot_row = slot_row; c.profile = profile;
    c.masked = true; c.n_real_slots = n_real;
    return p2v_step_impl(c);
}

extern "C" int pc_p2v_train_step_unique_masked(const pc_p2v_tensors* p, const pc_p2v_tensors* g, const float* table,
                                               const int32_t* anchor_idx, const int32_t* positive_idx,
                                               const int32_t* negative_idx, const int32_t* step_rows, const int32_t* nb_rows,
                                               const float* nb_weight, int n_unique, int n_real_slots, const int32_t* slot_row,
                                               const int32_t* ref_off, const int32_t* ref_slot, int B, int N, int K, float margin,
                                               float* loss, float* d_pos, float* d_neg, float* anchor_emb, void* profile, void* ws,
                                               size_t ws_bytes, const pc_adam_fused* adam, void* stream) {
    if (B <= 0 || !P2V_UNIQUE_OK || n_real_slots < 0) return PC_EINVAL;
    if (!step_rows && (!anchor_idx || !positive_idx || !negative_idx)) return PC_EINVAL;
    P2VStepCall c;
    P2V_STEP_UNIQUE(c);
    P2V_STEP_COMMON(c);
    if (step_rows) {
        c.anchor_idx = step_rows; c.positive_idx = step_rows + B + n_unique + 1; c.negative_idx = step_rows + 2 * B + n_unique + 1;
        c.rows_ready = step_rows;
    } else {
        P2V_STEP_TRIPLET(c);
    }
    c.adam = adam;
    c.masked = true; c.n_real_slots = n_real_slots;
    return p2v_step_impl(c);
}
