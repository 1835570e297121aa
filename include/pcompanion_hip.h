/* pcompanion_hip.h -- C ABI of libpcompanion_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the two embedding-learning hot paths of P-Companion.  The
 * reference is pure Python/PyTorch: its "FFI for this path" is the nn.Module surface of
 * src/models/{product2vec,type_transition,item_prediction,p_companion}.py plus the two
 * loop bodies (product2vec.py:126-164, train.py:34-52).  Each entry point below replaces
 * the ATen op sequence of one reference method (cited per function); the Python classes
 * in p_companion_amd/ keep the reference's names/signatures and call these through ctypes.
 *
 * Conventions:
 *   - raw DEVICE pointers + explicit sizes; fp32 data, int32 indices, row-major, dense;
 *   - `stream` is a hipStream_t passed as void* (the caller's current stream); every call
 *     is asynchronous w.r.t. the host and never synchronises, allocates or frees DEVICE MEMORY;
 *   - caller-allocated outputs and workspace (pc_*_workspace_bytes queries);
 *   - return: 0 ok, <0 invalid argument (PC_E*), >0 a hipError_t; nothing throws;
 *   - re-entrant across host threads, streams and devices: two threads may step two models on two
 *     streams of one device concurrently (tests/test_gpu_streams.py runs exactly that, bit-equal to serial).
 *   Exceptions: the host-side helpers (pc_mt_*, pc_rccl_unique_id) take HOST pointers; pc_rccl_comm_create / _destroy are
 *   RCCL's communicator setup (they block until every rank has arrived and RCCL allocates its own buffers).
 *
 * Library-owned device state (the ONE exception to "no global state"; ABI 5 states what ABI 4 did silently):
 *   the unsplit fused Product2Vec step -- pc_p2v_train_step, pc_p2v_train_step_compact, and
 *   pc_p2v_train_step_unique with phase = -1 -- moves three small launches that nothing on `stream` waits
 *   for until later in the step (the attention block's dq chain and its ten few-row weight gradients, the
 *   BatchNorm-backward finalize) onto a SIDE QUEUE: one non-blocking hipStream_t + six timing-disabled
 *   hipEvent_t per (device, calling stream), created on the first such call on that stream (a process-wide
 *   table of 32 entries behind a mutex; when it is full, or creation fails, the step stays on `stream`).
 *   Fork and join are events: when the call returns, everything it enqueued -- on either queue -- is ordered
 *   before whatever the caller enqueues on `stream` next, so a caller that synchronises `stream` or records an
 *   event on it sees no difference; results are bit-identical either way (tested).  On an error return the
 *   side queue is joined into `stream` first (no work is left behind that could outlive the caller's buffers).
 *   Not used: on a stream that is being captured into a graph; by any other entry point; when switched off.
 *     pc_set_option(PC_OPT_SIDE_QUEUE, 0 / 1)   process-wide switch (default 1); takes effect at the next step
 *     pc_release_device_state()                 destroys every side queue and its events (call with no pc_*
 *                                               call in flight and the streams drained, e.g. before
 *                                               hipDeviceReset or at interpreter exit); they are re-created on demand
 *   No environment variable is read anywhere in the library.
 */
#ifndef PCOMPANION_HIP_H
#define PCOMPANION_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PC_OK 0
#define PC_EINVAL (-1)   /* null pointer / non-positive size */
#define PC_ESHAPE (-2)   /* dimension not supported by the kernels (see each function) */
#define PC_EWORKSPACE (-3)
#define PC_EBATCHNORM (-4) /* a BatchNorm call group of ONE row in training mode: nn.BatchNorm1d raises
                             "Expected more than 1 value per channel when training" (product2vec.py:17,39) */
#define PC_ECOMM (-5)    /* the RCCL library could not be loaded, or a communicator call failed (pc_rccl_last_error) */

#define PC_D 128         /* PRODUCT_EMB_DIM (config.py:8) */
#define PC_H 256         /* HIDDEN_SIZE (config.py:10) */
#define PC_HEADS 4       /* NUM_ATTENTION_HEADS (config.py:11) */
#define PC_L 64          /* TYPE_EMB_DIM (config.py:9) */
#define PC_MAX_SEG 4     /* BatchNorm call groups per launch (anchor, neighbours, positive, negative) */
/* doubles in one cross-replica BatchNorm exchange buffer: [seg][2][H] sums then [seg] row counts */
#define PC_BN_SYNC_DOUBLES (PC_MAX_SEG * 2 * 256 + PC_MAX_SEG)

/* 3: pc_ffn_saved gained the optional `a1` member (round 2; a caller built against version 2 passes a shorter struct);
 * 2: pc_p2v_tensors / pc_joint_tensors gained `dropout` (and `dim`). */
/* 5: pc_set_option / pc_get_option / pc_release_device_state (the side queue of the fused Product2Vec step is part of the
 *    contract; the PC_NO_FORK environment variable of version 4 is gone). */
/* 6: the data-parallel exchange slot (pc_exchange_fn, pc_exchange_adam, pc_joint_train_epoch_dp) and the library's own RCCL
 *    communicator behind it (pc_rccl_*): the gradient exchange of a replica is issued from the step's own call, on the step's
 *    stream, not from a host-language hook per step. */
/* 7: pc_rccl_alltoall / pc_rccl_allreduce_sum_f64 / pc_rccl_comm_stats: every collective of a step on the library's ONE
 *    communicator, chained across streams (the lookup all-to-all used to be torch.distributed's, on a second communicator). */
/* 8: the optimizer SHARDED over the replicas (pc_exchange_plan, pc_exchange_adam_plan, pc_joint_train_epoch_plan,
 *    pc_rccl_reduce_scatter_mean, pc_rccl_all_gather): reduce-scatter of the flat gradient, Adam on this rank's 1/world of it,
 *    all-gather of the updated parameters -- instead of an all-reduce and the full dense Adam on every rank (the [num_types,64]
 *    tables of src/models/p_companion.py:36-43 are 17.8 MB at config.py:27's num_types = 34800). */
#define PC_ABI_VERSION 8
int pc_abi_version(void);
/* Process-wide options.  PC_OPT_SIDE_QUEUE: 1 (default) = the unsplit fused Product2Vec step may use its side queue
 * (see "Library-owned device state" above), 0 = every launch stays on the caller's stream.
 * PC_OPT_SORTED_TABLE_GRADIENTS (the fused joint step at num_types > 512; src/models/p_companion.py:36-43): how the gradients of
 * the two [num_types,64] tables are summed.  1 (default) = the sorted form: the source rows are sorted by destination and every
 * destination's run is added in ascending source order -- bitwise reproducible at ANY number of touched rows (with hidden-layer
 * dropout every sample selects its own K types: thousands).  0 = the sorted form only with hidden-layer dropout; without it the
 * per-workgroup LDS tables of the touched rows, reproducible up to 512 touched rows per table (float atomics beyond) -- the
 * default of ABI 7's first builds, 13 us slower per step at num_types = 34800, batch 4096, kept for comparison.  Lists that do
 * not fit the sort kernel's LDS (num_types > 65535, more than 24576 source rows) take the LDS-table form either way.
 * PC_OPT_BN_FINALIZE_SIDE (ABI 8): where the fused Product2Vec step runs its BatchNorm-backward finalize (BatchNorm1d of
 * product2vec.py:16; dgamma / dbeta and the coefficients dW0's loader applies).  0 (default) = on the step's own queue between
 * dZ1 and dW3 (12-14 us there, no hops); 1 = on the side queue beside dW3 (rounds 3-5: the kernel hidden, two ~7 us cross-queue hops exposed), kept for
 * comparison.
 * PC_OPT_BN_FINALIZE_RIDES (ABI 8, additive): 1 (default) = with many rows (the full-tile weight-gradient path, rows >= 8192) and
 * pc_ffn_saved.a1 given, that finalize has no launch of its own: eight workgroups of the dW3 launch -- which does not depend on
 * it and has workgroups without rows to spare -- run it and leave.  The same function on the same inputs: the same bits.
 * 0 = its own launch as described above.  PC_OPT_BN_FINALIZE_SIDE = 1 overrides it.
 * PC_OPT_FUSED_LOSS (ABI 8): 1 (default) = the fused Product2Vec step at PRODUCT_EMB_DIM = 128 forms the triplet hinge of
 * product2vec.py:137-154 and its three input gradients inside the first launch of the attention backward (the 16 samples of a
 * tile compute their own rows: the same arithmetic, the same bits); 0 = as its own launch (rounds 1-5), kept for comparison.
 * PC_OPT_FUSED_OUT_CHAIN (ABI 8; needs PC_OPT_FUSED_LOSS): 1 (default) = the attention forward's last launch (ctx and the
 * out-projection, MultiheadAttention of product2vec.py:23-28,48-68) runs in front of that prologue in the same launch -- per
 * 16-sample tile: out-projection forward, hinge, out-projection backward; 0 = its own launch.  Same bits.
 * PC_OPT_DW0_STAGED_H (ABI 8, additive): how the weight-gradient kernel of Linear0 (dW0, rows >= 8192, no dx consumer) gets the
 * H0 values its loader needs for the BatchNorm backward of dZ1 (product2vec.py:15-16).  0 (default) = from global memory into
 * the registers of the thread that transforms the element; the LDS stage holds dZ1 and the gathered rows only.  1 = staged
 * through LDS beside dZ1 (the form before; 16-row chunks in three stages at PRODUCT_EMB_DIM = 128), kept for comparison.
 * The same expression on the same rows in the same order: the same bits.
 * Unknown option / value: PC_EINVAL.  Thread-safe. */
enum { PC_OPT_SIDE_QUEUE = 1, PC_OPT_SORTED_TABLE_GRADIENTS = 2, PC_OPT_BN_FINALIZE_SIDE = 3, PC_OPT_FUSED_LOSS = 4,
       PC_OPT_FUSED_OUT_CHAIN = 5, PC_OPT_BN_FINALIZE_RIDES = 6, PC_OPT_DW0_STAGED_H = 7 };
int pc_set_option(int option, int value);
int pc_get_option(int option, int* value);
/* Destroys the library-owned device state (side queues and their events) of every device; 0 or a hipError_t. */
int pc_release_device_state(void);
/* Bitmask of the developer knobs this library was compiled with (0 = a production build).  PC_FLAG_EXP_*: a part of a
 * GEMM loop is compiled out to price it (scripts/dev/nt_decompose.sh) -- WRONG numbers by design; *_TIMING: in-kernel
 * clock reads.  Checked by tests/test_abi.py and __graft_entry__.build(). */
enum {
    PC_FLAG_EXP_NO_MFMA = 1, PC_FLAG_EXP_NO_SPLIT = 2, PC_FLAG_EXP_NO_LDSREAD = 4, PC_FLAG_EXP_NO_DMA = 8,
    PC_FLAG_EXP_NO_SLAB = 16, PC_FLAG_EXP_STAGGER = 32, PC_FLAG_EXP_DMA_L2 = 64, PC_FLAG_NT_TIMING = 128,
    PC_FLAG_JOINT_TIMING = 256, PC_FLAG_CHAIN_TIMING = 512, PC_FLAG_EXP_NO_BARRIER = 1024, PC_FLAG_EXP_NO_VMWAIT = 2048
};
unsigned pc_build_flags(void);

/* Training-mode dropout (config.py:12 DROPOUT = 0.1 is live in every reference training step: the attention
 * probabilities of product2vec.py:23-28 and the hidden layer of type_transition.py:13,17).  ATen's dropout stream
 * cannot be reproduced, so the mask is the build's own, counter-based and restated in oracle/philox_oracle.py:
 * element e of the dropped tensor belongs to group e >> 2, the four keep decisions of a group are the four words
 * of Philox4x32-10(counter = (group, stream, offset lo, offset hi), key = seed); word i keeps element 4*group + i
 * iff word >= floor(p * 2^32); kept values are multiplied by fp32 1/(1-p).  stream 0 = attention probabilities
 * [B,HEADS,N] (after the softmax, before the weighted sum: F.multi_head_attention_forward), 1 = hidden layer [B,32].
 * `offset`: the caller's step counter -- forward and backward of one step pass the same value.  p == 0: off. */
typedef struct {
    float p;
    uint64_t seed, offset;
} pc_dropout;

/* ---------------------------------------------------------------------------------
 * Product2Vec parameters, reference state_dict layout (product2vec.py:14-29):
 *   ffn.0 Linear(D->H) w0[H,D] b0[H]; ffn.1 BatchNorm1d(H) gamma/beta/running_*[H];
 *   ffn.3 Linear(H->H) w3[H,H] b3[H]; ffn.5 Linear(H->D) w5[D,H] b5[D];
 *   attention.in_proj_weight[3D,D] in_proj_bias[3D]; out_proj.weight[D,D] .bias[D].
 * The same struct type carries gradients (running_* / num_batches_tracked unused there).
 * --------------------------------------------------------------------------------- */
typedef struct {
    float *w0, *b0, *gamma, *beta, *w3, *b3, *w5, *b5;
    float *in_proj_w, *in_proj_b, *out_proj_w, *out_proj_b;
    float *running_mean, *running_var;
    int64_t *num_batches_tracked;
    pc_dropout dropout;   /* attention-weight dropout of nn.MultiheadAttention(dropout=config.DROPOUT) in
                           * training mode (product2vec.py:23-28); all-zero = off (eval, or DROPOUT = 0) */
    int dim;              /* D = config.PRODUCT_EMB_DIM (product2vec.py:14-29 take it from the config): 128, or 256
                           * (BASELINE configs[4]; head dim 64).  0 = 128.  Shapes above with that D; H stays 256. */
} pc_p2v_tensors;

/* Row groups ("segments") of one FFN launch.  The reference calls the FFN once per tensor
 * (anchor, neighbours, positive, negative: product2vec.py:132-134 via :73,:78) and
 * BatchNorm's batch statistics span exactly the rows of that call; a launch processes the
 * concatenation of up to PC_MAX_SEG such calls, segment s = rows [start[s], start[s+1]). */
typedef struct {
    int nseg;
    int start[PC_MAX_SEG + 1];
    /* Optional row multiplicity (index path): at most ONE row of the launch, `weighted_row`
     * (-1 = none), stands for `weight` identical rows -- the all-zero padding rows collate_fn
     * appends to short neighbour lists (data_loader.py:186-198) are bit-identical inputs, so
     * they are carried once.  count[s] (0 = physical row count) is the LOGICAL number of rows of
     * segment s, i.e. what BatchNorm divides by. */
    int count[PC_MAX_SEG];
    int weighted_row;
    float weight;
    /* General form of the same idea: rows [row_weight_start, row_weight_start + row_weight_rows) carry
     * the multiplicities row_weight[i] (device pointer, NULL = none) -- the unique-neighbour layout, where
     * every distinct product of the neighbour call is one row standing for all its slots. */
    const float *row_weight;
    int row_weight_start, row_weight_rows;
} pc_segments;

/* Saved-for-backward activations of one FFN launch over R rows (caller allocates). */
typedef struct {
    float *h0;        /* [R,H]  Linear0 output (pre-BatchNorm)                           */
    float *a2;        /* [R,H]  tanh(Linear3(...))                                       */
    float *bn_mean;   /* [nseg,H] batch mean per segment                                 */
    float *bn_invstd; /* [nseg,H] 1/sqrt(biased var + 1e-5)                              */
    float *bn_scale;  /* [nseg,H] gamma*invstd                                           */
    float *bn_shift;  /* [nseg,H] beta - mean*gamma*invstd                               */
    float *a1;        /* [R,H] tanh(BN(h0)), OPTIONAL (NULL: recomputed from h0 where needed): when given, the
                       * forward writes it on the way (its Linear3 forms it anyway) and the backward's dW3 reads it */
} pc_ffn_saved;

/* P6: Product2Vec.get_initial_embedding, training mode (product2vec.py:31-46; ffn :14-21).
 *   y[r] = W5 tanh(W3 tanh(BN_s(W0 x_r + b0)) + b3) + b5,  x_r = idx ? table[idx[r]] : table[r]
 * idx[r] == -1 gathers an all-zero row (collate_fn's zero padding, data_loader.py:186-198).
 * Updates running_mean/var once per segment in segment order (momentum 0.1, unbiased var)
 * and num_batches_tracked += nseg when `update_running` != 0.
 * D=128, H=256 only.  ws: pc_p2v_ffn_workspace_bytes(R). */
size_t pc_p2v_ffn_workspace_bytes(int rows);
int pc_p2v_ffn_forward_train(const pc_p2v_tensors *p, const float *table, const int32_t *idx,
                             int rows, const pc_segments *seg, int update_running,
                             float *y, const pc_ffn_saved *saved, void *ws, size_t ws_bytes,
                             void *stream);

/* P6 / P11 eval mode: BatchNorm uses running statistics (product2vec.py:83-111 runs the
 * model under self.eval()).  No saved activations. */
int pc_p2v_ffn_forward_eval(const pc_p2v_tensors *p, const float *table, const int32_t *idx,
                            int rows, float *y, void *ws, size_t ws_bytes, void *stream);

/* Backward of P6 (what autograd derives for ffn :14-21).  dy[R,D] -> g->{w0,b0,gamma,beta,
 * w3,b3,w5,b5}: overwritten when accumulate == 0, += otherwise.  dx (may be NULL) receives
 * d(loss)/d(input rows) [R,D] for dense-tensor callers whose autograd graph continues below
 * the features; the index path passes NULL (the feature table is frozen input data,
 * synthetic_data.py:50-58).  `dy` is not modified. */
int pc_p2v_ffn_backward(const pc_p2v_tensors *p, const pc_p2v_tensors *g, const float *table,
                        const int32_t *idx, int rows, const pc_segments *seg, const float *dy,
                        const pc_ffn_saved *saved, float *dx, int accumulate, void *ws,
                        size_t ws_bytes, void *stream);

/* P7: Product2Vec.apply_attention -> nn.MultiheadAttention(128, 4 heads), ONE query token
 * per sample, keys == values == neighbour embeddings, attention-weight dropout p->dropout (product2vec.py:48-68).  The
 * reference passes no key-padding mask and these two entries have none; the _masked forms below add one.
 * query[B,D], keys[B*N,D] -> out[B,D].
 * With ONE query token the K and V projections of the key rows are absorbed into the per-sample side (exact algebra,
 * csrc/attention.hip): score = (Wk_h^T q_h / sqrt(hd)) . key + const, ctx_h = Wv_h (sum_n pm_n key_n) + bv_h sum_n pm_n;
 * no [B*N, 2D] K|V buffer exists.
 * Saved for backward: q[B,D] (projected, unscaled), qt[B,HEADS,D] (Wk_h^T q_h), probs[B,HEADS,N] (before dropout),
 * c[B,HEADS,D] (sum_n pm_n key_n), sp[B,HEADS] (sum_n pm_n), ctx[B,D] (pre-out_proj).
 * ws: pc_p2v_attention_workspace_bytes(B,N). */
typedef struct {
    float *q, *qt, *probs, *c, *sp, *ctx;
} pc_attn_saved;
size_t pc_p2v_attention_workspace_bytes(int batch, int n_keys);                       /* D = 128 */
size_t pc_p2v_attention_workspace_bytes_dim(int batch, int n_keys, int dim);          /* D = 128 or 256 */
int pc_p2v_attention_forward(const pc_p2v_tensors *p, const float *query, const float *keys,
                             int batch, int n_keys, float *out, const pc_attn_saved *saved,
                             void *ws, size_t ws_bytes, void *stream);
/* Backward of P7: dout[B,D] -> dquery[B,D], dkeys[B*N,D]; g->{in_proj_w,in_proj_b,
 * out_proj_w,out_proj_b} overwritten (accumulate == 0) or +=. */
int pc_p2v_attention_backward(const pc_p2v_tensors *p, const pc_p2v_tensors *g,
                              const float *query, const float *keys, int batch, int n_keys,
                              const float *dout, const pc_attn_saved *saved, float *dquery,
                              float *dkeys, int accumulate, void *ws, size_t ws_bytes,
                              void *stream);
/* P7 with a key-padding mask -- a labelled deviation from the reference (nn.MultiheadAttention's key_padding_mask, which
 * product2vec.py never passes); the entries above stay the parity default.  key_pad[B*N] (uint8, device): nonzero = slot (b,n)
 * is padding and no key.  It is left out of the running maximum and of the softmax sum, its saved probability is exactly
 * 0.0f and its key row is never multiplied in (it may hold anything); the dropout multiplier of a real slot is the one it
 * draws without the mask (element (b,h,n) of the [B,HEADS,N] tensor).  A sample whose slots are all padding gets a zero
 * context: out = out_proj_b, every value finite (torch gives NaN there).  Backward: dkeys rows of padding slots come back as
 * zeros; such a sample sends nothing to dquery or to in_proj.  Same workspace and saved buffers as above. */
int pc_p2v_attention_forward_masked(const pc_p2v_tensors *p, const float *query, const float *keys,
                                    const uint8_t *key_pad, int batch, int n_keys, float *out,
                                    const pc_attn_saved *saved, void *ws, size_t ws_bytes, void *stream);
int pc_p2v_attention_backward_masked(const pc_p2v_tensors *p, const pc_p2v_tensors *g,
                                     const float *query, const float *keys, const uint8_t *key_pad, int batch,
                                     int n_keys, const float *dout, const pc_attn_saved *saved, float *dquery,
                                     float *dkeys, int accumulate, void *ws, size_t ws_bytes, void *stream);

/* P11 over a device CSR: Product2Vec.generate_all_embeddings (product2vec.py:83-111), eval mode, the whole table.
 *   e1[i]  = ffn(features[i])                                      every product (written; the caller keeps or drops it)
 *   out[i] = e1[i]                                                 cv_rowptr[i+1] == cv_rowptr[i]
 *   out[i] = attn(query = ffn(e1[i]), keys = e1[cv_col[cv_rowptr[i] : cv_rowptr[i+1]]])   otherwise (exact list, no padding)
 * features, e1, out [n_products, D] (D = p->dim: 128 or 256); cv_rowptr [n_products + 1], cv_col [cv_rowptr[n_products]],
 * int32, device-resident; neighbour ids are trusted (as in pc_gather_rows).  Any degree.  Products are processed in chunks
 * of chunk_rows (1 .. 2^20) on `stream`, a handful of launches per chunk, no host readback; the workspace depends on
 * chunk_rows only: pc_p2v_export_workspace_bytes(chunk_rows, D). */
size_t pc_p2v_export_workspace_bytes(int chunk_rows, int dim);
int pc_p2v_export_embeddings(const pc_p2v_tensors *p, const float *features, int64_t n_products,
                             const int32_t *cv_rowptr, const int32_t *cv_col, float *e1, float *out,
                             int chunk_rows, void *ws, size_t ws_bytes, void *stream);

/* P9: the loss of Product2Vec.train_model (product2vec.py:137-154), forward + backward:
 *   d+ = ||a - p + 1e-6||, d- = mean_j ||a - n_j + 1e-6||, loss = mean_b relu(margin - d+ + d-)
 * a[B,D], p[B,D], n[B*K,D] (row b*K+j).  Outputs: loss[1], d_pos[B], d_neg[B] and, when
 * non-NULL, da/dp/dn = d(loss)/d(.)  (already including the 1/B of the mean). */
int pc_p2v_triplet_loss(const float *a, const float *p, const float *n, int batch, int k_neg,
                        float margin, float *loss, float *d_pos, float *d_neg, float *da,
                        float *dp, float *dn, void *stream);                                   /* D = 128 */
int pc_p2v_triplet_loss_dim(const float *a, const float *p, const float *n, int batch, int k_neg, int dim,
                            float margin, float *loss, float *d_pos, float *d_neg, float *da,
                            float *dp, float *dn, void *stream);                               /* D = 128 or 256 */

/* P10: torch.optim.Adam (scripts/pretrain_product2vec.py:34, train.py:24; defaults beta
 * (0.9,0.999), eps 1e-8), no weight decay / amsgrad, bias-corrected, dense over `n` floats.
 * `step_count` is a DEVICE int64 incremented by the call (so a captured graph replays);
 * `scalars` is a DEVICE float[2] scratch.  All four arrays 16-byte aligned. */
int pc_adam_step(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, size_t n,
                 int64_t *step_count, float *scalars, double lr, double beta1, double beta2,
                 double eps, void *stream);
/* The same update as ONE launch when the caller knows the step number t (>= 1) on the host -- an optimizer that owns every
 * increment of its counter: the bias corrections are formed per workgroup by the same fp64 expressions (same bits as
 * pc_adam_step), *step_count (may be NULL) is left = t. */
int pc_adam_step_at(float *param, const float *grad, float *exp_avg, float *exp_avg_sq, size_t n,
                    int64_t *step_count, int64_t t, double lr, double beta1, double beta2, double eps,
                    void *stream);

/* P9 whole: one iteration of Product2Vec.train_model's loop body (product2vec.py:126-159)
 * in index form: gather -> 4 FFN calls -> attention -> loss -> backward -> grads in `g`
 * (overwritten, i.e. zero_grad + backward).  The optimizer step is a separate call.
 *   anchor_idx[B], positive_idx[B], negative_idx[B*K], neighbor_idx[B*N] (-1 = zero row)
 * Outputs: loss[1] (+ d_pos/d_neg[B], anchor_emb[B,D] when non-NULL).  profile: NULL, or a
 * pc_profile_create handle (see below).
 * ws: pc_p2v_train_step_workspace_bytes(B,N,K). */
size_t pc_p2v_train_step_workspace_bytes(int batch, int n_nbr, int k_neg);                  /* D = 128 */
size_t pc_p2v_train_step_workspace_bytes_dim(int batch, int n_nbr, int k_neg, int dim);     /* D = 128 or 256 (p->dim) */
int pc_p2v_train_step(const pc_p2v_tensors *p, const pc_p2v_tensors *g, const float *table,
                      const int32_t *anchor_idx, const int32_t *positive_idx,
                      const int32_t *negative_idx, const int32_t *neighbor_idx, int batch,
                      int n_nbr, int k_neg, float margin, float *loss, float *d_pos,
                      float *d_neg, float *anchor_emb, void *profile, void *ws, size_t ws_bytes,
                      void *stream);

/* Same step with the neighbour rows COMPACTED: collate_fn pads short neighbour lists with all-zero
 * rows (data_loader.py:186-198) which the reference pushes through the FFN, BatchNorm and the
 * attention like any other row.  They are bit-identical inputs, hence bit-identical rows at every
 * layer, so the step carries them ONCE: nb_rows[n_real+1] = the real neighbours of the batch in slot
 * order followed by one -1 row; slot_row[B*N] = row of each slot (padding slots -> n_real).  The
 * shared row enters BatchNorm's statistics with weight B*N - n_real and collects the summed gradient
 * of the slots it stands for (the backward is linear in it): same numbers as the dense step up to
 * fp32 summation order, ~30% fewer rows at the benchmark's degree distribution.
 * Built by pc_build_similarity_batch_compact (row_off: device scratch int32[B+1]). */
int pc_p2v_train_step_compact(const pc_p2v_tensors *p, const pc_p2v_tensors *g, const float *table,
                              const int32_t *anchor_idx, const int32_t *positive_idx,
                              const int32_t *negative_idx, const int32_t *nb_rows, int n_real,
                              const int32_t *slot_row, int batch, int n_nbr, int k_neg, float margin,
                              float *loss, float *d_pos, float *d_neg, float *anchor_emb, void *profile,
                              void *ws, size_t ws_bytes, void *stream);

/* The same loop body (product2vec.py:126-159) in the unique-neighbour layout: the co-view neighbours
 * (bpg.get_neighbors, bpg.py:24-38, gathered per sample by data_loader.py:71-88) of a batch repeat (about a third of the real slots of a
 * 4096-anchor batch over 100 k products); identical table rows are identical FFN rows inside one BatchNorm
 * call, so -- exactly as for the zero-padding rows -- every DISTINCT neighbour product is carried once:
 *   nb_rows[n_unique + 1]    the distinct products (ascending) then -1 (the shared padding row)
 *   nb_weight[n_unique + 1]  how many slots each stands for; last entry = number of padding slots
 *   slot_row[B * N]          row of every (sample, slot)
 *   ref_off / ref_slot       the inverse: slots of every row, ascending (see pc_build_similarity_batch_unique)
 * (pc_build_similarity_batch_unique builds all of them.)  A row's multiplicity weights its BatchNorm sums and
 * the BatchNorm-backward correction; the gradients of the slots that share a row are summed: the attention
 * backward forms dK/dV row by row over the row's slots in ascending slot order (it sorts the row's list:
 * fixed summation order, no float atomics; a row with more than 64 slots is summed in fp64 instead).  Loss and gradients equal the dense step's up to fp32 summation order (tested).
 * phase: -1 = the whole step with this replica's BatchNorm statistics (fwd_sums / bwd_* ignored); 0,1,2 = the
 * cross-replica phases described at pc_p2v_train_step_compact_sync. */
int pc_p2v_train_step_unique(const pc_p2v_tensors *p, const pc_p2v_tensors *g, const float *table,
                             const int32_t *anchor_idx, const int32_t *positive_idx,
                             const int32_t *negative_idx, const int32_t *nb_rows, const float *nb_weight,
                             int n_unique, const int32_t *slot_row, const int32_t *ref_off,
                             const int32_t *ref_slot, int batch, int n_nbr, int k_neg,
                             float margin, float *loss, float *d_pos, float *d_neg, float *anchor_emb,
                             void *profile, int phase, double *fwd_sums, double *bwd_local,
                             const double *bwd_global, void *ws, size_t ws_bytes, void *stream);

/* The same loop body (product2vec.py:126-159; its four BatchNorm1d calls are ffn[1] of :14-21 reached through
 * :73,:78) with cross-replica BatchNorm statistics for data-parallel replicas ("all_reduce(sum) of
 * [2,256] sums + row count, once per BN call"): the same step, cut at the two points where BatchNorm needs
 * batch-wide sums.  Every replica runs
 *   phase 0   batch rows + Linear0 + per-segment sums          -> fwd_sums  (this replica)
 *   [host: all-reduce(SUM) fwd_sums over the replicas, in place]
 *   phase 1   statistics from fwd_sums (all replicas' rows), rest of the forward, loss, backward up to the
 *             BatchNorm-backward sums                          -> bwd_local (this replica)
 *   [host: bwd_global = all-reduce(SUM) of bwd_local, kept beside it]
 *   phase 2   dgamma/dbeta from bwd_local, BN backward with the means of bwd_global, dW0/db0
 * Buffers are PC_BN_SYNC_DOUBLES fp64 each ([seg][2][256] sums: forward sum x, sum x^2; backward sum dz,
 * sum dz*h0; then [seg] row counts), device memory.  The workspace carries the step's state between the
 * phases and must not be touched in between.  Gradients are those of THIS replica's mean loss under
 * batch-wide statistics: averaging them over replicas gives the single-device gradient of the concatenated
 * batch (tested).  Running statistics are updated from the batch-wide values. */
int pc_p2v_train_step_compact_sync(const pc_p2v_tensors *p, const pc_p2v_tensors *g, const float *table,
                                   const int32_t *anchor_idx, const int32_t *positive_idx,
                                   const int32_t *negative_idx, const int32_t *nb_rows, int n_real,
                                   const int32_t *slot_row, int batch, int n_nbr, int k_neg, float margin,
                                   float *loss, float *d_pos, float *d_neg, float *anchor_emb, int phase,
                                   double *fwd_sums, double *bwd_local, const double *bwd_global,
                                   void *ws, size_t ws_bytes, void *stream);
int pc_build_similarity_batch_compact(const int32_t *pair_ids, int batch, const int32_t *sim_pairs,
                                      const int32_t *cv_rowptr, const int32_t *cv_col,
                                      const int32_t *sim_rowptr, const int32_t *sim_col,
                                      int n_products, int n_pad, int k_neg, uint64_t seed,
                                      uint64_t step, int32_t *anchor_idx, int32_t *positive_idx,
                                      int32_t *negative_idx, int32_t *nb_rows, int32_t *slot_row,
                                      int32_t *row_off, void *stream);

/* Same batch in the unique-neighbour layout (see pc_p2v_train_step_unique).  n_real = number of real
 * neighbour slots (host-known: sum of the capped degrees), the upper bound of n_unique: nb_rows / nb_weight
 * hold n_real + 1 entries; *n_unique (device int) receives the number of distinct products.  Also the inverse
 * map, for the attention backward: ref_slot[n_real] = the real slots (sample * n_pad + position) grouped by
 * row -- in arrival order inside a row: the consumer sorts the few entries of a row before it sums --, and
 * ref_off[n_real + 2] = where each row's slots start (the padding row lists none).  `scratch`:
 * pc_build_similarity_batch_unique_scratch_bytes(n_products, batch * n_pad) bytes whose first 4 * n_products
 * bytes are ZERO-FILLED before the first call and left zeroed by every call (per-product occurrence
 * counters).  Integer work only: deterministic. */
size_t pc_build_similarity_batch_unique_scratch_bytes(int n_products, int max_slots /* batch * n_pad */);
int pc_build_similarity_batch_unique(const int32_t *pair_ids, int batch, const int32_t *sim_pairs,
                                     const int32_t *cv_rowptr, const int32_t *cv_col,
                                     const int32_t *sim_rowptr, const int32_t *sim_col, int n_products,
                                     int n_pad, int k_neg, uint64_t seed, uint64_t step, int n_real,
                                     int32_t *anchor_idx, int32_t *positive_idx, int32_t *negative_idx,
                                     int32_t *nb_rows, float *nb_weight, int32_t *slot_row,
                                     int32_t *ref_off, int32_t *ref_slot, int32_t *n_unique, void *scratch,
                                     size_t scratch_bytes, void *stream);

/* Optional measurement aid (bench.py's roofline leg; NULL everywhere else): a pool of HIP
 * events that pc_p2v_train_step records on its stream around each of its GEMM launches.
 * After synchronising the stream, pc_profile_summary totals launches / milliseconds /
 * algorithmic FLOPs per kernel kind (0 = gemm_nt_kernel, 1 = gemm_tn_kernel). */
int pc_profile_create(int capacity, void **out);
int pc_profile_destroy(void *profile);
/* Restrict the recorded brackets to the kinds whose bit is set (bit 0 gemm_nt_kernel, bit 1 gemm_tn*,
 * bit 2 gemm_nt_small_kernel); default all. */
int pc_profile_set_kinds(void *prof, unsigned kinds);
int pc_profile_reset(void *profile);
int pc_profile_summary(void *profile, int kind, int *launches, double *total_ms,
                       double *total_flops);

/* P1-P4 on device: build one index batch from the CSR graph (bpg.py:24-38 get_neighbors,
 * data_loader.py:27-40 negative sampling rules, :186-198 padding).  pair_ids[B] selects
 * (anchor, positive) = sim_pairs[pair]; neighbours = co-view CSR row of the anchor, right
 * padded with -1 to n_pad; negatives: k distinct uniform draws (Philox4x32-10 keyed by
 * seed/step/sample) rejecting the anchor, the anchor's positives (sim CSR) and repeats. */
int pc_build_similarity_batch(const int32_t *pair_ids, int batch, const int32_t *sim_pairs,
                              const int32_t *cv_rowptr, const int32_t *cv_col,
                              const int32_t *sim_rowptr, const int32_t *sim_col, int n_products,
                              int n_pad, int k_neg, uint64_t seed, uint64_t step,
                              int32_t *anchor_idx, int32_t *positive_idx, int32_t *negative_idx,
                              int32_t *neighbor_idx, void *stream);

/* J1 on device: ComplementaryDataset.__getitem__ + collate_fn (data_loader.py:133-157) for `batch`
 * labelled pairs[b] = (query, target, label in {+1,-1}) (int32 x3): query_idx/query_types/
 * pos_types/neg_types [B] by the reference's label rules (:148-151), pos_items/neg_items [B,D] =
 * feat(target) or an N(0,1) filler (torch.randn_like in the reference: input data; here Philox +
 * Box-Muller keyed by seed/step), target_features [B,D] optional. */
int pc_build_complementary_batch(const int32_t *pairs, int batch, const float *features,
                                 const int32_t *type_idx, int n_types, uint64_t seed, uint64_t step,
                                 int32_t *query_idx, int32_t *query_types, int32_t *pos_types,
                                 int32_t *neg_types, float *pos_items, float *neg_items,
                                 float *target_features, void *stream);
/* The same contract at PRODUCT_EMB_DIM = dim (ABI 8, additive; BASELINE configs[4]): features [*,dim], pos_items / neg_items /
 * target_features [B,dim]; filler chunk t = b * (dim / 4) + c of row b is pc_filler_chunk(seed, step, t), so at dim = 128 the
 * output is bit-identical to pc_build_complementary_batch.  PC_EINVAL as there (or batch * dim / 4 >= 2^31); PC_ESHAPE: dim
 * not 128 / 256. */
int pc_build_complementary_batch_dim(const int32_t *pairs, int batch, const float *features,
                                     const int32_t *type_idx, int n_types, int dim, uint64_t seed, uint64_t step,
                                     int32_t *query_idx, int32_t *query_types, int32_t *pos_types,
                                     int32_t *neg_types, float *pos_items, float *neg_items,
                                     float *target_features, void *stream);

/* P2 exact (HOST pointers, host code): SimilarityDataset._get_negative_samples
 * (data_loader.py:27-40) on CPython's `random` stream: MT19937, random.seed(int) key
 * schedule, choice() = _randbelow_with_getrandbits.  Bit-exact negative indices.
 * `state` is an opaque buffer of pc_mt_state_bytes() bytes owned by the caller. */
size_t pc_mt_state_bytes(void);
int pc_mt_seed(void *state, uint64_t seed);
uint32_t pc_mt_getrandbits(void *state, int k);            /* 1 <= k <= 32 */
uint64_t pc_mt_randbelow(void *state, uint64_t n);
int pc_mt_shuffle(void *state, int64_t *perm, int64_t n);  /* random.shuffle of perm */
int pc_mt_negative_samples(void *state, int32_t n_products, const int32_t *sim_rowptr,
                           const int32_t *sim_col, const int32_t *anchors, int64_t n, int k,
                           int32_t *out);

/* ---------------------------------------------------------------------------------
 * P-Companion joint step.  Reference state_dict layout (p_companion.py:26-43,
 * type_transition.py:11-12, item_prediction.py:11-20).
 * --------------------------------------------------------------------------------- */
typedef struct {
    float *product_table;  /* [P,D] frozen (p_companion.py:26-29)                        */
    float *enc_w, *enc_b;  /* type_transition.encoder  [L/2,L], [L/2]                    */
    float *dec_w, *dec_b;  /* type_transition.decoder  [L,L/2], [L]                      */
    float *typ_w, *typ_b;  /* item_prediction.type_projection [D,L], [D]                 */
    float *itm_w, *itm_b;  /* item_prediction.item_projection [D,D], [D]                 */
    float *query_types;    /* query_type_embeddings.weight [T,L]                         */
    float *comp_types;     /* complementary_type_embeddings.weight [T,L]                 */
    pc_dropout dropout;    /* nn.Dropout on the hidden layer in training mode (type_transition.py:13,17);
                            * all-zero = off */
} pc_joint_tensors;

typedef struct {
    float *h;       /* [B,L/2] relu(encoder(E_q[query_types]))   (type_transition.py:17)  */
    float *c;       /* [B,L]   decoder(h)  (complementary base, type_transition.py:19)     */
    float *pi;      /* [B,D]   item_projection(E_prod[query_idx]) (item_prediction.py:31)  */
    float *tp;      /* [B*K,D] type_projection(E_c[topk])        (item_prediction.py:35)  */
} pc_joint_saved;

/* J3+J4+J5: PCompanion.forward (p_companion.py:45-77) with integer ids (the str->idx map
 * of :47-49 stays host-side).
 *   sims[B,T] = dec(relu(enc(E_q[query_types]))) . E_c^T ; topk[B,K] (int32, descending,
 *   ties -> lower index first); proj[B,K,D] = item_proj(E_prod[query_idx])[:,None,:] *
 *   type_proj(E_c[topk]).  D=128, L=64, K<=8, dropout 0.  The nn.Embedding lookups are
 *   fused into the GEMM loaders as row gathers. */
size_t pc_joint_workspace_bytes(int batch, int num_types, int k);
int pc_joint_forward(const pc_joint_tensors *p, const int32_t *query_idx,
                     const int32_t *query_types, int batch, int num_types, int k, float *sims,
                     int32_t *topk, float *proj, const pc_joint_saved *saved, void *ws,
                     size_t ws_bytes, void *stream);

/* J6: PCompanion.compute_loss (p_companion.py:79-119), forward + backward w.r.t. its two
 * differentiable inputs:  type = mean_b clamp(margin - S[b,pos_b] + S[b,neg_b], 0);
 * item = mean_{b,k} clamp(margin - ||proj-pos_item|| + ||proj-neg_item||, 0);
 * loss = alpha*item + (1-alpha)*type.  losses[3] = {loss, type, item}.
 * dsims is SPARSE: dsims_val[B,2] holds d(loss)/dS at columns (pos_b, neg_b) -- the only
 * non-zeros (the reference materialises a dense [B,T] zero gradient: SURVEY section 6).
 * dsims_val / dproj may be NULL (forward only).  partials: device scratch float[2*B].
 * At the kinks the gradients are torch's: a hinge of exactly 0 is active (clamp: slope 1 at 0), a
 * norm of exactly 0 sends nothing (subgradient 0). */
int pc_joint_loss(const float *sims, const float *proj, const int32_t *pos_types,
                  const int32_t *neg_types, const float *pos_items, const float *neg_items,
                  int batch, int num_types, int k, float margin, float alpha, float *losses,
                  float *dsims_val, float *dproj, float *partials, void *stream);
int pc_joint_loss_dim(const float *sims, const float *proj, const int32_t *pos_types, const int32_t *neg_types,
                      const float *pos_items, const float *neg_items, int batch, int num_types, int k, int dim,
                      float margin, float alpha, float *losses, float *dsims_val, float *dproj, float *partials,
                      void *stream);                                                   /* PRODUCT_EMB_DIM 128 or 256 */

/* Dense form of the sparse type-hinge gradient, for callers whose autograd graph needs
 * d(loss)/d(type_similarities) as a [B,T] tensor (what p_companion.py:96-97's advanced
 * indexing produces in the reference): dense = 0; dense[b,pos_b] += v[b,0]; dense[b,neg_b] += v[b,1]. */
int pc_expand_type_grad(const float *dsims_val, const int32_t *pos_types,
                        const int32_t *neg_types, int batch, int num_types, float *dense,
                        void *stream);

/* Backward of J3-J5 from (dsims_val, dproj) -> g (overwritten = zero_grad + backward),
 * including the row-sparse scatter-add into the two [T,L] type tables (J7): only rows
 * query_types[b], topk[b,:], pos_types[b], neg_types[b] receive gradient. */
int pc_joint_backward(const pc_joint_tensors *p, const pc_joint_tensors *g,
                      const int32_t *query_idx, const int32_t *query_types,
                      const int32_t *pos_types, const int32_t *neg_types, const int32_t *topk,
                      int batch, int num_types, int k, const float *dsims_val,
                      const float *dproj, const pc_joint_saved *saved, void *ws,
                      size_t ws_bytes, void *stream);

/* J8 loop body (train.py:42-46): forward + loss + backward; Adam is pc_adam_step. */
int pc_joint_train_step(const pc_joint_tensors *p, const pc_joint_tensors *g,
                        const int32_t *query_idx, const int32_t *query_types,
                        const int32_t *pos_types, const int32_t *neg_types,
                        const float *pos_items, const float *neg_items, int batch,
                        int num_types, int k, float margin, float alpha, float *losses,
                        int32_t *topk, void *ws, size_t ws_bytes, void *stream);

/* J8 loop body, FUSED (train.py:42-48: forward, compute_loss, zero_grad, backward and -- optionally --
 * optimizer.step as TWO launches at num_types <= 128): one kernel over 16-sample tiles computes the whole per-sample
 * part (row gathers, type transition with dropout, similarities + top-K, item projection, both hinges, the dX chain)
 * and, from the operands it holds in LDS, the tile's share of the gradients of the four Linears and of both [T,64] tables
 * (one-hot products; the type hinge's two dE_c rows per sample ride in the same product: no float atomics, bitwise
 * reproducible) as one slab per tile; one kernel sums the slabs in fixed order into g, forms losses[3] = {loss, type,
 * item} and, when exp_avg / exp_avg_sq are given, applies torch.optim.Adam's update (defaults of train.py:24) to p in the
 * same pass (*step_count is advanced by one).  128 < num_types <= 512: the gradient products run as their own kernel
 * over row buffers (three launches).
 * exp_avg == NULL: gradients only (a data-parallel caller all-reduces g, then pc_adam_step).
 * T <= 512: as above.  T > 512 (config.py:27 NUM_TYPES = 34800): the similarity row and its top-K are formed once per
 * DISTINCT query type of the batch (it is a function of the type alone), the [B,T] matrix never exists; the table
 * gradients are fixed-order sums over the touched rows (per-workgroup partial tables in LDS, added in source order, then a
 * fixed-order fold: bitwise reproducible) while a table has <= 512 touched rows in the batch -- the reference's catalogue
 * has 20 live types, the benchmark's 100 -- and float atomics into the cleared dense g beyond that.  With hidden-layer
 * dropout (p > 0: config.py:12 ships 0.1) c differs from sample to sample: the similarity row and its top-K are then formed
 * per SAMPLE (the [B,64] x [64,T] product of p_companion.py:60-63 through the 32-wide hidden layer on the bf16 matrix cores;
 * still never written), everything else as above (ABI 5; version 4 refused this combination).  Either way the selection is
 * exact (descending, ties -> the lower index, like torch.topk): a first pass keeps the maximum of every 64-type sub-chunk of a
 * row with a rigorous error bound, a second re-forms in fp32 the sub-chunks that can hold one of the K best and selects there.
 * Ids outside their tables (query_idx vs num_products, the three type arrays vs num_types) are clamped, counted into
 * *bad_count (may be NULL) and never dereferenced out of bounds -- the reference raises at the lookup
 * (p_companion.py:48-54), the caller raises when it reads the counter.
 * pc_joint_fused_supported: 1 iff (num_types, k, dropout p) is served (k <= 4; see above), else use pc_joint_train_step. */
size_t pc_joint_fused_workspace_bytes(int batch, int num_types, int k);
int pc_joint_fused_supported(int num_types, int k, float dropout_p);
/* After a fused step at num_types > 512: the touched rows of the two [T,64] table gradients -- ascending distinct row ids
 * rows_comp / rows_query and their counts n_touched (device int32[2]) -- as pointers INTO `ws` (valid until the next step
 * on it).  The row list a data-parallel job exchanges instead of the dense tables (north_star: "reduce-scatter for the
 * sparse grads"; src/models/p_companion.py:36-43 + train.py:46-48): 17.8 MB of dense tables at T = 34800 against
 * 260 B per touched row. */
int pc_joint_fused_touched(void *ws, size_t ws_bytes, int batch, int num_types, int k, const int32_t **rows_comp,
                           const int32_t **rows_query, const int32_t **n_touched);
int pc_joint_fused_step(const pc_joint_tensors *p, const pc_joint_tensors *g, const pc_joint_tensors *exp_avg,
                        const pc_joint_tensors *exp_avg_sq, int64_t *step_count, double lr, double beta1,
                        double beta2, double eps, const int32_t *query_idx, const int32_t *query_types,
                        const int32_t *pos_types, const int32_t *neg_types, const float *pos_items,
                        const float *neg_items, int batch, int num_types, int k, int num_products, float margin,
                        float alpha, float *losses, int32_t *topk, int32_t *bad_count, void *ws, size_t ws_bytes,
                        void *stream);

/* The loader's batch construction (pc_build_complementary_batch, data_loader.py:133-157) and the fused step as ONE call
 * over `batch` labelled pairs[b] = (query, target, label): query_idx .. neg_items are OUTPUT buffers here -- after the call
 * they hold the batch exactly as pc_build_complementary_batch(pairs, ..., seed, step) writes it (same filler bits), for
 * whoever reads the batch afterwards (metrics, logging).  num_types <= 128 or > 512: the step's own kernels derive the ids
 * and the item rows (one launch and a 4 MB round trip less); 128 < num_types <= 512: the builder's launch, then the step.
 * `features` [num_products, 128] is the table the dataset serves item rows from (train.py:115: the exported Product2Vec
 * embeddings), `type_idx` [num_products] the products' type ids, `n_types` the dataset's modulus for the negative type. */
int pc_joint_fused_step_pairs(const pc_joint_tensors *p, const pc_joint_tensors *g, const pc_joint_tensors *exp_avg,
                              const pc_joint_tensors *exp_avg_sq, int64_t *step_count, double lr, double beta1,
                              double beta2, double eps, const int32_t *pairs, const float *features,
                              const int32_t *type_idx, int n_types, uint64_t seed, uint64_t step,
                              int32_t *query_idx, int32_t *query_types, int32_t *pos_types, int32_t *neg_types,
                              float *pos_items, float *neg_items, int batch, int num_types, int k, int num_products,
                              float margin, float alpha, float *losses, int32_t *topk, int32_t *bad_count, void *ws,
                              size_t ws_bytes, void *stream);

/* train.py:36-57 train_epoch (for batch in loader: forward, loss, zero_grad, backward, optimizer.step) over `n_pairs`
 * labelled pairs in epoch order on the device, as ONE call: full batches of `batch` pairs, then (unless drop_last) the
 * ragged rest, each through pc_joint_fused_step_pairs with the loader's step counter first_step + i and the dropout
 * offset p->dropout.offset + i.  losses_out[3 * i ..] = {loss, type, item} of step i, on the device (the reference's
 * loss.item() per step is one device round trip per batch).  The batch buffers (sized for `batch`) hold the last batch
 * afterwards; ws as for pc_joint_fused_step at `batch`.  exp_avg / exp_avg_sq are required. */
int pc_joint_train_epoch(const pc_joint_tensors *p, const pc_joint_tensors *g, const pc_joint_tensors *exp_avg,
                         const pc_joint_tensors *exp_avg_sq, int64_t *step_count, double lr, double beta1,
                         double beta2, double eps, const int32_t *pairs, int64_t n_pairs, const float *features,
                         const int32_t *type_idx, int n_types, uint64_t seed, uint64_t first_step,
                         int32_t *query_idx, int32_t *query_types, int32_t *pos_types, int32_t *neg_types,
                         float *pos_items, float *neg_items, int batch, int drop_last, int num_types, int k,
                         int num_products, float margin, float alpha, float *losses_out, int32_t *topk,
                         int32_t *bad_count, void *ws, size_t ws_bytes, void *stream);

/* --- ABI 8: the optimizer step inside the Product2Vec step's last gradient launch.
 * product2vec.py:156-158 is optimizer.zero_grad(); loss.backward(); optimizer.step(): the step functions above are the first two,
 * pc_adam_step[_at] the third -- one more launch over 0.8 MB behind a step whose last kernel (the slab reduce of the weight
 * gradients) has every gradient in hand.  With `adam` the reduce applies torch.optim.Adam's update to each parameter right
 * behind its gradient (and rider workgroups to the parameters whose gradients other kernels finished): the same expressions as
 * pc_adam_step_at(t), the same bits, one launch fewer.  adam->grad must be the flat buffer `g`'s tensors are views of,
 * param / exp_avg / exp_avg_sq the buffers with the same offsets (n floats, n % 4 == 0, 16-byte aligned); t >= 1 the step number
 * (the host's count: *step_count is set to t).  adam == NULL: pc_p2v_train_step_unique.  phase must be -1 (the unsplit step: a
 * replica that exchanges gradients or BatchNorm sums between the phases keeps its optimizer step apart). */
typedef struct pc_adam_fused {
    float *param, *grad, *exp_avg, *exp_avg_sq;
    size_t n;
    int64_t *step_count;
    int64_t t;
    double lr, beta1, beta2, eps;
} pc_adam_fused;
int pc_p2v_train_step_unique_adam(const pc_p2v_tensors *p, const pc_p2v_tensors *g, const float *table,
                                  const int32_t *anchor_idx, const int32_t *positive_idx,
                                  const int32_t *negative_idx, const int32_t *nb_rows, const float *nb_weight,
                                  int n_unique, const int32_t *slot_row, const int32_t *ref_off,
                                  const int32_t *ref_slot, int batch, int n_nbr, int k_neg, float margin,
                                  float *loss, float *d_pos, float *d_neg, float *anchor_emb, void *profile,
                                  void *ws, size_t ws_bytes, const pc_adam_fused *adam, void *stream);

/* The same step without a launch of its own in front of Linear0 (product2vec.py:73, the first nn.Linear of self.ffn).  The step
 * functions above begin by concatenating the four index arrays of product2vec.py:132-134 into the row list the segmented FFN
 * runs over; a loader that builds its batches on another stream (DeviceSimilarityLoader) does that there instead:
 * pc_p2v_concat_step_rows, queued behind pc_build_similarity_batch_unique, writes rows_out = [anchor_idx[B] | nb_rows[0 .. n_unique]
 * (n_unique read from the DEVICE: n_unique_dev, clamped to nb_capacity - 1) | positive_idx[B] | negative_idx[B*K]];
 * rows_capacity >= B * (2 + K) + nb_capacity entries.  pc_p2v_train_step_unique_rows then takes step_rows = rows_out in
 * place of the three index arrays (n_unique: the host's copy of the same count); the transposed weights of the step ride in
 * the FFN forward's BatchNorm finalize launch.  Same results, bit for bit, as pc_p2v_train_step_unique_adam. */
int pc_p2v_concat_step_rows(const int32_t *anchor_idx, const int32_t *positive_idx, const int32_t *negative_idx,
                            const int32_t *nb_rows, const int32_t *n_unique_dev, int nb_capacity, int batch, int k_neg,
                            int32_t *rows_out, int rows_capacity, void *stream);
int pc_p2v_train_step_unique_rows(const pc_p2v_tensors *p, const pc_p2v_tensors *g, const float *table,
                                  const int32_t *step_rows, const int32_t *nb_rows, const float *nb_weight, int n_unique,
                                  const int32_t *slot_row, const int32_t *ref_off, const int32_t *ref_slot, int batch,
                                  int n_nbr, int k_neg, float margin, float *loss, float *d_pos, float *d_neg,
                                  float *anchor_emb, void *profile, void *ws, size_t ws_bytes, const pc_adam_fused *adam,
                                  void *stream);

/* The fused step with the key-padding mask (a labelled deviation, see pc_p2v_attention_forward_masked; the entries above stay
 * the parity default).  A padding slot is a slot that slot_row maps to the shared padding row (the last of nb_rows).
 *   attention: padding slots are no keys; a sample without a real slot gets out_proj_b and sends no gradient to keys or in_proj.
 *   BatchNorm of the neighbour call: statistics, running-statistics update and backward sums span the real slots only.  The
 *     padding row weighs 0 (nb_weight's last entry is NOT read and the array is not written: one batch serves both modes) and
 *     adds nothing to any weight or bias gradient.
 *   one real slot in the batch: PC_EBATCHNORM, as one row.  None (a batch of padding alone): the neighbour call did not
 *     happen -- three BatchNorm calls update the running statistics and num_batches_tracked, nothing is divided by zero.
 * _compact_masked: pc_p2v_train_step_compact's arguments (n_real real slots, one row each).
 * _unique_masked: the unique layout plus n_real_slots = the number of real slots (the sum of nb_weight[0 .. n_unique), which the
 *   host knows: the loader's n_real); step_rows optional (NULL, or pc_p2v_concat_step_rows' list, which then replaces the three
 *   index arrays as in pc_p2v_train_step_unique_rows); adam optional (NULL, or the optimizer riding in the last launch as in
 *   pc_p2v_train_step_unique_adam).  Unsplit step only: cross-replica masked statistics are not built. */
int pc_p2v_train_step_compact_masked(const pc_p2v_tensors *p, const pc_p2v_tensors *g, const float *table,
                                     const int32_t *anchor_idx, const int32_t *positive_idx,
                                     const int32_t *negative_idx, const int32_t *nb_rows, int n_real,
                                     const int32_t *slot_row, int batch, int n_nbr, int k_neg, float margin,
                                     float *loss, float *d_pos, float *d_neg, float *anchor_emb, void *profile,
                                     void *ws, size_t ws_bytes, void *stream);
int pc_p2v_train_step_unique_masked(const pc_p2v_tensors *p, const pc_p2v_tensors *g, const float *table,
                                    const int32_t *anchor_idx, const int32_t *positive_idx,
                                    const int32_t *negative_idx, const int32_t *step_rows, const int32_t *nb_rows,
                                    const float *nb_weight, int n_unique, int n_real_slots, const int32_t *slot_row,
                                    const int32_t *ref_off, const int32_t *ref_slot, int batch, int n_nbr, int k_neg,
                                    float margin, float *loss, float *d_pos, float *d_neg, float *anchor_emb,
                                    void *profile, void *ws, size_t ws_bytes, const pc_adam_fused *adam, void *stream);

/* ---------------------------------------------------------------------------------
 * Data-parallel replicas (the reference is single-process: train.py:46-48 is loss.backward(); optimizer.step()
 * with nothing between -- a replica of a data-parallel job averages the gradients there).  ABI 6.
 *
 * pc_exchange_fn: called between a step's last gradient kernel and its Adam launch, ON THE STEP'S STREAM: it must leave in
 * grad[0 .. n) the mean over the replicas of what it found there, ordered on `stream` like a kernel (enqueue only; a host
 * implementation may block).  Returns 0, or an error code the step's call then returns.  Every replica must make the same
 * sequence of calls (same n): the entry points below call it exactly once per step.
 * pc_rccl_allreduce_mean is the native implementation: ncclAllReduce(ncclAvg) of RCCL over xGMI on the library's own
 * communicator, enqueued on `stream` -- no host round trip, no host-language call per step.
 * --------------------------------------------------------------------------------- */
typedef int (*pc_exchange_fn)(void *ctx, float *grad, size_t n, void *stream);

/* exchange(ctx, grad, n, stream) -- skipped when exchange is NULL -- then torch.optim.Adam's update over the flat
 * buffers as pc_adam_step_at(t) when the caller knows the step number (t >= 1), as pc_adam_step (device counter;
 * `scalars` required) when t == 0: loss.backward() is behind, optimizer.step() of a replica as ONE call
 * (scripts/pretrain_product2vec.py:34 + product2vec.py:157-158; train.py:47-48). */
int pc_exchange_adam(pc_exchange_fn exchange, void *exchange_ctx, float *param, float *grad, float *exp_avg,
                     float *exp_avg_sq, size_t n, int64_t *step_count, int64_t t, float *scalars, double lr,
                     double beta1, double beta2, double eps, void *stream);

/* --- ABI 8: the optimizer state sharded over the replicas ("ZeRO-1"; north_star: "reduce-scatter for the sparse grads").
 * The reference's optimizer is torch.optim.Adam over EVERY parameter of one process (train.py:24,46-48): dense moments and a
 * dense update for the two [num_types,64] tables (src/models/p_companion.py:36-43) whichever rows a batch touched.  G replicas
 * that all-reduce the flat gradient each repeat that whole update (7 passes over 17.8 MB per step at num_types = 34800).
 * Sharded: buf = world slices of n / world floats;
 *   reduce_scatter_mean(ctx, grad, n / world, stream)   leaves in slice `rank` of grad the mean over the ranks of that slice
 *                                                       (the other slices: unspecified), ordered on `stream`;
 *   Adam (pc_adam_step / pc_adam_step_at) over slice `rank` of param / grad / exp_avg / exp_avg_sq only;
 *   all_gather(ctx, param, n / world, stream)           every rank's slice `rank` of param -> all ranks, in place.
 * The same bytes on the wire as the all-reduce (which is these two phases back to back), 1 / world of the update's traffic and
 * of the moments' state that matters (this library keeps the moment buffers whole; only slice `rank` is ever read or written).
 * Adam is elementwise, so the parameters after a step are those of the all-reduce form whenever the two reductions sum in
 * the same order (always for world = 2; a ring all-reduce is this reduce-scatter + all-gather).
 * plan->shard_optimizer == 0 (or world == 1 with reduce_scatter_mean == NULL): the plain form -- all_reduce_mean (may be NULL:
 * no exchange) then Adam over all n.  n must be a multiple of world when sharded (the host pads the flat buffers), else PC_EINVAL.
 * SLICE ALIGNMENT: the Adam kernels move 16-byte chunks, so every slice must start on a 16-byte boundary: (n / world) % 4 != 0 is
 * PC_ESHAPE -- on EVERY rank (rank 0's slice starts aligned whatever n is) and BEFORE the reduce-scatter is issued, so that no
 * rank is left waiting in a collective its peers never enter.  The host pads the flat buffers to a multiple of 4 * world floats.
 * The moments of the other slices are neither read nor written: a checkpoint of the whole optimizer state needs an all-gather of
 * exp_avg / exp_avg_sq over the same slices first (the all_gather member serves it).
 * pc_rccl_reduce_scatter_mean / pc_rccl_all_gather are the native members: ncclReduceScatter(ncclAvg) / ncclAllGather in place
 * on the library's communicator, chained like its other collectives. */
typedef int (*pc_shard_collective_fn)(void *ctx, float *buf, size_t n_per_rank, void *stream);
typedef struct pc_exchange_plan {
    pc_exchange_fn all_reduce_mean;            /* the plain form's exchange (NULL: none) */
    pc_shard_collective_fn reduce_scatter_mean;
    pc_shard_collective_fn all_gather;
    void *ctx;                                 /* handed to all three */
    int rank, world;
    int shard_optimizer;                       /* 1: reduce-scatter -> Adam on slice `rank` -> all-gather */
} pc_exchange_plan;
int pc_rccl_reduce_scatter_mean(void *comm, float *buf, size_t n_per_rank, void *stream);
int pc_rccl_all_gather(void *comm, float *buf, size_t n_per_rank, void *stream);
/* pc_exchange_adam with a plan (plan == NULL: no exchange, Adam over all n). */
int pc_exchange_adam_plan(const pc_exchange_plan *plan, float *param, float *grad, float *exp_avg, float *exp_avg_sq,
                          size_t n, int64_t *step_count, int64_t t, float *scalars, double lr, double beta1, double beta2,
                          double eps, void *stream);

/* pc_joint_train_epoch for a replica: every step is the fused step WITHOUT its Adam (gradients only), the exchange, then
 * Adam over the flat buffers -- train.py:36-57 with the replicas' mean gradient, all steps of the epoch enqueued by this one
 * call.  p / g must be views INTO param_flat / grad_flat (the [num_types,64] tables included: at num_types > 512 their dense
 * gradients hold zeros outside the touched rows, so the flat mean is the mean of the dense gradients the reference's autograd
 * would form).  t_first: the Adam step number of the epoch's first step (>= 1), or 0 = read the device counter
 * (adam_scalars: device float[2], required then).  Every replica must run the same number of steps (same n_pairs, batch,
 * drop_last): the exchange is a collective.  exchange == NULL: a single process (no exchange; same bits as
 * pc_joint_train_epoch, tested). */
int pc_joint_train_epoch_dp(const pc_joint_tensors *p, const pc_joint_tensors *g, float *param_flat, float *grad_flat,
                            float *exp_avg_flat, float *exp_avg_sq_flat, size_t n_flat, int64_t *step_count,
                            int64_t t_first, float *adam_scalars, double lr, double beta1, double beta2, double eps,
                            pc_exchange_fn exchange, void *exchange_ctx, const int32_t *pairs, int64_t n_pairs,
                            const float *features, const int32_t *type_idx, int n_types, uint64_t seed,
                            uint64_t first_step, int32_t *query_idx, int32_t *query_types, int32_t *pos_types,
                            int32_t *neg_types, float *pos_items, float *neg_items, int batch, int drop_last,
                            int num_types, int k, int num_products, float margin, float alpha, float *losses_out,
                            int32_t *topk, int32_t *bad_count, void *ws, size_t ws_bytes, void *stream);

/* pc_joint_train_epoch_dp with a plan in place of (exchange, exchange_ctx): per step the fused step without its Adam, then
 * pc_exchange_adam_plan -- at num_types > 512 p_companion_amd passes shard_optimizer = 1.  The sharded form's conditions on
 * n_flat (a multiple of world: PC_EINVAL; slices of a multiple of 4 floats: PC_ESHAPE) are checked at entry, before the first
 * step's first launch. */
int pc_joint_train_epoch_plan(const pc_joint_tensors *p, const pc_joint_tensors *g, float *param_flat, float *grad_flat,
                              float *exp_avg_flat, float *exp_avg_sq_flat, size_t n_flat, int64_t *step_count,
                              int64_t t_first, float *adam_scalars, double lr, double beta1, double beta2, double eps,
                              const pc_exchange_plan *plan, const int32_t *pairs, int64_t n_pairs,
                              const float *features, const int32_t *type_idx, int n_types, uint64_t seed,
                              uint64_t first_step, int32_t *query_idx, int32_t *query_types, int32_t *pos_types,
                              int32_t *neg_types, float *pos_items, float *neg_items, int batch, int drop_last,
                              int num_types, int k, int num_products, float margin, float alpha, float *losses_out,
                              int32_t *topk, int32_t *bad_count, void *ws, size_t ws_bytes, void *stream);

/* The library's own RCCL communicator (librccl.so.1 is resolved at run time with dlopen -- the copy the process has
 * loaded already, e.g. torch's, else the system's; the library has no link-time dependency on it).
 *   pc_rccl_available()          1 if the RCCL entry points could be resolved, else 0
 *   pc_rccl_unique_id(out)       ncclGetUniqueId into 128 HOST bytes (one rank calls it and hands the bytes to the others
 *                                by whatever channel the job has: torch.distributed.broadcast in p_companion_amd/distributed.py)
 *   pc_rccl_comm_create(...)     ncclCommInitRank on the calling thread's current HIP device: a collective over the
 *                                `world` ranks; *comm_out is the handle (the `ctx` of pc_rccl_allreduce_mean)
 *   pc_rccl_comm_destroy(comm)   ncclCommDestroy (streams drained by the caller)
 *   pc_rccl_allreduce_mean       a pc_exchange_fn: in-place ncclAllReduce(ncclFloat32, ncclAvg) of grad[0 .. n) on `stream`;
 *                                every rank receives the same bits
 *   pc_rccl_allreduce_sum_f64    in-place ncclAllReduce(ncclFloat64, ncclSum) of buf[0 .. n): the cross-replica BatchNorm sums
 *                                (ops.p2v_train_step(sync_reduce=...); replaces torch.distributed.all_reduce there)
 *   pc_rccl_alltoall             the lookup all-to-all of the row-sharded table (the reference keeps its table in one
 *                                process: src/models/p_companion.py:20-29, src/data/data_loader.py:45-55): bytes
 *                                [p * bytes_per_peer, (p + 1) * bytes_per_peer) of `send` go to rank p, which finds them in its
 *                                `recv` at [rank * bytes_per_peer, ...); one grouped ncclSend / ncclRecv per peer, constant splits
 *                                (send != recv; both device buffers of world * bytes_per_peer bytes)
 *   pc_rccl_comm_stats           {collectives issued on the communicator, cross-stream waits inserted}
 *   pc_rccl_last_error()         text of the calling thread's last PC_ECOMM (static storage; "" if none)
 * ORDER.  Every collective of a step goes through this ONE communicator, and the communicator chains them: a collective
 * enqueued on a stream other than its predecessor's first makes that stream wait for the predecessor.  Until the first change
 * of stream nothing is recorded (collectives that follow each other on one stream are ordered by it: the joint step, a
 * replicated table); at the first change the event is recorded at the tail of the predecessor's stream; from then on every
 * collective records the event right behind itself on its own stream, so a later change of stream waits for the collective
 * alone, not for whatever was enqueued behind it (the loader's look-ahead all-to-all is not serialised behind the step's
 * kernels).  Streams handed to the communicator must outlive it.
 * The replicas issue the same sequence of calls, so the device-side order of the collectives is the same on every rank
 * whichever streams carry them (the loader's side stream: pc_rccl_alltoall a few batches ahead; the step's stream:
 * pc_rccl_allreduce_mean) -- two collectives of one job never race for the links in different orders on different ranks.
 * One host thread at a time per communicator (calls are serialised by a mutex inside).
 * Returns PC_OK, PC_EINVAL, or PC_ECOMM. */
int pc_rccl_available(void);
int pc_rccl_unique_id(void *out_128_bytes);
int pc_rccl_comm_create(const void *unique_id_128_bytes, int rank, int world, void **comm_out);
int pc_rccl_comm_destroy(void *comm);
int pc_rccl_allreduce_mean(void *comm, float *grad, size_t n, void *stream);
int pc_rccl_allreduce_sum_f64(void *comm, double *buf, size_t n, void *stream);
int pc_rccl_alltoall(void *comm, const void *send, void *recv, size_t bytes_per_peer, void *stream);
int pc_rccl_comm_stats(void *comm, int64_t *issued, int64_t *chained);
const char *pc_rccl_last_error(void);

/* ---------------------------------------------------------------------------------
 * Building blocks the Python modules compose their autograd from (module / dense mode).
 * --------------------------------------------------------------------------------- */
/* nn.Linear forward (type_transition.py:11-12, item_prediction.py:11-20, and the
 * similarity product p_companion.py:60-63 with b = NULL):
 *   y[r] = act(W x_r + b), x_r = idx ? x[idx[r]] (zero row if idx[r] < 0) : x[r]
 * w[out_dim,in_dim]; act 0 none, 1 tanh, 2 relu; in_dim % 4 == 0. */
int pc_linear_forward(const float *x, const int32_t *idx, int rows, int in_dim, const float *w,
                      const float *b, int out_dim, int act, float *y, void *stream);
/* dx[rows,in_dim] = dy[rows,out_dim] W.  wt_scratch: in_dim*out_dim floats (holds W^T).
 * act must be 0 (callers fold act' into dy); y_saved unused. */
int pc_linear_backward_input(const float *dy, int rows, int out_dim, const float *w, int in_dim,
                             int act, const float *y_saved, float *dx, float *wt_scratch,
                             void *stream);
/* dW[out,in] (+)= dy^T x, db[out] (+)= sum_r dy[r] (db may be NULL); x rows gathered by idx
 * when non-NULL.  Fixed-order split-K reduction: bitwise reproducible. out_dim, in_dim % 4 == 0. */
size_t pc_linear_backward_weight_workspace_bytes(int rows, int out_dim, int in_dim);
int pc_linear_backward_weight(const float *dy, int rows, int out_dim, const float *x,
                              const int32_t *idx, int in_dim, float *dw, float *db,
                              int accumulate, void *ws, size_t ws_bytes, void *stream);
/* torch.topk(sims, k, dim=1) (p_companion.py:64; metrics.py:21): idx_out[B,k] int32,
 * val_out[B,k] (may be NULL); descending, ties -> lower index first; k <= 8. */
int pc_topk_rows(const float *sims, int batch, int num_types, int k, int32_t *idx_out,
                 float *val_out, void *stream);
/* Metrics.evaluate_model pieces (src/utils/metrics.py:62-117).
 * pc_hit_rank: rank[r] = number of entries of sims[r,:] that beat the ground-truth column
 *   gt = r (ties towards the lower index); hit@k <=> rank[r] < k.  Rows r >= cols can never
 *   hit (rank = INT_MAX): the reference compares arange(B*K) with B columns (metrics.py:95-100).
 * pc_cosine_rows: out[b*K+k] = cosine_similarity(x[b,k,:], y[b,:]) with torch's eps 1e-8
 *   (metrics.py:44-60).  D = 128. */
int pc_hit_rank(const float *sims, int rows, int cols, int32_t *rank, void *stream);
int pc_cosine_rows(const float *x, const float *y, int batch, int k, float *out, void *stream);
int pc_cosine_rows_dim(const float *x, const float *y, int batch, int k, int dim, float *out, void *stream);

/* --- ABI 8, additive: Metrics.evaluate_model without the [B*K, B] score matrix, and as one call per evaluation.
 * pc_eval_batch_stats (metrics.py:88-109 for tensors the caller holds): proj [B,K,dim], targets [B,dim], pos_items [B,dim],
 *   types [B,K] int32 (any integers), dim 128 or 256, k <= 8.  stats[5] (device int32) = {hits_1, hits_3, hits_10,
 *   distinct_columns, rows = B}: for the eligible rows r in [0, B) of the flat [B*K, dim] projection (the reference compares
 *   arange(B*K) with B columns, metrics.py:95-100: rows r >= B never hit), beat_r = #{c in [0,B): s_rc > g_r or (s_rc == g_r
 *   and c < r)}, s_rc = proj_r . targets_c, g_r = s_rr (the same bits: a row never counts itself), and
 *   hits_k = #{r: beat_r < min(k, B)} for k = 1, 3, min(10, B) (metrics.py:7-27, :103); the products are exact-fp32 matrix
 *   instructions (v_mfma_f32_16x16x4_f32), nothing of size B x B is written.  distinct_columns = number of distinct columns of
 *   `types` (metrics.py:29-42).  *cos_sum (device float) = sum over (b,k) of cosine_similarity(proj[b,k], pos_items[b]) with
 *   torch's eps 1e-8 (metrics.py:44-60), in a fixed order.  No float atomics: bitwise repeatable.
 *   ws: pc_joint_eval_workspace_bytes(batch, 1, k, dim) bytes.  PC_EINVAL: null pointer / non-positive size; PC_ESHAPE: dim, k;
 *   PC_EWORKSPACE.
 * pc_joint_eval_epoch (metrics.py:62-117 over a device-resident split): `n_pairs` labelled pairs[i] = (query, target, label)
 *   in loader order -- full batches of `batch`, then the ragged rest -- each batch as pc_build_complementary_batch[_dim](pairs,
 *   ..., seed, first_step + i) would build it (positive_items = features[target] for label +1, else the filler row: the same
 *   bits; data_loader.py:133-157) and PCompanion.forward in eval mode would project it (p_companion.py:45-77; the top-K of a
 *   sample is a function of its query type alone, so it is formed once per TYPE, not per sample).  Per batch i:
 *   stats_out[5*i ..] and cos_sum_out[i] as above (device, one entry per batch); metrics_out (device double[5]) = {hit@1, hit@3,
 *   hit@10, type_diversity, mean_relevance}: per batch hits_k / (B_i*k) and cos_sum / (B_i*k) in fp32, distinct / k, then the
 *   mean over the batches in fp64, in batch order (metrics.py:101-117 adds Python floats).  Nothing is read back and the host
 *   does not synchronise inside the call.  `features` [num_products, dim], `type_idx` [num_products]; p->product_table
 *   [num_products, dim]; n_types: the dataset's modulus, as in the builder (> 0).  Ids outside their tables (query / target vs
 *   num_products, the query's type vs num_types) are clamped, counted into *bad_count (may be NULL), never dereferenced.
 *   n_types is part of the loader's source tuple (features, type_idx, n_types, seed) and is only range-checked here: the
 *   evaluation reads no negative type, the one thing the builder uses it for.
 *   For tests and probes ONLY (not a promise to other callers; the rest of the workspace's layout is private): after the
 *   call the first num_types * k int32 of ws hold the plan's complementary types [num_types, k].
 *   PC_EINVAL: null pointer / non-positive size; PC_ESHAPE: dim not 128 / 256, k (1..8, <= num_types), a ragged rest -- or a
 *   batch -- of 1..9 pairs (metrics.py:103's key min(10, cols) is then not 'hit@10': the caller's loop reproduces what the
 *   reference does there); PC_EWORKSPACE: ws_bytes < pc_joint_eval_workspace_bytes(batch, num_types, k, dim), which is linear
 *   in num_types (the plan runs over row chunks of types).  All checked before anything is launched. */
int pc_eval_batch_stats(const float *proj, const float *targets, const float *pos_items, const int32_t *types, int batch,
                        int k, int dim, int32_t *stats, float *cos_sum, void *ws, size_t ws_bytes, void *stream);
size_t pc_joint_eval_workspace_bytes(int batch, int num_types, int k, int dim);
int pc_joint_eval_epoch(const pc_joint_tensors *p, const int32_t *pairs, int64_t n_pairs, const float *features,
                        const int32_t *type_idx, int n_types, int dim, uint64_t seed, uint64_t first_step, int batch,
                        int num_types, int k, int num_products, int32_t *stats_out, float *cos_sum_out, double *metrics_out,
                        int32_t *bad_count, void *ws, size_t ws_bytes, void *stream);

/* item_prediction.py:38: proj[b,k,:] = pi[b,:] * tp[b*K+k,:] and its backward
 * (dpi[b] = sum_k dproj[b,k]*tp[b,k]; dtp[b,k] = dproj[b,k]*pi[b]).  D = 128. */
int pc_hadamard_forward(const float *pi, const float *tp, int batch, int k, float *proj,
                        void *stream);
int pc_hadamard_forward_dim(const float *pi, const float *tp, int batch, int k, int dim, float *proj, void *stream);   /* PRODUCT_EMB_DIM 128 or 256 (item_prediction.py:11-20 takes it from config) */
int pc_hadamard_backward(const float *dproj, const float *pi, const float *tp, int batch, int k,
                         float *dpi, float *dtp, void *stream);
int pc_hadamard_backward_dim(const float *dproj, const float *pi, const float *tp, int batch, int k, int dim,
                             float *dpi, float *dtp, void *stream);

/* ---------------------------------------------------------------------------------
 * Row movers used by the sharded-table exchange and the modules.
 * --------------------------------------------------------------------------------- */
/* out[r] = idx[r] >= 0 ? table[idx[r]] : 0   (nn.Embedding lookup p_companion.py:51,54,65;
 * feature gather of data_loader.py:50-55 in index form).  width % 4 == 0. */
int pc_gather_rows(const float *table, const int32_t *idx, int rows, int width, float *out,
                   void *stream);
/* table[idx[r]] += src[r] (row-sparse embedding gradient, J7), deterministic per row order
 * is NOT guaranteed (float atomics); idx < 0 skipped. */
int pc_scatter_add_rows(float *table, const int32_t *idx, int rows, int width, const float *src,
                        void *stream);
/* Same for a SMALL destination table (table_rows*width*4 <= 64 KB, e.g. the [T,64] type tables
 * at T ~ 100): source rows are first summed into a per-workgroup LDS copy of the table. Falls
 * back to pc_scatter_add_rows for larger tables. */
int pc_scatter_add_rows_small(float *table, int table_rows, const int32_t *idx, int rows, int width,
                              const float *src, void *stream);

/* out[idx[r]] = src[r] (row assignment, idx < 0 skipped): writes the attention-updated rows
 * back into the embedding table in the batched generate_all_embeddings pass
 * (product2vec.py:108-109). width % 4 == 0. */
int pc_scatter_rows(float *out, const int32_t *idx, int rows, int width, const float *src,
                    void *stream);
/* dx = dy * act'(y) for a stand-alone activation: act 1 = tanh (1 - y^2), 2 = relu (y > 0)
 * (F.relu of type_transition.py:17 in module mode). */
int pc_act_backward(const float *dy, const float *y, size_t n, int act, float *dx, void *stream);

/* Zipf(s = 1) negative sampling (BASELINE configs[4]; an extension: the reference draws its negatives uniformly,
 * data_loader.py:34).  Replaces negative_idx[batch,k_neg] of an already built batch: candidate = perm[rank - 1]
 * (perm NULL: product id = rank - 1) with P(rank) ~ 1 / rank over ranks 1..n_products, under the reference's rejection
 * rules (data_loader.py:33-38: not the anchor, not one of its positives, no repeats).  Integer-only: an octave
 * [2^j, 2^(j+1)) is chosen by the first j with draw <= octave_cum[j] (n_octaves = floor(log2(n_products)) + 1 cumulative
 * 32-bit thresholds of the octaves' probability masses, last = 0xFFFFFFFF), a rank in it uniformly (j bits), accepted
 * with probability 2^j / rank.  Philox4x32-10 keyed by (seed ^ "ZIPF"; sample, step). */
int pc_sample_negatives_zipf(const int32_t *pair_ids, int batch, const int32_t *sim_pairs,
                             const int32_t *sim_rowptr, const int32_t *sim_col, int n_products, int k_neg,
                             uint64_t seed, uint64_t step, const uint32_t *octave_cum, int n_octaves,
                             const int32_t *perm, int32_t *negative_idx, int32_t *failed, void *stream);
/* (`failed`, optional device int32: += 1 for every sample that ran out of its 4096 proposals -- an anchor whose positives
 * cover the head of the popularity order, or one with fewer than k_neg eligible products; such a sample's remaining
 * negatives are the first eligible products in rank order, -1 when none is left.  Every wave terminates.) */

/* ---- The synthetic catalogue generated ON THE DEVICE (csrc/generator.hip): SyntheticDataGenerator
 * (src/data/synthetic_data.py:11-153) restated per source node like data.generate_scaled_bpg, but as kernels that write
 * straight into HBM -- BASELINE configs[3]/[4] (10 M / 100 M products) cannot exist as host numpy arrays.  Every array is a
 * pure function of (seed, product id) through Philox4x32-10, so a rank generates exactly its rows of the feature table
 * (rows first, first + stride, ...: the cyclic shard r % world of SURVEY 8e) and the replicated graph arrays are identical
 * on every rank.  Distributions: type uniform (synthetic_data.py:35-46); features N(0,1)^dim + 1.0 on the category's 20-dim
 * block (:50-52); co-view out-degree Poisson(2 mean (1 - u)) capped, targets uniform, different-category targets kept with
 * probability 2/3 (:107-108), distinct per row; similarity = co-view & purchase-after-view (0.2) & not co-purchase (0.075
 * same category / 0.15) (:110-121); complementary = Poisson(comp_mean) targets, same-category kept 0.5, not co-viewed
 * (:122-127).  Call order: pc_gen_degrees -> pc_exclusive_scan_i32 (cv_rowptr) -> pc_gen_coview -> scan (sim_rowptr) ->
 * pc_gen_similarity; pc_gen_complementary(count) -> scan -> pc_gen_complementary(pairs). */
int pc_gen_types(int64_t n_products, int num_types, uint64_t seed, int32_t *type_idx, void *stream);
/* features[k][0:dim] = the feature row of product first + k * stride, k < n_local; dim >= 100, dim % 4 == 0 */
int pc_gen_features(int64_t first, int64_t stride, int64_t n_local, int dim, int num_types, uint64_t seed,
                    float *features, void *stream);
/* deg[P]: co-view out-degrees; comp_cand[P] (optional): complementary candidates per product.  degree_cap <= 64 */
int pc_gen_degrees(int64_t n_products, double mean_degree, int degree_cap, double comp_mean, uint64_t seed,
                   int32_t *deg, int32_t *comp_cand, void *stream);
size_t pc_scan_scratch_bytes(int64_t n);
/* out[i] = sum_{j<i} in[j] for i = 0..n (out has n + 1 entries); total_out (optional): device int64 = out[n] unrounded
 * (check it against 2^31 on the host: the offsets are int32) */
int pc_exclusive_scan_i32(const int32_t *in, int64_t n, int32_t *out, int64_t *total_out, void *scratch,
                          size_t scratch_bytes, void *stream);
/* cv_col[cv_rowptr[i] + j] = j-th co-view target of product i, bit 31 = "this edge is a similarity pair" (cleared by
 * pc_gen_similarity); sim_count[i] = number of such edges */
int pc_gen_coview(int64_t n_products, int num_types, uint64_t seed, const int32_t *cv_rowptr, int32_t *cv_col,
                  int32_t *sim_count, void *stream);
/* sim_pairs[S][2] in source order, sim_col[S] (= the positives' CSR with sim_rowptr), pair_deg[S] (optional): co-view
 * degree of each pair's anchor (what the loader pads to, data_loader.py:186-198) */
int pc_gen_similarity(int64_t n_products, const int32_t *cv_rowptr, int32_t *cv_col, const int32_t *sim_rowptr,
                      int32_t *sim_pairs, int32_t *sim_col, int32_t *pair_deg, void *stream);
/* count != NULL: count[i] = complementary pairs of product i; comp_pairs != NULL: pairs written at comp_rowptr[i] */
int pc_gen_complementary(int64_t n_products, int num_types, uint64_t seed, const int32_t *comp_cand,
                         const int32_t *cv_rowptr, const int32_t *cv_col, int32_t *count,
                         const int32_t *comp_rowptr, int32_t *comp_pairs, void *stream);

/* ---- The catalogue INGESTED on the device (csrc/ingest.hip, ABI 8, additive): the same arrays from the three edge sets of a
 * BehaviorProductGraph (src/data/bpg.py:4-22: co_view, purchase_after_view, co_purchase) given as unsorted, directed int32
 * [E][2] lists of (source, target) with duplicates, E < 2^31, ids in [0, n_products).  Semantics (DESIGN.md "Ingestion"):
 * self-loops dropped, duplicates collapsed, a co_view edge's number of occurrences is its weight; a co_view row keeps its
 * degree_cap distinct targets of greatest weight (equal weights: the lower id), ascending; similarity = kept co-view & PAV -
 * co-purchase; complementary = co-purchase - PAV - the FULL co-view set; both sorted by (s, t).  No global sort: per list,
 * pc_ingest_count -> pc_exclusive_scan_i32 (raw row offsets) -> pc_ingest_scatter (buckets) -> pc_ingest_rows (each row
 * sorted, run-length coded and capped in its bucket); then pc_ingest_emit (cv_col) and pc_ingest_flag -> scan ->
 * pc_ingest_emit per pair array.  Integer atomics only; every output is a function of the lists as sets (co_view: as a
 * multiset), bit-identical under any permutation of the input.  ops.build_catalogue is the call order. */
/* cnt[s] += 1 (cnt zeroed by the caller) for every edge (s, t), s != t, of one list.  Every id is compared with [0, n_products)
 * BEFORE it indexes anything: an edge with an id outside is skipped (by pc_ingest_scatter too) and ORs list_bit (> 0) into
 * the device word *bad, which the caller reads once.  n_edges = 0: nothing is launched. */
int pc_ingest_count(const int32_t *edges, int64_t n_edges, int64_t n_products, int list_bit, int32_t *cnt, int32_t *bad,
                    void *stream);
/* bucket[rowptr[s] + j] = the targets of s in arbitrary order, through the integer cursor cursor[s]: the counts of
 * pc_ingest_count on entry, zero on exit (rowptr = their exclusive scan) */
int pc_ingest_scatter(const int32_t *edges, int64_t n_edges, int64_t n_products, const int32_t *rowptr, int32_t *cursor,
                      int32_t *bucket, void *stream);
/* the raw row lengths at which pc_ingest_rows changes path: up to *wave_row_max one wave per row (bitonic network in
 * registers), up to *lds_row_max one workgroup per row sorting in LDS, above it one workgroup per row sorting between the
 * bucket and the scratch buffer (LSD radix, 8-bit digits); no length is refused */
int pc_ingest_row_limits(int *wave_row_max, int *lds_row_max);
size_t pc_ingest_rows_workspace_bytes(int64_t n_products);
/* Every row of the bucket array in place: the row's D distinct ids ascending in bucket[rowptr[s], rowptr[s] + D),
 * full_cnt[s] = D.  degree_cap in 1..64: bit 31 marks the kept ids, kept_cnt[s] = min(D, degree_cap), *max_kept (zeroed by
 * the caller) = the largest of them.  degree_cap = 0: a plain set, no bits, kept_cnt / max_kept unused (may be NULL).
 * scratch: as many int32 as the bucket array (touched only under rows longer than *lds_row_max). */
int pc_ingest_rows(int64_t n_products, const int32_t *rowptr, int32_t *bucket, int32_t *scratch, int degree_cap,
                   int32_t *full_cnt, int32_t *kept_cnt, int32_t *max_kept, void *ws, size_t ws_bytes, void *stream);
/* Set algebra over sorted rows.  A set is (buf, rowptr, cnt): row s = buf[rowptr[s], rowptr[s] + cnt[s]) (cnt NULL: up to
 * rowptr[s + 1]), ids ascending, bit 31 ignored; buf NULL = the set is not given.  Bit 31 of every entry (s, t) of src is SET
 * when t is in need[s] (if given) and in neither forbid1[s] nor forbid2[s] (if given), cleared otherwise; count[s] = the
 * number of entries set.  src must not be one of the three sets. */
int pc_ingest_flag(int64_t n_products, int32_t *src, const int32_t *src_rowptr, const int32_t *src_cnt, const int32_t *need,
                   const int32_t *need_rowptr, const int32_t *need_cnt, const int32_t *forbid1,
                   const int32_t *forbid1_rowptr, const int32_t *forbid1_cnt, const int32_t *forbid2,
                   const int32_t *forbid2_rowptr, const int32_t *forbid2_cnt, int32_t *count, void *stream);
/* The entries of src with bit 31 set, row by row in order, to positions out_rowptr[s] onwards (out_rowptr = the scan of their
 * counts) of out_col (the id), out_pairs ((s, id), [n][2]) and out_deg (deg_rowptr[s + 1] - deg_rowptr[s]: pair_deg) -- each
 * optional, at least one given.  clear != 0: bit 31 is removed from src on the way. */
int pc_ingest_emit(int64_t n_products, int32_t *src, const int32_t *src_rowptr, const int32_t *src_cnt,
                   const int32_t *out_rowptr, int32_t *out_col, int32_t *out_pairs, int32_t *out_deg,
                   const int32_t *deg_rowptr, int clear, void *stream);

/* ---- The three edge lists above DERIVED from a shopper event log on the device (csrc/events.hip, ABI 8, additive).
 * events [N][4] int32, 16-byte aligned, rows (session, product, kind, time) in any order: session in [0, n_sessions), product in
 * [0, n_products), kind 0 = view / 1 = purchase, time >= 0; N < 2^31.  Semantics (DESIGN.md "Edge lists from shopper
 * events"): a session with more than max_events (2..1024) raw rows is skipped whole; the items of a kept session are its distinct
 * products, fv(x) = the earliest view time of item x, lp(x) = its latest purchase time (-1 = none), V(x) = fv(x) >= 0, U(x) =
 * lp(x) >= 0; per kept session and ordered pair of items a != b: co_purchase U(a) & U(b); co_view V(a) & V(b) [exclusive: and not
 * (U(a) & U(b))]; purchase_after_view V(a) & U(b) & fv(a) <= lp(b) [exclusive: and not U(a)].  Each list is written as (a, b)
 * rows ordered by (session, a, b): an edge appears once per session that shows it.  Integer atomics only; every output is a
 * function of the log as a multiset of rows.  Call order (ops.event_edges): pc_events_count -> read *bad -> pc_exclusive_scan_i32
 * (rowptr) -> pc_events_scatter -> pc_events_sessions -> read totals -> pc_exclusive_scan_i32 per list -> pc_events_emit. */
/* the largest max_events, and the number of int64 words of pc_events_sessions' totals */
int pc_events_limits(int *max_events, int *n_totals);
/* cnt[session] += 1 (cnt zeroed by the caller) for every row.  Every field is compared with its range BEFORE it indexes
 * anything: an offending row is skipped (by pc_events_scatter too) and ORs 1 (session), 2 (product), 4 (kind), 8 (time) into
 * the device word *bad, which the caller reads once.  n_events = 0: nothing is launched.  PC_ESHAPE: events not 16-byte
 * aligned. */
int pc_events_count(const int32_t *events, int64_t n_events, int64_t n_sessions, int64_t n_products, int32_t *cnt,
                    int32_t *bad, void *stream);
/* bucket[rowptr[s] + j][2] = (product, (kind ^ 1) << 31 | time) of the rows of session s in arbitrary order, through the
 * integer cursor cursor[s] (the counts of pc_events_count on entry; rowptr = their exclusive scan).  The rows of a session
 * longer than max_events are not written. */
int pc_events_scatter(const int32_t *events, int64_t n_events, int64_t n_sessions, int64_t n_products, int max_events,
                      const int32_t *rowptr, int32_t *cursor, int32_t *bucket, void *stream);
/* Every kept session in place, one wave each: its items ascending by product as (product, fv) in bucket[rowptr[s] + i][2] and
 * lp in last_purchase[rowptr[s] + i], i < n_items[s]; count_cv / count_pv / count_cp [s] = its rows of co_view,
 * purchase_after_view, co_purchase (0 for an empty or a skipped session).  totals[5] (int64, zeroed by the caller): the three
 * lists' rows over all sessions, the items, the skipped sessions -- 64-bit sums the caller checks before it scans offsets. */
int pc_events_sessions(int64_t n_sessions, const int32_t *rowptr, int32_t *bucket, int32_t *last_purchase, int max_events,
                       int exclusive, int32_t *n_items, int32_t *count_cv, int32_t *count_pv, int32_t *count_cp,
                       int64_t *totals, void *stream);
/* out_cv / out_pv / out_cp [.][2]: the (a, b) rows of every session at off_*[s] onwards (off_* [n_sessions + 1] = the exclusive
 * scans of pc_events_sessions' counts), a ascending, inside a the b ascending.  max_events and exclusive as given there. */
int pc_events_emit(int64_t n_sessions, const int32_t *rowptr, const int32_t *bucket, const int32_t *last_purchase,
                   const int32_t *n_items, int max_events, int exclusive, const int32_t *off_cv, const int32_t *off_pv,
                   const int32_t *off_cp, int32_t *out_cv, int32_t *out_pv, int32_t *out_cp, void *stream);

/* The epoch order of DataLoader(shuffle=True) (scripts/pretrain_product2vec.py:24-30, train.py:115-121) as a keyed
 * bijection: out[i] = perm_{seed,epoch}(i), i in [0, n) -- a six-round balanced Feistel network over the even number of
 * bits covering n, cycle-walked into [0, n).  No sort, no storage, deterministic in (seed, epoch); restated in
 * oracle/philox_oracle.py::epoch_permutation.  (The reference's order comes from torch's CPU generator and cannot be
 * bit-matched; parity mode replays CPython's random.shuffle on the host instead: pc_mt_shuffle.) */
int pc_epoch_permutation(int n, uint64_t seed, uint64_t epoch, int32_t *out, void *stream);
/* out[i][0:width] = rows[perm_{seed,epoch}(i)][0:width] (int32 rows, e.g. the labelled pairs [n,3] of
 * ComplementaryDataset, data_loader.py:113-126): one epoch's shuffled order in one launch.  out != rows. */
int pc_shuffle_rows_i32(const int32_t *rows, int n, int width, uint64_t seed, uint64_t epoch, int32_t *out,
                        void *stream);
/* ComplementaryDataset's shuffle and 80/10/10 split (data_loader.py:113-126) over device pair arrays (ABI 8, additive): with
 * L = [comp_pairs[j] (label +1) for j < n_comp] + [sim_pairs[j] (label -1) for j < n_sim] and n = n_comp + n_sim,
 * out[i] = (query, target, label) of L[perm(lo + i)] for i in [0, hi - lo), int32 [hi - lo][3], where perm is the bijection of
 * pc_epoch_permutation(n, seed, mode) (mode 0 / 1 / 2 = train / val / test).  Neither L nor the permutation is stored: one
 * pass writes the mode's rows only.  The caller computes lo / hi (the host split: 0.8 n, 0.9 n).  PC_EINVAL: a null pointer
 * (comp_pairs / sim_pairs may be NULL when their count is 0), n = 0, n >= 2^31, 0 <= lo <= hi <= n violated, mode outside
 * 0..2.  Integer work only, no atomics. */
int pc_comp_split_pairs(const int32_t *comp_pairs, int64_t n_comp, const int32_t *sim_pairs, int64_t n_sim, int64_t lo,
                        int64_t hi, uint64_t seed, int mode, int32_t *out, void *stream);
/* collate_fn pads every neighbour list to the batch maximum (data_loader.py:186-198), so the host needs two integers per
 * batch to size it: plan[b] = (max, sum) of deg[order[i]] over positions i in [b*batch, (b+1)*batch), i < n
 * (order NULL: the identity).  plan: device int64 [n_batches][2]. */
int pc_epoch_plan(const int32_t *order, const int32_t *deg, int n, int batch, int n_batches, int64_t *plan,
                  void *stream);

/* Row-sharded feature table, device-resident request bucketing (north_star: "embedding table row-shards across up
 * to 8 MI355X with RCCL all-to-all for cross-shard lookups"; the reference's table is one in-process dict,
 * src/data/bpg.py:4-22, data_loader.py:50-55).  Product r lives on rank r % world as local row r / world.
 * Up to `count` <= 4 id arrays ids[a][n[a]] (global product ids, < 0 = padding; only the first *n_dev[a] + n_dev_add[a]
 * entries are live when n_dev[a] != NULL -- the unique-neighbour list's length exists on the device only) become
 *   send_ids[world][capacity]   per-owner request lists (local row indices; unused slots -1), and
 *   remap_out[a][n[a]]          the same arrays as indices into the [world][capacity][D] buffer the exchange returns
 *                               (row = owner * capacity + slot; padding and non-live entries -> -1).
 * counts[world] receives the bucket sizes; *overflow is incremented for every id that did not fit its bucket (that id
 * maps to -1).  Nothing is read back to the host: shapes are constant, the two all-to-all rounds need no size exchange. */
int pc_shard_bucket(const int32_t *const *ids, const int *n, const int32_t *const *n_dev, const int *n_dev_add,
                    int32_t *const *remap_out, int count, int world, int capacity, int32_t *counts,
                    int32_t *send_ids, int32_t *overflow, void *stream);
/* The same with a REPLICATED HOT SET (ABI 8; BASELINE configs[4]: "Zipf-skewed negative sampling + hot-row cache"; the
 * reference draws negatives uniformly, src/data/data_loader.py:27-40, and keeps its table in one process): the hot_rows most
 * popular products live on EVERY rank as rows [world * capacity, world * capacity + hot_rows) of the table the step reads
 * (the caller keeps that replica behind the exchange buffer), and an id of the set maps there instead of taking a request slot.
 * hot_ids: the set as ascending product ids [hot_rows] (device; NULL = the ids [0, hot_rows): popularity rank = product id, the
 * Zipf sampler's default); hot slot = position in the set.  *hot_served (device, may be NULL) is increased by the number of
 * live entries served from the replica.  hot_rows = 0: pc_shard_bucket.  Lookups stay constant-shape. */
int pc_shard_bucket_hot(const int32_t *const *ids, const int *n, const int32_t *const *n_dev, const int *n_dev_add,
                        int32_t *const *remap_out, int count, int world, int capacity, const int32_t *hot_ids,
                        int hot_rows, int32_t *counts, int32_t *send_ids, int32_t *overflow, int32_t *hot_served,
                        void *stream);

/* nn.Dropout of ComplementaryTypeTransition (type_transition.py:13,17) in training mode on the hidden activations
 * x[n] (n % 4 == 0, rows of 32): y = x * mask, mask = stream 1 of pc_dropout (0 or 1/(1-p)).  The same call with the
 * same (seed, offset) is its backward (dx = dy * mask).  In place (y == x) allowed.  0 < p < 1. */
int pc_dropout_hidden(const float *x, size_t n, const pc_dropout *d, float *y, void *stream);

/* Index validation.  The reference's lookups raise for an id outside its table (nn.Embedding: IndexError;
 * product_to_idx: KeyError -- p_companion.py:48-54); here up to `count` <= 4 int32 index arrays idx[a][n[a]] are
 * checked against [0, hi[a]) (or [-1, hi[a]) where allow_pad[a] != 0: -1 is the collate padding sentinel) in one
 * launch, and the number of offending entries is ADDED to the device counter *bad.  The caller reads the counter
 * when it synchronises anyway (PCompanion.raise_index_errors) and raises IndexError. */
int pc_check_indices(const int32_t *const *idx, const int *n, const int *hi, const int *allow_pad, int count,
                     int32_t *bad, void *stream);

/* ---------------------------------------------------------------------------------
 * Serving: type-filtered top-n retrieval -- the candidate search of
 * PCompanionInference.recommend (inference.py:90-118): for row r (one predicted complementary
 * type of one query), scores = proj[r] . features[c] over the products c of type types[r]
 * (CSR type_rowptr[n_types+1] / type_col, products in node order = bpg.get_products_by_type),
 * torch.topk(scores, min(n, count)).  out_idx / out_score [rows, n]; missing entries (fewer than
 * n products of that type, or a type outside [0, n_types)) are -1 / -inf.  1 <= n <= 16.
 * --------------------------------------------------------------------------------- */
int pc_retrieve_topk(const float *proj, const int32_t *types, int rows, const int32_t *type_rowptr,
                     const int32_t *type_col, const float *table, int n_types, int n, int32_t *out_idx,
                     float *out_score, void *stream);
int pc_retrieve_topk_dim(const float *proj, const int32_t *types, int rows, const int32_t *type_rowptr,
                        const int32_t *type_col, const float *table, int n_types, int n, int dim, int32_t *out_idx,
                        float *out_score, void *stream);
/* The same contract over a catalogue of any size (ABI 8, additive; inference.py:90-118 for a 10 M / 100 M catalogue): the
 * rows are grouped by type on the device and each type's candidates are scored as an fp32 GEMM on v_mfma_f32_16x16x4_f32
 * (tiles of 64 rows at dim 128, 32 at dim 256), so a candidate row is read once per tile instead of once per row.  A type's
 * candidates are split over at most `slices` slices (0 = automatic, 16; at most 64; a slice takes at least 4096
 * candidates), each writing a partial top-n per row that one wave per row merges.  Same out_idx / out_score as
 * pc_retrieve_topk_dim, equal scores to the lower product index; bitwise deterministic and independent of `slices` and of
 * the order of type_col inside a type.  No host readback: the launch geometry and the workspace
 * (pc_retrieve_topk_grouped_workspace_bytes, 0 for arguments out of range) depend on rows, n_types, n and slices only.
 * PC_EINVAL: null pointer, rows or n_types <= 0; PC_ESHAPE: n outside [1, 16], dim not 128 / 256, slices outside [0, 64];
 * PC_EWORKSPACE: ws_bytes too small. */
size_t pc_retrieve_topk_grouped_workspace_bytes(int rows, int n_types, int n, int slices);
int pc_retrieve_topk_grouped(const float *proj, const int32_t *types, int rows, const int32_t *type_rowptr,
                             const int32_t *type_col, const float *table, int n_types, int n, int dim, int slices,
                             int32_t *out_idx, float *out_score, void *ws, size_t ws_bytes, void *stream);

/* The rank of a known product in the list the retrieval above orders (ABI 8, additive; PCompanionInference.rank_targets /
 * evaluate_catalogue: is the held-out complement among what is served?).  For row r with c = types[r], y = targets[r] and
 * g = <proj[r], table[y]>:
 *   rank_out[r] = #{ p in type_col[type_rowptr[c] : type_rowptr[c+1]] : s_p > g or (s_p == g and p < y) },  s_p = <proj[r], table[p]>
 * -- y need not be of type c; where it is, it does not count itself.  g and every s_p are formed through
 * pc_retrieve_topk_grouped's own fp32 MFMA chain, so rank_out[r] < n exactly when that entry's top n holds y at position
 * rank_out[r].  types[r] < 0 ("no type matched"): the row is skipped, rank_out[r] = -1.  A type >= n_types or a target outside
 * [0, num_products) never reaches memory: the row gets -1 and *bad_count (a device counter the caller owns) is incremented.
 * The same schedule as the retrieval (rows grouped by type on the device, tiles of 64 rows at dim 128 and 32 at dim 256,
 * at most `slices` candidate slices per type, 0 = automatic), the selection replaced by a compare and an integer add: no
 * score matrix, no float atomics, no host readback; bitwise deterministic and independent of `slices` and of the order of
 * type_col inside a type.  The launch geometry and the workspace (pc_rank_grouped_workspace_bytes, 0 for arguments out of
 * range) depend on rows, n_types and slices only.  PC_EINVAL: null pointer, rows, n_types or num_products <= 0; PC_ESHAPE:
 * dim not 128 / 256, slices outside [0, 64]; PC_EWORKSPACE: ws_bytes too small -- each checked before anything is launched. */
size_t pc_rank_grouped_workspace_bytes(int rows, int n_types, int slices);
int pc_rank_grouped(const float *proj, const int32_t *types, const int32_t *targets, int rows,
                    const int32_t *type_rowptr, const int32_t *type_col, const float *table,
                    int n_types, int num_products, int dim, int slices,
                    int32_t *rank_out, int32_t *bad_count, void *ws, size_t ws_bytes, void *stream);

/* The two entries above with named products kept out (ABI 8, additive; PCompanionInference.set_exclusions: a complementary
 * recommender must not serve the query itself, its co-viewed substitutes or what is in the basket, and the caller cannot strike
 * them out afterwards -- a list of at most 16 whose head is taken comes back short, and a rank counts them in front of the
 * held-out complement).  An exclusion set is a CSR over KEYS: ex_rowptr [n_keys + 1], ex_col [E], the ids of one key strictly
 * ascending (searched by bisection; ops.exclusion_csr builds one from any device CSR).  row_key[r] in [-1, n_keys) names row r's
 * list, -1 = none; a key outside that range is served as -1, never indexes memory and is counted in *bad_count (a device
 * counter the caller owns; added to).  List ids outside the table are passed over.
 *
 * pc_retrieve_topk_grouped_excluding: out_idx / out_score = the first n products of the row's type that are NOT in the row's
 * list, under pc_retrieve_topk_grouped's total order (score descending, product index ascending), -1 / -inf past the end.  The
 * same plan, merge, tiling and score chain; a candidate is looked up in the list only after it has beaten its row's running
 * threshold and is dropped before it enters a list, so it never moves the threshold.  The filter is a predicate of
 * (row, product): the same bits for every `slices`, every placement of the rows and every order of type_col.  Error codes and
 * workspace as pc_retrieve_topk_grouped (pc_retrieve_topk_grouped_excluding_workspace_bytes: the same size), PC_EINVAL also for
 * a null row_key / ex_rowptr / ex_col / bad_count or n_keys < 0.
 *
 * pc_rank_grouped_excluding: cand_type [num_products] = the type under which product p is a candidate, -1 if it is none; it
 * must agree with type_rowptr / type_col.  rank_out[r] = the number of NON-excluded products of type types[r] ordered in front
 * of the target; -1 if the target is in the row's list or cand_type[targets[r]] != types[r]; -1 and *bad_count as
 * pc_rank_grouped otherwise.  pc_rank_grouped's launches as they are, then one wave per row scores the row's list and its
 * target through the same MFMA chain and takes the excluded products of the type that stand in front of the target off the
 * count: rank_out[r] < n exactly when pc_retrieve_topk_grouped_excluding's top n holds the target at that position.  Workspace:
 * pc_rank_grouped_workspace_bytes.  Error codes as pc_rank_grouped, PC_EINVAL also for a null row_key / ex_rowptr / ex_col /
 * cand_type or n_keys < 0. */
size_t pc_retrieve_topk_grouped_excluding_workspace_bytes(int rows, int n_types, int n, int slices);
int pc_retrieve_topk_grouped_excluding(const float *proj, const int32_t *types, const int32_t *row_key, int rows,
                                       const int32_t *type_rowptr, const int32_t *type_col, const float *table, int n_types,
                                       const int32_t *ex_rowptr, const int32_t *ex_col, int n_keys, int n, int dim, int slices,
                                       int32_t *out_idx, float *out_score, int32_t *bad_count, void *ws, size_t ws_bytes,
                                       void *stream);
int pc_rank_grouped_excluding(const float *proj, const int32_t *types, const int32_t *targets, const int32_t *row_key, int rows,
                              const int32_t *type_rowptr, const int32_t *type_col, const float *table, int n_types,
                              int num_products, const int32_t *ex_rowptr, const int32_t *ex_col, int n_keys,
                              const int32_t *cand_type, int dim, int slices, int32_t *rank_out, int32_t *bad_count, void *ws,
                              size_t ws_bytes, void *stream);

/* Long lists (ABI 8, additive; PCompanionInference.recommend_batch above 16: a candidate generator feeds a re-ranker, a
 * business-rule filter or a page of several slots with 50 to 200 products per type).  pc_retrieve_list_grouped is
 * pc_retrieve_topk_grouped's contract for 1 <= n <= 256, and pc_retrieve_topk_grouped_excluding's when row_key is given:
 * out_idx [rows, n] / out_score [rows, n] = the first n products of type types[r] that are not in the list of row_key[r], under
 * the same total order (score descending, product index ascending), -1 / -inf past the end of a short type and for a type
 * outside [0, n_types).  row_key == NULL: no lists (ex_rowptr, ex_col NULL, n_keys 0; bad_count may be NULL).  With row_key
 * the exclusion set is the CSR over keys described above; a key outside [-1, n_keys) is served as -1, never indexes memory and
 * is counted in *bad_count (required then; added to).  The scores are formed through pc_retrieve_topk_grouped's own fp32 MFMA
 * chain and every selection is under its total order: for n <= 16 the output is that entry's bit for bit, for every n it does
 * not depend on `slices`, on the placement of the rows or on the order of type_col inside a type, and pc_rank_grouped[_excluding]
 * is < n exactly when the list holds the target at that position.  The same plan over tiles of 16 rows; a row keeps an
 * unsorted candidate buffer and a threshold on chip, compacted by a sorting network when it fills; the slices' sorted partial
 * lists are merged by one wave per row.  No float atomics, no host readback: the launch geometry and the workspace
 * (pc_retrieve_list_grouped_workspace_bytes, 0 for arguments out of range) depend on rows, n_types, n and slices only.
 * PC_EINVAL: null pointer, rows or n_types <= 0; with row_key a null ex_rowptr / ex_col / bad_count or n_keys < 0; without it a
 * list or n_keys != 0; PC_ESHAPE: n outside [1, 256], dim not 128 / 256, slices outside [0, 64]; PC_EWORKSPACE: ws_bytes too
 * small -- each checked before anything is launched. */
size_t pc_retrieve_list_grouped_workspace_bytes(int rows, int n_types, int n, int slices);
int pc_retrieve_list_grouped(const float *proj, const int32_t *types, const int32_t *row_key, int rows,
                             const int32_t *type_rowptr, const int32_t *type_col, const float *table, int n_types,
                             const int32_t *ex_rowptr, const int32_t *ex_col, int n_keys, int n, int dim, int slices,
                             int32_t *out_idx, float *out_score, int32_t *bad_count, void *ws, size_t ws_bytes,
                             void *stream);

/* A bf16 copy of the catalogue (ABI 8, additive; PCompanionInference(..., catalogue=): the fp32 table is the largest thing in
 * HBM while a model is served -- 5.1 GB at 10 M x 128 -- and the bf16 copy is half of it).  pc_retrieve_topk_grouped_bf16 is
 * pc_retrieve_topk_grouped's contract, and pc_retrieve_topk_grouped_excluding's when row_key is given, over table_bf16
 * [num_products, dim]: bf16 bit patterns, row-major, 16-byte aligned (the fp32 features rounded to nearest even).  The stored
 * table is scored against the UNROUNDED query: each fp32 query row is split into three bf16 pieces by truncation
 * (q = p0 + p1 + p2 to 2^-24 |q|) and p0 . t, p1 . t, p2 . t are accumulated in fp32 on v_mfma_f32_16x16x32_bf16.  Every
 * product is exact, so the score is the fp32-grade dot product of proj[r] with the ROUNDED table row -- not that of the fp32
 * table: the lists can differ from pc_retrieve_topk_grouped's wherever two products lie within bf16 rounding of each other.
 * The same plan, work items, selection, merge and total order (score descending, product index ascending); the order of a
 * score's chain depends on the dimension index and the piece alone, so the output is bitwise deterministic and does not
 * depend on `slices`, on the placement of the rows or on the order of type_col inside a type.  row_key == NULL: no lists
 * (ex_rowptr, ex_col NULL, n_keys 0; bad_count may be NULL).  With row_key the exclusion set is the CSR over keys described
 * above; a key outside [-1, n_keys) is served as -1, never indexes memory and is counted in *bad_count (required then; added
 * to).  No float atomics, no host readback: the launch geometry and the workspace
 * (pc_retrieve_topk_grouped_bf16_workspace_bytes, 0 for arguments out of range; pc_retrieve_topk_grouped's size) depend on
 * rows, n_types, n and slices only.  PC_EINVAL: null pointer, rows or n_types <= 0; with row_key a null ex_rowptr / ex_col /
 * bad_count or n_keys < 0; without it a list or n_keys != 0; PC_ESHAPE: n outside [1, 16], dim not 128 / 256, slices outside
 * [0, 64], table_bf16 not 16-byte aligned; PC_EWORKSPACE: ws_bytes too small -- each checked before anything is launched. */
size_t pc_retrieve_topk_grouped_bf16_workspace_bytes(int rows, int n_types, int n, int slices);
int pc_retrieve_topk_grouped_bf16(const float *proj, const int32_t *types, const int32_t *row_key, int rows,
                                  const int32_t *type_rowptr, const int32_t *type_col, const uint16_t *table_bf16,
                                  int n_types, const int32_t *ex_rowptr, const int32_t *ex_col, int n_keys, int n, int dim,
                                  int slices, int32_t *out_idx, float *out_score, int32_t *bad_count, void *ws,
                                  size_t ws_bytes, void *stream);

/* A per-product additive term on the score (ABI 8, additive; inference.SimilarProducts: Product2Vec is trained for the
 * Euclidean order, and |q - e_p|^2 = |q|^2 - 2 (<q, e_p> - |e_p|^2 / 2), so the nearest product under L2 is the largest
 * <q, e_p> + b_p with b_p = -|e_p|^2 / 2; the same term carries a popularity prior or a business boost).  bias
 * [num_products] fp32; the score of row r and product p is
 *   s(r, p) = fl(d(r, p) + bias[p]),  d(r, p) = pc_retrieve_topk_grouped's own fp32 MFMA chain over table [num_products, dim],
 * one fp32 addition after the chain, so a zero bias gives the unbiased entries' output bit for bit.
 *
 * pc_half_sq_norm_bias: out[p] = -0.5f * sum_d table[p][d]^2 for p < rows, one fixed summation order per row (16 partial sums
 * over the dimensions 4 l + 64 j + e, met in a butterfly), no atomics: the same bits for every launch geometry and run.
 * PC_EINVAL: null pointer, rows <= 0; PC_ESHAPE: dim not 128 / 256.
 *
 * pc_retrieve_topk_grouped_biased: pc_retrieve_topk_grouped's contract, and pc_retrieve_topk_grouped_excluding's when row_key
 * is given, under s: out_idx / out_score [rows, n] = the first n products of type types[r] (not in the list of row_key[r])
 * under (s descending, product index ascending), out_score = s, -1 / -inf past the end of a short type and for a type outside
 * [0, n_types).  row_key == NULL: no lists (ex_rowptr, ex_col NULL, n_keys 0; bad_count may be NULL).  With row_key the
 * exclusion set is the CSR over keys described above; a key outside [-1, n_keys) is served as -1, never indexes memory and is
 * counted in *bad_count (required then; added to).  The same plan, work items, selection, merge and workspace size
 * (pc_retrieve_topk_grouped_biased_workspace_bytes, 0 for arguments out of range); bitwise deterministic and independent of
 * `slices`, of the placement of the rows and of the order of type_col inside a type; no float atomics, no host readback.
 * PC_EINVAL: null pointer, rows or n_types <= 0; with row_key a null ex_rowptr / ex_col / bad_count or n_keys < 0; without it a
 * list or n_keys != 0; PC_ESHAPE: n outside [1, 16], dim not 128 / 256, slices outside [0, 64]; PC_EWORKSPACE: ws_bytes too
 * small -- each checked before anything is launched.
 *
 * pc_rank_grouped_biased: pc_rank_grouped's contract under s -- rank_out[r] = #{ p of type types[r] : s_p > g or (s_p == g
 * and p < y) }, g = s(r, y), y = targets[r] -- and, when row_key is given (then with ex_rowptr, ex_col and cand_type: all four
 * or none), pc_rank_grouped_excluding's: the excluded products are not counted, and rank_out[r] = -1 where the target is in
 * the row's list or cand_type[y] != types[r].  -1 and *bad_count for rows without a type or with an id out of range as
 * pc_rank_grouped.  rank_out[r] < n exactly when pc_retrieve_topk_grouped_biased's top n (same lists) holds the target at
 * that position.  Workspace: pc_rank_grouped_biased_workspace_bytes (pc_rank_grouped's size).  PC_EINVAL: null pointer, rows,
 * n_types or num_products <= 0, n_keys < 0, half-given exclusion arguments; PC_ESHAPE: dim not 128 / 256, slices outside
 * [0, 64]; PC_EWORKSPACE: ws_bytes too small -- each checked before anything is launched. */
int pc_half_sq_norm_bias(const float *table, int rows, int dim, float *out, void *stream);
size_t pc_retrieve_topk_grouped_biased_workspace_bytes(int rows, int n_types, int n, int slices);
int pc_retrieve_topk_grouped_biased(const float *proj, const int32_t *types, const int32_t *row_key, int rows,
                                    const int32_t *type_rowptr, const int32_t *type_col, const float *table,
                                    const float *bias, int n_types, const int32_t *ex_rowptr, const int32_t *ex_col,
                                    int n_keys, int n, int dim, int slices, int32_t *out_idx, float *out_score,
                                    int32_t *bad_count, void *ws, size_t ws_bytes, void *stream);
size_t pc_rank_grouped_biased_workspace_bytes(int rows, int n_types, int slices);
int pc_rank_grouped_biased(const float *proj, const int32_t *types, const int32_t *targets, const int32_t *row_key, int rows,
                           const int32_t *type_rowptr, const int32_t *type_col, const float *table, const float *bias,
                           int n_types, int num_products, const int32_t *ex_rowptr, const int32_t *ex_col, int n_keys,
                           const int32_t *cand_type, int dim, int slices, int32_t *rank_out, int32_t *bad_count, void *ws,
                           size_t ws_bytes, void *stream);

/* A trainable product table in the joint step (ABI 8, additive; csrc/table_train.hip; a labelled extension -- the reference's
 * table is frozen -- for one device).  In the batch layout only the query row reaches the table (p_companion.py:51), so the
 * rows with a gradient are query_idx and the only path is the item hinge through item_projection.
 *
 * pc_joint_query_grad: dq [B, dim] = d(loss)/d(E_prod[query_idx[b]]) of pc_joint_train_step's loss for the K predicted types
 * topk [B, K] of the step that just ran (the type branch does not depend on the query row, topk carries no gradient):
 *   pi_b = W_item q_b + b_item;  tp_bk = W_type E_c[topk[b,k]] + b_type;  x_bk = pi_b * tp_bk
 *   np = |x_bk - pos_b|, nn = |x_bk - neg_b| (no eps), l = margin - np + nn, g = l > 0 ? alpha / (B K) : 0
 *   dx_bk = -(x_bk - pos_b) (np > 0 ? g / np : 0) + (x_bk - neg_b) (nn > 0 ? g / nn : 0)
 *   dq_b = W_item^T sum_k dx_bk * tp_bk
 * -- the fused joint step's conventions (strict hinge, subgradient 0 at a zero norm).  p: the step's parameters with product_table
 * [num_products, dim] set; dim 128 or 256; dq is written for every row.  A query_idx outside [0, num_products) or a topk id
 * outside [0, T) never indexes anything: the sample's dq row is zero and every such id adds one to *bad (int32 [1], added to).
 * Six launches on `stream` (id check, the two projections, W_item^T, the row-wise pass, the product with W_item^T), no host
 * readback; ws: pc_joint_query_grad_workspace_bytes(B, K, dim) (0 for arguments out of range).  PC_EINVAL: null pointer,
 * B, T or num_products <= 0; PC_ESHAPE: K outside [1, 8] or > T, dim not 128 / 256, pos_items / neg_items / dq / ws not
 * 16-byte aligned; PC_EWORKSPACE: ws_bytes too small -- each checked before anything is launched.
 *
 * pc_sparse_adam_rows: torch.optim.SparseAdam (no weight decay) over table [P, dim] with moments exp_avg / exp_avg_sq [P, dim]:
 * moments and parameter of a row move only in a step that names it.  idx [R] int32 (duplicates expected), grad [R, dim],
 * step number t >= 1 owned by the host.  For every distinct id u in [0, P), with every fl one fp32 rounding (no contraction,
 * division and square root correctly rounded):
 *   g_u = grad[r1] + grad[r2] + ...   over all r with idx[r] = u, sequential fp32 adds in ascending r
 *   m_u += fl(fl(g_u - m_u) fl32(1 - beta1));  v_u += fl(fl(fl(g_u g_u) - v_u) fl32(1 - beta2))
 *   p_u += fl(fl32(-s) fl(m_u / fl(sqrt(v_u) + fl32(eps)))),  s = lr sqrt(1 - beta2^t) / (1 - beta1^t) in fp64
 * An id of -1 is skipped (padding); any other id outside [0, P) is skipped, never indexes anything and adds one to *bad
 * (int32 [1], added to).  Rows not named keep their bits.  The sources of a row are brought together by a stable LSD radix
 * sort of (id, r) (8-bit digits over bit_length(P) bits; one launch up to R = 8192, three per digit above) and one wave per
 * distinct row applies the update: no float atomics, the result is a function of the inputs alone.  1 <= R <= 2^20; ws:
 * pc_sparse_adam_rows_workspace_bytes(R) (0 for R out of range).  PC_EINVAL: null pointer, P < 1 or >= 2^31, R out of
 * range, t < 1; PC_ESHAPE: dim not 128 / 256, table / exp_avg / exp_avg_sq / grad / ws not 16-byte aligned, idx / bad not
 * 4-byte aligned; PC_EWORKSPACE: ws_bytes too small -- each checked before anything is launched. */
size_t pc_joint_query_grad_workspace_bytes(int batch, int k, int dim);
int pc_joint_query_grad(const pc_joint_tensors *p, const int32_t *query_idx, const int32_t *topk, const float *pos_items,
                        const float *neg_items, int batch, int64_t num_products, int num_types, int k, int dim, float margin,
                        float alpha, float *dq, int32_t *bad, void *ws, size_t ws_bytes, void *stream);
size_t pc_sparse_adam_rows_workspace_bytes(int rows);
int pc_sparse_adam_rows(float *table, float *exp_avg, float *exp_avg_sq, int64_t num_products, int dim, const int32_t *idx,
                        const float *grad, int rows, int64_t t, double lr, double beta1, double beta2, double eps,
                        int32_t *bad, void *ws, size_t ws_bytes, void *stream);

/* A k-means cell index over the product table (ABI 8, additive; csrc/cells.hip; ops.build_cell_index,
 * inference.IndexedSimilarProducts).  The assignment of a Lloyd iteration and the search inside the probed cells are
 * pc_retrieve_topk_grouped_biased with a cell in the place of a type; these two entries are what it does not provide.
 *
 * pc_cell_means: the centroid update.  cell_rowptr [n_cells + 1] / cell_col: a CSR of product ids per cell (ops.type_csr of the
 * assignment); centroids [n_cells, dim] fp32, read and written:
 *   centroids[c] = (sum of table[cell_col[i]], i in [cell_rowptr[c], cell_rowptr[c + 1])) / m_c   in fp32,
 * m_c the number of those ids inside [0, num_products).  A cell with m_c == 0 keeps the centroid it had.  An id outside
 * [0, num_products) is passed over: never read, not summed and not counted in m_c -- the mean is over the rows that were
 * summed.  Passed-over ids are NOT reported (no bad_count argument): the CSR is the project's own (type_csr yields ids in
 * range by construction), so an id out of range is a caller's slip that must do no harm, not a served condition to count.
 * One workgroup per cell; 1024 / dim thread groups take the members g, g + G, .. of the cell in turn (16-byte loads of the
 * rows, sequential fp32 additions from zero), the groups' sums meet in a fixed tree in LDS, one correctly rounded division by
 * (float) m_c.  The summation order is a function of the member's position in the cell and of the dimension alone: the same
 * bits on every run and for every grid; no atomics.  m_c above 2^24 is rounded to fp32 before the division.
 * PC_EINVAL: null pointer, n_cells or num_products <= 0; PC_ESHAPE: dim not 128 / 256, table / centroids not 16-byte aligned.
 *
 * pc_merge_lists: idx / score [rows, L, n]: L lists per row, each sorted under (score descending, product index ascending)
 * with -1 / -inf behind its last entry (the output format of the grouped retrievals); the lists of one row hold disjoint
 * products.  out_idx / out_score [rows, n] = the first n of their union under the same total order, the scores copied bit
 * for bit, -1 / -inf past the end.  One wave per row, lane l a cursor into list l, n rounds of a wave-wide best head.
 * PC_EINVAL: null pointer, rows <= 0; PC_ESHAPE: L outside [1, 64], n outside [1, 256]. */
int pc_cell_means(const float *table, const int32_t *cell_rowptr, const int32_t *cell_col, int n_cells, int num_products,
                  int dim, float *centroids, void *stream);
int pc_merge_lists(const int32_t *idx, const float *score, int rows, int L, int n, int32_t *out_idx, float *out_score,
                   void *stream);

/* The cell index over the bf16 copy of the catalogue (ABI 8, additive; csrc/cells_bf16.hip; ops.cell_means_bf16,
 * ops.build_cell_index_bf16, inference.IndexedCompactSimilarProducts).
 *
 * pc_cell_means_bf16: pc_cell_means' contract over table [num_products, dim] bf16 (the patterns of ops.catalogue_bf16, 8-byte
 * aligned); cell_rowptr, cell_col and centroids [n_cells, dim] fp32 (read and written, 16-byte aligned) as there:
 *   centroids[c] = (sum of widen(table[cell_col[i]]), i in [cell_rowptr[c], cell_rowptr[c + 1])) / m_c   in fp32,
 * widen the exact bf16 -> fp32 conversion (the pattern shifted left by 16), m_c the number of those ids inside
 * [0, num_products).  A cell with m_c == 0 keeps the centroid it had; an id outside [0, num_products) is passed over: never
 * read, not summed, not counted in m_c, not reported.  The ownership and the order are pc_cell_means': lane c of a group of
 * dim / 4 lanes owns the columns 4 c .. 4 c + 3 (here one 8-byte load of four patterns), the 1024 / dim groups take the
 * members g, g + G, .. in turn (sequential fp32 additions from zero), the same tree in LDS, one correctly rounded division by
 * (float) m_c -- every addition is pc_cell_means' addition of the same operands, so centroids are bit for bit pc_cell_means'
 * on the widened table, which is never formed.  The same bits on every run and for every grid; no atomics.
 * PC_EINVAL: null pointer, n_cells or num_products <= 0; then PC_ESHAPE: dim not 128 / 256; then PC_ESHAPE: table not 8-byte
 * or centroids not 16-byte aligned -- each checked before anything is launched. */
int pc_cell_means_bf16(const void *table, const int32_t *cell_rowptr, const int32_t *cell_col, int n_cells, int num_products,
                       int dim, float *centroids, void *stream);

/* Diversified lists (ABI 8, additive; csrc/diversify.hip; ops.diversify_lists, ops.inv_norm,
 * PCompanionInference.recommend_diverse_batch): a greedy maximal-marginal-relevance re-rank of a served pool, on the device.
 *
 * pc_diversify_lists: idx / score [rows, m], 1 <= m <= 256: a pool of candidates per row as pc_retrieve_list_grouped and
 * pc_retrieve_topk_grouped return it, in any order.  A slot is no candidate if its id is -1 or its score is not finite,
 * wherever it stands; a slot whose id lies outside [-1, num_products) is no candidate either, is never dereferenced and adds
 * one to *bad_count (int32 [1], optional, added to).  table [num_products, dim] fp32, 16-byte aligned, dim 128 or 256; scale
 * [num_products] fp32 or NULL.  The similarity of two products is
 *   sim(a, b) = fl(d(a, b) * fl(scale[a] * scale[b]))    (scale == NULL: d(a, b)),
 * d the fp32 dot product of table[a] and table[b] from zero: four fused-multiply-add chains per 128 dimensions (chain e over
 * the dimensions 128 h + 4 k + e, k ascending) joined as (c0 + c2) + (c1 + c3), the two halves of a 256-dimension row added
 * last.  It is symmetric bit for bit, and its order depends on the dimension index alone.  With mu = fl(1 - lam) in fp32, the
 * rounds t = 0 .. n - 1 give every remaining candidate the value
 *   v_j = fl(lam * score_j)                               (t = 0),
 *   v_j = fl(fl(lam * score_j) - fl(mu * pen_j))          (t > 0), pen_j = max of sim(j, i) over the products i picked so far,
 * three separately rounded operations, and pick the best under (value descending, product index ascending).  out_idx
 * [rows, n]: the picks in pick order; out_score [rows, n]: each pick's INPUT score; -1 / -inf past the end of a pool with fewer
 * than n candidates.  Distinct ids within a row are the caller's contract: duplicates are served as separate candidates, and
 * which of two slots equal in (value, id) is picked is unspecified.  lam = 1 returns the first n of the pool under the total
 * order -- of a grouped entry's list its own first n, bit for bit --, n = m returns every candidate once, and a permutation of
 * a row's slots changes no output bit.  One workgroup per row holds the pool's table rows in registers, gathered once;
 * 64 slots per workgroup for m <= 64, 256 above, the same bits from both.  No workspace, no float atomics, no host readback.
 * PC_ESHAPE: rows < 0, m outside [1, 256], n outside [1, m], dim not 128 / 256, num_products < 1, lam outside [0, 1] or NaN, a
 * null idx / score / table / out_idx / out_score, table not 16-byte aligned -- each checked before anything is launched;
 * rows == 0 succeeds without a launch.
 *
 * pc_inv_norm: out[p] = 1 / |table[p]|_2 for p < rows, the scale under which sim is the cosine: the sum of squares in
 * pc_half_sq_norm_bias's fixed order (16 partial sums over the dimensions 4 l + 64 j + e, met in a butterfly), one correctly
 * rounded square root, one correctly rounded division; an all-zero row gives 0.  The same bits for every launch geometry and
 * run.  PC_EINVAL: null pointer, rows <= 0; PC_ESHAPE: dim not 128 / 256, table not 16-byte aligned. */
int pc_diversify_lists(const int32_t *idx, const float *score, int rows, int m, const float *table, const float *scale,
                       int num_products, int dim, int n, float lam, int32_t *out_idx, float *out_score, int32_t *bad_count,
                       void *stream);
int pc_inv_norm(const float *table, int rows, int dim, float *out, void *stream);

/* Long and diversified lists from the bf16 copy alone (ABI 8, additive; csrc/retrieve_list_bf16.hip, csrc/diversify.hip;
 * ops.CompactCatalogue, PCompanionInference(..., catalogue=ops.CompactCatalogue(...))): a server that shows a page of 50 to 200
 * products per type, or a diversified row, without the fp32 table in HBM.  table_bf16 [num_products, dim] everywhere: bf16 bit
 * patterns, row-major, 16-byte aligned, dim 128 or 256 (pc_retrieve_topk_grouped_bf16's table).
 *
 * pc_retrieve_list_grouped_bf16: pc_retrieve_list_grouped's contract and argument list for 1 <= n <= 256 -- out_idx / out_score
 * [rows, n] = the first n products of type types[r] that are not in the list of row_key[r] (row_key == NULL: no lists), -1 /
 * -inf past the end -- over table_bf16.  The score of a (row, product) pair is formed through pc_retrieve_topk_grouped_bf16's
 * own chain (the unrounded fp32 query split into three bf16 pieces, k-block by k-block on v_mfma_f32_16x16x32_bf16 into one
 * accumulator) and has that entry's bits; everything else is pc_retrieve_list_grouped's own code -- one kernel body and one host
 * path for the two tables (csrc/grouped_list.h), the score chain its only parameter: a row's unsorted candidate buffer and
 * threshold on chip, compacted by a sorting network, the slices' sorted partial lists merged by one wave per row, every step
 * under the total order (score descending, product index ascending).  For n <= 16 the output is
 * pc_retrieve_topk_grouped_bf16's bit for bit; for every n it does not depend on `slices`, on the placement of the rows or on
 * the order of type_col inside a type.  A key outside [-1, n_keys) is served as -1, never indexes memory and is counted in
 * *bad_count (required with row_key; added to).  No float atomics, no host readback; the workspace
 * (pc_retrieve_list_grouped_bf16_workspace_bytes, 0 for arguments out of range) is pc_retrieve_list_grouped's size.
 * PC_EINVAL: null pointer, rows or n_types <= 0; with row_key a null ex_rowptr / ex_col / bad_count or n_keys < 0; without it a
 * list or n_keys != 0; PC_ESHAPE: n outside [1, 256], dim not 128 / 256, slices outside [0, 64], table_bf16 not 16-byte
 * aligned; PC_EWORKSPACE: ws_bytes too small -- each checked before anything is launched.
 *
 * pc_diversify_lists_bf16 / pc_inv_norm_bf16: pc_diversify_lists' / pc_inv_norm's contracts and return codes over table_bf16.
 * The result is, bit for bit, what the fp32 entry returns on the widened table (every bf16 value is an fp32 value): the rows
 * are widened as they are gathered, and the dot product's chains, the similarity, the rounds' values, the pick rule and the
 * norm's summation order are the fp32 entries' own code.  scale is fp32 [num_products] or NULL as there (pc_inv_norm_bf16 of
 * the same table: the cosine between the rows that are stored). */
size_t pc_retrieve_list_grouped_bf16_workspace_bytes(int rows, int n_types, int n, int slices);
int pc_retrieve_list_grouped_bf16(const float *proj, const int32_t *types, const int32_t *row_key, int rows,
                                  const int32_t *type_rowptr, const int32_t *type_col, const uint16_t *table_bf16,
                                  int n_types, const int32_t *ex_rowptr, const int32_t *ex_col, int n_keys, int n, int dim,
                                  int slices, int32_t *out_idx, float *out_score, int32_t *bad_count, void *ws,
                                  size_t ws_bytes, void *stream);
int pc_diversify_lists_bf16(const int32_t *idx, const float *score, int rows, int m, const uint16_t *table_bf16,
                            const float *scale, int num_products, int dim, int n, float lam, int32_t *out_idx,
                            float *out_score, int32_t *bad_count, void *stream);
int pc_inv_norm_bf16(const uint16_t *table_bf16, int rows, int dim, float *out, void *stream);

/* Group caps and the merged page (ABI 8, additive; csrc/cap_lists.hip; ops.cap_lists,
 * PCompanionInference.recommend_capped_batch / recommend_page_batch, SimilarProducts.similar_capped_batch): at most `cap`
 * products of one product group (a parent item, a brand, a seller) in a served row, as a post-pass over a pool, on the device.
 *
 * pc_cap_lists: idx / score [rows, m], 1 <= m <= 256: a pool of candidates per row as the grouped retrievals return it -- or
 * several of their lists side by side --, in any order.  A slot is a candidate iff its id lies in [0, num_products) and its
 * score is finite; a slot with id -1 or a score that is not finite (+-inf, NaN) is none, wherever it stands; a slot whose id
 * lies outside [-1, num_products) is none either, is never used as an index and adds one to *bad_count (int32 [1], optional,
 * added to).  group [num_products] int32 or NULL: group[p] < 0 says that product p is ungrouped and never capped; group ids are
 * only compared, so every non-negative int32 is one; NULL: no product is grouped.  row_ban [rows] int32 or NULL: with
 * row_ban[r] = b >= 0 a candidate whose group is b is no candidate of row r ("never a variant of the query itself"); a negative
 * entry or NULL bans nothing; row_ban needs group.  The candidates of a row are walked under the total order of the grouped
 * retrievals (score descending, product index ascending): a grouped candidate is kept iff fewer than `cap` candidates of its
 * group stand in front of it -- the greedy "keep while the group has room": the first `cap` of a group and none after them --,
 * an ungrouped candidate always.  out_idx / out_score [rows, n]: the first n kept candidates in that order, each with its INPUT
 * score bits (a -0.0 stays -0.0); -1 / -inf past the end.  Distinct ids within a row are the caller's contract: duplicates are
 * separate candidates, and two slots equal in (score, id) are interchangeable.  Consequences: cap >= m or group == NULL returns
 * the pool's first n under the total order -- of a grouped entry's list its own first n, bit for bit: the sort / merge alone --;
 * a permutation of a row's slots changes no output bit; n = m returns every kept candidate; the result is the same for every
 * launch geometry and run.  One wave per row sorts the row in registers (64 lanes x 2 slots for m <= 128, x 4 above, the same
 * bits from both), counts for every slot the earlier slots of its group, and compacts.  Integer and float compares only: no
 * workspace, no float atomics, no host readback.
 * PC_ESHAPE: rows < 0, m outside [1, 256], n outside [1, m], cap < 1, num_products < 1, row_ban without group, a null idx /
 * score / out_idx / out_score -- each checked before anything is launched; rows == 0 succeeds without a launch. */
int pc_cap_lists(const int32_t *idx, const float *score, int rows, int m, const int32_t *group, const int32_t *row_ban,
                 int num_products, int n, int cap, int32_t *out_idx, float *out_score, int32_t *bad_count, void *stream);

/* Long substitute lists (ABI 8, additive; csrc/nearest_list.hip; SimilarProducts.similar_list_batch and
 * similar_capped_list_batch: a product's nearest neighbours are its own variants, so a group cap over a pool of 16 leaves the
 * served list short).  pc_retrieve_list_grouped_biased is pc_retrieve_list_grouped's contract and argument list, bias
 * [num_products] fp32 directly behind the table, for 1 <= n <= 256 under the biased score
 *   s(r, p) = fl(d(r, p) + bias[p]),  d(r, p) = pc_retrieve_list_grouped's own fp32 MFMA chain over table [num_products, dim],
 * one fp32 addition after the chain (the accumulator starts at zero): out_idx / out_score [rows, n] = the first n products of
 * type types[r] that are not in the list of row_key[r] under (s descending, product index ascending), out_score = s, -1 / -inf
 * past the end of a short type and for a type outside [0, n_types).  row_key == NULL: no lists (ex_rowptr, ex_col NULL, n_keys
 * 0; bad_count may be NULL); with row_key a key outside [-1, n_keys) is served as -1, never indexes memory and is counted in
 * *bad_count (required then; added to).  A (row, product) score has pc_retrieve_topk_grouped_biased's and
 * pc_rank_grouped_biased's bits: for n <= 16 the output is pc_retrieve_topk_grouped_biased's bit for bit, with a zero bias it is
 * pc_retrieve_list_grouped's, and pc_rank_grouped_biased is < n exactly when the list holds the target at that position.  The
 * kernel body, the merge and the host path are pc_retrieve_list_grouped's own code: bitwise deterministic and independent of
 * `slices`, of the placement of the rows and of the order of type_col inside a type; no float atomics, no host readback.  The
 * workspace (pc_retrieve_list_grouped_biased_workspace_bytes, 0 for arguments out of range) is pc_retrieve_list_grouped's size.
 * PC_EINVAL: null pointer (bias among them), rows or n_types <= 0; with row_key a null ex_rowptr / ex_col / bad_count or
 * n_keys < 0; without it a list or n_keys != 0; PC_ESHAPE: n outside [1, 256], dim not 128 / 256, slices outside [0, 64];
 * PC_EWORKSPACE: ws_bytes too small -- each checked before anything is launched. */
size_t pc_retrieve_list_grouped_biased_workspace_bytes(int rows, int n_types, int n, int slices);
int pc_retrieve_list_grouped_biased(const float *proj, const int32_t *types, const int32_t *row_key, int rows,
                                    const int32_t *type_rowptr, const int32_t *type_col, const float *table,
                                    const float *bias, int n_types, const int32_t *ex_rowptr, const int32_t *ex_col,
                                    int n_keys, int n, int dim, int slices, int32_t *out_idx, float *out_score,
                                    int32_t *bad_count, void *ws, size_t ws_bytes, void *stream);

/* Ranks and substitutes from the bf16 copy alone (ABI 8, additive; csrc/rank_bf16.hip, csrc/nearest_list_bf16.hip;
 * ops.rank_grouped_bf16, ops.retrieve_list_grouped_bf16_biased, ops.half_sq_norm_bias_bf16; inference.CompactInference and
 * inference.CompactSimilarProducts): a deployment that gave the fp32 table back measures hit@k / MRR of what it serves and
 * serves Euclidean neighbours, over the stored (rounded) rows.  table_bf16 [num_products, dim] everywhere: bf16 bit patterns,
 * row-major, 16-byte aligned, dim 128 or 256 (pc_retrieve_topk_grouped_bf16's table).  The score of row r and product p is
 *   s(r, p) = fl(d(r, p) + bias[p]),  d(r, p) = pc_retrieve_topk_grouped_bf16's own chain (the unrounded fp32 query split into
 * three bf16 pieces, k-block by k-block on v_mfma_f32_16x16x32_bf16 into one accumulator), one fp32 addition after the chain
 * (the accumulator starts at zero); bias [num_products] fp32.
 *
 * pc_half_sq_norm_bias_bf16: out[p] = -0.5f * sum_d e[p][d]^2 over the stored rows, in pc_half_sq_norm_bias's summation order
 * (16 partial sums over the dimensions 4 l + 64 j + e, met in a butterfly over the lane distances 8, 4, 2, 1): bit for bit
 * pc_half_sq_norm_bias on the widened table, which is never formed.  PC_EINVAL: null pointer, rows <= 0; PC_ESHAPE: dim not
 * 128 / 256, table_bf16 not 8-byte aligned.
 *
 * pc_retrieve_list_grouped_bf16_biased: pc_retrieve_list_grouped_biased's contract and argument list over table_bf16, for
 * 1 <= n <= 256 (it serves n <= 16 too: there is no 16-entry biased bf16 entry).  pc_retrieve_list_grouped_bf16's kernel body,
 * merge and host path with the body's bias hook: with a zero bias the output is pc_retrieve_list_grouped_bf16's bit for bit;
 * out_score = fl(that entry's score + bias[p]); the same bits for every `slices`, placement of the rows and order of type_col
 * inside a type.  Error codes as pc_retrieve_list_grouped_biased, and PC_ESHAPE for a table_bf16 that is not 16-byte aligned.
 * Workspace: pc_retrieve_list_grouped_bf16_biased_workspace_bytes (pc_retrieve_list_grouped's size).
 *
 * pc_rank_grouped_bf16: pc_rank_grouped_biased's contract and argument list over table_bf16, with a bias that may be NULL
 * (then s = d): rank_out[r] = #{ p of type types[r], not in the row's list : s_p > g or (s_p == g and p < y) }, g = s(r, y),
 * y = targets[r]; row_key, ex_rowptr, ex_col and cand_type all four or none; with them rank_out[r] = -1 where the target is in
 * the row's list or cand_type[y] != types[r]; -1 and *bad_count for rows without a type or with an id out of range as
 * pc_rank_grouped.  A (row, product) score has the bits pc_retrieve_topk_grouped_bf16, pc_retrieve_list_grouped_bf16 and, with
 * a bias, pc_retrieve_list_grouped_bf16_biased give it: rank_out[r] < n exactly when that list (same bias, same lists) holds
 * the target at that position.  pc_rank_grouped's plan, work items and count (integer atomics, one per (row, slice)); the same
 * result for every `slices`; no float atomics, no host readback.  Workspace: pc_rank_grouped_bf16_workspace_bytes
 * (pc_rank_grouped's size).  PC_EINVAL: null pointer (bias apart), rows, n_types or num_products <= 0, n_keys < 0, half-given
 * exclusion arguments; PC_ESHAPE: dim not 128 / 256, slices outside [0, 64], table_bf16 not 16-byte aligned; PC_EWORKSPACE:
 * ws_bytes too small -- each checked before anything is launched. */
int pc_half_sq_norm_bias_bf16(const uint16_t *table_bf16, int rows, int dim, float *out, void *stream);
size_t pc_retrieve_list_grouped_bf16_biased_workspace_bytes(int rows, int n_types, int n, int slices);
int pc_retrieve_list_grouped_bf16_biased(const float *proj, const int32_t *types, const int32_t *row_key, int rows,
                                         const int32_t *type_rowptr, const int32_t *type_col, const uint16_t *table_bf16,
                                         const float *bias, int n_types, const int32_t *ex_rowptr, const int32_t *ex_col,
                                         int n_keys, int n, int dim, int slices, int32_t *out_idx, float *out_score,
                                         int32_t *bad_count, void *ws, size_t ws_bytes, void *stream);
size_t pc_rank_grouped_bf16_workspace_bytes(int rows, int n_types, int slices);
int pc_rank_grouped_bf16(const float *proj, const int32_t *types, const int32_t *targets, const int32_t *row_key, int rows,
                         const int32_t *type_rowptr, const int32_t *type_col, const uint16_t *table_bf16, const float *bias,
                         int n_types, int num_products, const int32_t *ex_rowptr, const int32_t *ex_col, int n_keys,
                         const int32_t *cand_type, int dim, int slices, int32_t *rank_out, int32_t *bad_count, void *ws,
                         size_t ws_bytes, void *stream);

/* Basket recommendations (ABI 8, additive; csrc/fuse_lists.hip; ops.fuse_lists, PCompanionInference.recommend_basket_batch):
 * the lists served for the items of a basket fused into one list, on the device.
 *
 * pc_fuse_lists: idx / score [baskets, sources, w], 1 <= sources * w <= 1024: `sources` rows of w slots per basket, each row
 * what a grouped retrieval returned for one basket item -- its K type lists side by side --, the slots in any order.  source
 * [baskets, sources] int32 or NULL: the product id of the item behind each row, -1 = no item here (padding); NULL: every row
 * counts and nothing is banned.  ex_rowptr [num_products + 1] / ex_col: an exclusion CSR keyed by product id with strictly
 * ascending rows (ops.exclusion_csr), both or neither, and only with source.
 *   candidate  a slot whose row's source is not -1, whose id lies in [0, num_products) and whose score is finite.  An id
 *              outside [-1, num_products) is never used as an index and adds one to *bad_count (int32 [1], optional, added to),
 *              whatever its row; a source outside [-1, num_products) does the same, once, and its row is dropped.
 *   ban set    the basket's own source ids and, with the CSR, every id in the exclusion rows of those sources.  A banned
 *              product is no candidate, whichever row offered it: a substitute of item A is not served through item B, and
 *              nothing already in the basket is served.
 *   fusion     all candidate slots of a basket that hold one product id are one product.  With its slot scores in descending
 *              order s1 >= s2 >= ... (+0.0 before -0.0) -- combine 0 (sum): f = s1, then f = fl(f + s2), and so on:
 *              sequential fp32, the largest first; this order is part of the contract and makes the bits independent of the
 *              order of the slots.  combine 1 (max): f = s1.  support = the number of slots fused.  A sum that overflows is
 *              served as the infinity it became, where the order below puts it.
 *   order      out_idx / out_score / out_support [baskets, n], 1 <= n <= min(sources * w, 256): the first n products under
 *              (fused score descending, product index ascending); -1 / -inf / 0 past the end.
 * One wave per basket sorts the slots in registers (64 lanes x 2, 4, 8 or 16 slots for pools up to 128, 256, 512, 1024, the
 * same bits from all four), compares them with the ban ids streamed through LDS, fuses equal ids by a walk over the sorted
 * row, sorts the products again under their sums and compacts.  Integer compares, float compares and the fp32 additions above
 * only: no workspace, no float atomics, no host readback; the result is the same for every launch geometry and run and under
 * a permutation of a basket's rows (with their sources) or of the slots inside rows.
 * PC_ESHAPE: baskets < 0, sources < 1, w < 1, sources * w > 1024, n outside [1, min(sources * w, 256)], num_products < 1,
 * combine not 0 / 1, one of ex_rowptr / ex_col without the other or without source, a null idx / score / out_idx / out_score /
 * out_support -- each checked before anything is launched; baskets == 0 succeeds without a launch. */
int pc_fuse_lists(const int32_t *idx, const float *score, const int32_t *source, int baskets, int sources, int w,
                  const int32_t *ex_rowptr, const int32_t *ex_col, int num_products, int n, int combine, int32_t *out_idx,
                  float *out_score, int32_t *out_support, int32_t *bad_count, void *stream);

/* Session recommendations (ABI 8, additive; csrc/fuse_sessions.hip; ops.fuse_sessions,
 * PCompanionInference.recommend_session_batch): pc_fuse_lists' fusion for ragged sessions with a weight per item, built on a
 * walk that is linear in the pool.
 *
 * pc_fuse_sessions: idx / score [rows, w], 1 <= w <= 1024: row r is what a grouped retrieval returned for item r -- its K type
 * lists side by side --, the slots in any order, -1 ids and non-finite scores anywhere.  source [rows] int32 or NULL: the
 * item's product id, -1 = no item; NULL: every row qualifies and nothing is banned.  weight [rows] fp32 or NULL: NULL means
 * every weight is 1.  seg_rowptr [sessions + 1] int32: session b owns the rows [seg_rowptr[b], seg_rowptr[b + 1]).  ex_rowptr
 * [num_products + 1] / ex_col: an exclusion CSR keyed by product id with strictly ascending rows (ops.exclusion_csr), both or
 * neither, and only with source.
 *   live rows     L = min(1024 / w, max_items if max_items != 0).  Only the LAST L rows of a session -- its most recent items --
 *                 offer candidates; a session with more rows adds one to *truncated_count (int32 [1], optional, added to).
 *                 Every row of the session still bans, however long the session is.
 *   offering row  a live row whose source lies in [0, num_products) (without source every row qualifies) and whose weight is
 *                 finite and > 0.  A row with weight 0, a negative weight, NaN or +-inf offers nothing; its source still bans:
 *                 the "already bought" case.
 *   term          t = fl(weight[r] * score): one fp32 multiplication, rounded, formed before anything is added and never
 *                 contracted with an addition.  A slot is a candidate iff its row offers, its id lies in [0, num_products) and
 *                 t is finite: an overflowed term is no candidate.  Terms in the subnormal range are outside the contract
 *                 (whether they are flushed is the device's floating-point mode, not this entry's).
 *   ban set       the sources of all rows of the session and, with the CSR, every id in the exclusion rows of those sources:
 *                 pc_fuse_lists' rule.  A banned product is no candidate, whichever row offered it.
 *   fusion        all candidate slots of a session that hold one product id are one product.  With its terms in descending
 *                 order t1 >= t2 >= ... (+0.0 before -0.0) -- combine 0 (sum): f = t1, then f = fl(f + t2), and so on:
 *                 sequential fp32, the largest first.  combine 1 (max): f = t1.  support = the number of slots fused.  A sum
 *                 that overflows is served as the infinity it became.
 *   order         out_idx / out_score / out_support [sessions, n], 1 <= n <= 256: the first n products under (fused score
 *                 descending, product index ascending); -1 / -inf / 0 past the end; an empty session is all padding.
 *   bad inputs    an id of a live row or a source of any row outside [-1, num_products) is never used as an index and adds one
 *                 to *bad_count (int32 [1], optional, added to); such a source's row offers nothing; the slots of rows that
 *                 are not live are not read.  A seg_rowptr entry outside [0, rows] or below its predecessor adds one and is
 *                 clamped -- lo to [0, rows], hi to [lo, rows] --: nothing outside the arrays is read.
 * One wave per session; 64 lanes x 2, 4, 8 or 16 register slots serve effective pools min(len, L) * w of up to 128, 256, 512
 * and 1024.  The pools differ per session and are not read back: every variant that L * w can reach is launched on the one
 * stream, and a wave passes over the sessions of the other variants, so every session is written by exactly one launch.  The
 * slots are sorted by (id ascending, term descending), so that a product's slots are adjacent; the head of each run adds the
 * run in that order; the heads are sorted again under their fused scores and compacted.  No workspace, no float atomics
 * (integer atomics for the two counters only), no host readback; the result does not depend on the launch geometry, the run,
 * the variant that served the session, a permutation of a session's rows together with their sources and weights among the
 * rows of one truncation status, or a permutation of the slots inside rows.
 * PC_ESHAPE: rows < 0, sessions < 0, w outside [1, 1024], n outside [1, 256], max_items < 0, combine not 0 / 1, num_products
 * < 1, one of ex_rowptr / ex_col without the other or without source, and, when sessions > 0, a null seg_rowptr / out_idx /
 * out_score / out_support or (when rows > 0) a null idx / score -- each checked before anything is launched; sessions == 0
 * succeeds without a launch. */
int pc_fuse_sessions(const int32_t *idx, const float *score, const int32_t *source, const float *weight,
                     const int32_t *seg_rowptr, int rows, int sessions, int w, int max_items, const int32_t *ex_rowptr,
                     const int32_t *ex_col, int num_products, int n, int combine, int32_t *out_idx, float *out_score,
                     int32_t *out_support, int32_t *bad_count, int32_t *truncated_count, void *stream);

/* Per-query attribute filters (ABI 8, additive; csrc/where_list.hip, csrc/where_list_bf16.hip; ops.RowWhere,
 * ops.retrieve_list_grouped_where, PCompanionInference.recommend_where_batch, SimilarProducts.similar_where_batch): lists
 * narrowed by a condition on both the query and a property of the candidate -- complements within 0.5x to 2x of the query's
 * price, only what ships to this shopper's region, nothing from a blocked seller tier.
 *
 * pc_row_where: per-product attributes, installed once per catalogue, either may be NULL:
 *   value [num_products] fp32 (a price, a rating, a delivery time), flags [num_products] int32 read as 32 bits;
 * and the per-row predicate, one entry per row of the call:
 *   lo, hi [rows] fp32:      p passes iff lo[r] <= value[p] && value[p] <= hi[r], two fp32 compares: the ends are inclusive, a
 *                            NaN value or bound passes nothing, lo > hi passes nothing, -inf / +inf pass every non-NaN value,
 *                            -0.0 == 0.0.  Both with value, neither without: a one-sided caller passes an infinite bound.
 *   need, deny [rows] int32: p passes iff (flags[p] & need[r]) == need[r] && (flags[p] & deny[r]) == 0; bit 31 is a bit like
 *                            the others.  Only with flags; with flags either may be NULL (read as 0).
 * A product that fails is treated exactly as an excluded product is: never buffered, the row's threshold does not move.  A
 * row's list is the unfiltered order (score descending, product index ascending) with the failing products taken out, -1 / -inf
 * past its end; the score bits are those of the entry underneath (the predicate reads no score).  It composes with the
 * exclusion lists (both must let a product through) and with an eligibility CSR.  Every array NULL: the entry underneath's
 * output, bit for bit.
 *
 * pc_retrieve_list_grouped_where / _bf16_where / _biased_where / _bf16_biased_where: the contract and argument list of
 * pc_retrieve_list_grouped / _bf16 / _biased / _bf16_biased for every 1 <= n <= 256, with `where` in front of ws.  The kernel
 * body, the merge and the host path are pc_retrieve_list_grouped's own code with the body's filter hook: value[p] and flags[p]
 * are gathered per chunk column a chunk ahead and staged on chip, a candidate that beat the row's threshold is tested before
 * the exclusion search.  Bitwise deterministic and independent of `slices`, of the placement of the rows and of the order of
 * type_col inside a type; no float atomics, no host readback.  The workspace (NAME_workspace_bytes, 0 for arguments out of
 * range) is pc_retrieve_list_grouped's size.
 * PC_EINVAL: a null where; lo or hi without value, value without both; need or deny without flags; and everything the entry
 * underneath answers with PC_EINVAL; PC_ESHAPE and PC_EWORKSPACE as there -- each checked before anything is launched: the
 * outputs are untouched. */
typedef struct pc_row_where {
    const float   *value, *lo, *hi;
    const int32_t *flags, *need, *deny;
} pc_row_where;

size_t pc_retrieve_list_grouped_where_workspace_bytes(int rows, int n_types, int n, int slices);
int pc_retrieve_list_grouped_where(const float *proj, const int32_t *types, const int32_t *row_key, int rows,
                                   const int32_t *type_rowptr, const int32_t *type_col, const float *table, int n_types,
                                   const int32_t *ex_rowptr, const int32_t *ex_col, int n_keys, int n, int dim, int slices,
                                   int32_t *out_idx, float *out_score, int32_t *bad_count, const pc_row_where *where,
                                   void *ws, size_t ws_bytes, void *stream);
size_t pc_retrieve_list_grouped_bf16_where_workspace_bytes(int rows, int n_types, int n, int slices);
int pc_retrieve_list_grouped_bf16_where(const float *proj, const int32_t *types, const int32_t *row_key, int rows,
                                        const int32_t *type_rowptr, const int32_t *type_col, const uint16_t *table_bf16,
                                        int n_types, const int32_t *ex_rowptr, const int32_t *ex_col, int n_keys, int n,
                                        int dim, int slices, int32_t *out_idx, float *out_score, int32_t *bad_count,
                                        const pc_row_where *where, void *ws, size_t ws_bytes, void *stream);
size_t pc_retrieve_list_grouped_biased_where_workspace_bytes(int rows, int n_types, int n, int slices);
int pc_retrieve_list_grouped_biased_where(const float *proj, const int32_t *types, const int32_t *row_key, int rows,
                                          const int32_t *type_rowptr, const int32_t *type_col, const float *table,
                                          const float *bias, int n_types, const int32_t *ex_rowptr, const int32_t *ex_col,
                                          int n_keys, int n, int dim, int slices, int32_t *out_idx, float *out_score,
                                          int32_t *bad_count, const pc_row_where *where, void *ws, size_t ws_bytes,
                                          void *stream);
size_t pc_retrieve_list_grouped_bf16_biased_where_workspace_bytes(int rows, int n_types, int n, int slices);
int pc_retrieve_list_grouped_bf16_biased_where(const float *proj, const int32_t *types, const int32_t *row_key, int rows,
                                               const int32_t *type_rowptr, const int32_t *type_col,
                                               const uint16_t *table_bf16, const float *bias, int n_types,
                                               const int32_t *ex_rowptr, const int32_t *ex_col, int n_keys, int n, int dim,
                                               int slices, int32_t *out_idx, float *out_score, int32_t *bad_count,
                                               const pc_row_where *where, void *ws, size_t ws_bytes, void *stream);

/* Ranks under a predicate (ABI 8, additive; csrc/where_rank.hip, csrc/where_rank_bf16.hip; ops.rank_grouped_where,
 * PCompanionInference.rank_targets_where / evaluate_catalogue_where, SimilarProducts.rank_pairs_where / evaluate_pairs_where):
 * the rank twin of the filtered lists above -- where a known product stands in the list a row is served under its predicate,
 * over the whole type, from the list's own score bits.
 *
 * pc_rank_grouped_where (fp32 table) / pc_rank_grouped_bf16_where (table_bf16): pc_rank_grouped_bf16's argument list -- row_key,
 * a bias that may be NULL (then s = d), the exclusion CSR, cand_type, dim, slices -- with `where` in front of ws.  For row r
 * with type c = types[r], target y = targets[r] and predicate w_r, s the score pc_retrieve_list_grouped[_bf16][_biased]_where
 * gives the pair, bit for bit:
 *   rank_out[r] = #{ p of type c : p passes w_r, p not in the row's list : s_p > s_y or (s_p == s_y and p < y) }.
 * The predicate is pc_row_where's as stated above, unchanged: inclusive fp32 ends, a NaN value or bound passes nothing, lo > hi
 * passes nothing, infinite bounds pass every non-NaN value, -0.0 == 0.0, need / deny on 32 bits, every part optional.
 * rank_out[r] = -1 wherever pc_rank_grouped_bf16 / pc_rank_grouped_biased give -1 -- types[r] < 0; a type or target out of range
 * (counted in *bad_count); with lists, the target in the row's list or cand_type[y] != c -- and where the target itself fails
 * its row's predicate.  row_key, ex_rowptr, ex_col and cand_type all four or none.  So rank_out[r] < n exactly when
 * pc_retrieve_list_grouped[_bf16][_biased]_where with the same lists, bias and table holds y at position rank_out[r]; over rows
 * that share one predicate it is pc_rank_grouped_biased / pc_rank_grouped_bf16 over a type CSR and cand_type rebuilt from the
 * passing products; with every array of the filter NULL it is those entries' output bit for bit.
 * pc_rank_grouped's plan and work items; the test sits inside the count: value[p] and flags[p] are gathered per chunk column a
 * chunk ahead with the product id, the rows' lo / hi / need / deny are staged on chip once per work item, a candidate is counted
 * where it beats (or ties and precedes) the target AND passes that row's predicate.  A row post-pass (one wave per row, in every
 * call) writes the -1 of a failing target after all slices' counts have landed and, with lists, takes out the list entries that
 * pass the predicate and were counted.  Integer counts, one integer atomic per (row, slice); bitwise deterministic, the same for
 * every `slices`, placement of the rows and order of type_col inside a type; no float atomics, no host readback.
 * Workspace: NAME_workspace_bytes(rows, n_types, slices) = pc_rank_grouped_workspace_bytes.
 * PC_EINVAL: a null where; lo or hi without value, value without both; need or deny without flags; a null pointer (bias apart),
 * rows, n_types or num_products <= 0, n_keys < 0, half-given exclusion arguments; PC_ESHAPE: dim not 128 / 256, slices outside
 * [0, 64], table_bf16 not 16-byte aligned; PC_EWORKSPACE: ws_bytes too small -- each checked before anything is launched: the
 * outputs are untouched. */
size_t pc_rank_grouped_where_workspace_bytes(int rows, int n_types, int slices);
int pc_rank_grouped_where(const float *proj, const int32_t *types, const int32_t *targets, const int32_t *row_key, int rows,
                          const int32_t *type_rowptr, const int32_t *type_col, const float *table, const float *bias,
                          int n_types, int num_products, const int32_t *ex_rowptr, const int32_t *ex_col, int n_keys,
                          const int32_t *cand_type, int dim, int slices, int32_t *rank_out, int32_t *bad_count,
                          const pc_row_where *where, void *ws, size_t ws_bytes, void *stream);
size_t pc_rank_grouped_bf16_where_workspace_bytes(int rows, int n_types, int slices);
int pc_rank_grouped_bf16_where(const float *proj, const int32_t *types, const int32_t *targets, const int32_t *row_key,
                               int rows, const int32_t *type_rowptr, const int32_t *type_col, const uint16_t *table_bf16,
                               const float *bias, int n_types, int num_products, const int32_t *ex_rowptr,
                               const int32_t *ex_col, int n_keys, const int32_t *cand_type, int dim, int slices,
                               int32_t *rank_out, int32_t *bad_count, const pc_row_where *where, void *ws, size_t ws_bytes,
                               void *stream);

/* Score moments (ABI 8, additive; csrc/score_moments.hip, csrc/score_moments_bf16.hip; ops.score_moments_grouped,
 * PCompanionInference.score_moments and the normalise="zscore" keyword of the serving methods): the mean and the standard
 * deviation of a row's scores over ALL candidates of its type -- what a served score is standardised against before the lists of
 * different types are merged into a page or fused into a basket's list, whose raw dot products differ in scale from type to type.
 *
 * pc_score_moments_grouped (fp32 table) / pc_score_moments_grouped_bf16 (table_bf16): pc_rank_grouped's rows, type CSR, dim and
 * slices, without targets.  For row r with type c = types[r], n = type_rowptr[c+1] - type_rowptr[c] candidates, s the score
 * pc_retrieve_list_grouped[_bf16] gives a (row, product) pair, bit for bit, and the pivot g = s of the type's FIRST candidate
 * type_col[type_rowptr[c]]:
 *   count[r] = n,   pivot[r] = g,   s1[r] = sum_p fl(s_p - g),   s2[r] = sum_p fl(s_p - g)^2   over the products p of type c,
 *   mean[r] = g + s1 / n,   std[r] = sqrt(max(s2 / n - (s1 / n)^2, 0))   (the population form; fp32, one rounding per operation
 *   in this order, nothing fused).
 * The sums are centred on a score of the type itself, so s2 carries no term of the size of mean^2 and keeps its digits where
 * |mean| >> std.  types[r] < 0 ("no type matched"): the row is skipped, count 0 and zeros.  A type >= n_types never reaches
 * memory: count 0 and zeros, and *bad_count (a device counter the caller owns) is incremented.  An empty type: count 0 and zeros.
 * pc_rank_grouped's plan and work items and its kernel's shape -- the pivot formed as the rank forms its target's score, the
 * candidates through the same chain -- with a subtraction, an addition and a fused multiply-add per (row, candidate) where the
 * rank compares and counts; the (row, slice) partial sums go to the workspace as plain stores and a finishing kernel adds them
 * in slice order.  No float atomics, no host readback.  Bitwise reproducible from run to run for a given `slices`; across
 * different `slices`, or orders of type_col inside a type (its first entry apart: the pivot), the fp32 sums may differ in their
 * last bits -- unlike the rank's integer count -- and are identical where every sum is exact.
 * Workspace: pc_score_moments_grouped_workspace_bytes(rows, n_types, slices), for both entries (0 for arguments out of range).
 * PC_EINVAL: null pointer, rows or n_types <= 0; PC_ESHAPE: dim not 128 / 256, slices outside [0, 64], table_bf16 not 16-byte
 * aligned; PC_EWORKSPACE: ws_bytes too small -- each checked before anything is launched: the outputs are untouched. */
size_t pc_score_moments_grouped_workspace_bytes(int rows, int n_types, int slices);
int pc_score_moments_grouped(const float *proj, const int32_t *types, int rows, const int32_t *type_rowptr,
                             const int32_t *type_col, const float *table, int n_types, int dim, int slices, int32_t *count,
                             float *pivot, float *s1, float *s2, float *mean, float *std_out, int32_t *bad_count, void *ws,
                             size_t ws_bytes, void *stream);
int pc_score_moments_grouped_bf16(const float *proj, const int32_t *types, int rows, const int32_t *type_rowptr,
                                  const int32_t *type_col, const uint16_t *table_bf16, int n_types, int dim, int slices,
                                  int32_t *count, float *pivot, float *s1, float *s2, float *mean, float *std_out,
                                  int32_t *bad_count, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif
