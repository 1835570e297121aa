"""Tensor-level wrappers over the C ABI (include/pcompanion_hip.h).

torch is used here for device memory and the current stream only: every computation is a
HIP kernel of libpcompanion_hip.so.  All tensors must be CUDA(ROCm), contiguous, fp32 /
int32; anything else raises (no silent conversion on the hot path, no CPU fallback).
"""
import ctypes
from typing import NamedTuple

import numpy as np
import torch

from . import _lib
from ._lib import D, H, HEADS, L, PC_MAX_SEG, AttnSaved, FfnSaved, JointSaved, JointTensors, P2VTensors, Segments, check

P2V_KEYS = ("ffn.0.weight", "ffn.0.bias", "ffn.1.weight", "ffn.1.bias", "ffn.3.weight", "ffn.3.bias",
            "ffn.5.weight", "ffn.5.bias", "attention.in_proj_weight", "attention.in_proj_bias",
            "attention.out_proj.weight", "attention.out_proj.bias")
P2V_FIELDS = ("w0", "b0", "gamma", "beta", "w3", "b3", "w5", "b5", "in_proj_w", "in_proj_b", "out_proj_w",
              "out_proj_b")
P2V_SHAPES = ((H, D), (H,), (H,), (H,), (H, H), (H,), (D, H), (D,), (3 * D, D), (3 * D,), (D, D), (D,))
P2V_BUFFERS = (("ffn.1.running_mean", "running_mean"), ("ffn.1.running_var", "running_var"),
               ("ffn.1.num_batches_tracked", "num_batches_tracked"))

JOINT_KEYS = ("type_transition.encoder.weight", "type_transition.encoder.bias",
              "type_transition.decoder.weight", "type_transition.decoder.bias",
              "item_prediction.type_projection.weight", "item_prediction.type_projection.bias",
              "item_prediction.item_projection.weight", "item_prediction.item_projection.bias",
              "query_type_embeddings.weight", "complementary_type_embeddings.weight")
JOINT_FIELDS = ("enc_w", "enc_b", "dec_w", "dec_b", "typ_w", "typ_b", "itm_w", "itm_b", "query_types",
                "comp_types")


def _req(t, dtype, name, shape=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise TypeError(f"{name}: expected a CUDA/ROCm tensor (the HIP path has no CPU fallback)")
    if t.dtype != dtype:
        raise TypeError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


_ws_cache = {}


def _default_alloc(n, dtype, device, zero=False):
    return (torch.zeros if zero else torch.empty)(int(n), dtype=dtype, device=device)


# Every device buffer the kernels WRITE through this package's own allocations -- workspaces (slabs included), the flat
# parameter / gradient / moment buffers, the fixed batch and output buffers of the prepared steps -- comes from this hook.
# tests/test_gpu_soak.py swaps in an allocator that brackets each buffer with sentinel-filled guard bands and checks them
# after hundreds of thousands of steps; production code never touches it.
_allocator = _default_alloc


def alloc(n, dtype, device, zero=False):
    return _allocator(n, dtype, device, zero)


def workspace(nbytes, device, tag="ws"):
    """Grow-only scratch buffer per (device, stream, tag); contents never outlive a call."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream, tag, _allocator)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = alloc(max(int(nbytes), 256), torch.uint8, device)
        _ws_cache[key] = buf
    return buf


def make_segments(starts, rows, row_weight=None, counts=None):
    """starts: row starts of each BatchNorm call group, e.g. [0, B, B+B*N]; rows = total.
    row_weight (optional): fp32 device tensor [rows], how many identical logical rows each row stands for (0 = the row enters no
    statistic); counts (optional): the logical row count of each group, i.e. what BatchNorm divides by (0 = its physical rows)."""
    if not 1 <= len(starts) <= PC_MAX_SEG:
        raise ValueError("1..4 segments")
    s = Segments()
    s.weighted_row = -1
    s.weight = 1.0
    s.nseg = len(starts)
    arr = list(starts) + [rows] * (PC_MAX_SEG + 1 - len(starts))
    for i, v in enumerate(arr):
        s.start[i] = int(v)
    if counts is not None:
        if len(counts) != s.nseg or any(int(c) < 0 for c in counts):
            raise ValueError("counts: one non-negative logical row count per segment")
        for i, c in enumerate(counts):
            s.count[i] = int(c)
    if row_weight is not None:
        _req(row_weight, torch.float32, "row_weight", (rows,))
        s.row_weight, s.row_weight_start, s.row_weight_rows = row_weight.data_ptr(), 0, rows
    for i in range(s.nseg):
        n = s.count[i] if s.count[i] > 0 else s.start[i + 1] - s.start[i]
        if n == 1:
            # nn.BatchNorm1d raises the same in training mode (torch/nn/functional.py _verify_batch_size)
            raise ValueError("Expected more than 1 value per channel when training, got input size "
                             f"torch.Size([1, {H}])")
    return s


def p2v_shapes(d=D):
    """Parameter shapes of product2vec.py:14-29 for PRODUCT_EMB_DIM = d (128, or 256: BASELINE configs[4]); HIDDEN_SIZE
    stays 256."""
    return ((H, d), (H,), (H,), (H,), (H, H), (H,), (d, H), (d,), (3 * d, d), (3 * d,), (d, d), (d,))


def p2v_dim(tensors):
    d = int(tensors["ffn.0.weight"].shape[1])
    if d not in (128, 256):
        raise ValueError(f"the gfx950 kernels are built for PRODUCT_EMB_DIM 128 or 256, got {d}")
    return d


def p2v_struct(tensors, with_buffers=True):
    """tensors: mapping reference-state_dict-key -> tensor (parameters or gradients)."""
    st = P2VTensors()
    dev = None
    d = p2v_dim(tensors)
    st.dim = d
    for key, field, shape in zip(P2V_KEYS, P2V_FIELDS, p2v_shapes(d)):
        t = _req(tensors[key], torch.float32, key, shape)
        dev = t.device
        setattr(st, field, t.data_ptr())
    if with_buffers:
        for key, field in P2V_BUFFERS:
            t = tensors.get(key)
            if t is not None:
                _req(t, torch.int64 if "num_batches" in key else torch.float32, key)
                setattr(st, field, t.data_ptr())
    _set_dropout(st, tensors.get(DROPOUT_KEY))
    return st, dev


DROPOUT_KEY = "__dropout__"      # optional entry of a tensor dict: (p, seed, offset) of the module's training-mode dropout


def _set_dropout(st, d):
    if d is not None and float(d[0]) > 0.0:
        if not 0.0 < float(d[0]) < 1.0:
            raise ValueError(f"dropout probability has to be between 0 and 1, but got {d[0]}")
        st.dropout.p, st.dropout.seed, st.dropout.offset = float(d[0]), int(d[1]), int(d[2])


def _new_p2v_grads(device, d=D):
    return {k: torch.empty(s, dtype=torch.float32, device=device) for k, s in zip(P2V_KEYS, p2v_shapes(d))}


# ----------------------------------------------------------------------------- P6
def ffn_forward_train(params, table, idx, rows, seg_starts, update_running=True, row_weight=None, counts=None):
    """Product2Vec.get_initial_embedding in training mode over `rows` rows made of
    len(seg_starts) BatchNorm call groups.  Returns (y[rows,D], saved).
    row_weight / counts: see make_segments (pc_segments' row multiplicities and logical counts); the backward reads them from
    `saved`.  A row of weight 0 still gets its y, but BatchNorm's statistics do not see it."""
    st, dev = p2v_struct(params)
    _req(table, torch.float32, "table")
    if idx is not None:
        _req(idx, torch.int32, "idx", (rows,))
    seg = make_segments(seg_starts, rows, row_weight, counts)
    y = torch.empty(rows, st.dim, dtype=torch.float32, device=dev)
    sv = {"h0": torch.empty(rows, H, dtype=torch.float32, device=dev),
          "a2": torch.empty(rows, H, dtype=torch.float32, device=dev),
          "a1": torch.empty(rows, H, dtype=torch.float32, device=dev),      # tanh(BN(h0)): written by Linear3's kernel, read by dW3
          "bn": torch.empty(4, PC_MAX_SEG, H, dtype=torch.float32, device=dev),
          "seg_starts": list(seg_starts), "rows": rows, "row_weight": row_weight,
          "counts": None if counts is None else list(counts)}
    nbytes = _lib.lib().pc_p2v_ffn_workspace_bytes(rows)
    ws = workspace(nbytes, dev)
    check(_lib.lib().pc_p2v_ffn_forward_train(ctypes.byref(st), _p(table), _p(idx), rows, ctypes.byref(seg),
                                              1 if update_running else 0, _p(y), ctypes.byref(_ffn_saved(sv)),
                                              _p(ws), nbytes, _stream()), "pc_p2v_ffn_forward_train")
    return y, sv


def _ffn_saved(sv):
    s = FfnSaved()
    s.h0, s.a2 = sv["h0"].data_ptr(), sv["a2"].data_ptr()
    s.a1 = sv["a1"].data_ptr() if sv.get("a1") is not None else None
    bn = sv["bn"]
    s.bn_mean, s.bn_invstd, s.bn_scale, s.bn_shift = (bn[i].data_ptr() for i in range(4))
    return s


def ffn_forward_eval(params, table, idx, rows):
    st, dev = p2v_struct(params)
    _req(table, torch.float32, "table")
    if idx is not None:
        _req(idx, torch.int32, "idx", (rows,))
    y = torch.empty(rows, st.dim, dtype=torch.float32, device=dev)
    nbytes = _lib.lib().pc_p2v_ffn_workspace_bytes(rows)
    ws = workspace(nbytes, dev)
    check(_lib.lib().pc_p2v_ffn_forward_eval(ctypes.byref(st), _p(table), _p(idx), rows, _p(y), _p(ws), nbytes,
                                             _stream()), "pc_p2v_ffn_forward_eval")
    return y


def ffn_backward(params, table, idx, dy, sv, need_dx=False, grads=None, accumulate=False):
    st, dev = p2v_struct(params)
    rows = sv["rows"]
    d = st.dim
    _req(dy, torch.float32, "dy", (rows, d))
    if grads is None:
        grads = _new_p2v_grads(dev, d)
        accumulate = False
    gst, _ = p2v_struct(grads, with_buffers=False)
    seg = make_segments(sv["seg_starts"], rows, sv.get("row_weight"), sv.get("counts"))
    dx = torch.empty(rows, d, dtype=torch.float32, device=dev) if need_dx else None
    nbytes = _lib.lib().pc_p2v_ffn_workspace_bytes(rows)
    ws = workspace(nbytes, dev)
    check(_lib.lib().pc_p2v_ffn_backward(ctypes.byref(st), ctypes.byref(gst), _p(table), _p(idx), rows,
                                         ctypes.byref(seg), _p(dy), ctypes.byref(_ffn_saved(sv)), _p(dx),
                                         1 if accumulate else 0, _p(ws), nbytes, _stream()), "pc_p2v_ffn_backward")
    return grads, dx


# ----------------------------------------------------------------------------- P7
def _attn_saved(sv):
    s = AttnSaved()
    s.q, s.qt, s.probs, s.c, s.sp, s.ctx = (sv[k].data_ptr() for k in ("q", "qt", "probs", "c", "sp", "ctx"))
    return s


def _key_pad(key_pad, b, n):
    """A [B,N] key-padding mask (bool or uint8, nonzero / True = padding) as the uint8 tensor the masked kernels read."""
    if not isinstance(key_pad, torch.Tensor) or not key_pad.is_cuda:
        raise TypeError("key_pad: expected a CUDA/ROCm tensor (the HIP path has no CPU fallback)")
    if key_pad.dtype not in (torch.bool, torch.uint8):
        raise TypeError(f"key_pad: expected torch.bool or torch.uint8, got {key_pad.dtype}")
    if tuple(key_pad.shape) != (b, n):
        raise ValueError(f"key_pad: expected shape {(b, n)}, got {tuple(key_pad.shape)}")
    kp = key_pad.contiguous()
    return kp.view(torch.uint8) if kp.dtype == torch.bool else kp


def attention_forward(params, query, keys, key_pad=None):
    """query [B,D], keys [B,N,D] -> out [B,D], saved.
    key_pad (optional, [B,N] bool / uint8, True = padding): the key-padding mask, a labelled deviation from the reference
    (pc_p2v_attention_forward_masked): padding slots are no keys, a sample without a real slot gets out_proj.bias."""
    st, dev = p2v_struct(params)
    b, n, _ = keys.shape
    d = st.dim
    _req(query, torch.float32, "query", (b, d))
    _req(keys, torch.float32, "keys", (b, n, d))
    out = torch.empty(b, d, dtype=torch.float32, device=dev)
    sv = {"q": torch.empty(b, d, dtype=torch.float32, device=dev),
          "qt": torch.empty(b, HEADS, d, dtype=torch.float32, device=dev),      # Wk_h^T q_h: the key projection, absorbed
          "c": torch.empty(b, HEADS, d, dtype=torch.float32, device=dev),       # sum_n pm_n key_n per head (value projection follows)
          "sp": torch.empty(b, HEADS, dtype=torch.float32, device=dev),
          "probs": torch.empty(b, HEADS, n, dtype=torch.float32, device=dev),
          "ctx": torch.empty(b, d, dtype=torch.float32, device=dev)}
    nbytes = _lib.lib().pc_p2v_attention_workspace_bytes_dim(b, n, d)
    ws = workspace(nbytes, dev)
    if key_pad is not None:
        sv["key_pad"] = _key_pad(key_pad, b, n)
        check(_lib.lib().pc_p2v_attention_forward_masked(ctypes.byref(st), _p(query), _p(keys), _p(sv["key_pad"]), b, n, _p(out),
                                                         ctypes.byref(_attn_saved(sv)), _p(ws), nbytes, _stream()),
              "pc_p2v_attention_forward_masked")
        return out, sv
    check(_lib.lib().pc_p2v_attention_forward(ctypes.byref(st), _p(query), _p(keys), b, n, _p(out),
                                              ctypes.byref(_attn_saved(sv)), _p(ws), nbytes, _stream()),
          "pc_p2v_attention_forward")
    return out, sv


def attention_backward(params, query, keys, dout, sv, grads=None, accumulate=False, key_pad=None):
    """key_pad: the mask of the forward call (default: the one that call saved); dkeys of padding slots are zeros."""
    st, dev = p2v_struct(params)
    b, n, _ = keys.shape
    d = st.dim
    _req(dout, torch.float32, "dout", (b, d))
    if grads is None:
        grads = _new_p2v_grads(dev, d)
        accumulate = False
    gst, _ = p2v_struct(grads, with_buffers=False)
    dq = torch.empty(b, d, dtype=torch.float32, device=dev)
    dk = torch.empty(b, n, d, dtype=torch.float32, device=dev)
    nbytes = _lib.lib().pc_p2v_attention_workspace_bytes_dim(b, n, d)
    ws = workspace(nbytes, dev)
    kp = _key_pad(key_pad, b, n) if key_pad is not None else sv.get("key_pad")
    if kp is not None:
        check(_lib.lib().pc_p2v_attention_backward_masked(ctypes.byref(st), ctypes.byref(gst), _p(query), _p(keys), _p(kp), b, n,
                                                          _p(dout), ctypes.byref(_attn_saved(sv)), _p(dq), _p(dk),
                                                          1 if accumulate else 0, _p(ws), nbytes, _stream()),
              "pc_p2v_attention_backward_masked")
        return grads, dq, dk
    check(_lib.lib().pc_p2v_attention_backward(ctypes.byref(st), ctypes.byref(gst), _p(query), _p(keys), b, n,
                                               _p(dout), ctypes.byref(_attn_saved(sv)), _p(dq), _p(dk),
                                               1 if accumulate else 0, _p(ws), nbytes, _stream()),
          "pc_p2v_attention_backward")
    return grads, dq, dk


# ----------------------------------------------------------------------------- P9 / P10
def triplet_loss(a, p, n, margin, need_grad=True):
    """a,p [B,D]; n [B,K,D].  Returns dict(loss[1], d_pos[B], d_neg[B], da, dp, dn)."""
    b, k, d = n.shape
    if d not in (128, 256):
        raise ValueError(f"embedding width {d}: the gfx950 kernels serve 128 and 256")
    _req(a, torch.float32, "anchor_emb", (b, d)); _req(p, torch.float32, "positive_emb", (b, d))
    _req(n, torch.float32, "negative_emb", (b, k, d))
    dev = a.device
    out = {"loss": torch.empty(1, dtype=torch.float32, device=dev),
           "d_pos": torch.empty(b, dtype=torch.float32, device=dev),
           "d_neg": torch.empty(b, dtype=torch.float32, device=dev)}
    if need_grad:
        out.update(da=torch.empty_like(a), dp=torch.empty_like(p), dn=torch.empty_like(n))
    check(_lib.lib().pc_p2v_triplet_loss_dim(_p(a), _p(p), _p(n), b, k, d, float(margin), _p(out["loss"]),
                                             _p(out["d_pos"]), _p(out["d_neg"]), _p(out.get("da")), _p(out.get("dp")),
                                             _p(out.get("dn")), _stream()), "pc_p2v_triplet_loss_dim")
    return out


def _adam_buffers(what, param, grad, exp_avg, exp_avg_sq, step_count):
    """The flat-buffer check of adam_step / adam_step_at: four float32 tensors of one size, an int64 step count.  Returns the size."""
    n = param.numel()
    for t, nm in ((param, "param"), (grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _req(t, torch.float32, nm)
        if t.numel() != n:
            raise ValueError(f"{what}: size mismatch")
    _req(step_count, torch.int64, "step_count")
    return n


def adam_step(param, grad, exp_avg, exp_avg_sq, step_count, scalars, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
    n = _adam_buffers("adam_step", param, grad, exp_avg, exp_avg_sq, step_count)
    _req(scalars, torch.float32, "scalars", (2,))
    check(_lib.lib().pc_adam_step(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), n, _p(step_count), _p(scalars),
                                  float(lr), float(betas[0]), float(betas[1]), float(eps), _stream()), "pc_adam_step")


def adam_step_at(param, grad, exp_avg, exp_avg_sq, step_count, t, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
    """pc_adam_step_at: the update of step number t (host-known) as one launch; step_count (device int64 [1]) is left = t."""
    n = _adam_buffers("adam_step_at", param, grad, exp_avg, exp_avg_sq, step_count)
    check(_lib.lib().pc_adam_step_at(_p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), n, _p(step_count), int(t), float(lr),
                                     float(betas[0]), float(betas[1]), float(eps), _stream()), "pc_adam_step_at")


# ----------------------------------------------------------------------------- data-parallel exchange slot (ABI 6)
# A pc_exchange_fn travels through ctypes as a plain address (fn) with its context (ctx): the native one is the library's own
# pc_rccl_allreduce_mean over its own RCCL communicator -- no Python between a step's gradient kernels and its Adam launch;
# CallbackExchange wraps a Python callable for backends RCCL does not serve (gloo in the tests).
EXCHANGE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p)


class ExchangePlan(ctypes.Structure):
    """pc_exchange_plan (ABI 8): the plain exchange (all_reduce_mean) and the two halves of the sharded optimizer's."""
    _fields_ = [("all_reduce_mean", ctypes.c_void_p), ("reduce_scatter_mean", ctypes.c_void_p), ("all_gather", ctypes.c_void_p),
                ("ctx", ctypes.c_void_p), ("rank", ctypes.c_int), ("world", ctypes.c_int), ("shard_optimizer", ctypes.c_int)]


class Exchange:
    fn = None       # ctypes.c_void_p: address of a pc_exchange_fn
    ctx = None      # ctypes.c_void_p
    rs_fn = ag_fn = None      # ctypes.c_void_p: addresses of the pc_shard_collective_fn pair (None: no sharded form)
    rank, world = 0, 1

    def plan(self, shard=False):
        """The pc_exchange_plan of this exchange (kept alive by the caller for the duration of the foreign call).
        shard=True: reduce-scatter -> Adam on this rank's slice -> all-gather (needs the sharded pair)."""
        if shard and (self.rs_fn is None or self.ag_fn is None):
            raise ValueError("this exchange has no reduce-scatter / all-gather pair")
        val = lambda f: f.value if f is not None else None
        return ExchangePlan(val(self.fn), val(self.rs_fn), val(self.ag_fn), val(self.ctx), int(self.rank), int(self.world),
                            1 if shard else 0)

    def all_reduce_mean_(self, t):
        """The exchange applied to a device tensor, in place, on the current stream (what a step's call does through the slot)."""
        _req(t, torch.float32, "grad")
        rc = EXCHANGE_FN(self.fn.value)(self.ctx, _p(t), t.numel(), _stream())
        check(rc, "pc_exchange_fn")
        return t

    def all_gather_(self, t):
        """The all-gather half of the sharded pair applied to a device tensor of world equal slices, in place, on the current
        stream: every rank's slice `rank` -> all ranks' t (FusedAdam.gather_state: the moments of a sharded optimizer)."""
        _req(t, torch.float32, "buf")
        if self.ag_fn is None:
            raise ValueError("this exchange has no reduce-scatter / all-gather pair")
        if t.numel() % self.world:
            raise ValueError("all_gather_: a multiple of the world size")
        rc = EXCHANGE_FN(self.ag_fn.value)(self.ctx, _p(t), t.numel() // self.world, _stream())
        if rc and isinstance(self, CallbackExchange):
            self.reraise()
        check(rc, "pc_shard_collective_fn (all_gather)")
        return t


def rccl_available():
    return bool(_lib.lib().pc_rccl_available())


class RcclExchange(Exchange):
    """The library's own RCCL communicator (pc_rccl_*): ncclAllReduce(ncclAvg) behind the exchange slot, plus the step's
    other collectives -- all_to_all (the row-sharded table's two lookup rounds) and all_reduce_sum_f64_ (cross-replica
    BatchNorm sums) -- so that everything a step exchanges runs on ONE communicator, chained inside the library when two of
    them sit on different streams (include/pcompanion_hip.h, "ORDER").  One rank draws the unique id
    (RcclExchange.unique_id()), every rank constructs with the same 128 bytes -- a collective (ncclCommInitRank) on the
    current device."""

    @staticmethod
    def unique_id():
        buf = ctypes.create_string_buffer(128)
        check(_lib.lib().pc_rccl_unique_id(buf), "pc_rccl_unique_id")
        return buf.raw

    def __init__(self, unique_id, rank, world):
        if len(unique_id) != 128:
            raise ValueError("RcclExchange: a 128-byte ncclUniqueId")
        L = _lib.lib()
        h = ctypes.c_void_p()
        check(L.pc_rccl_comm_create(ctypes.c_char_p(bytes(unique_id)), int(rank), int(world), ctypes.byref(h)), "pc_rccl_comm_create")
        self.ctx = h
        self.fn = ctypes.cast(L.pc_rccl_allreduce_mean, ctypes.c_void_p)
        self.rs_fn = ctypes.cast(L.pc_rccl_reduce_scatter_mean, ctypes.c_void_p)
        self.ag_fn = ctypes.cast(L.pc_rccl_all_gather, ctypes.c_void_p)
        self.rank, self.world = int(rank), int(world)
        self.kind = "rccl (library-owned communicator, ncclAvg)"

    def close(self):
        if self.ctx is not None and self.ctx.value:
            torch.cuda.synchronize()
            check(_lib.lib().pc_rccl_comm_destroy(self.ctx), "pc_rccl_comm_destroy")
            self.ctx = None

    def all_to_all(self, send, recv):
        """pc_rccl_alltoall on the current stream: equal splits, peer p's slice of `send` lands in peer p's `recv` at this
        rank's slot.  Any dtype; both contiguous device tensors of the same byte size, a multiple of the world size."""
        nbytes = send.numel() * send.element_size()
        if not (send.is_cuda and recv.is_cuda and send.is_contiguous() and recv.is_contiguous()):
            raise ValueError("all_to_all: contiguous device tensors")
        if recv.numel() * recv.element_size() != nbytes or nbytes % self.world or send.data_ptr() == recv.data_ptr():
            raise ValueError("all_to_all: send / recv of equal size (a multiple of the world size), not aliased")
        check(_lib.lib().pc_rccl_alltoall(self.ctx, _p(send), _p(recv), nbytes // self.world, _stream()), "pc_rccl_alltoall")
        return recv

    def all_reduce_sum_f64_(self, t):
        """pc_rccl_allreduce_sum_f64 on the current stream (cross-replica BatchNorm: ops.p2v_train_step(sync_reduce=...))."""
        _req(t, torch.float64, "buf")
        check(_lib.lib().pc_rccl_allreduce_sum_f64(self.ctx, _p(t), t.numel(), _stream()), "pc_rccl_allreduce_sum_f64")
        return t

    def reduce_scatter_mean_(self, t):
        """pc_rccl_reduce_scatter_mean on the current stream: slice `rank` of t <- the mean over the ranks of that slice."""
        _req(t, torch.float32, "buf")
        if t.numel() % self.world:
            raise ValueError("reduce_scatter_mean_: a multiple of the world size")
        check(_lib.lib().pc_rccl_reduce_scatter_mean(self.ctx, _p(t), t.numel() // self.world, _stream()), "pc_rccl_reduce_scatter_mean")
        return t

    def all_gather_(self, t):
        """pc_rccl_all_gather on the current stream: every rank's slice `rank` of t -> all ranks' t."""
        _req(t, torch.float32, "buf")
        if t.numel() % self.world:
            raise ValueError("all_gather_: a multiple of the world size")
        check(_lib.lib().pc_rccl_all_gather(self.ctx, _p(t), t.numel() // self.world, _stream()), "pc_rccl_all_gather")
        return t

    def stats(self):
        """{collectives issued on the communicator, cross-stream waits the library inserted between them}."""
        a, b = ctypes.c_int64(0), ctypes.c_int64(0)
        check(_lib.lib().pc_rccl_comm_stats(self.ctx, ctypes.byref(a), ctypes.byref(b)), "pc_rccl_comm_stats")
        return {"issued": int(a.value), "chained": int(b.value)}


class CallbackExchange(Exchange):
    """A Python callable behind the slot: pyfn(ptr, n, stream) must leave the mean over the replicas in the n floats at
    device address ptr, ordered on the stream (it may block).  An exception inside is reported as PC_ECOMM and re-raised by
    the wrapper that made the call."""

    def __init__(self, pyfn, kind="python callback", reduce_scatter=None, all_gather=None, rank=0, world=1):
        """reduce_scatter / all_gather (optional): pyfn-style callables (ptr, n_per_rank, stream) for the sharded optimizer's
        two halves over the buffer at device address ptr (world * n_per_rank floats)."""
        self.error = None

        def wrap(f):
            def tramp(_ctx, buf, n, stream):
                try:
                    f(int(buf or 0), int(n), int(stream or 0))
                    return 0
                except BaseException as e:            # noqa: BLE001 -- nothing may unwind through the C frames
                    self.error = e
                    return -5
            return EXCHANGE_FN(tramp)

        self._tramp = wrap(pyfn)                      # (kept alive with the object: the C side holds a bare address)
        self.fn = ctypes.cast(self._tramp, ctypes.c_void_p)
        if reduce_scatter is not None and all_gather is not None:
            self._tramp_rs, self._tramp_ag = wrap(reduce_scatter), wrap(all_gather)
            self.rs_fn = ctypes.cast(self._tramp_rs, ctypes.c_void_p)
            self.ag_fn = ctypes.cast(self._tramp_ag, ctypes.c_void_p)
        self.rank, self.world = int(rank), int(world)
        self.ctx = ctypes.c_void_p(0)
        self.kind = kind

    def reraise(self):
        e, self.error = self.error, None
        if e is not None:
            raise e


def exchange_adam(exchange, param, grad, exp_avg, exp_avg_sq, step_count, t, scalars, lr=1e-3, betas=(0.9, 0.999), eps=1e-8,
                  shard=False):
    """pc_exchange_adam: the replicas' mean gradient (exchange may be None: single process), then Adam -- optimizer.step() of a
    replica as one foreign call.  t >= 1: the host-known step number; t == 0: the device counter (scalars required).
    shard=True (pc_exchange_adam_plan, ABI 8): reduce-scatter of the flat gradient, Adam on this rank's 1/world of the flat
    buffers, all-gather of the updated parameters; the buffers' length must be a multiple of 4 * exchange.world (world slices,
    each a whole number of the Adam kernel's 16-byte chunks: the library answers PC_ESHAPE on every rank, before the
    reduce-scatter, for slices that are not)."""
    n = param.numel()
    if shard:
        if exchange is None:
            raise ValueError("exchange_adam(shard=True) needs an exchange")
        for x, nm in ((param, "param"), (grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
            _req(x, torch.float32, nm, (n,))
        if n % exchange.world:
            raise ValueError(f"exchange_adam(shard=True): {n} floats are not a multiple of the world size {exchange.world}; pad "
                             f"the flat buffers to a multiple of 4 * world = {4 * exchange.world} "
                             "(flatten_parameters(pad_multiple=4 * world): 16-byte aligned slices)")
        _req(step_count, torch.int64, "step_count")
        plan = exchange.plan(shard=True)
        rc = _lib.lib().pc_exchange_adam_plan(ctypes.byref(plan), _p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), n, _p(step_count),
                                              int(t), _p(scalars), float(lr), float(betas[0]), float(betas[1]), float(eps), _stream())
        if rc and isinstance(exchange, CallbackExchange):
            exchange.reraise()
        check(rc, "pc_exchange_adam_plan")
        return
    for x, nm in ((param, "param"), (grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _req(x, torch.float32, nm)
        if x.numel() != n:
            raise ValueError("exchange_adam: size mismatch")
    _req(step_count, torch.int64, "step_count")
    rc = _lib.lib().pc_exchange_adam(exchange.fn if exchange is not None else None, exchange.ctx if exchange is not None else None,
                                     _p(param), _p(grad), _p(exp_avg), _p(exp_avg_sq), n, _p(step_count), int(t), _p(scalars),
                                     float(lr), float(betas[0]), float(betas[1]), float(eps), _stream())
    if rc and isinstance(exchange, CallbackExchange):
        exchange.reraise()
    check(rc, "pc_exchange_adam")


class KernelProfile:
    """HIP-event brackets around the GEMM launches of the fused step (bench.py roofline leg)."""
    KINDS = {"gemm_nt_kernel": 0, "gemm_tn_kernel": 1, "gemm_nt_small_kernel": 2}

    def __init__(self, capacity):
        self.handle = ctypes.c_void_p()
        check(_lib.lib().pc_profile_create(int(capacity), ctypes.byref(self.handle)), "pc_profile_create")

    def reset(self):
        check(_lib.lib().pc_profile_reset(self.handle), "pc_profile_reset")

    def set_kinds(self, names):
        """Record only the brackets of these kernel families (each bracket costs two event packets)."""
        mask = 0
        for n in names:
            mask |= 1 << self.KINDS[n]
        check(_lib.lib().pc_profile_set_kinds(self.handle, mask), "pc_profile_set_kinds")

    def summary(self, kind):
        n, ms, fl = ctypes.c_int(), ctypes.c_double(), ctypes.c_double()
        check(_lib.lib().pc_profile_summary(self.handle, self.KINDS[kind], ctypes.byref(n), ctypes.byref(ms),
                                            ctypes.byref(fl)), "pc_profile_summary")
        return {"launches": n.value, "total_ms": ms.value, "total_flops": fl.value}

    def close(self):
        if self.handle:
            _lib.lib().pc_profile_destroy(self.handle)
            self.handle = ctypes.c_void_p()


BN_SYNC_DOUBLES = PC_MAX_SEG * 2 * H + PC_MAX_SEG


def p2v_train_step(params, grads, table, anchor_idx, positive_idx, negative_idx, neighbor_idx, margin,
                   want_emb=False, profile=None, sync_reduce=None, adam=None, structs=None, masked=False):
    """One loop-body iteration of Product2Vec.train_model in index form (grads overwritten).

    sync_reduce: None = BatchNorm statistics of this batch; else a callable `reduce(buf)` that sums a
    [BN_SYNC_DOUBLES] float64 device tensor over the data-parallel replicas in place (e.g.
    `lambda t: dist.all_reduce(t)`): the step then runs as pc_p2v_train_step_compact_sync's three phases
    with batch-wide (cross-replica) BatchNorm statistics.  Compact neighbour layout only.

    adam (unique-neighbour layout, no sync_reduce): {"param", "grad", "exp_avg", "exp_avg_sq" (the flat buffers `grads` are views
    of), "step_count", "t" >= 1, "lr", "betas", "eps"} -- torch.optim.Adam's update inside the step's last gradient launch
    (pc_p2v_train_step_unique_adam): optimizer.step() costs no launch of its own.

    structs: (st, gst, dev) built earlier by p2v_struct over the SAME tensors (a training loop whose parameters are views of
    fixed flat buffers builds them once: ~25 tensor checks per step less between a drained device and the step's first launch);
    the dropout entry of `params` is applied to it per call.

    masked: the key-padding mask, a labelled deviation from the reference (pc_p2v_train_step_compact_masked / _unique_masked):
    the -1 slots are no keys of the attention and the neighbour call's BatchNorm spans the real slots only.  A dense [B,N] index
    matrix goes through compact_neighbors (one host pass); a unique layout carries "n_real", its number of real slots
    (unique_neighbors returns it; the device loader knows it).  Not with sync_reduce."""
    if masked and sync_reduce is not None:
        raise ValueError("p2v_train_step(masked=True): cross-replica (sync_reduce) masked BatchNorm statistics are not built")
    masked = bool(masked) and neighbor_idx is not None          # (no neighbour slots: nothing to mask)
    if masked and neighbor_idx is not None and not isinstance(neighbor_idx, dict):
        _req(neighbor_idx, torch.int32, "neighbor_idx")
        neighbor_idx = compact_neighbors(neighbor_idx)
    if structs is not None:
        st, gst, dev = structs
        st.dropout.p = 0.0
        _set_dropout(st, params.get(DROPOUT_KEY))
    else:
        st, dev = p2v_struct(params)
        gst, _ = p2v_struct(grads, with_buffers=False)
    b = anchor_idx.numel()
    k = negative_idx.shape[1]
    compact = isinstance(neighbor_idx, dict)          # {"nb_rows": [M+1], "slot_row": [B,N]} (+ "weight", "n_unique")
    unique = compact and "weight" in neighbor_idx
    if compact:
        nb_rows, slot_row = neighbor_idx["nb_rows"], neighbor_idx["slot_row"]
        n = slot_row.shape[1]
        n_real = int(neighbor_idx["n_unique"]) if unique else nb_rows.numel() - 1
        _req(nb_rows, torch.int32, "nb_rows"); _req(slot_row, torch.int32, "slot_row", (b, n))
        if unique:
            _req(neighbor_idx["weight"], torch.float32, "weight")
            if nb_rows.numel() < n_real + 1 or neighbor_idx["weight"].numel() < n_real + 1:
                raise ValueError("nb_rows / weight shorter than n_unique + 1")
    else:
        n = 0 if neighbor_idx is None else neighbor_idx.shape[1]
    _req(table, torch.float32, "table")
    _req(anchor_idx, torch.int32, "anchor_idx", (b,)); _req(positive_idx, torch.int32, "positive_idx", (b,))
    _req(negative_idx, torch.int32, "negative_idx", (b, k))
    if n and not compact:
        _req(neighbor_idx, torch.int32, "neighbor_idx", (b, n))
    out = {"loss": alloc(1, torch.float32, dev), "d_pos": alloc(b, torch.float32, dev), "d_neg": alloc(b, torch.float32, dev)}
    if table.shape[1] != st.dim:
        raise ValueError(f"feature table width {table.shape[1]} != PRODUCT_EMB_DIM {st.dim} of the parameters")
    if want_emb:
        out["anchor_emb"] = torch.empty(b, st.dim, dtype=torch.float32, device=dev)
    nbytes = _lib.lib().pc_p2v_train_step_workspace_bytes_dim(b, n, k, st.dim)
    ws = workspace(nbytes, dev, "step")
    # the argument groups the five entry points share, marshalled once (include/pcompanion_hip.h gives each one's order)
    lib = _lib.lib()
    head = (ctypes.byref(st), ctypes.byref(gst), _p(table))
    sizes = (b, n, k, float(margin))
    outs = (_p(out["loss"]), _p(out["d_pos"]), _p(out["d_neg"]), _p(out.get("anchor_emb")))
    prof = profile.handle if profile else None
    wsa = (_p(ws), nbytes)
    if unique:
        layout = (_p(nb_rows), _p(neighbor_idx["weight"]), n_real, _p(slot_row), _p(neighbor_idx["ref_off"]),
                  _p(neighbor_idx["ref_slot"]))
    elif compact:
        layout = (_p(nb_rows), n_real, _p(slot_row))
    if sync_reduce is not None:
        if not compact:
            raise ValueError("cross-replica BatchNorm needs the compact neighbour layout")
        triplet = (_p(anchor_idx), _p(positive_idx), _p(negative_idx))
        fwd = torch.zeros(BN_SYNC_DOUBLES, dtype=torch.float64, device=dev)
        bwd_local = torch.zeros(BN_SYNC_DOUBLES, dtype=torch.float64, device=dev)
        bwd_global = None

        def phase(ph):
            sums = (ph, _p(fwd), _p(bwd_local), _p(bwd_global))
            if unique:
                check(lib.pc_p2v_train_step_unique(*head, *triplet, *layout, *sizes, *outs, None, *sums, *wsa, _stream()),
                      "pc_p2v_train_step_unique")
            else:
                check(lib.pc_p2v_train_step_compact_sync(*head, *triplet, *layout, *sizes, *outs, *sums, *wsa, _stream()),
                      "pc_p2v_train_step_compact_sync")
        phase(0)
        sync_reduce(fwd)
        phase(1)
        bwd_global = bwd_local.clone()
        sync_reduce(bwd_global)
        phase(2)
        return out
    if adam is not None and not unique:
        raise ValueError("p2v_train_step(adam=...): the unique-neighbour layout (the device loader's) carries the fused optimizer step")
    step_rows = neighbor_idx.get("step_rows") if unique else None
    if masked:
        if unique:
            if neighbor_idx.get("n_real") is None:
                raise ValueError('p2v_train_step(masked=True): the unique layout needs "n_real", its number of real slots')
            if step_rows is not None:
                _req(step_rows, torch.int32, "step_rows")
                if step_rows.numel() < b * (2 + k) + n_real + 1:
                    raise ValueError("step_rows shorter than B * (2 + K) + n_unique + 1")
            triplet = (_p(anchor_idx), _p(positive_idx), _p(negative_idx))
            check(lib.pc_p2v_train_step_unique_masked(*head, *triplet, _p(step_rows), *layout[:3], int(neighbor_idx["n_real"]),
                                                      *layout[3:], *sizes, *outs, prof, *wsa, _adam_fused(adam), _stream()),
                  "pc_p2v_train_step_unique_masked")
        else:
            check(lib.pc_p2v_train_step_compact_masked(*head, _p(anchor_idx), _p(positive_idx), _p(negative_idx), *layout, *sizes,
                                                       *outs, prof, *wsa, _stream()), "pc_p2v_train_step_compact_masked")
        return out
    if step_rows is not None:
        # the loader concatenated the step's row indices behind its builder (concat_step_rows): the step starts with Linear0
        _req(step_rows, torch.int32, "step_rows")
        if step_rows.numel() < b * (2 + k) + n_real + 1:
            raise ValueError("step_rows shorter than B * (2 + K) + n_unique + 1")
        check(lib.pc_p2v_train_step_unique_rows(*head, _p(step_rows), *layout, *sizes, *outs, prof, *wsa, _adam_fused(adam), _stream()),
              "pc_p2v_train_step_unique_rows")
        return out
    triplet = (_p(anchor_idx), _p(positive_idx), _p(negative_idx))
    if unique and adam is not None:
        check(lib.pc_p2v_train_step_unique_adam(*head, *triplet, *layout, *sizes, *outs, prof, *wsa, _adam_fused(adam), _stream()),
              "pc_p2v_train_step_unique_adam")
    elif unique:
        check(lib.pc_p2v_train_step_unique(*head, *triplet, *layout, *sizes, *outs, prof, -1, None, None, None, *wsa, _stream()),
              "pc_p2v_train_step_unique")
    elif compact:
        check(lib.pc_p2v_train_step_compact(*head, *triplet, *layout, *sizes, *outs, prof, *wsa, _stream()),
              "pc_p2v_train_step_compact")
    else:
        check(lib.pc_p2v_train_step(*head, *triplet, _p(neighbor_idx) if n else None, *sizes, *outs, prof, *wsa, _stream()),
              "pc_p2v_train_step")
    return out


def _adam_fused(adam):
    """p2v_train_step's adam= dict as a pc_adam_fused by reference (None: no optimizer rides in the step)."""
    if adam is None:
        return None
    af = _lib.AdamFused()
    n_flat = adam["param"].numel()
    for key in ("param", "grad", "exp_avg", "exp_avg_sq"):
        _req(adam[key], torch.float32, key, (n_flat,))
    _req(adam["step_count"], torch.int64, "step_count")
    af.param, af.grad, af.exp_avg, af.exp_avg_sq = (adam[key].data_ptr() for key in ("param", "grad", "exp_avg", "exp_avg_sq"))
    af.n, af.step_count, af.t = n_flat, adam["step_count"].data_ptr(), int(adam["t"])
    af.lr, af.beta1, af.beta2, af.eps = float(adam["lr"]), float(adam["betas"][0]), float(adam["betas"][1]), float(adam["eps"])
    return ctypes.byref(af)


# ----------------------------------------------------------------------------- P1-P4
def build_similarity_batch(pair_ids, graph, n_pad, k_neg, seed, step):
    """graph: dict of int32 CUDA tensors sim_pairs[S,2], cv_rowptr, cv_col, sim_rowptr, sim_col
    and n_products.  Returns anchor_idx, positive_idx, negative_idx[B,K], neighbor_idx[B,n_pad]."""
    b = pair_ids.numel()
    dev = pair_ids.device
    _req(pair_ids, torch.int32, "pair_ids")
    for k in ("sim_pairs", "cv_rowptr", "cv_col", "sim_rowptr", "sim_col"):
        _req(graph[k], torch.int32, k)
    a = torch.empty(b, dtype=torch.int32, device=dev)
    p = torch.empty(b, dtype=torch.int32, device=dev)
    ng = torch.empty(b, k_neg, dtype=torch.int32, device=dev)
    nb = torch.empty(b, n_pad, dtype=torch.int32, device=dev) if n_pad > 0 else None
    check(_lib.lib().pc_build_similarity_batch(_p(pair_ids), b, _p(graph["sim_pairs"]), _p(graph["cv_rowptr"]),
                                               _p(graph["cv_col"]), _p(graph["sim_rowptr"]), _p(graph["sim_col"]),
                                               int(graph["n_products"]), n_pad, k_neg, int(seed), int(step), _p(a),
                                               _p(p), _p(ng), _p(nb), _stream()), "pc_build_similarity_batch")
    return a, p, ng, nb


class BatchBuffers:
    """One slot of a loader's ring of batch buffers, sized for the largest batch (B samples, n_max neighbour slots each):
    the builders write into views of it (`out=`), so a steady-state step allocates nothing and -- the point -- frees
    nothing: every tensor that is allocated on the builder's stream, used on the training stream and then freed costs
    the TRAINING stream an event-record packet at the free (torch's allocator does that for record_stream'ed blocks);
    nine such tensors per batch were a 40-70 us hole at every step boundary (scripts/dev/fixed_batch_probe.py)."""

    def __init__(self, b, n_max, k_neg, device):
        i32 = lambda n: torch.empty(n, dtype=torch.int32, device=device)
        slots = b * max(n_max, 1)
        self.b, self.n_max, self.k = b, n_max, k_neg
        self.a, self.p, self.ng = i32(b), i32(b), i32(b * k_neg)
        self.nb_rows, self.ref_off, self.ref_slot, self.slot_row = i32(slots + 2), i32(slots + 3), i32(slots + 1), i32(slots)
        self.weight = torch.empty(slots + 2, dtype=torch.float32, device=device)
        self.n_unique, self.row_off = i32(1), i32(b + 1)
        self.step_rows = i32(b * (2 + k_neg) + slots + 2)      # [anchor | nb_rows | positive | negatives] (concat_step_rows)
        self.host_n = torch.empty(1, dtype=torch.int32).pin_memory()

    def views(self, b, n_pad, n_real, unique):
        if b > self.b or n_pad > self.n_max or n_real > self.b * max(self.n_max, 1):
            raise ValueError("batch larger than the ring's buffers")
        v = {"a": self.a[:b], "p": self.p[:b], "ng": self.ng[:b * self.k].view(b, self.k), "nb_rows": self.nb_rows[:n_real + 1],
             "slot_row": self.slot_row[:b * n_pad].view(b, n_pad), "row_off": self.row_off[:b + 1]}
        if unique:
            v.update(weight=self.weight[:n_real + 1], ref_off=self.ref_off[:n_real + 2], ref_slot=self.ref_slot[:max(n_real, 1)],
                     n_unique=self.n_unique, step_rows=self.step_rows[:b * (2 + self.k) + n_real + 1])
        return v


def build_similarity_batch_compact(pair_ids, graph, n_pad, k_neg, seed, step, n_real, out=None):
    """Same batch with the neighbour rows compacted (pc_build_similarity_batch_compact): returns
    anchor_idx, positive_idx, negative_idx, {"nb_rows": [n_real+1], "slot_row": [B,n_pad]}.  n_real =
    sum of the batch's (capped) co-view degrees, known to the host loader."""
    b = pair_ids.numel()
    dev = pair_ids.device
    _req(pair_ids, torch.int32, "pair_ids")
    if out is not None:
        a, p, ng, nb_rows, slot_row, row_off = (out[k] for k in ("a", "p", "ng", "nb_rows", "slot_row", "row_off"))
    else:
        a = torch.empty(b, dtype=torch.int32, device=dev)
        p = torch.empty(b, dtype=torch.int32, device=dev)
        ng = torch.empty(b, k_neg, dtype=torch.int32, device=dev)
        nb_rows = torch.empty(n_real + 1, dtype=torch.int32, device=dev)
        slot_row = torch.empty(b, n_pad, dtype=torch.int32, device=dev)
        row_off = torch.empty(b + 1, dtype=torch.int32, device=dev)
    check(_lib.lib().pc_build_similarity_batch_compact(
        _p(pair_ids), b, _p(graph["sim_pairs"]), _p(graph["cv_rowptr"]), _p(graph["cv_col"]), _p(graph["sim_rowptr"]),
        _p(graph["sim_col"]), int(graph["n_products"]), n_pad, k_neg, int(seed), int(step), _p(a), _p(p), _p(ng),
        _p(nb_rows), _p(slot_row), _p(row_off), _stream()), "pc_build_similarity_batch_compact")
    return a, p, ng, {"nb_rows": nb_rows, "slot_row": slot_row}


_uq_scratch = {}


def build_similarity_batch_unique(pair_ids, graph, n_pad, k_neg, seed, step, n_real, out=None):
    """Same batch in the unique-neighbour layout (pc_build_similarity_batch_unique): returns anchor_idx,
    positive_idx, negative_idx, {"nb_rows": [n_real+1], "weight": [n_real+1] fp32, "slot_row": [B,n_pad],
    "n_unique": [1] int32 DEVICE tensor}.  Only the first n_unique+1 entries of nb_rows / weight are meaningful;
    the caller reads n_unique back (the loader does so asynchronously, one batch ahead)."""
    b = pair_ids.numel()
    dev = pair_ids.device
    _req(pair_ids, torch.int32, "pair_ids")
    npr = int(graph["n_products"])
    slots = b * n_pad
    key = (dev, npr, torch.cuda.current_stream(dev).cuda_stream)      # (per stream: two loaders over one graph must not share counters)
    need = _lib.lib().pc_build_similarity_batch_unique_scratch_bytes(npr, slots)
    if key not in _uq_scratch or _uq_scratch[key].numel() < need:
        # per-product counters (first 4*P bytes): zero-filled once, every call leaves them zeroed
        _uq_scratch[key] = torch.zeros(max(need, _lib.lib().pc_build_similarity_batch_unique_scratch_bytes(npr, 2 * slots)),
                                       dtype=torch.uint8, device=dev)
    scratch = _uq_scratch[key]
    if out is not None:
        a, p, ng, nb_rows, weight, slot_row, n_unique, ref_off, ref_slot = (
            out[k] for k in ("a", "p", "ng", "nb_rows", "weight", "slot_row", "n_unique", "ref_off", "ref_slot"))
    else:
        a = torch.empty(b, dtype=torch.int32, device=dev)
        p = torch.empty(b, dtype=torch.int32, device=dev)
        ng = torch.empty(b, k_neg, dtype=torch.int32, device=dev)
        nb_rows = torch.empty(n_real + 1, dtype=torch.int32, device=dev)
        weight = torch.empty(n_real + 1, dtype=torch.float32, device=dev)
        slot_row = torch.empty(b, n_pad, dtype=torch.int32, device=dev)
        n_unique = torch.empty(1, dtype=torch.int32, device=dev)
        ref_off = torch.empty(n_real + 2, dtype=torch.int32, device=dev)
        ref_slot = torch.empty(max(n_real, 1), dtype=torch.int32, device=dev)
    check(_lib.lib().pc_build_similarity_batch_unique(
        _p(pair_ids), b, _p(graph["sim_pairs"]), _p(graph["cv_rowptr"]), _p(graph["cv_col"]), _p(graph["sim_rowptr"]),
        _p(graph["sim_col"]), npr, n_pad, k_neg, int(seed), int(step), int(n_real), _p(a), _p(p), _p(ng), _p(nb_rows),
        _p(weight), _p(slot_row), _p(ref_off), _p(ref_slot), _p(n_unique), _p(scratch), scratch.numel(), _stream()),
        "pc_build_similarity_batch_unique")
    return a, p, ng, {"nb_rows": nb_rows, "weight": weight, "slot_row": slot_row, "ref_off": ref_off,
                      "ref_slot": ref_slot, "n_unique": n_unique}


def concat_step_rows(anchor_idx, positive_idx, negative_idx, nb_rows, n_unique_dev, out=None):
    """pc_p2v_concat_step_rows on the current stream: [anchor | nb_rows[0 .. n_unique] | positive | negatives] with n_unique read
    on the device -- what the fused step would otherwise concatenate in a launch of its own.  nb_rows: the builder's [n_real + 1]
    buffer.  Returns the int32 row list (`out` or a new tensor of B * (2 + K) + n_real + 1 entries)."""
    b, k = anchor_idx.numel(), negative_idx.shape[1]
    cap = nb_rows.numel()
    for t, nm in ((anchor_idx, "anchor_idx"), (positive_idx, "positive_idx"), (negative_idx, "negative_idx"), (nb_rows, "nb_rows"),
                  (n_unique_dev, "n_unique")):
        _req(t, torch.int32, nm)
    need = b * (2 + k) + cap
    if out is None:
        out = torch.empty(need, dtype=torch.int32, device=anchor_idx.device)
    _req(out, torch.int32, "step_rows")
    if out.numel() < need:
        raise ValueError(f"step_rows: {out.numel()} entries, B * (2 + K) + len(nb_rows) = {need} needed")
    check(_lib.lib().pc_p2v_concat_step_rows(_p(anchor_idx), _p(positive_idx), _p(negative_idx), _p(nb_rows), _p(n_unique_dev), cap, b,
                                             k, _p(out), out.numel(), _stream()), "pc_p2v_concat_step_rows")
    return out


def unique_neighbors(neighbor_idx):
    """Host-side construction of the unique-neighbour layout from a dense [B,N] index matrix (-1 = padding)."""
    idx = neighbor_idx.cpu().numpy()
    real = idx >= 0
    u, inv, cnt = np.unique(idx[real], return_inverse=True, return_counts=True)
    nb_rows = np.concatenate([u, [-1]]).astype(np.int32)
    weight = np.concatenate([cnt, [idx.size - int(real.sum())]]).astype(np.float32)
    slot = np.full(idx.shape, len(u), np.int32)
    slot[real] = inv.astype(np.int32)
    order = np.argsort(slot.reshape(-1), kind="stable").astype(np.int32)[:int(real.sum())]   # real slots grouped by row
    if order.size == 0:
        order = np.zeros(1, np.int32)     # a batch of padding alone: no row lists a slot, but the C ABI refuses a NULL ref_slot
    ref_off = np.concatenate([[0], np.cumsum(cnt), [int(real.sum())]]).astype(np.int32)      # [U + 2]: padding row lists none
    dev = neighbor_idx.device
    return {"nb_rows": torch.from_numpy(nb_rows).to(dev), "weight": torch.from_numpy(weight).to(dev),
            "slot_row": torch.from_numpy(slot).to(dev), "ref_off": torch.from_numpy(ref_off).to(dev),
            "ref_slot": torch.from_numpy(order).to(dev), "n_unique": int(len(u)), "n_real": int(real.sum())}


def compact_neighbors(neighbor_idx):
    """Host-side compaction of a dense [B,N] neighbour index matrix (-1 = padding slot)."""
    idx = neighbor_idx.cpu().numpy()
    real = idx >= 0
    nb_rows = np.concatenate([idx[real], [-1]]).astype(np.int32)
    slot = np.full(idx.shape, int(real.sum()), np.int32)
    slot[real] = np.arange(int(real.sum()), dtype=np.int32)
    dev = neighbor_idx.device
    return {"nb_rows": torch.from_numpy(nb_rows).to(dev), "slot_row": torch.from_numpy(slot).to(dev)}


class CPythonRandom:
    """Host-side exact restatement of the CPython `random` stream the reference samples
    from (csrc/host_mt.cpp).  Host numpy arrays in, host numpy arrays out."""

    def __init__(self, seed=0):
        L_ = _lib.lib()
        self._buf = ctypes.create_string_buffer(L_.pc_mt_state_bytes())
        self.seed(seed)

    def seed(self, s):
        check(_lib.lib().pc_mt_seed(self._buf, abs(int(s))), "pc_mt_seed")

    def getrandbits(self, k):
        return int(_lib.lib().pc_mt_getrandbits(self._buf, k))

    def randbelow(self, n):
        return int(_lib.lib().pc_mt_randbelow(self._buf, n))

    def shuffle(self, n):
        perm = np.arange(n, dtype=np.int64)
        check(_lib.lib().pc_mt_shuffle(self._buf, perm.ctypes.data, n), "pc_mt_shuffle")
        return perm

    def negative_samples(self, n_products, sim_rowptr, sim_col, anchors, k=5):
        sim_rowptr = np.ascontiguousarray(sim_rowptr, np.int32)
        sim_col = np.ascontiguousarray(sim_col, np.int32)
        anchors = np.ascontiguousarray(anchors, np.int32)
        out = np.empty((len(anchors), k), np.int32)
        check(_lib.lib().pc_mt_negative_samples(self._buf, n_products, sim_rowptr.ctypes.data, sim_col.ctypes.data,
                                                anchors.ctypes.data, len(anchors), k, out.ctypes.data),
              "pc_mt_negative_samples")
        return out


# ----------------------------------------------------------------------------- joint step
def joint_struct(tensors, table=None):
    st = JointTensors()
    dev = None
    for key, field in zip(JOINT_KEYS, JOINT_FIELDS):
        t = _req(tensors[key], torch.float32, key)
        dev = t.device
        setattr(st, field, t.data_ptr())
    tbl = tensors.get("product_embeddings.weight") if table is None else table
    if tbl is not None:
        _req(tbl, torch.float32, "product_embeddings.weight")
        st.product_table = tbl.data_ptr()
    _set_dropout(st, tensors.get(DROPOUT_KEY))
    return st, dev


def _joint_saved(sv):
    s = JointSaved()
    s.h, s.c, s.pi, s.tp = (sv[k].data_ptr() for k in ("h", "c", "pi", "tp"))
    return s


def joint_forward(params, query_idx, query_types, k):
    st, dev = joint_struct(params)
    b = query_idx.numel()
    t = params["query_type_embeddings.weight"].shape[0]
    _req(query_idx, torch.int32, "query_idx", (b,)); _req(query_types, torch.int32, "query_types", (b,))
    f = dict(dtype=torch.float32, device=dev)
    sims = torch.empty(b, t, **f)
    topk = torch.empty(b, k, dtype=torch.int32, device=dev)
    proj = torch.empty(b, k, D, **f)
    sv = {"h": torch.empty(b, L // 2, **f), "c": torch.empty(b, L, **f), "pi": torch.empty(b, D, **f),
          "tp": torch.empty(b * k, D, **f)}
    check(_lib.lib().pc_joint_forward(ctypes.byref(st), _p(query_idx), _p(query_types), b, t, k, _p(sims), _p(topk),
                                      _p(proj), ctypes.byref(_joint_saved(sv)), None, 0, _stream()),
          "pc_joint_forward")
    return sims, topk, proj, sv


def _width(d):
    """PRODUCT_EMB_DIM of the row-wise joint kernels (item_prediction.py:11-20, p_companion.py:105-119 take it from config)."""
    if int(d) not in (128, 256):
        raise ValueError(f"embedding width {d}: the gfx950 kernels serve PRODUCT_EMB_DIM 128 and 256")
    return int(d)


def joint_loss(sims, proj, pos_types, neg_types, pos_items, neg_items, margin, alpha, need_grad=True):
    b, t = sims.shape
    k, d = proj.shape[1], _width(proj.shape[2])
    dev = sims.device
    _req(sims, torch.float32, "type_similarities"); _req(proj, torch.float32, "projected_embeddings", (b, k, d))
    _req(pos_types, torch.int32, "positive_types", (b,)); _req(neg_types, torch.int32, "negative_types", (b,))
    _req(pos_items, torch.float32, "positive_items", (b, d)); _req(neg_items, torch.float32, "negative_items", (b, d))
    losses = torch.empty(3, dtype=torch.float32, device=dev)
    dsv = torch.empty(b, 2, dtype=torch.float32, device=dev) if need_grad else None
    dproj = torch.empty_like(proj) if need_grad else None
    partials = torch.empty(2 * b, dtype=torch.float32, device=dev)
    check(_lib.lib().pc_joint_loss_dim(_p(sims), _p(proj), _p(pos_types), _p(neg_types), _p(pos_items), _p(neg_items),
                                       b, t, k, d, float(margin), float(alpha), _p(losses), _p(dsv), _p(dproj),
                                       _p(partials), _stream()), "pc_joint_loss_dim")
    return losses, dsv, dproj


def expand_type_grad(dsv, pos_types, neg_types, num_types):
    b = dsv.shape[0]
    dense = torch.empty(b, num_types, dtype=torch.float32, device=dsv.device)
    check(_lib.lib().pc_expand_type_grad(_p(dsv), _p(pos_types), _p(neg_types), b, num_types, _p(dense), _stream()),
          "pc_expand_type_grad")
    return dense


def joint_train_step(params, grads, query_idx, query_types, pos_types, neg_types, pos_items, neg_items, k, margin,
                     alpha):
    st, dev = joint_struct(params)
    gst, _ = joint_struct(grads, table=params["product_embeddings.weight"])
    b = query_idx.numel()
    t = params["query_type_embeddings.weight"].shape[0]
    for x, nm in ((query_idx, "query_idx"), (query_types, "query_types"), (pos_types, "positive_types"),
                  (neg_types, "negative_types")):
        _req(x, torch.int32, nm, (b,))
    _req(pos_items, torch.float32, "positive_items", (b, D)); _req(neg_items, torch.float32, "negative_items", (b, D))
    losses = torch.empty(3, dtype=torch.float32, device=dev)
    topk = torch.empty(b, k, dtype=torch.int32, device=dev)
    nbytes = _lib.lib().pc_joint_workspace_bytes(b, t, k)
    ws = workspace(nbytes, dev, "joint")
    check(_lib.lib().pc_joint_train_step(ctypes.byref(st), ctypes.byref(gst), _p(query_idx), _p(query_types),
                                         _p(pos_types), _p(neg_types), _p(pos_items), _p(neg_items), b, t, k,
                                         float(margin), float(alpha), _p(losses), _p(topk), _p(ws), nbytes, _stream()),
          "pc_joint_train_step")
    return losses, topk


def _bad_counter(bad, device):
    if bad is None:
        return torch.zeros(1, dtype=torch.int32, device=device)
    return _req(bad, torch.int32, "bad", (1,))


def joint_query_grad(params, query_idx, topk, pos_items, neg_items, margin, alpha, bad=None):
    """pc_joint_query_grad: dq [B, D] = d(loss)/d(product_embeddings.weight[query_idx[b]]) of the joint step's loss for the
    predicted types topk [B, K] of the step that just ran -- the only rows of the product table the batch reaches, through the
    item hinge alone.  params: the step's tensor dict with "product_embeddings.weight" [P, D], D = 128 or 256.  A query_idx
    outside the table or a topk id outside the type table gives a zero row and one count in `bad` (int32 [1], added to)."""
    table = params.get("product_embeddings.weight")
    _req(table, torch.float32, "product_embeddings.weight")
    if table.dim() != 2:
        raise ValueError(f"product_embeddings.weight: expected [P, D], got shape {tuple(table.shape)}")
    d = _width(table.shape[1])
    _req(query_idx, torch.int32, "query_idx")
    if query_idx.dim() != 1 or query_idx.numel() < 1:
        raise ValueError(f"query_idx: expected [B], got shape {tuple(query_idx.shape)}")
    b = query_idx.numel()
    _req(topk, torch.int32, "topk")
    if topk.dim() != 2 or topk.shape[0] != b:
        raise ValueError(f"topk: expected [B, K] with B = {b}, got shape {tuple(topk.shape)}")
    k = topk.shape[1]
    t = params["complementary_type_embeddings.weight"].shape[0]
    if not 1 <= k <= min(8, t):
        raise ValueError(f"topk: K = {k} outside [1, min(8, NUM_TYPES = {t})]")
    _req(pos_items, torch.float32, "positive_items", (b, d)); _req(neg_items, torch.float32, "negative_items", (b, d))
    st, dev = joint_struct(params)
    if tuple(params["item_prediction.item_projection.weight"].shape) != (d, d) or \
            tuple(params["item_prediction.type_projection.weight"].shape) != (d, L):
        raise ValueError(f"the projections do not match the table's width {d}")
    bad = _bad_counter(bad, dev)
    dq = torch.empty(b, d, dtype=torch.float32, device=dev)
    nbytes = _lib.lib().pc_joint_query_grad_workspace_bytes(b, k, d)
    ws = workspace(nbytes, dev, "query_grad")
    check(_lib.lib().pc_joint_query_grad(ctypes.byref(st), _p(query_idx), _p(topk), _p(pos_items), _p(neg_items), b,
                                         table.shape[0], t, k, d, float(margin), float(alpha), _p(dq), _p(bad), _p(ws), nbytes,
                                         _stream()), "pc_joint_query_grad")
    return dq


SPARSE_ADAM_MAX_ROWS = 1 << 20


def sparse_adam_rows(table, exp_avg, exp_avg_sq, idx, grad, t, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, bad=None):
    """pc_sparse_adam_rows: torch.optim.SparseAdam's step number t (>= 1, owned by the caller) over the rows idx [R] of table
    [P, D] (in place, with its moments): duplicates are summed in ascending position, -1 is skipped, any other id outside
    [0, P) is skipped and counted in `bad` (int32 [1], added to); rows not named keep their bits.  No float atomics: the same
    bits on every run."""
    _req(table, torch.float32, "table")
    if table.dim() != 2 or table.shape[0] < 1:
        raise ValueError(f"table: expected [P, D], got shape {tuple(table.shape)}")
    p, d = table.shape[0], _width(table.shape[1])
    _req(exp_avg, torch.float32, "exp_avg", (p, d)); _req(exp_avg_sq, torch.float32, "exp_avg_sq", (p, d))
    _req(idx, torch.int32, "idx")
    if idx.dim() != 1 or not 1 <= idx.numel() <= SPARSE_ADAM_MAX_ROWS:
        raise ValueError(f"idx: expected [R] with 1 <= R <= {SPARSE_ADAM_MAX_ROWS}, got shape {tuple(idx.shape)}")
    r = idx.numel()
    _req(grad, torch.float32, "grad", (r, d))
    if int(t) < 1:
        raise ValueError(f"t = {t}: the step number starts at 1")
    bad = _bad_counter(bad, table.device)
    nbytes = _lib.lib().pc_sparse_adam_rows_workspace_bytes(r)
    ws = workspace(nbytes, table.device, "sparse_adam")
    check(_lib.lib().pc_sparse_adam_rows(_p(table), _p(exp_avg), _p(exp_avg_sq), p, d, _p(idx), _p(grad), r, int(t), float(lr),
                                         float(betas[0]), float(betas[1]), float(eps), _p(bad), _p(ws), nbytes, _stream()),
          "pc_sparse_adam_rows")


def joint_fused_supported(num_types, k, dropout_p=0.0):
    return bool(_lib.lib().pc_joint_fused_supported(int(num_types), int(k), float(dropout_p)))


class _JointStepArgs:
    """The fused joint step's arguments, checked once and marshalled into named groups (include/pcompanion_hip.h,
    pc_joint_fused_step, gives their order; each foreign call below assembles it from the groups beside the call):
    tensors (parameters, gradients), opt (both moments, the step count -- all None without adam), hyper (lr, beta1, beta2, eps),
    batch (the six batch pointers), b, sizes (num_types, k, num_products), loss (margin, alpha), bad."""

    def __init__(self, params, grads, query_idx, query_types, pos_types, neg_types, pos_items, neg_items, k, margin, alpha,
                 bad, adam):
        table = params["product_embeddings.weight"]
        self.st, self.dev = joint_struct(params)
        self.gst, _ = joint_struct(grads, table=table)
        self.b = b = query_idx.numel()
        self.t, self.k, self.num_products = params["query_type_embeddings.weight"].shape[0], k, int(table.shape[0])
        for x, nm in ((query_idx, "query_idx"), (query_types, "query_types"), (pos_types, "positive_types"),
                      (neg_types, "negative_types")):
            _req(x, torch.int32, nm, (b,))
        _req(pos_items, torch.float32, "positive_items", (b, D)); _req(neg_items, torch.float32, "negative_items", (b, D))
        self.tensors = (ctypes.byref(self.st), ctypes.byref(self.gst))
        self.opt, self.hyper = (None, None, None), (0.0, 0.0, 0.0, 0.0)
        if adam is not None:
            self.mst, _ = joint_struct(adam["exp_avg"], table=table)
            self.vst, _ = joint_struct(adam["exp_avg_sq"], table=table)
            self.opt = (ctypes.byref(self.mst), ctypes.byref(self.vst), _p(_req(adam["step_count"], torch.int64, "step_count")))
            self.hyper = (float(adam["lr"]), float(adam["betas"][0]), float(adam["betas"][1]), float(adam["eps"]))
        if bad is not None:
            _req(bad, torch.int32, "bad", (1,))
        self.batch = (_p(query_idx), _p(query_types), _p(pos_types), _p(neg_types), _p(pos_items), _p(neg_items))
        self.sizes = (self.t, k, self.num_products)
        self.loss = (float(margin), float(alpha))
        self.bad = _p(bad)
        self.ws_bytes = _lib.lib().pc_joint_fused_workspace_bytes(b, self.t, k)


def joint_fused_step(params, grads, query_idx, query_types, pos_types, neg_types, pos_items, neg_items, k, margin, alpha,
                     bad=None, adam=None):
    """pc_joint_fused_step: the joint loop body as two launches (T <= 128; the gradient products get their own kernel up to 512).  adam: None (gradients only) or a dict with
    'exp_avg' / 'exp_avg_sq' (tensor dicts keyed like `params`), 'step_count' ([1] int64), 'lr', 'betas', 'eps': the
    optimizer update then happens in the last kernel.  Returns (losses[3], complementary_types[B,K])."""
    a = _JointStepArgs(params, grads, query_idx, query_types, pos_types, neg_types, pos_items, neg_items, k, margin, alpha, bad, adam)
    losses = torch.empty(3, dtype=torch.float32, device=a.dev)
    topk = torch.empty(a.b, k, dtype=torch.int32, device=a.dev)
    ws = workspace(a.ws_bytes, a.dev, "joint_fused")
    check(_lib.lib().pc_joint_fused_step(*a.tensors, *a.opt, *a.hyper, *a.batch, a.b, *a.sizes, *a.loss, _p(losses), _p(topk), a.bad,
                                         _p(ws), a.ws_bytes, _stream()), "pc_joint_fused_step")
    return losses, topk


def joint_fused_touched(ws, b, t, k):
    """pc_joint_fused_touched: (rows_comp, rows_query, n_touched) -- int32 device tensors aliasing the fused step's
    workspace `ws` (a uint8 tensor): ascending touched rows of the two [T,64] tables (capacity-sized; the first
    n_touched[0] / n_touched[1] entries are live) after a step at T > 512."""
    rc, rq, nt = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    check(_lib.lib().pc_joint_fused_touched(_p(ws), ws.numel(), int(b), int(t), int(k), ctypes.byref(rc), ctypes.byref(rq),
                                            ctypes.byref(nt)), "pc_joint_fused_touched")
    base = ws.data_ptr()

    def view(ptr, n):
        off = ptr.value - base
        return ws[off:off + 4 * n].view(torch.int32)
    return view(rc, min(b * (k + 2), t)), view(rq, min(b, t)), view(nt, 2)


class PreparedJointStep:
    """pc_joint_fused_step with every argument resolved once: the loop body then costs one foreign call (the per-step
    argument marshalling of joint_fused_step -- ~50 tensor checks, dict and struct building -- is as long as the three
    kernels themselves).  All buffers are fixed: parameters / gradients / moments (flat-buffer views), the batch
    tensors, the workspace, the outputs.  dropout: (p, seed) or None; the offset advances with every call."""

    def __init__(self, params, grads, batch, k, margin, alpha, bad=None, adam=None, dropout=None):
        self._keep = (params, grads, batch, bad, adam)
        qi, qt, pt, nt = (batch[n].reshape(-1) for n in ("query_idx", "query_types", "positive_types", "negative_types"))
        a = self._a = _JointStepArgs(params, grads, qi, qt, pt, nt, batch["positive_items"], batch["negative_items"], k, margin,
                                     alpha, bad, adam)
        self._idx = (qi, qt, pt, nt)
        self.st, self.gst = a.st, a.gst
        self.losses = alloc(3, torch.float32, a.dev)
        self.topk = alloc(a.b * k, torch.int32, a.dev).view(a.b, k)
        self.ws = alloc(max(int(a.ws_bytes), 256), torch.uint8, a.dev)
        self.dropout = dropout
        self.calls = 0
        if dropout is not None:
            self.st.dropout.p, self.st.dropout.seed = float(dropout[0]), int(dropout[1])
        # the groups of _JointStepArgs, and what this object owns: the losses pointer, outs (top-k, bad count), wsa (workspace, bytes)
        self._tensors, self._opt, self._batch, self._b, self._sizes, self._loss = a.tensors, a.opt, a.batch, a.b, a.sizes, a.loss
        self._has_adam = adam is not None
        self._step_hyper = a.hyper                      # what the step's own Adam uses (zeros without adam=)
        self._hyper = (1e-3, 0.9, 0.999, 1e-8)          # what set_hyper last gave: run_epoch_dp's Adam over the flat buffers
        self._losses_p, self._outs, self._wsa = _p(self.losses), (_p(self.topk), a.bad), (_p(self.ws), a.ws_bytes)
        self._fn = _lib.lib().pc_joint_fused_step
        self._pairs_fn = _lib.lib().pc_joint_fused_step_pairs
        self._pairs_src = None

    def set_hyper(self, lr, betas, eps):
        """The optimizer's hyper-parameters are plain doubles among the resolved arguments: refreshed from
        optimizer.param_groups by the caller before a step / an epoch, so that an LR scheduler or a load_state_dict()
        after preparation reaches the fused update exactly as it reaches the eager path."""
        self._hyper = (float(lr), float(betas[0]), float(betas[1]), float(eps))
        if self._has_adam:
            self._step_hyper = self._hyper

    def __call__(self, dropout_offset=0):
        if self.dropout is not None:
            self.st.dropout.offset = int(dropout_offset)
        rc = self._fn(*self._tensors, *self._opt, *self._step_hyper, *self._batch, self._b, *self._sizes, *self._loss,
                      self._losses_p, *self._outs, *self._wsa, _stream())
        if rc:
            check(rc, "pc_joint_fused_step")
        self.calls += 1
        return self.losses, self.topk

    def _source(self, source):
        """(features, type_idx, n_types, seed) of the dataset, checked against the catalogue's size: marshalled."""
        features, type_idx, n_types, seed = source
        _req(features, torch.float32, "features", (self._a.num_products, D))
        _req(type_idx, torch.int32, "type_idx", (self._a.num_products,))
        return (_p(features), _p(type_idx), int(n_types), int(seed))

    def from_pairs(self, rows_dev, source, step, dropout_offset=0):
        """The loader's batch construction and the step as one call (pc_joint_fused_step_pairs): `rows_dev` [B,3] int32
        labelled pairs, `source` = (features, type_idx, n_types, seed) of the dataset, `step` the loader's batch counter.
        The batch tensors this object was prepared with are OUTPUTS here: they hold the batch afterwards."""
        if self._pairs_src is None or self._pairs_src[0] is not source:
            self._pairs_src = (source, self._source(source))
        _req(rows_dev, torch.int32, "pairs", (self._b, 3))
        if self.dropout is not None:
            self.st.dropout.offset = int(dropout_offset)
        rc = self._pairs_fn(*self._tensors, *self._opt, *self._step_hyper, ctypes.c_void_p(rows_dev.data_ptr()),
                            *self._pairs_src[1], int(step), *self._batch, self._b, *self._sizes, *self._loss,
                            self._losses_p, *self._outs, *self._wsa, _stream())
        if rc:
            check(rc, "pc_joint_fused_step_pairs")
        self.calls += 1
        return self.losses, self.topk

    def _epoch(self, pairs_dev, drop_last, dropout_offset):
        """What both epoch calls prepare: the pair count, the number of steps and their loss rows."""
        n = int(pairs_dev.shape[0])
        _req(pairs_dev, torch.int32, "pairs", (n, 3))
        steps = n // self._b if drop_last else (n + self._b - 1) // self._b
        losses = torch.empty(max(steps, 1), 3, dtype=torch.float32, device=pairs_dev.device)
        if self.dropout is not None:
            self.st.dropout.offset = int(dropout_offset)
        return n, steps, losses

    def run_epoch(self, pairs_dev, source, first_step, drop_last=False, dropout_offset=0):
        """train.py:36-57 over `pairs_dev` [n,3] (epoch order, on the device) as one foreign call (pc_joint_train_epoch).
        Returns the per-step losses [n_steps,3] (device) and the number of steps."""
        if not self._has_adam:
            raise ValueError("run_epoch needs the optimizer state (PreparedJointStep(adam=...))")
        src = self._source(source)
        n, steps, losses = self._epoch(pairs_dev, drop_last, dropout_offset)
        rc = _lib.lib().pc_joint_train_epoch(*self._tensors, *self._opt, *self._step_hyper, _p(pairs_dev), n, *src, int(first_step),
                                             *self._batch, self._b, int(bool(drop_last)), *self._sizes, *self._loss, _p(losses),
                                             *self._outs, *self._wsa, _stream())
        if rc:
            check(rc, "pc_joint_train_epoch")
        self.calls += steps
        self._keep_epoch = (pairs_dev, source)
        return losses[:steps], steps

    def run_epoch_dp(self, pairs_dev, source, first_step, flat, gflat, exp_avg, exp_avg_sq, step_count, t_first, scalars,
                     exchange, drop_last=True, dropout_offset=0, shard=False):
        """pc_joint_train_epoch_plan: the epoch of a data-parallel REPLICA as one foreign call -- per step the fused step without its
        Adam, the exchange (ops.RcclExchange / CallbackExchange / None) and Adam over the flat buffers; shard=True: reduce-scatter,
        Adam on this rank's slice, all-gather (ABI 8).  The object must have been prepared WITHOUT adam (gradients only) over
        parameters / gradients that are views of flat / gflat."""
        if self._has_adam:
            raise ValueError("run_epoch_dp: prepare the step without adam= (the epoch applies Adam over the flat buffers itself)")
        src = self._source(source)
        n, steps, losses = self._epoch(pairs_dev, drop_last, dropout_offset)
        nf = flat.numel()
        for x, nm in ((flat, "param_flat"), (gflat, "grad_flat"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
            _req(x, torch.float32, nm, (nf,))
        _req(step_count, torch.int64, "step_count")
        if shard and (exchange is None or nf % exchange.world):
            raise ValueError("run_epoch_dp(shard=True): an exchange, and flat buffers whose length is a multiple of its world size "
                             "(padded to a multiple of 4 * world: flatten_parameters(pad_multiple=4 * world))")
        plan = exchange.plan(shard=bool(shard)) if exchange is not None else None
        rc = _lib.lib().pc_joint_train_epoch_plan(*self._tensors, _p(flat), _p(gflat), _p(exp_avg), _p(exp_avg_sq), nf, _p(step_count),
                                                  int(t_first), _p(scalars), *self._hyper,
                                                  ctypes.byref(plan) if plan is not None else None, _p(pairs_dev), n, *src,
                                                  int(first_step), *self._batch, self._b, int(bool(drop_last)), *self._sizes,
                                                  *self._loss, _p(losses), *self._outs, *self._wsa, _stream())
        if rc and isinstance(exchange, CallbackExchange):
            exchange.reraise()
        if rc:
            check(rc, "pc_joint_train_epoch_plan")
        self.calls += steps
        self._keep_epoch = (pairs_dev, source, flat, gflat, exp_avg, exp_avg_sq, step_count, scalars, exchange)
        return losses[:steps], steps


class PreparedComplementaryBuilder:
    """pc_build_complementary_batch into FIXED output buffers with the arguments resolved once (see PreparedJointStep)."""

    def __init__(self, features, type_idx, n_types, seed, out):
        _req(features, torch.float32, "features"); _req(type_idx, torch.int32, "type_idx")
        self.b = out["query_idx"].numel()
        for k in ("query_idx", "query_types", "positive_types", "negative_types"):
            _req(out[k], torch.int32, k)
        for k in ("positive_items", "negative_items"):
            _req(out[k], torch.float32, k, (self.b, D))
        self._keep = (features, type_idx, out)
        self._fn = _lib.lib().pc_build_complementary_batch
        self._tail = [_p(out["query_idx"]), _p(out["query_types"]), _p(out["positive_types"]), _p(out["negative_types"]),
                      _p(out["positive_items"]), _p(out["negative_items"]), _p(out.get("target_features"))]
        self._head = [_p(features), _p(type_idx), int(n_types), int(seed)]

    def __call__(self, rows_dev, step):
        rc = self._fn(ctypes.c_void_p(rows_dev.data_ptr()), self.b, *self._head, int(step), *self._tail, _stream())
        if rc:
            check(rc, "pc_build_complementary_batch")


# ----------------------------------------------------------------------------- building blocks
def _pad_cols(t, mult=4):
    """[..., c] -> [..., ceil(c / mult) * mult] with zero columns (the kernels move 16-byte chunks: contraction and
    gradient dimensions that are not multiples of 4 -- an odd NUM_TYPES in module mode -- are zero-padded here)."""
    c = t.shape[-1]
    return t if c % mult == 0 else torch.nn.functional.pad(t, (0, mult - c % mult)).contiguous()


def linear_forward(x, w, b=None, idx=None, act=0, rows=None):
    out_dim, in_dim = w.shape
    if in_dim % 4:                                   # zero columns add nothing to x . w
        x, w = _pad_cols(x.reshape(-1, in_dim)), _pad_cols(w)
        in_dim = w.shape[1]
    _req(x, torch.float32, "x"); _req(w, torch.float32, "weight")
    if b is not None:
        _req(b, torch.float32, "bias", (out_dim,))
    if idx is not None:
        _req(idx, torch.int32, "idx")
        rows = idx.numel()
    elif rows is None:
        rows = x.numel() // in_dim
    y = torch.empty(rows, out_dim, dtype=torch.float32, device=w.device)
    check(_lib.lib().pc_linear_forward(_p(x), _p(idx), rows, in_dim, _p(w), _p(b), out_dim, act, _p(y), _stream()),
          "pc_linear_forward")
    return y


def linear_backward_input(dy, w):
    out_dim, in_dim = w.shape
    rows = dy.numel() // out_dim
    if out_dim % 4:                                  # dx = dy . w contracts over out_dim
        dy = _pad_cols(dy.reshape(rows, out_dim))
        w = torch.cat([w, w.new_zeros(dy.shape[1] - out_dim, in_dim)])
        out_dim = dy.shape[1]
    _req(dy, torch.float32, "dy"); _req(w, torch.float32, "weight")
    dx = torch.empty(rows, in_dim, dtype=torch.float32, device=w.device)
    wt = torch.empty(in_dim, out_dim, dtype=torch.float32, device=w.device)
    check(_lib.lib().pc_linear_backward_input(_p(dy), rows, out_dim, _p(w), in_dim, 0, None, _p(dx), _p(wt),
                                              _stream()), "pc_linear_backward_input")
    return dx


def linear_backward_weight(dy, x, out_dim, in_dim, idx=None, want_bias=True):
    rows = dy.numel() // out_dim
    if out_dim % 4 or in_dim % 4:
        dyp, xp = _pad_cols(dy.reshape(rows, out_dim)), _pad_cols(x.reshape(-1, in_dim))
        dw, db = linear_backward_weight(dyp, xp, dyp.shape[1], xp.shape[1], idx, want_bias)
        return dw[:out_dim, :in_dim].contiguous(), (db[:out_dim].contiguous() if db is not None else None)
    _req(dy, torch.float32, "dy"); _req(x, torch.float32, "x")
    if idx is not None:
        _req(idx, torch.int32, "idx", (rows,))
    dev = dy.device
    dw = torch.empty(out_dim, in_dim, dtype=torch.float32, device=dev)
    db = torch.empty(out_dim, dtype=torch.float32, device=dev) if want_bias else None
    nbytes = _lib.lib().pc_linear_backward_weight_workspace_bytes(rows, out_dim, in_dim)
    ws = workspace(nbytes, dev)
    check(_lib.lib().pc_linear_backward_weight(_p(dy), rows, out_dim, _p(x), _p(idx), in_dim, _p(dw), _p(db), 0,
                                               _p(ws), nbytes, _stream()), "pc_linear_backward_weight")
    return dw, db


def topk_rows(sims, k, want_values=False):
    b, t = sims.shape
    _req(sims, torch.float32, "sims")
    idx = torch.empty(b, k, dtype=torch.int32, device=sims.device)
    val = torch.empty(b, k, dtype=torch.float32, device=sims.device) if want_values else None
    check(_lib.lib().pc_topk_rows(_p(sims), b, t, k, _p(idx), _p(val), _stream()), "pc_topk_rows")
    return (idx, val) if want_values else idx


def hadamard_forward(pi, tp, k):
    b, d = pi.shape[0], _width(pi.shape[1])
    _req(pi, torch.float32, "pi", (b, d)); _req(tp, torch.float32, "tp", (b * k, d))
    proj = torch.empty(b, k, d, dtype=torch.float32, device=pi.device)
    check(_lib.lib().pc_hadamard_forward_dim(_p(pi), _p(tp), b, k, d, _p(proj), _stream()), "pc_hadamard_forward_dim")
    return proj


def hadamard_backward(dproj, pi, tp):
    b, k, d = dproj.shape
    _width(d)
    _req(dproj, torch.float32, "dproj", (b, k, d))
    dpi = torch.empty(b, d, dtype=torch.float32, device=pi.device)
    dtp = torch.empty(b * k, d, dtype=torch.float32, device=pi.device)
    check(_lib.lib().pc_hadamard_backward_dim(_p(dproj), _p(pi), _p(tp), b, k, d, _p(dpi), _p(dtp), _stream()),
          "pc_hadamard_backward_dim")
    return dpi, dtp


# ----------------------------------------------------------------------------- P11 over a device CSR
EXPORT_CHUNK_ROWS = 65536          # products per chunk of pc_p2v_export_embeddings (workspace 0.78 GB at D = 128)
EXPORT_MAX_CHUNK_ROWS = 1 << 20


def export_embeddings(params, features, cv_rowptr, cv_col, chunk_rows=None, out=None):
    """Product2Vec.generate_all_embeddings (product2vec.py:83-111), eval mode, over a co-view CSR that stays on the device:
    features [P,D] fp32, cv_rowptr [P+1] / cv_col [E] int32, all CUDA -> the embedding table [P,D] (into `out` when given).
    One call of pc_p2v_export_embeddings: chunks of `chunk_rows` products, workspace bounded by the chunk, not by P.
    Neighbour ids are trusted (as in gather_rows); the CSR's shape is checked here, before anything is launched."""
    st, dev = p2v_struct(params)
    d = st.dim
    _req(features, torch.float32, "features")
    _req(cv_rowptr, torch.int32, "cv_rowptr")
    _req(cv_col, torch.int32, "cv_col")
    if features.dim() != 2 or features.shape[1] != d:
        raise ValueError(f"features: expected [P, {d}], got {tuple(features.shape)}")
    P = int(features.shape[0])
    if P == 0:
        raise ValueError("features: no products")
    if cv_rowptr.dim() != 1 or cv_rowptr.numel() != P + 1:
        raise ValueError(f"cv_rowptr: expected {P + 1} offsets for {P} products, got shape {tuple(cv_rowptr.shape)}")
    if cv_col.dim() != 1:
        raise ValueError(f"cv_col: expected a 1-D id list, got shape {tuple(cv_col.shape)}")
    for name, t in (("features", features), ("cv_rowptr", cv_rowptr), ("cv_col", cv_col)):
        if t.device != dev:
            raise ValueError(f"{name}: on {t.device}, the parameters are on {dev}")
    ends = cv_rowptr[[0, P]].cpu()                    # (the one readback: a CSR that does not close is refused before launch)
    if int(ends[0]) != 0 or int(ends[1]) != cv_col.numel():
        raise ValueError(f"cv_rowptr must run from 0 to len(cv_col) = {cv_col.numel()}, got {int(ends[0])} .. {int(ends[1])}")
    chunk = EXPORT_CHUNK_ROWS if chunk_rows is None else int(chunk_rows)
    if not 1 <= chunk <= EXPORT_MAX_CHUNK_ROWS:
        raise ValueError(f"chunk_rows must be in [1, {EXPORT_MAX_CHUNK_ROWS}], got {chunk}")
    chunk = min(chunk, P)
    if out is not None:
        _req(out, torch.float32, "out", (P, d))
    nbytes = _lib.lib().pc_p2v_export_workspace_bytes(chunk, d)
    need = nbytes + P * d * 4 * (2 if out is None else 1)         # workspace, e1, (out)
    free = torch.cuda.mem_get_info(dev)[0] + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)   # (+ torch's cache)
    if need > free:
        raise MemoryError(f"export of {P} x {d} embeddings needs {need / 2**30:.1f} GiB more device memory "
                          f"(e1 and the output table, {P * d * 4 / 2**30:.1f} GiB each, plus the chunk workspace), "
                          f"{free / 2**30:.1f} GiB free on {dev}")
    if out is None:
        out = torch.empty(P, d, dtype=torch.float32, device=dev)
    e1 = torch.empty(P, d, dtype=torch.float32, device=dev)
    ws = alloc(nbytes, torch.uint8, dev)
    check(_lib.lib().pc_p2v_export_embeddings(ctypes.byref(st), _p(features), P, _p(cv_rowptr), _p(cv_col), _p(e1), _p(out),
                                              chunk, _p(ws), nbytes, _stream()), "pc_p2v_export_embeddings")
    return out


def gather_rows(table, idx):
    rows = idx.numel()
    width = table.shape[1]
    _req(table, torch.float32, "table"); _req(idx, torch.int32, "idx")
    out = torch.empty(rows, width, dtype=torch.float32, device=table.device)
    check(_lib.lib().pc_gather_rows(_p(table), _p(idx), rows, width, _p(out), _stream()), "pc_gather_rows")
    return out


def scatter_add_rows(table, idx, src):
    rows = idx.numel()
    width = table.shape[1]
    _req(table, torch.float32, "table"); _req(idx, torch.int32, "idx"); _req(src, torch.float32, "src", (rows, width))
    check(_lib.lib().pc_scatter_add_rows(_p(table), _p(idx), rows, width, _p(src), _stream()), "pc_scatter_add_rows")
    return table


def scatter_rows(out, idx, src):
    rows, width = idx.numel(), out.shape[1]
    _req(out, torch.float32, "out"); _req(idx, torch.int32, "idx"); _req(src, torch.float32, "src", (rows, width))
    check(_lib.lib().pc_scatter_rows(_p(out), _p(idx), rows, width, _p(src), _stream()), "pc_scatter_rows")
    return out


def act_backward(dy, y, act):
    _req(dy, torch.float32, "dy"); _req(y, torch.float32, "y", dy.shape)
    dx = torch.empty_like(dy)
    check(_lib.lib().pc_act_backward(_p(dy), _p(y), dy.numel(), act, _p(dx), _stream()), "pc_act_backward")
    return dx


def zipf_octave_thresholds(n_products):
    """Cumulative 32-bit thresholds of the octave masses of P(rank) ~ 1 / rank, rank = 1..n_products (host, float64 once;
    the device and the oracle then compare integers only).  octave j = ranks [2^j, min(2^(j+1), P + 1))."""
    n_oct = int(n_products).bit_length()
    mass = []
    for j in range(n_oct):
        lo, hi = 1 << j, min((1 << (j + 1)) - 1, int(n_products))
        if hi - lo < 4096:
            mass.append(float(np.sum(1.0 / np.arange(lo, hi + 1, dtype=np.float64))))
        else:                                    # Euler-Maclaurin: sum_{k=lo}^{hi} 1/k, error < 1e-12 for lo >= 4096
            mass.append(float(np.log(hi / lo) + 0.5 / lo + 0.5 / hi + (1.0 / lo ** 2 - 1.0 / hi ** 2) / 12.0))
    cum = np.cumsum(mass) / np.sum(mass)
    thr = np.minimum(np.floor(cum * 4294967296.0), 4294967295.0).astype(np.uint64).astype(np.uint32)
    thr[-1] = 0xFFFFFFFF
    return thr


def exclusive_scan_i32(counts):
    """pc_exclusive_scan_i32: int32 [n] on the device -> (offsets int32 [n + 1], total as a Python int; raises when the
    total does not fit the int32 offsets)."""
    _req(counts, torch.int32, "counts")
    n = counts.numel()
    out = torch.empty(n + 1, dtype=torch.int32, device=counts.device)
    total = torch.zeros(1, dtype=torch.int64, device=counts.device)
    nbytes = _lib.lib().pc_scan_scratch_bytes(n)
    scratch = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=counts.device)
    check(_lib.lib().pc_exclusive_scan_i32(_p(counts), n, _p(out), _p(total), _p(scratch), nbytes, _stream()),
          "pc_exclusive_scan_i32")
    t = int(total.item())
    if t >= 2 ** 31:
        raise OverflowError(f"{t} entries do not fit int32 offsets")
    return out, t


def generate_catalogue(num_products, num_types, seed, mean_degree, degree_cap, dim, device, rank=0, world=1,
                       comp_mean=4.5, with_complementary=True, with_features=True):
    """csrc/generator.hip end to end; returns a dict of device tensors (see data.DeviceBPG)."""
    L = _lib.lib()
    P = int(num_products)
    dev = torch.device(device)
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    out = {"n_products": P}
    type_idx = i32(P)
    check(L.pc_gen_types(P, int(num_types), int(seed), _p(type_idx), _stream()), "pc_gen_types")
    out["type_idx"] = type_idx
    if with_features:
        n_local = (P - rank + world - 1) // world
        feats = torch.empty(n_local, dim, dtype=torch.float32, device=dev)
        check(L.pc_gen_features(rank, world, n_local, int(dim), int(num_types), int(seed), _p(feats), _stream()), "pc_gen_features")
        out["features"] = feats
    deg, cand = i32(P), (i32(P) if with_complementary else None)
    check(L.pc_gen_degrees(P, float(mean_degree), int(degree_cap), float(comp_mean), int(seed), _p(deg), _p(cand), _stream()),
          "pc_gen_degrees")
    cv_rowptr, n_edges = exclusive_scan_i32(deg)
    # (offsets and ids are int32: exclusive_scan_i32 raises when a total reaches 2^31; the kernels index the two-int pair
    # array with size_t, so pair counts up to that limit are safe -- 100 M products: 1.6e9 edges, 275 M pairs)
    cv_col, sim_count = i32(max(n_edges, 1)), i32(P)
    check(L.pc_gen_coview(P, int(num_types), int(seed), _p(cv_rowptr), _p(cv_col), _p(sim_count), _stream()), "pc_gen_coview")
    sim_rowptr, n_sim = exclusive_scan_i32(sim_count)
    sim_pairs, sim_col, pair_deg = i32(max(n_sim, 1), 2), i32(max(n_sim, 1)), i32(max(n_sim, 1))
    check(L.pc_gen_similarity(P, _p(cv_rowptr), _p(cv_col), _p(sim_rowptr), _p(sim_pairs), _p(sim_col), _p(pair_deg), _stream()),
          "pc_gen_similarity")
    out.update(cv_rowptr=cv_rowptr, cv_col=cv_col[:n_edges], sim_rowptr=sim_rowptr, sim_pairs=sim_pairs[:n_sim],
               sim_col=sim_col[:n_sim], pair_deg=pair_deg[:n_sim], max_degree=int(degree_cap))
    del deg, sim_count
    if with_complementary:
        cnt = i32(P)
        check(L.pc_gen_complementary(P, int(num_types), int(seed), _p(cand), _p(cv_rowptr), _p(cv_col), _p(cnt), None, None,
                                     _stream()), "pc_gen_complementary")
        comp_rowptr, n_comp = exclusive_scan_i32(cnt)
        comp = i32(max(n_comp, 1), 2)
        check(L.pc_gen_complementary(P, int(num_types), int(seed), _p(cand), _p(cv_rowptr), _p(cv_col), None, _p(comp_rowptr),
                                     _p(comp), _stream()), "pc_gen_complementary")
        out["comp_pairs"] = comp[:n_comp]
    return out


INGEST_CAP_MAX = 64                # = GEN_CAP_MAX: the degree bound under which the device loaders are tested
INGEST_WAVE_ROW_MAX = 128          # raw row length up to which pc_ingest_rows sorts a row in one wave's registers
INGEST_LDS_ROW_MAX = 4096          # ... and up to which one workgroup sorts it in LDS (above: between two global buffers);
#                                    pc_ingest_row_limits reports the library's own values (tests/test_ingest_host.py compares)
INGEST_LISTS = ("co_view", "purchase_after_view", "co_purchase")


def _check_catalogue_args(type_idx, lists, degree_cap, features, n_types):
    """build_catalogue's checks that need neither the library nor a device."""
    if isinstance(degree_cap, bool) or not isinstance(degree_cap, (int, np.integer)) or not 1 <= degree_cap <= INGEST_CAP_MAX:
        raise ValueError(f"build_catalogue: degree_cap must be an integer in 1..{INGEST_CAP_MAX}, got {degree_cap!r}")
    if n_types is not None and int(n_types) <= 0:
        raise ValueError("build_catalogue: n_types must be positive")
    if not isinstance(type_idx, torch.Tensor) or type_idx.dtype != torch.int32 or type_idx.dim() != 1 or type_idx.numel() < 1:
        raise ValueError("build_catalogue: type_idx must be a 1-D int32 tensor of P >= 1 type ids")
    P = type_idx.numel()
    if P >= 2 ** 31:
        raise ValueError(f"build_catalogue: {P} products do not fit int32 ids")
    for name, e in zip(INGEST_LISTS, lists):
        if not isinstance(e, torch.Tensor) or e.dtype != torch.int32 or e.dim() != 2 or e.shape[1] != 2:
            raise ValueError(f"build_catalogue: {name} must be an int32 tensor of shape [E, 2] (source, target)")
        if e.shape[0] >= 2 ** 31:
            raise ValueError(f"build_catalogue: {name} holds {e.shape[0]} edges; a list is limited to 2^31 - 1")
    if features is not None:
        if not isinstance(features, torch.Tensor) or features.dtype != torch.float32 or features.dim() != 2 or features.shape[0] != P:
            raise ValueError(f"build_catalogue: features must be a float32 tensor of shape [{P}, D] or None")
    for name, t in zip(("type_idx",) + INGEST_LISTS, (type_idx,) + tuple(lists)):
        _req(t, torch.int32, name)
    if features is not None:
        _req(features, torch.float32, "features")
    return P


def build_catalogue(type_idx, co_view, purchase_after_view, co_purchase, degree_cap=32, features=None, n_types=None):
    """csrc/ingest.hip end to end: the dict of device tensors of generate_catalogue (see data.DeviceBPG) from the three edge
    sets of a BehaviorProductGraph as unsorted, directed int32 [E, 2] device tensors of (source, target) with duplicates
    (DESIGN.md "Ingestion" has the semantics; data.IntBPG.from_edges is the host twin, equal bit for bit).  An id outside
    [0, P) raises ValueError naming its list: the device compares every id before using it and reports through one flag word.
    Host synchronisations: that word, the totals of the scans (as in generate_catalogue) and max_degree."""
    lists = (co_view, purchase_after_view, co_purchase)
    P = _check_catalogue_args(type_idx, lists, degree_cap, features, n_types)
    lo, hi = (int(x) for x in torch.aminmax(type_idx))
    n_types = hi + 1 if n_types is None else int(n_types)
    if lo < 0 or hi >= n_types:
        raise ValueError(f"build_catalogue: type ids must lie in [0, {n_types}), got {lo} .. {hi}")
    L = _lib.lib()
    dev = type_idx.device
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    z32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
    # ---- bucket every list by source
    bad = z32(1)
    cnt = [z32(P) for _ in lists]
    for k, e in enumerate(lists):
        check(L.pc_ingest_count(_p(e), e.shape[0], P, 1 << k, _p(cnt[k]), _p(bad), _stream()), "pc_ingest_count")
    flag = int(bad.item())
    if flag:
        names = ", ".join(n for k, n in enumerate(INGEST_LISTS) if flag >> k & 1)
        raise ValueError(f"build_catalogue: product ids outside [0, {P}) in {names}")
    rowptr, bucket = [], []
    for k, e in enumerate(lists):
        rp, n = exclusive_scan_i32(cnt[k])
        b = i32(max(n, 1))
        check(L.pc_ingest_scatter(_p(e), e.shape[0], P, _p(rp), _p(cnt[k]), _p(b), _stream()), "pc_ingest_scatter")
        rowptr.append(rp)
        bucket.append(b)
    # ---- every row sorted, run-length coded and (co_view) capped in its bucket; cnt[k] becomes the distinct counts
    scratch = i32(max(b.numel() for b in bucket))
    nbytes = L.pc_ingest_rows_workspace_bytes(P)
    ws = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)      # (O(P): not kept in the grow-only workspace cache)
    kept, max_kept = i32(P), z32(1)
    for k in range(3):
        cap = int(degree_cap) if k == 0 else 0
        check(L.pc_ingest_rows(P, _p(rowptr[k]), _p(bucket[k]), _p(scratch), cap, _p(cnt[k]), _p(kept) if k == 0 else None,
                               _p(max_kept) if k == 0 else None, _p(ws), nbytes, _stream()), "pc_ingest_rows")
    del scratch
    (cv_raw, pv_raw, cp_raw), (cv_b, pv_b, cp_b), (cv_n, pv_n, cp_n) = rowptr, bucket, cnt
    # ---- neighbour lists: the kept ids of every co-view row
    cv_rowptr, n_edges = exclusive_scan_i32(kept)
    cv_col = i32(max(n_edges, 1))
    check(L.pc_ingest_emit(P, _p(cv_b), _p(cv_raw), _p(cv_n), _p(cv_rowptr), _p(cv_col), None, None, None, 0, _stream()),
          "pc_ingest_emit")
    # ---- similarity = kept co-view & purchase-after-view - co-purchase
    count = kept                                             # (free now)
    check(L.pc_ingest_flag(P, _p(cv_col), _p(cv_rowptr), None, _p(pv_b), _p(pv_raw), _p(pv_n), _p(cp_b), _p(cp_raw), _p(cp_n),
                           None, None, None, _p(count), _stream()), "pc_ingest_flag")
    sim_rowptr, n_sim = exclusive_scan_i32(count)
    sim_pairs, sim_col, pair_deg = i32(max(n_sim, 1), 2), i32(max(n_sim, 1)), i32(max(n_sim, 1))
    check(L.pc_ingest_emit(P, _p(cv_col), _p(cv_rowptr), None, _p(sim_rowptr), _p(sim_col), _p(sim_pairs), _p(pair_deg),
                           _p(cv_rowptr), 1, _stream()), "pc_ingest_emit")
    # ---- complementary = co-purchase - purchase-after-view - the FULL co-view set (an edge the cap dropped is still co-viewed)
    check(L.pc_ingest_flag(P, _p(cp_b), _p(cp_raw), _p(cp_n), None, None, None, _p(pv_b), _p(pv_raw), _p(pv_n), _p(cv_b),
                           _p(cv_raw), _p(cv_n), _p(count), _stream()), "pc_ingest_flag")
    comp_rowptr, n_comp = exclusive_scan_i32(count)
    comp = i32(max(n_comp, 1), 2)
    check(L.pc_ingest_emit(P, _p(cp_b), _p(cp_raw), _p(cp_n), _p(comp_rowptr), None, _p(comp), None, None, 0, _stream()),
          "pc_ingest_emit")
    out = {"n_products": P, "type_idx": type_idx}
    if features is not None:
        out["features"] = features
    out.update(cv_rowptr=cv_rowptr, cv_col=cv_col[:n_edges], sim_rowptr=sim_rowptr, sim_pairs=sim_pairs[:n_sim],
               sim_col=sim_col[:n_sim], pair_deg=pair_deg[:n_sim], max_degree=int(max_kept.item()), comp_pairs=comp[:n_comp])
    return out


EVENT_MAX_EVENTS = 1024            # the longest session pc_events_sessions sorts (one wave, 16 register slots per lane);
#                                    pc_events_limits reports the library's own value (tests/test_events_host.py compares)
EVENT_EDGE_LIMIT = 2 ** 31 - 1     # rows of one derived edge list at most: offsets are int32 (and build_catalogue's limit)
EVENT_COLUMNS = ("session", "product", "kind", "time")


class EventEdges(NamedTuple):
    """What event_edges (device tensors) and data.event_edges_host (numpy arrays) return: the three int32 [E, 2] lists of
    (a, b), each ordered by (session, a, b), and the counts."""
    co_view: object
    purchase_after_view: object
    co_purchase: object
    n_sessions: int
    skipped_sessions: int
    n_items: int


def _check_event_args(events, n_products, n_sessions, max_events, who="event_edges"):
    """event_edges' checks that need neither the library nor a device; every refusal is a ValueError.  Returns N."""
    if not isinstance(events, torch.Tensor) or not events.is_cuda:
        raise ValueError(f"{who}: events must be a tensor on the device (the HIP path has no CPU fallback)")
    if events.dtype != torch.int32:
        raise ValueError(f"{who}: events must be int32, got {events.dtype}")
    if events.dim() != 2 or events.shape[1] != 4:
        raise ValueError(f"{who}: events must have shape [N, 4] (session, product, kind, time), got {tuple(events.shape)}")
    if not events.is_contiguous():
        raise ValueError(f"{who}: events must be contiguous")
    if events.shape[0] >= 2 ** 31:
        raise ValueError(f"{who}: {events.shape[0]} rows; a log is limited to 2^31 - 1")
    if isinstance(n_products, bool) or not isinstance(n_products, (int, np.integer)) or not 1 <= n_products < 2 ** 31:
        raise ValueError(f"{who}: n_products must be an integer in 1..2^31 - 1, got {n_products!r}")
    if n_sessions is not None and (isinstance(n_sessions, bool) or not isinstance(n_sessions, (int, np.integer))
                                   or not 1 <= n_sessions < 2 ** 31):
        raise ValueError(f"{who}: n_sessions must be None or an integer in 1..2^31 - 1, got {n_sessions!r}")
    if isinstance(max_events, bool) or not isinstance(max_events, (int, np.integer)) or not 2 <= max_events <= EVENT_MAX_EVENTS:
        raise ValueError(f"{who}: max_events must be an integer in 2..{EVENT_MAX_EVENTS}, got {max_events!r}")
    if events.shape[0] and events.data_ptr() % 16:
        raise ValueError(f"{who}: events must be 16-byte aligned (a row is read as one word)")
    return int(events.shape[0])


def event_edges(events, n_products, n_sessions=None, max_events=256, exclusive=True):
    """csrc/events.hip end to end: the co_view, purchase_after_view and co_purchase lists build_catalogue reads, derived from a
    raw event log on the device (DESIGN.md "Edge lists from shopper events" has the semantics; data.event_edges_host is the
    host twin, equal bit for bit).  events: int32 [N, 4] device tensor, rows (session, product, kind 0 view / 1 purchase,
    time >= 0) in any order.  Session ids are dense in [0, n_sessions) (None: the largest id + 1, one more read-back); a
    caller with sparse ids densifies them first (torch.unique(ids, return_inverse=True)).  A session with more than max_events
    raw rows is skipped whole and counted.  Returns an EventEdges of device tensors.  A field outside its range raises
    ValueError naming its column: the device compares every field before using it and reports through one flag word.  A
    list of more than EVENT_EDGE_LIMIT rows raises ValueError before anything is emitted.  Host synchronisations: the flag
    word and the 64-bit totals."""
    N = _check_event_args(events, n_products, n_sessions, max_events)
    P, cap, dev = int(n_products), int(max_events), events.device
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    z32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
    if n_sessions is None:
        n_sessions = max(int(events[:, 0].max()) + 1, 1) if N else 0          # (a negative id is then reported by the device)
    S = int(n_sessions)
    if N == 0:
        return EventEdges(i32(0, 2), i32(0, 2), i32(0, 2), S, 0, 0)
    L = _lib.lib()
    # ---- bucket the rows by session
    cnt, bad = z32(S), z32(1)
    check(L.pc_events_count(_p(events), N, S, P, _p(cnt), _p(bad), _stream()), "pc_events_count")
    flag = int(bad.item())
    if flag:
        names = ", ".join(n for k, n in enumerate(EVENT_COLUMNS) if flag >> k & 1)
        raise ValueError(f"event_edges: rows with {names} out of range (session in [0, {S}), product in [0, {P}), "
                         "kind 0 or 1, time >= 0)")
    nbytes = L.pc_scan_scratch_bytes(S)
    scratch = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)

    def scan(counts):                                        # (no total is read back: the rows, and the totals below)
        out = i32(S + 1)
        check(L.pc_exclusive_scan_i32(_p(counts), S, _p(out), None, _p(scratch), nbytes, _stream()), "pc_exclusive_scan_i32")
        return out

    rowptr = scan(cnt)
    bucket, last = i32(N, 2), i32(N)
    check(L.pc_events_scatter(_p(events), N, S, P, cap, _p(rowptr), _p(cnt), _p(bucket), _stream()), "pc_events_scatter")
    # ---- every kept session sorted into its items; the rows it gives each list
    n_items, count = i32(S), i32(3, S)
    totals = torch.zeros(8, dtype=torch.int64, device=dev)
    check(L.pc_events_sessions(S, _p(rowptr), _p(bucket), _p(last), cap, int(bool(exclusive)), _p(n_items), _p(count[0]),
                               _p(count[1]), _p(count[2]), _p(totals), _stream()), "pc_events_sessions")
    n_cv, n_pv, n_cp, items, skipped = totals[:5].tolist()
    for name, n in zip(INGEST_LISTS, (n_cv, n_pv, n_cp)):
        if n > EVENT_EDGE_LIMIT:
            raise ValueError(f"event_edges: {name} would hold {n} edges; a list is limited to {EVENT_EDGE_LIMIT} -- "
                             "lower max_events (the expansion is quadratic in a session's items)")
    # ---- offsets, then the rows
    off = [scan(count[k]) for k in range(3)]
    out = [i32(max(n, 1), 2) for n in (n_cv, n_pv, n_cp)]
    check(L.pc_events_emit(S, _p(rowptr), _p(bucket), _p(last), _p(n_items), cap, int(bool(exclusive)), _p(off[0]), _p(off[1]),
                           _p(off[2]), _p(out[0]), _p(out[1]), _p(out[2]), _stream()), "pc_events_emit")
    return EventEdges(out[0][:n_cv], out[1][:n_pv], out[2][:n_cp], S, int(skipped), int(items))


def epoch_permutation(n, seed, epoch, device):
    """pc_epoch_permutation: the epoch's order of n dataset positions, int32 [n] on the device (keyed Feistel bijection,
    cycle-walked: no sort kernels, no torch.randperm)."""
    out = torch.empty(int(n), dtype=torch.int32, device=device)
    check(_lib.lib().pc_epoch_permutation(int(n), int(seed) & (2 ** 64 - 1), int(epoch), _p(out), _stream()), "pc_epoch_permutation")
    return out


def shuffle_rows_i32(rows, seed, epoch):
    """pc_shuffle_rows_i32: rows [n,w] int32 -> the rows in the epoch's order (a new tensor)."""
    _req(rows, torch.int32, "rows")
    n, w = rows.shape
    out = torch.empty_like(rows)
    check(_lib.lib().pc_shuffle_rows_i32(_p(rows), n, w, int(seed) & (2 ** 64 - 1), int(epoch), _p(out), _stream()), "pc_shuffle_rows_i32")
    return out


def epoch_plan(order, deg, n, batch, n_batches):
    """pc_epoch_plan: per batch (padded neighbour count, real neighbour slots) -> int64 [n_batches,2] on the device."""
    _req(deg, torch.int32, "deg")
    if order is not None:
        _req(order, torch.int32, "order")
    plan = torch.empty(n_batches, 2, dtype=torch.int64, device=deg.device)
    check(_lib.lib().pc_epoch_plan(_p(order), _p(deg), int(n), int(batch), int(n_batches), _p(plan), _stream()), "pc_epoch_plan")
    return plan


def sample_negatives_zipf(pair_ids, graph, k_neg, seed, step, thresholds, perm=None, out=None, failed=None):
    """pc_sample_negatives_zipf: returns negative_idx [B,k_neg] (int32, device).  thresholds: uint32 device tensor from
    zipf_octave_thresholds (viewed as int32 storage).  failed: optional int32 [1] device counter of samples that ran out
    of proposals (see the header)."""
    b = pair_ids.numel()
    _req(pair_ids, torch.int32, "pair_ids"); _req(thresholds, torch.int32, "thresholds")
    if perm is not None:
        _req(perm, torch.int32, "perm", (int(graph["n_products"]),))
    ng = out if out is not None else torch.empty(b, k_neg, dtype=torch.int32, device=pair_ids.device)
    check(_lib.lib().pc_sample_negatives_zipf(_p(pair_ids), b, _p(graph["sim_pairs"]), _p(graph["sim_rowptr"]), _p(graph["sim_col"]),
                                              int(graph["n_products"]), int(k_neg), int(seed), int(step), _p(thresholds),
                                              thresholds.numel(), _p(perm), _p(ng), _p(failed), _stream()), "pc_sample_negatives_zipf")
    return ng


def shard_bucket(arrays, world, capacity, counts, send_ids, overflow, hot_rows=0, hot_ids=None, hot_served=None):
    """pc_shard_bucket[_hot].  arrays: up to four (ids int32 tensor, live-length device tensor or None, add) triples; returns
    the remapped index tensors (same shapes).  counts [world], send_ids [world*capacity], overflow [1]: int32 device.
    hot_rows > 0: ids of the replicated hot set (hot_ids ascending [hot_rows] int32, None = the ids below hot_rows) map to
    world * capacity + their position in the set and take no request slot; hot_served [1] int32 counts them."""
    n = len(arrays)
    if not 1 <= n <= 4:
        raise ValueError("1..4 id arrays per launch")
    outs = [torch.empty_like(_req(t, torch.int32, "ids")) for t, _, _ in arrays]
    _req(counts, torch.int32, "counts", (world,)); _req(send_ids, torch.int32, "send_ids", (world * capacity,))
    _req(overflow, torch.int32, "overflow", (1,))
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t, _, _ in arrays])
    lens = (ctypes.c_int * n)(*[t.numel() for t, _, _ in arrays])
    ndev = (ctypes.c_void_p * n)(*[(_req(d, torch.int32, "live length").data_ptr() if d is not None else None) for _, d, _ in arrays])
    nadd = (ctypes.c_int * n)(*[int(a) for _, _, a in arrays])
    optrs = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs])
    if hot_rows:
        if hot_ids is not None:
            _req(hot_ids, torch.int32, "hot_ids", (int(hot_rows),))
        if hot_served is not None:
            _req(hot_served, torch.int32, "hot_served", (1,))
        check(_lib.lib().pc_shard_bucket_hot(ptrs, lens, ndev, nadd, optrs, n, int(world), int(capacity), _p(hot_ids), int(hot_rows),
                                             _p(counts), _p(send_ids), _p(overflow), _p(hot_served), _stream()), "pc_shard_bucket_hot")
        return outs
    check(_lib.lib().pc_shard_bucket(ptrs, lens, ndev, nadd, optrs, n, int(world), int(capacity), _p(counts), _p(send_ids),
                                     _p(overflow), _stream()), "pc_shard_bucket")
    return outs


def dropout_hidden(x, dropout):
    """x * mask for the type-transition hidden layer (pc_dropout_hidden); dropout = (p, seed, offset)."""
    _req(x, torch.float32, "x")
    d = _lib.Dropout()
    d.p, d.seed, d.offset = float(dropout[0]), int(dropout[1]), int(dropout[2])
    if not 0.0 < d.p < 1.0:
        raise ValueError(f"dropout probability has to be between 0 and 1, but got {dropout[0]}")
    y = torch.empty_like(x)
    check(_lib.lib().pc_dropout_hidden(_p(x), x.numel(), ctypes.byref(d), _p(y), _stream()), "pc_dropout_hidden")
    return y


def check_indices(jobs, bad):
    """jobs: up to four (int32 index tensor, table rows, allow -1) triples; adds the number of out-of-range entries
    to the device counter `bad` ([1] int32).  Asynchronous: nothing is read back here."""
    n = len(jobs)
    if not 1 <= n <= 4:
        raise ValueError("1..4 index arrays per launch")
    _req(bad, torch.int32, "bad", (1,))
    ptrs = (ctypes.c_void_p * n)(*[_req(t, torch.int32, "idx").data_ptr() for t, _, _ in jobs])
    cnt = (ctypes.c_int * n)(*[t.numel() for t, _, _ in jobs])
    hi = (ctypes.c_int * n)(*[int(h) for _, h, _ in jobs])
    pad = (ctypes.c_int * n)(*[1 if a else 0 for _, _, a in jobs])
    check(_lib.lib().pc_check_indices(ptrs, cnt, hi, pad, n, _p(bad), _stream()), "pc_check_indices")


def hit_rank(sims):
    rows, cols = sims.shape
    _req(sims, torch.float32, "similarities")
    rank = torch.empty(rows, dtype=torch.int32, device=sims.device)
    check(_lib.lib().pc_hit_rank(_p(sims), rows, cols, _p(rank), _stream()), "pc_hit_rank")
    return rank


def cosine_rows(x, y):
    b, k, d = x.shape
    _width(d)
    _req(x, torch.float32, "predictions", (b, k, d)); _req(y, torch.float32, "ground_truth", (b, d))
    out = torch.empty(b * k, dtype=torch.float32, device=x.device)
    check(_lib.lib().pc_cosine_rows_dim(_p(x), _p(y), b, k, d, _p(out), _stream()), "pc_cosine_rows_dim")
    return out


def eval_batch_stats(proj, targets, pos_items, types):
    """metrics.py:88-109 for one batch without the [B*K, B] score matrix (pc_eval_batch_stats): proj [B,K,d], targets [B,d],
    pos_items [B,d], types [B,K] int32 -> (stats int32[5] = {hits_1, hits_3, hits_10, distinct_columns, rows}, cos_sum float[1]),
    both on the device; nothing is read back."""
    b, k, d = proj.shape
    _width(d)
    _req(proj, torch.float32, "projected_embeddings", (b, k, d)); _req(targets, torch.float32, "target_features", (b, d))
    _req(pos_items, torch.float32, "positive_items", (b, d)); _req(types, torch.int32, "complementary_types", (b, k))
    dev = proj.device
    stats = torch.empty(5, dtype=torch.int32, device=dev)
    cos_sum = torch.empty(1, dtype=torch.float32, device=dev)
    nbytes = _lib.lib().pc_joint_eval_workspace_bytes(b, 1, k, d)
    if nbytes == 0:
        raise ValueError(f"eval_batch_stats: batch {b}, k {k} (1..8), width {d} not served")
    ws = workspace(nbytes, dev, "eval")
    check(_lib.lib().pc_eval_batch_stats(_p(proj), _p(targets), _p(pos_items), _p(types), b, k, d, _p(stats), _p(cos_sum),
                                         _p(ws), ws.numel(), _stream()), "pc_eval_batch_stats")
    return stats, cos_sum


def joint_eval_epoch(params, pairs, source, first_step, batch, k, bad=None):
    """Metrics.evaluate_model (metrics.py:62-117) over `pairs` [n,3] int32 (loader order, on the device) as ONE foreign call
    (pc_joint_eval_epoch).  params: the model's tensors plus "product_embeddings.weight"; source = (features, type_idx,
    n_types, seed) of the loader; first_step: its step counter.  Returns a dict of device tensors -- "metrics" double[5] =
    (hit@1, hit@3, hit@10, type_diversity, mean_relevance), "stats" int32[n_batches,5], "cos_sum" float[n_batches],
    "topk_table" int32[T,k] (the plan's complementary types, a view into the workspace: valid until the next evaluation on
    this stream) -- and nothing is read back here."""
    st, dev = joint_struct(params)
    features, type_idx, n_types, seed = source
    table = params["product_embeddings.weight"]
    n_products, d = table.shape
    _width(d)
    _req(features, torch.float32, "features", (n_products, d)); _req(type_idx, torch.int32, "type_idx", (n_products,))
    n = int(pairs.shape[0])
    _req(pairs, torch.int32, "pairs", (n, 3))
    if bad is not None:
        _req(bad, torch.int32, "bad", (1,))
    t = params["query_type_embeddings.weight"].shape[0]
    b = int(batch)
    n_batches = (n + b - 1) // b
    stats = torch.empty(max(n_batches, 1), 5, dtype=torch.int32, device=dev)
    cos_sum = torch.empty(max(n_batches, 1), dtype=torch.float32, device=dev)
    metrics = torch.empty(5, dtype=torch.float64, device=dev)
    nbytes = _lib.lib().pc_joint_eval_workspace_bytes(b, t, int(k), d)
    ws = workspace(max(nbytes, 256), dev, "eval")
    check(_lib.lib().pc_joint_eval_epoch(ctypes.byref(st), _p(pairs), n, _p(features), _p(type_idx), int(n_types), d, int(seed),
                                         int(first_step), b, t, int(k), n_products, _p(stats), _p(cos_sum), _p(metrics),
                                         _p(bad), _p(ws), ws.numel(), _stream()), "pc_joint_eval_epoch")
    topk_table = ws[:t * int(k) * 4].view(torch.int32).view(t, int(k))
    return {"metrics": metrics, "stats": stats[:n_batches], "cos_sum": cos_sum[:n_batches], "topk_table": topk_table}


def build_complementary_batch(pairs, features, type_idx, n_types, seed, step, want_targets=True, out=None):
    """pairs [B,3] int32 (query, target, label) on the device -> the joint-step batch dict.  `out`: a dict of
    preallocated tensors of those shapes to build into (fixed buffers of a graphed step).  The item rows are as wide as
    `features`: 128 (pc_build_complementary_batch) or 256 (pc_build_complementary_batch_dim, BASELINE configs[4])."""
    b = pairs.shape[0]
    _req(pairs, torch.int32, "pairs", (b, 3)); _req(features, torch.float32, "features"); _req(type_idx, torch.int32, "type_idx")
    d = features.shape[1] if features.dim() == 2 else -1
    if d not in (D, 2 * D):
        raise ValueError(f"build_complementary_batch: features must be [P, {D}] or [P, {2 * D}], got {tuple(features.shape)}")
    dev = pairs.device
    i32 = lambda: torch.empty(b, dtype=torch.int32, device=dev)
    f32 = lambda: torch.empty(b, d, dtype=torch.float32, device=dev)
    if out is not None:
        out = dict(out)
        for k in ("query_idx", "query_types", "positive_types", "negative_types"):
            _req(out[k], torch.int32, k)
            if out[k].numel() != b:
                raise ValueError("build_complementary_batch: out[%r] has %d elements, batch is %d" % (k, out[k].numel(), b))
        for k in ("positive_items", "negative_items"):
            _req(out[k], torch.float32, k, (b, d))
        want_targets = "target_features" in out
    else:
        out = {"query_idx": i32(), "query_types": i32(), "positive_types": i32(), "negative_types": i32(),
               "positive_items": f32(), "negative_items": f32()}
        if want_targets:
            out["target_features"] = f32()
    if d == D:
        check(_lib.lib().pc_build_complementary_batch(
            _p(pairs), b, _p(features), _p(type_idx), int(n_types), int(seed), int(step), _p(out["query_idx"]),
            _p(out["query_types"]), _p(out["positive_types"]), _p(out["negative_types"]), _p(out["positive_items"]),
            _p(out["negative_items"]), _p(out.get("target_features")), _stream()), "pc_build_complementary_batch")
    else:
        check(_lib.lib().pc_build_complementary_batch_dim(
            _p(pairs), b, _p(features), _p(type_idx), int(n_types), d, int(seed), int(step), _p(out["query_idx"]),
            _p(out["query_types"]), _p(out["positive_types"]), _p(out["negative_types"]), _p(out["positive_items"]),
            _p(out["negative_items"]), _p(out.get("target_features")), _stream()), "pc_build_complementary_batch_dim")
    out["positive_types"] = out["positive_types"].view(b, 1)
    out["negative_types"] = out["negative_types"].view(b, 1)
    return out


SPLIT_MODES = {"train": 0, "val": 1, "test": 2}


def split_bounds(n, mode):
    """[lo, hi) of a mode in the shuffled labelled list of n pairs: the host split of data.py (data_loader.py:121-126)."""
    return {"train": (0, int(0.8 * n)), "val": (int(0.8 * n), int(0.9 * n)), "test": (int(0.9 * n), n)}[mode]


def comp_split_pairs(comp_pairs, sim_pairs, seed, mode):
    """pc_comp_split_pairs: the labelled pairs [n_mode,3] int32 (query, target, +1 / -1) of `mode` ('train' / 'val' / 'test')
    on the device -- L = [comp_pairs (+1) ..., sim_pairs (-1) ...] in the keyed order of epoch_permutation(n, seed, mode),
    rows [lo, hi) of the host split.  Neither L nor the permutation is built."""
    _req(comp_pairs, torch.int32, "comp_pairs"); _req(sim_pairs, torch.int32, "sim_pairs")
    for t, nm in ((comp_pairs, "comp_pairs"), (sim_pairs, "sim_pairs")):
        if t.dim() != 2 or t.shape[1] != 2:
            raise ValueError(f"comp_split_pairs: {nm} must be [n, 2], got {tuple(t.shape)}")
    if mode not in SPLIT_MODES:
        raise ValueError("comp_split_pairs: mode must be 'train', 'val' or 'test'")
    n_comp, n_sim = comp_pairs.shape[0], sim_pairs.shape[0]
    lo, hi = split_bounds(n_comp + n_sim, mode)
    out = torch.empty(max(hi - lo, 1), 3, dtype=torch.int32, device=comp_pairs.device)
    check(_lib.lib().pc_comp_split_pairs(_p(comp_pairs) if n_comp else None, n_comp, _p(sim_pairs) if n_sim else None, n_sim,
                                         lo, hi, int(seed) & (2 ** 64 - 1), SPLIT_MODES[mode], _p(out), _stream()),
          "pc_comp_split_pairs")
    return out[:hi - lo]


def retrieve_topk(proj, types, type_rowptr, type_col, table, n):
    """pc_retrieve_topk: proj [R,128] fp32, types [R] int32 -> (idx [R,n] int32 product indices, -1 = none;
    scores [R,n] fp32).  inference.py:90-118 for all rows at once."""
    d = _width(table.shape[1])
    proj = _req(proj.reshape(-1, d), torch.float32, "proj")
    r = proj.shape[0]
    _req(types, torch.int32, "types", (r,))
    _req(type_rowptr, torch.int32, "type_rowptr")
    _req(type_col, torch.int32, "type_col")
    _req(table, torch.float32, "table")
    out_idx = torch.empty(r, n, dtype=torch.int32, device=proj.device)
    out_sc = torch.empty(r, n, dtype=torch.float32, device=proj.device)
    check(_lib.lib().pc_retrieve_topk_dim(_p(proj), _p(types), r, _p(type_rowptr), _p(type_col), _p(table),
                                          type_rowptr.numel() - 1, int(n), d, _p(out_idx), _p(out_sc), _stream()),
          "pc_retrieve_topk_dim")
    return out_idx, out_sc


RETRIEVE_MAX_SLICES = 64


def _table_width(table, name="table", rows=False, dtype=torch.float32):
    """D of a [P, D] fp32 device table (dtype: of another element type), D 128 or 256 (rows: P >= 1 too)."""
    _req(table, dtype, name)
    if table.dim() != 2:
        raise ValueError(f"{name}: expected [P, D], got shape {tuple(table.shape)}")
    d = _width(table.shape[1])
    if rows and table.shape[0] < 1:
        raise ValueError(f"{name}: expected at least one row")
    return d


def catalogue_bf16(features):
    """The bf16 copy of a catalogue that retrieve_topk_grouped serves from: [P, D] fp32 on the device -> [P, D] torch.bfloat16,
    rounded to nearest even, half the bytes.  Once per catalogue, off the serving path: no kernel of its own."""
    _table_width(features, "features")
    return features.to(torch.bfloat16)


def _check_exclude(what, exclude, rows):
    """exclude = (row_key [rows] int32, ex_rowptr [n_keys + 1] int32, ex_col [E] int32), checked on the host side alone (dtypes
    and shapes: ValueError) before any tensor is handed to the device."""
    if not isinstance(exclude, (tuple, list)) or len(exclude) != 3 or not all(isinstance(t, torch.Tensor) for t in exclude):
        raise ValueError(f"{what}: exclude must be the triple (row_key, ex_rowptr, ex_col) of tensors")
    row_key, ex_rowptr, ex_col = exclude
    for name, t in (("row_key", row_key), ("ex_rowptr", ex_rowptr), ("ex_col", ex_col)):
        if t.dtype != torch.int32:
            raise ValueError(f"{what}: exclude {name} must be int32, got {t.dtype}")
        if t.dim() != 1:
            raise ValueError(f"{what}: exclude {name} must be 1-D, got shape {tuple(t.shape)}")
    if row_key.shape[0] != rows:
        raise ValueError(f"{what}: exclude row_key must hold one key per row ({rows}), got {row_key.shape[0]}")
    if ex_rowptr.numel() < 1:
        raise ValueError(f"{what}: exclude ex_rowptr must hold n_keys + 1 >= 1 entries")
    return row_key, ex_rowptr, ex_col


def _filter_args(exclude, bad, device, counted=False):
    """A checked triple and the caller's counter as device arguments: (row_key, ex_rowptr, ex_col -- one unread entry where
    every list is empty --, n_keys, bad -- a fresh zero where the caller gave none).  Without a triple: (None, None, None, 0,
    None) -- null pointers -- and, for an entry that counts other things too (counted), the counter."""
    if exclude is None:
        return None, None, None, 0, _bad_counter(bad, device) if counted else None
    row_key, ex_rowptr, ex_col = exclude
    _req(row_key, torch.int32, "exclude row_key")
    _req(ex_rowptr, torch.int32, "exclude ex_rowptr")
    if ex_col.numel() == 0:
        ex_col = torch.zeros(1, dtype=torch.int32, device=ex_rowptr.device)
    _req(ex_col, torch.int32, "exclude ex_col")
    return row_key, ex_rowptr, ex_col, ex_rowptr.numel() - 1, _bad_counter(bad, device)


def _list_pair(what, idx, score, shape):
    """idx int32 / score fp32 of one shape, as many dimensions as `shape` ("[R, m]": the function's own wording) names -> the
    shape."""
    _req(idx, torch.int32, "idx")
    _req(score, torch.float32, "score")
    if idx.dim() != shape.count(",") + 1 or tuple(score.shape) != tuple(idx.shape):
        raise ValueError(f"{what}: expected idx and score of one shape {shape}, got {tuple(idx.shape)} and "
                         f"{tuple(score.shape)}")
    return tuple(idx.shape)


def _optional(what, t, dtype, name, wording, shape=None):
    """An optional device tensor argument (None passes): anything but a tensor is refused under the function's name with the
    wording of the shape ("[P]"), a tensor goes through _req."""
    if t is None:
        return
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{what}: {name} must be a {wording} {str(dtype)[6:]} device tensor, got {type(t).__name__}")
    _req(t, dtype, name, shape)


def _counters(**counters):
    """The [1] int32 device counters a caller may pass to see a count (None: not asked for)."""
    for name, t in counters.items():
        if t is not None:
            _req(t, torch.int32, name, (1,))


def _exclusion_pair(what, exclude, source, num_products, device):
    """fuse_lists' / fuse_sessions' exclude = (ex_rowptr [P + 1], ex_col) beside their num_products -> (ex_rowptr, ex_col,
    num_products) as device arguments: without a pair (None, None, the argument or 2^31 - 1); with one, num_products is the
    pair's P (an argument that disagrees is refused) and an empty ex_col is one unread entry, so that the pointer is not null."""
    ex_rowptr = ex_col = None
    if exclude is not None:
        if source is None:
            raise ValueError(f"{what}: exclude is keyed by the rows' source ids and needs source")
        if not isinstance(exclude, (tuple, list)) or len(exclude) != 2 or not all(isinstance(t, torch.Tensor) for t in exclude):
            raise ValueError(f"{what}: exclude must be the pair (ex_rowptr, ex_col) of int32 device tensors")
        ex_rowptr, ex_col = exclude
        _req(ex_rowptr, torch.int32, "ex_rowptr")
        _req(ex_col, torch.int32, "ex_col")
        if ex_rowptr.dim() != 1 or ex_rowptr.numel() < 2 or ex_col.dim() != 1:
            raise ValueError(f"{what}: expected ex_rowptr [P + 1] with P >= 1 and a 1-D ex_col, got "
                             f"{tuple(ex_rowptr.shape)} and {tuple(ex_col.shape)}")
        if num_products is not None and int(num_products) != ex_rowptr.numel() - 1:
            raise ValueError(f"{what}: num_products {int(num_products)} does not match the exclusion set's "
                             f"{ex_rowptr.numel() - 1} keys")
        num_products = ex_rowptr.numel() - 1
        if ex_col.numel() == 0:
            ex_col = torch.zeros(1, dtype=torch.int32, device=device)
    num_products = 2 ** 31 - 1 if num_products is None else int(num_products)
    if not 1 <= num_products <= 2 ** 31 - 1:
        raise ValueError(f"{what}: num_products must be in [1, 2^31 - 1], got {num_products}")
    return ex_rowptr, ex_col, num_products


def _list_out(rows, n, device, support=False):
    """The served lists' outputs: (idx [rows, n] int32, score [rows, n] fp32) and, with support, support [rows, n] int32."""
    out = (torch.empty(rows, n, dtype=torch.int32, device=device), torch.empty(rows, n, dtype=torch.float32, device=device))
    return out + (torch.empty(rows, n, dtype=torch.int32, device=device),) if support else out


def half_sq_norm_bias(table):
    """pc_half_sq_norm_bias: bias[p] = -0.5 * |table[p]|^2 for a [P, D] fp32 device table -> [P] fp32, the per-product term under
    which retrieve_topk_grouped / rank_grouped (bias=) order by Euclidean distance: |q - e|^2 = |q|^2 - 2 (<q, e> + bias).  One
    fixed summation order per row, no atomics: the same bits on every run.  Once per catalogue."""
    d = _table_width(table, rows=True)
    out = torch.empty(table.shape[0], dtype=torch.float32, device=table.device)
    check(_lib.lib().pc_half_sq_norm_bias(_p(table), table.shape[0], d, _p(out), _stream()), "pc_half_sq_norm_bias")
    return out


def _check_bias(what, bias, table):
    """bias: a [P] fp32 tensor beside an fp32 table, checked on the host side alone (ValueError) before any launch."""
    if not isinstance(bias, torch.Tensor):
        raise ValueError(f"{what}: bias must be a [P] float32 device tensor, got {type(bias).__name__}")
    if isinstance(table, torch.Tensor) and table.dtype == torch.bfloat16:
        raise ValueError(f"{what}: bias with a bf16 table is not supported (the biased entries read the fp32 table)")
    if bias.dtype != torch.float32:
        raise ValueError(f"{what}: bias of dtype {bias.dtype} is not supported: it must be float32")
    if bias.dim() != 1 or bias.shape[0] != table.shape[0]:
        raise ValueError(f"{what}: bias of shape {tuple(bias.shape)} is not supported: it must hold one entry per product "
                         f"({table.shape[0]})")


def _grouped_rows(proj, types, type_rowptr, type_col, table, table_dtype, slices):
    """The rows of a grouped call, checked: (proj as [R, D], R, the number of types, D, slices)."""
    slices = int(slices)
    if not 0 <= slices <= RETRIEVE_MAX_SLICES:
        raise ValueError(f"slices must be in [0, {RETRIEVE_MAX_SLICES}] (0 = automatic), got {slices}")
    d = _width(table.shape[1])
    proj = _req(proj.reshape(-1, d), torch.float32, "proj")
    r = proj.shape[0]
    _req(types, torch.int32, "types", (r,))
    _req(type_rowptr, torch.int32, "type_rowptr")
    _req(type_col, torch.int32, "type_col")
    _req(table, table_dtype, "table")
    return proj, r, type_rowptr.numel() - 1, d, slices


def _grouped_call(name, tag, device, sizes, args, sized_as=None):
    """Entry `name` of the grouped family with `args`, its arguments in the header's order up to the workspace; behind them
    go the workspace that NAME_workspace_bytes(*sizes) asks for (sized_as: another entry's query), its byte count and the
    stream.  In the lists of this family a tensor that is always there travels as its data_ptr() -- the address that _p wraps,
    without a call and an object per pointer -- and one that may be absent through _p (None: a null pointer)."""
    lib = _lib.lib()
    ws = workspace(getattr(lib, (sized_as or name) + "_workspace_bytes")(*sizes), device, tag)
    check(getattr(lib, name)(*args, ws.data_ptr(), ws.numel(), _stream()), name)


def _retrieve_grouped(name, proj, types, type_rowptr, type_col, table, n, slices, exclude, bad, *, bias=None,
                      what="retrieve_topk_grouped", tag="retrieve_grouped", table_dtype=torch.float32, where=None):
    """retrieve_topk_grouped / retrieve_list_grouped behind the choice of the entry (where: a RowWhere, for the entries that
    take a pc_row_where behind bad_count)."""
    if exclude is not None:
        exclude = _check_exclude(what, exclude, types.shape[0] if isinstance(types, torch.Tensor) else -1)
    elif bad is not None:
        raise ValueError(f"{what}: bad counts keys out of range and is read with an exclude triple only")
    proj, r, t, d, slices = _grouped_rows(proj, types, type_rowptr, type_col, table, table_dtype, slices)
    device = proj.device
    out_idx = torch.empty(r, n, dtype=torch.int32, device=device)
    out_sc = torch.empty(r, n, dtype=torch.float32, device=device)
    if name == "pc_retrieve_topk_grouped":
        args = (proj.data_ptr(), types.data_ptr(), r, type_rowptr.data_ptr(), type_col.data_ptr(), table.data_ptr(), t, n, d,
                slices, out_idx.data_ptr(), out_sc.data_ptr())
    else:
        # (the filtered entries' list, bias behind table where the entry has it; without a triple row_key, ex_rowptr, ex_col
        # and bad are None: null pointers, n_keys 0)
        row_key, ex_rowptr, ex_col, n_keys, bad = _filter_args(exclude, bad, device)
        bias = () if bias is None else (_req(bias, torch.float32, "bias", (table.shape[0],)).data_ptr(),)
        args = (proj.data_ptr(), types.data_ptr(), _p(row_key), r, type_rowptr.data_ptr(), type_col.data_ptr(), table.data_ptr(),
                *bias, t, _p(ex_rowptr), _p(ex_col), n_keys, n, d, slices, out_idx.data_ptr(), out_sc.data_ptr(), _p(bad))
        if where is not None:
            args += (ctypes.byref(where._struct(what, table.shape[0], r)),)
    _grouped_call(name, tag, device, (r, t, n, slices), args)
    return out_idx, out_sc


def retrieve_topk_grouped(proj, types, type_rowptr, type_col, table, n, slices=0, exclude=None, bad=None, bias=None):
    """pc_retrieve_topk_grouped: retrieve_topk's contract (idx [R,n] int32, -1 = none; scores [R,n] fp32, -inf = none) for a
    catalogue of any size -- rows grouped by type on the device, each type's candidates scored as a tiled fp32 MFMA GEMM,
    large types split over up to `slices` candidate slices (0 = automatic).  Bitwise deterministic, the same bits for every
    `slices`.  Nothing is read back to the host.
    exclude = (row_key [R] int32, ex_rowptr [n_keys + 1] int32, ex_col [E] int32), an exclusion CSR over keys as
    exclusion_csr builds it (the ids of a key strictly ascending): pc_retrieve_topk_grouped_excluding -- the first n products of
    the type that are NOT in the list of row_key[r] (-1: no list), the same order and the same bits.  A key outside
    [-1, n_keys) is served as -1 and counted in `bad` (a [1] int32 device counter the caller passes to see the count; added
    to).  exclude=None: exactly the unfiltered call.
    table: [P, D] fp32, or the [P, D] torch.bfloat16 copy catalogue_bf16 makes of it: pc_retrieve_topk_grouped_bf16 -- the
    same contract, order and determinism over half the bytes, with or without exclude; the scores are the fp32-grade dot
    products of the unrounded proj with the ROUNDED table (the query is split into three bf16 pieces, the products are
    exact), so a list can differ from the fp32 table's where two products lie within bf16 rounding of each other.
    bias: a [P] fp32 device tensor (fp32 table only): pc_retrieve_topk_grouped_biased -- the same contract, order and
    determinism under the score fl(<proj[r], table[p]> + bias[p]), one fp32 addition after the unbiased entry's own chain (a
    zero bias gives that entry's bits), with or without exclude; half_sq_norm_bias(table) makes the order Euclidean.
    bias=None: exactly the calls above."""
    bf16 = isinstance(table, torch.Tensor) and table.dtype == torch.bfloat16
    if bias is not None:
        _check_bias("retrieve_topk_grouped", bias, table)
        name = "pc_retrieve_topk_grouped_biased"
    elif bf16:
        name = "pc_retrieve_topk_grouped_bf16"
    else:
        name = "pc_retrieve_topk_grouped" if exclude is None else "pc_retrieve_topk_grouped_excluding"
    return _retrieve_grouped(name, proj, types, type_rowptr, type_col, table, int(n), slices, exclude, bad, bias=bias,
                             table_dtype=torch.bfloat16 if bf16 else torch.float32)


RETRIEVE_LIST_MAX_N = 256


def retrieve_list_grouped(proj, types, type_rowptr, type_col, table, n, slices=0, exclude=None, bad=None):
    """pc_retrieve_list_grouped: retrieve_topk_grouped's contract (idx [R,n] int32, -1 = none; scores [R,n] fp32, -inf = none)
    for lists of 1 <= n <= RETRIEVE_LIST_MAX_N products -- the same plan, candidate slices and score chain; a row keeps an
    unsorted candidate buffer and a threshold on chip in place of the per-thread lists of 16.  Bitwise deterministic, the same
    bits for every `slices`, and for n <= 16 retrieve_topk_grouped's own bits.  Nothing is read back to the host.
    exclude = (row_key [R] int32, ex_rowptr [n_keys + 1] int32, ex_col [E] int32) and `bad` as in retrieve_topk_grouped: the
    first n products of the type that are NOT in the list of row_key[r].  exclude=None: the unfiltered list.
    table: [P, D] fp32, or the [P, D] torch.bfloat16 copy catalogue_bf16 makes of it: pc_retrieve_list_grouped_bf16 -- the same
    contract, selection and determinism over half the bytes, the scores formed through retrieve_topk_grouped's bf16 chain (the
    unrounded proj against the ROUNDED table): for n <= 16 that call's own bits."""
    n = int(n)
    if not 1 <= n <= RETRIEVE_LIST_MAX_N:
        raise ValueError(f"retrieve_list_grouped: n must be in [1, {RETRIEVE_LIST_MAX_N}], got {n}")
    bf16 = isinstance(table, torch.Tensor) and table.dtype == torch.bfloat16
    return _retrieve_grouped("pc_retrieve_list_grouped_bf16" if bf16 else "pc_retrieve_list_grouped", proj, types, type_rowptr,
                             type_col, table, n, slices, exclude, bad, what="retrieve_list_grouped", tag="retrieve_list",
                             table_dtype=torch.bfloat16 if bf16 else torch.float32)


def retrieve_list_grouped_biased(proj, types, type_rowptr, type_col, table, bias, n, slices=0, exclude=None, bad=None):
    """pc_retrieve_list_grouped_biased: retrieve_list_grouped's contract (idx [R,n] int32, -1 = none; scores [R,n] fp32, -inf =
    none; 1 <= n <= RETRIEVE_LIST_MAX_N; exclude and `bad` as there) under retrieve_topk_grouped(bias=)'s score
    fl(<proj[r], table[p]> + bias[p]) -- one fp32 addition after retrieve_list_grouped's own chain.  bias: a [P] fp32 device
    tensor beside an fp32 table; half_sq_norm_bias(table) makes the order Euclidean.  The same kernel body, merge and
    determinism: the same bits for every `slices`; for n <= 16 retrieve_topk_grouped(bias=)'s own bits, with a zero bias
    retrieve_list_grouped's, and rank_grouped(bias=) < n exactly when the list holds the target at that position.  Nothing is
    read back to the host."""
    n = int(n)
    if not 1 <= n <= RETRIEVE_LIST_MAX_N:
        raise ValueError(f"retrieve_list_grouped_biased: n must be in [1, {RETRIEVE_LIST_MAX_N}], got {n}")
    _check_bias("retrieve_list_grouped_biased", bias, table)
    return _retrieve_grouped("pc_retrieve_list_grouped_biased", proj, types, type_rowptr, type_col, table, n, slices, exclude, bad,
                             bias=bias, what="retrieve_list_grouped_biased", tag="retrieve_list")


def _check_rank_lists(what, exclude, cand_type, types, table):
    """A rank function's exclude triple beside its cand_type, checked on the host side alone (ValueError): both or neither, the
    triple as _check_exclude has it, cand_type an int32 tensor of one entry per product -> the checked triple (None: none)."""
    if exclude is None:
        if cand_type is not None:
            raise ValueError(f"{what}: cand_type is read with an exclude triple only")
        return None
    exclude = _check_exclude(what, exclude, types.shape[0] if isinstance(types, torch.Tensor) else -1)
    if cand_type is None:
        raise ValueError(f"{what}: exclude needs cand_type (the type under which each product is a candidate)")
    if not isinstance(cand_type, torch.Tensor) or cand_type.dtype != torch.int32 or cand_type.dim() != 1 \
            or cand_type.shape[0] != table.shape[0]:
        raise ValueError(f"{what}: cand_type must be an int32 tensor of one entry per product")
    return exclude


def _req_rank_extras(exclude, cand_type, bias, p):
    """The device checks of a rank call's cand_type (read with a triple only) and bias."""
    if exclude is not None:
        _req(cand_type, torch.int32, "cand_type", (p,))
    if bias is not None:
        _req(bias, torch.float32, "bias", (p,))


def _rank_call(name, what, proj, types, targets, type_rowptr, type_col, table, table_dtype, slices, bad, exclude, cand_type, bias,
               where=None, sized_as=None):
    """Rank entry `name` behind its function's own checks -> (rank [R] int32, bad [1] int32): the rows, the outputs, the lists
    as device arguments and the device checks of cand_type and bias, then the arguments in the header's order --
    pc_rank_grouped's short list, or the filtered entries' (bias behind table in every entry but pc_rank_grouped_excluding, a
    pc_row_where behind bad_count).  Without a triple row_key, ex_rowptr, ex_col and cand_type are None, without a bias it
    too: null pointers, n_keys 0.  where (a RowWhere): its lengths against P and R and the device checks come before anything
    is allocated; the functions without one have always allocated first, and keep that order."""
    proj, r, t, d, slices = _grouped_rows(proj, types, type_rowptr, type_col, table, table_dtype, slices)
    _req(targets, torch.int32, "targets", (r,))
    p, device = table.shape[0], proj.device
    tail = ()
    if where is not None:
        tail = (ctypes.byref(where._struct(what, p, r)),)
        _req_rank_extras(exclude, cand_type, bias, p)
    rank = torch.empty(r, dtype=torch.int32, device=device)
    row_key, ex_rowptr, ex_col, n_keys, bad = _filter_args(exclude, bad, device, counted=True)
    if where is None:
        _req_rank_extras(exclude, cand_type, bias, p)
    if name == "pc_rank_grouped":
        args = (proj.data_ptr(), types.data_ptr(), targets.data_ptr(), r, type_rowptr.data_ptr(), type_col.data_ptr(),
                table.data_ptr(), t, p, d, slices, rank.data_ptr(), bad.data_ptr())
    else:
        args = (proj.data_ptr(), types.data_ptr(), targets.data_ptr(), _p(row_key), r, type_rowptr.data_ptr(), type_col.data_ptr(),
                table.data_ptr(), *(() if name == "pc_rank_grouped_excluding" else (_p(bias),)), t, p, _p(ex_rowptr), _p(ex_col),
                n_keys, _p(cand_type), d, slices, rank.data_ptr(), bad.data_ptr(), *tail)
    _grouped_call(name, "rank_grouped", device, (r, t, slices), args, sized_as)
    return rank, bad


def rank_grouped(proj, types, targets, type_rowptr, type_col, table, slices=0, bad=None, exclude=None, cand_type=None,
                 bias=None):
    """pc_rank_grouped: for row r the number of products of type types[r] that retrieve_topk_grouped orders in front of
    targets[r] under proj[r] (score descending, product index ascending) -- the position of the target in the served list,
    over the whole type, from the retrieval's own score bits: rank < n exactly when retrieve_topk_grouped(..., n) holds the
    target at position rank.  Returns (rank [R] int32, bad [1] int32): rank -1 for a row with types[r] < 0 (skipped) and for
    a type >= the CSR's or a target outside the table, which `bad` counts (`bad`: a device counter to add to; a fresh zero
    otherwise).  Bitwise deterministic, the same for every `slices`.  Nothing is read back to the host.
    exclude = (row_key, ex_rowptr, ex_col) as in retrieve_topk_grouped, with cand_type [P] int32 (the type under which product
    p is a candidate, -1 if none; it must agree with type_rowptr / type_col): pc_rank_grouped_excluding -- the number of
    NON-excluded products of the type in front of the target, -1 where the target is in the row's list or is no candidate of
    the row's type; rank < n exactly when the filtered retrieval holds the target at position rank.  A key outside
    [-1, n_keys) is served as -1 and counted in `bad`.  exclude=None: exactly the unfiltered call.
    bias: a [P] fp32 device tensor: pc_rank_grouped_biased -- the same counts under retrieve_topk_grouped(bias=)'s score
    fl(<proj[r], table[p]> + bias[p]), with or without exclude / cand_type: rank < n exactly when that call holds the target at
    position rank.  bias=None: exactly the calls above."""
    if bias is not None:
        _check_bias("rank_grouped", bias, table)
    exclude = _check_rank_lists("rank_grouped", exclude, cand_type, types, table)
    if bias is not None:
        name, sized_as = "pc_rank_grouped_biased", None
    else:
        name, sized_as = ("pc_rank_grouped" if exclude is None else "pc_rank_grouped_excluding"), "pc_rank_grouped"
    return _rank_call(name, "rank_grouped", proj, types, targets, type_rowptr, type_col, table, torch.float32, slices, bad, exclude,
                      cand_type, bias, sized_as=sized_as)


def half_sq_norm_bias_bf16(table):
    """pc_half_sq_norm_bias_bf16: half_sq_norm_bias for the [P, D] torch.bfloat16 copy of a catalogue (catalogue_bf16; a
    CompactCatalogue's .table) -> [P] fp32: the terms of the ROUNDED rows, bit for bit half_sq_norm_bias(table.float()),
    without the fp32 table ever being formed.  Under it retrieve_list_grouped_bf16_biased / rank_grouped_bf16 order by Euclidean
    distance to the stored rows."""
    if isinstance(table, torch.Tensor) and table.dtype == torch.float32:
        raise ValueError("half_sq_norm_bias_bf16: an fp32 table is half_sq_norm_bias's; this function reads the bf16 copy")
    d = _table_width(table, rows=True, dtype=torch.bfloat16)
    out = torch.empty(table.shape[0], dtype=torch.float32, device=table.device)
    check(_lib.lib().pc_half_sq_norm_bias_bf16(_p(table), table.shape[0], d, _p(out), _stream()), "pc_half_sq_norm_bias_bf16")
    return out


def _check_bf16_table(what, table, fp32_name):
    """table: a [P, D] torch.bfloat16 tensor, checked on the host side alone (ValueError) before any launch; an fp32 table
    is pointed at the fp32 function."""
    if not isinstance(table, torch.Tensor):
        raise ValueError(f"{what}: table must be a [P, D] bfloat16 device tensor, got {type(table).__name__}")
    if table.dtype == torch.float32:
        raise ValueError(f"{what}: an fp32 table is {fp32_name}'s; this function reads the bf16 copy (catalogue_bf16)")
    if table.dtype != torch.bfloat16:
        raise ValueError(f"{what}: table of dtype {table.dtype} is not supported: it must be bfloat16")
    if table.dim() != 2:
        raise ValueError(f"{what}: table must be [P, D], got shape {tuple(table.shape)}")


def _check_bias_bf16(what, bias, table):
    """bias: a [P] fp32 tensor beside a bf16 table, checked on the host side alone (ValueError) before any launch."""
    if not isinstance(bias, torch.Tensor):
        raise ValueError(f"{what}: bias must be a [P] float32 device tensor, got {type(bias).__name__}")
    if bias.dtype != torch.float32:
        raise ValueError(f"{what}: bias of dtype {bias.dtype} is not supported: it must be float32")
    if bias.dim() != 1 or bias.shape[0] != table.shape[0]:
        raise ValueError(f"{what}: bias of shape {tuple(bias.shape)} is not supported: it must hold one entry per product "
                         f"({table.shape[0]})")


def retrieve_list_grouped_bf16_biased(proj, types, type_rowptr, type_col, table, bias, n, slices=0, exclude=None, bad=None):
    """pc_retrieve_list_grouped_bf16_biased: retrieve_list_grouped_biased's contract (idx [R,n] int32, -1 = none; scores [R,n]
    fp32, -inf = none; 1 <= n <= RETRIEVE_LIST_MAX_N; exclude and `bad` as there) over the [P, D] torch.bfloat16 copy of a
    catalogue, under the score fl(s + bias[p]) with s retrieve_list_grouped's own bf16 score of the pair -- one fp32 addition
    after that chain.  bias: a [P] fp32 device tensor; half_sq_norm_bias_bf16(table) makes the order Euclidean over the stored
    rows.  The same kernel body, merge and determinism: the same bits for every `slices`; with a zero bias
    retrieve_list_grouped(table)'s bit for bit; rank_grouped_bf16(bias=) < n exactly when the list holds the target at that
    position.  It serves n <= 16 too (there is no 16-entry biased bf16 kernel).  A function of its own:
    retrieve_list_grouped_biased refuses a bf16 table.  Nothing is read back to the host."""
    what = "retrieve_list_grouped_bf16_biased"
    n = int(n)
    if not 1 <= n <= RETRIEVE_LIST_MAX_N:
        raise ValueError(f"{what}: n must be in [1, {RETRIEVE_LIST_MAX_N}], got {n}")
    _check_bf16_table(what, table, "retrieve_list_grouped_biased")
    _check_bias_bf16(what, bias, table)
    return _retrieve_grouped("pc_retrieve_list_grouped_bf16_biased", proj, types, type_rowptr, type_col, table, n, slices, exclude,
                             bad, bias=bias, what=what, tag="retrieve_list", table_dtype=torch.bfloat16)


class RowWhere:
    """pc_row_where, checked: the per-product attributes of a catalogue and a per-row predicate over them, for
    retrieve_list_grouped_where.  Every part may be None.
      value [P] float32, flags [P] int32 (read as 32 bits): the attributes, installed once per catalogue;
      lo, hi [R] float32: product p passes row r iff lo[r] <= value[p] <= hi[r] -- two fp32 compares: the ends are inclusive,
                          a NaN value or bound passes nothing, lo > hi passes nothing, -inf / +inf pass every non-NaN value;
                          both with value and neither without (a one-sided caller passes an infinite bound);
      need, deny [R] int32: p passes iff (flags[p] & need[r]) == need[r] and (flags[p] & deny[r]) == 0; only with flags, an
                          absent one is 0.
    Dtypes, 1-D shapes, one device for all parts and the pairing rule are checked here, on the host side alone (ValueError);
    the lengths against P and R at the call."""

    ATTRIBUTES = (("value", torch.float32), ("flags", torch.int32))
    PREDICATE = (("lo", torch.float32), ("hi", torch.float32), ("need", torch.int32), ("deny", torch.int32))

    def __init__(self, value=None, flags=None, lo=None, hi=None, need=None, deny=None):
        parts = dict(value=value, flags=flags, lo=lo, hi=hi, need=need, deny=deny)
        device = None
        for name, dtype in self.ATTRIBUTES + self.PREDICATE:
            t = parts[name]
            if t is None:
                continue
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"RowWhere: {name} must be None or a 1-D {dtype} device tensor, got {type(t).__name__}")
            if t.dtype != dtype:
                raise ValueError(f"RowWhere: {name} of dtype {t.dtype} is not supported: it must be {dtype}")
            if t.dim() != 1:
                raise ValueError(f"RowWhere: {name} must be 1-D, got shape {tuple(t.shape)}")
            if device is not None and t.device != device:
                raise ValueError(f"RowWhere: {name} is on {t.device}, the parts before it on {device}: one device for all")
            device = t.device
        if value is None and (lo is not None or hi is not None):
            raise ValueError("RowWhere: lo / hi bound `value`, which is absent")
        if value is not None and (lo is None or hi is None):
            raise ValueError("RowWhere: value needs both lo and hi (a one-sided band passes an infinite bound)")
        if flags is None and (need is not None or deny is not None):
            raise ValueError("RowWhere: need / deny test `flags`, which is absent")
        self.__dict__.update(parts)

    def _struct(self, what, p, r):
        """The _lib.RowWhere of a call over p products and r rows: lengths (ValueError), device and layout (_req) checked."""
        st = _lib.RowWhere()
        for names, length, of in ((self.ATTRIBUTES, p, "product"), (self.PREDICATE, r, "row")):
            for name, dtype in names:
                t = getattr(self, name)
                if t is None:
                    continue
                if t.shape[0] != length:
                    raise ValueError(f"{what}: where.{name} must hold one entry per {of} ({length}), got {t.shape[0]}")
                setattr(st, name, _req(t, dtype, "where." + name).data_ptr())
        return st


def retrieve_list_grouped_where(proj, types, type_rowptr, type_col, table, n, where, slices=0, exclude=None, bad=None,
                                bias=None):
    """pc_retrieve_list_grouped_where and its three twins: retrieve_list_grouped's contract (idx [R,n] int32, -1 = none; scores
    [R,n] fp32, -inf = none; 1 <= n <= RETRIEVE_LIST_MAX_N; exclude and `bad` as there) over the products that pass the row's
    predicate `where` (a RowWhere: a band on a per-product value, masks on per-product flags).  A product that fails is treated
    exactly as an excluded one: the list is the unfiltered order (score descending, product index ascending) with the failing
    products taken out -- what retrieve_list_grouped serves over a CSR of the passing products, bit for bit, in ONE call for
    rows that each have their own predicate.  The score bits are the underlying entry's; a RowWhere() with every part absent
    gives that entry's output.  The entry goes by the table and the bias:
      table [P, D] fp32, bias None          pc_retrieve_list_grouped_where           (retrieve_list_grouped)
      table [P, D] bfloat16, bias None      pc_retrieve_list_grouped_bf16_where      (retrieve_list_grouped, bf16 copy)
      table fp32, bias [P] fp32             pc_retrieve_list_grouped_biased_where    (retrieve_list_grouped_biased's checks)
      table bfloat16, bias [P] fp32         pc_retrieve_list_grouped_bf16_biased_where (retrieve_list_grouped_bf16_biased's)
    The same kernel body, merge and determinism: the same bits for every `slices`.  Nothing is read back to the host."""
    what = "retrieve_list_grouped_where"
    n = int(n)
    if not 1 <= n <= RETRIEVE_LIST_MAX_N:
        raise ValueError(f"{what}: n must be in [1, {RETRIEVE_LIST_MAX_N}], got {n}")
    if not isinstance(where, RowWhere):
        raise ValueError(f"{what}: where must be an ops.RowWhere, got {type(where).__name__}")
    bf16 = isinstance(table, torch.Tensor) and table.dtype == torch.bfloat16
    if bias is not None:
        if bf16:
            _check_bf16_table(what, table, "retrieve_list_grouped_biased")
            _check_bias_bf16(what, bias, table)
        else:
            _check_bias(what, bias, table)
    name = "pc_retrieve_list_grouped" + ("_bf16" if bf16 else "") + ("_biased" if bias is not None else "") + "_where"
    return _retrieve_grouped(name, proj, types, type_rowptr, type_col, table, n, slices, exclude, bad, bias=bias, what=what,
                             tag="retrieve_list", table_dtype=torch.bfloat16 if bf16 else torch.float32, where=where)


def rank_grouped_bf16(proj, types, targets, type_rowptr, type_col, table, slices=0, bad=None, exclude=None, cand_type=None,
                      bias=None):
    """pc_rank_grouped_bf16: rank_grouped's contract over the [P, D] torch.bfloat16 copy of a catalogue -- for row r the number
    of products of type types[r] that retrieve_list_grouped(table) (bias: retrieve_list_grouped_bf16_biased) orders in front
    of targets[r], from that call's own score bits: rank < n exactly when the list holds the target at position rank.  Returns
    (rank [R] int32, bad [1] int32) with rank_grouped's -1 rows and `bad` count; exclude = (row_key, ex_rowptr, ex_col) with
    cand_type [P] int32, and bias [P] fp32, as there.  Bitwise deterministic, the same for every `slices`; it reads half the
    candidate bytes of rank_grouped and no fp32 table.  A function of its own: rank_grouped refuses a bf16 table.  Nothing is
    read back to the host."""
    what = "rank_grouped_bf16"
    _check_bf16_table(what, table, "rank_grouped")
    if bias is not None:
        _check_bias_bf16(what, bias, table)
    exclude = _check_rank_lists(what, exclude, cand_type, types, table)
    return _rank_call("pc_rank_grouped_bf16", what, proj, types, targets, type_rowptr, type_col, table, torch.bfloat16, slices, bad,
                      exclude, cand_type, bias)


def rank_grouped_where(proj, types, targets, type_rowptr, type_col, table, where, slices=0, bad=None, exclude=None,
                       cand_type=None, bias=None):
    """pc_rank_grouped_where / pc_rank_grouped_bf16_where: the rank twin of retrieve_list_grouped_where -- for row r the number
    of products of type types[r] that PASS the row's predicate `where` (a RowWhere: a band on a per-product value, masks on
    per-product flags) and that retrieve_list_grouped_where orders in front of targets[r], from that call's own score bits:
    rank < n exactly when retrieve_list_grouped_where(..., n, where, ...) with the same exclude / bias / table holds the target
    at position rank.  Returns (rank [R] int32, bad [1] int32): rank -1 wherever rank_grouped / rank_grouped_bf16 give -1
    (types[r] < 0; a type or target out of range, which `bad` counts; with exclude, a target in the row's list or no candidate
    of the row's type) and where the target itself fails its row's predicate.  The entry goes by the table's dtype:
      table [P, D] fp32      pc_rank_grouped_where       (rank_grouped's checks; bias None or [P] fp32)
      table [P, D] bfloat16  pc_rank_grouped_bf16_where  (rank_grouped_bf16's checks; bias None or [P] fp32)
    exclude = (row_key, ex_rowptr, ex_col) with cand_type [P] int32, `bad` and `slices` as in rank_grouped.  Over rows that
    share one predicate it is rank_grouped / rank_grouped_bf16 over a type CSR (and cand_type) rebuilt from the passing
    products; a RowWhere() with every part absent gives those functions' output bit for bit.  Bitwise deterministic, the same
    for every `slices`.  Every host-side check (ValueError) happens before any launch; nothing is read back to the host."""
    what = "rank_grouped_where"
    if not isinstance(where, RowWhere):
        raise ValueError(f"{what}: where must be an ops.RowWhere, got {type(where).__name__}")
    bf16 = isinstance(table, torch.Tensor) and table.dtype == torch.bfloat16
    if bf16:
        _check_bf16_table(what, table, "rank_grouped")
        if bias is not None:
            _check_bias_bf16(what, bias, table)
    else:
        if not isinstance(table, torch.Tensor) or table.dtype != torch.float32 or table.dim() != 2:
            raise ValueError(f"{what}: table must be a [P, D] float32 or bfloat16 device tensor, got "
                             f"{(table.dtype, tuple(table.shape)) if isinstance(table, torch.Tensor) else type(table).__name__}")
        if bias is not None:
            _check_bias(what, bias, table)
    exclude = _check_rank_lists(what, exclude, cand_type, types, table)
    return _rank_call("pc_rank_grouped_bf16_where" if bf16 else "pc_rank_grouped_where", what, proj, types, targets, type_rowptr,
                      type_col, table, torch.bfloat16 if bf16 else torch.float32, slices, bad, exclude, cand_type, bias, where=where)


class ScoreMoments:
    """What score_moments_grouped returns, one entry per row, on the device: count [R] int32 (the candidates of the row's type),
    mean / std [R] fp32 of the row's scores over them (the population form), and the sums behind them -- pivot (the score of the
    type's first candidate), s1 = sum(s - pivot), s2 = sum((s - pivot)^2) -- with `bad` [1] int32."""
    __slots__ = ("count", "mean", "std", "pivot", "s1", "s2", "bad")

    def __init__(self, count, mean, std, pivot, s1, s2, bad):
        self.count, self.mean, self.std, self.pivot, self.s1, self.s2, self.bad = count, mean, std, pivot, s1, s2, bad


def score_moments_grouped(proj, types, type_rowptr, type_col, table, slices=0, bad=None):
    """pc_score_moments_grouped / pc_score_moments_grouped_bf16: for row r the mean and the standard deviation of the scores of
    ALL products of type types[r] under proj[r] -- the distribution retrieve_list_grouped's list is the head of, from that call's
    own score bits -- as a ScoreMoments: count = the type's size n, pivot g = the score of the type's first candidate
    type_col[type_rowptr[t]], s1 = sum fl(s - g), s2 = sum fl(s - g)^2, mean = g + s1 / n, std = sqrt(max(s2 / n - (s1 / n)^2, 0)).
    A row with types[r] < 0, with a type >= the CSR's (which `bad` counts: a device counter to add to, a fresh zero otherwise) or
    of an empty type: count 0 and zeros.  The entry goes by the table's dtype:
      table [P, D] fp32      pc_score_moments_grouped
      table [P, D] bfloat16  pc_score_moments_grouped_bf16  (the unrounded proj against the ROUNDED rows)
    The rank entries' plan, query tile, score chain and candidate stream, and `slices` as there.  Bitwise reproducible for a given
    `slices`; across `slices` the fp32 sums may differ in their last bits (where they are exact they do not).  Every host-side
    check (ValueError) happens before any launch; nothing is read back to the host."""
    what = "score_moments_grouped"
    if not isinstance(table, torch.Tensor) or table.dtype not in (torch.float32, torch.bfloat16) or table.dim() != 2:
        raise ValueError(f"{what}: table must be a [P, D] float32 or bfloat16 device tensor, got "
                         f"{(table.dtype, tuple(table.shape)) if isinstance(table, torch.Tensor) else type(table).__name__}")
    bf16 = table.dtype == torch.bfloat16
    if table.shape[0] < 1 or table.shape[1] not in (128, 256):
        raise ValueError(f"{what}: table must hold at least one row of 128 or 256 columns, got shape {tuple(table.shape)}")
    if not isinstance(proj, torch.Tensor) or proj.numel() == 0 or proj.numel() % table.shape[1]:
        raise ValueError(f"{what}: proj must be a non-empty tensor of rows of {table.shape[1]} columns")
    rows = proj.numel() // table.shape[1]
    if not isinstance(types, torch.Tensor) or types.dtype != torch.int32 or tuple(types.shape) != (rows,):
        raise ValueError(f"{what}: types must be an int32 tensor of one entry per row ({rows},), got "
                         f"{(types.dtype, tuple(types.shape)) if isinstance(types, torch.Tensor) else type(types).__name__}")
    if not isinstance(type_rowptr, torch.Tensor) or type_rowptr.dim() != 1 or type_rowptr.numel() < 2:
        raise ValueError(f"{what}: type_rowptr must be a [T + 1] int32 tensor with T >= 1")
    proj, r, t, d, slices = _grouped_rows(proj, types, type_rowptr, type_col, table, torch.bfloat16 if bf16 else torch.float32,
                                          slices)
    _counters(bad=bad)
    device = proj.device
    count = torch.empty(r, dtype=torch.int32, device=device)
    pivot, s1, s2, mean, std = torch.empty(5, r, dtype=torch.float32, device=device).unbind(0)
    bad = _bad_counter(bad, device)
    args = (proj.data_ptr(), types.data_ptr(), r, type_rowptr.data_ptr(), type_col.data_ptr(), table.data_ptr(), t, d, slices,
            count.data_ptr(), pivot.data_ptr(), s1.data_ptr(), s2.data_ptr(), mean.data_ptr(), std.data_ptr(), bad.data_ptr())
    _grouped_call("pc_score_moments_grouped_bf16" if bf16 else "pc_score_moments_grouped", "score_moments", device,
                  (r, t, slices), args, "pc_score_moments_grouped")
    return ScoreMoments(count, mean, std, pivot, s1, s2, bad)


def standardise_scores(score, mean, std, count):
    """z = (score - mean) / std in fp32, as torch operations on the tensors' device: how exceptional a served product is among
    ALL candidates of its slot (mean / std / count: score_moments_grouped's, broadcast against score -- [R, 1] beside [R, n]).
    z = 0 where count < 2 or std == 0 (one candidate, or all alike: nothing stands out); -inf (the padding of a short list)
    stays -inf.  Inside one row the map is monotone: a list keeps its order."""
    if not all(isinstance(t, torch.Tensor) for t in (score, mean, std, count)):
        raise ValueError("standardise_scores: score, mean, std and count must be tensors")
    if score.dtype != torch.float32 or mean.dtype != torch.float32 or std.dtype != torch.float32:
        raise ValueError(f"standardise_scores: score, mean and std must be float32, got {score.dtype}, {mean.dtype}, {std.dtype}")
    flat = (count < 2) | (std == 0)
    z = (score - mean) / torch.where(flat, torch.ones_like(std), std)
    z = torch.where(flat, torch.zeros_like(z), z)
    return torch.where(score == float("-inf"), score, z)


def type_csr(type_idx, n_types):
    """The type-grouped product CSR of PCompanionInference (bpg.get_products_by_type, bpg.py:40-43), built on the device from
    an int32 CUDA type_idx [P]: rowptr [T+1] int32, col [P] int32 = the products of each type in ascending node order (the
    stable sort; equal to np.argsort(type_idx, kind='stable') / np.bincount / np.cumsum).  Torch's device stable sort and
    bincount: this runs once per catalogue, not on the serving path.  Type ids outside [0, n_types) are refused."""
    _req(type_idx, torch.int32, "type_idx")
    n_types = int(n_types)
    if type_idx.dim() != 1 or n_types <= 0:
        raise ValueError("type_csr: expected a 1-D type_idx and n_types > 0")
    if type_idx.numel():
        lo, hi = (int(x) for x in torch.aminmax(type_idx))
        if lo < 0 or hi >= n_types:
            raise ValueError(f"type_csr: type ids must lie in [0, {n_types}), got {lo} .. {hi}")
    counts = torch.bincount(type_idx, minlength=n_types)
    rowptr = torch.zeros(n_types + 1, dtype=torch.int32, device=type_idx.device)
    rowptr[1:] = torch.cumsum(counts, 0).to(torch.int32)
    col = torch.argsort(type_idx, stable=True).to(torch.int32)
    return rowptr, col


def exclusion_csr(rowptr, col, include_self=True, num_products=None):
    """An exclusion set as pc_retrieve_topk_grouped_excluding / pc_rank_grouped_excluding read it, from any device CSR over keys
    (normally the co-view graph: cv_rowptr / cv_col, key = the query product): inside every row the ids are sorted, duplicates
    and ids outside [0, num_products) are dropped and, with include_self, the key itself is inserted (keys below num_products).
    num_products defaults to the number of keys.  Returns (ex_rowptr [n_keys + 1] int32, ex_col [E'] int32), the ids of a key
    strictly ascending.  Torch's device sort and scan over (key, id) pairs as one int64 each; nothing is read back per row.
    Runs once per catalogue, off the serving path, as type_csr does.  E + num_products >= 2^31 is refused."""
    for name, t in (("rowptr", rowptr), ("col", col)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or t.dim() != 1:
            raise ValueError(f"exclusion_csr: {name} must be a 1-D int32 tensor")
    n_keys = rowptr.numel() - 1
    if n_keys < 0:
        raise ValueError("exclusion_csr: rowptr must hold n_keys + 1 >= 1 entries")
    p = n_keys if num_products is None else int(num_products)
    if p < 0:
        raise ValueError("exclusion_csr: num_products must not be negative")
    if col.numel() + p >= 2 ** 31:
        raise ValueError(f"exclusion_csr: {col.numel()} entries + {p} products do not fit 31 bits")
    _req(rowptr, torch.int32, "rowptr")
    _req(col, torch.int32, "col")
    dev = rowptr.device
    keys = torch.arange(n_keys, dtype=torch.int64, device=dev)
    row = torch.repeat_interleave(keys, (rowptr[1:] - rowptr[:-1]).long(), output_size=col.numel())
    ids = col.long()
    if include_self:
        own = keys[:min(n_keys, p)]
        row, ids = torch.cat([row, own]), torch.cat([ids, own])
    inside = (ids >= 0) & (ids < p)
    pairs = torch.unique(row[inside] * max(p, 1) + ids[inside])              # sorted: by key, then by id; no duplicates
    row, ids = pairs // max(p, 1), pairs % max(p, 1)
    ex_rowptr = torch.zeros(n_keys + 1, dtype=torch.int32, device=dev)
    if n_keys:
        ex_rowptr[1:] = torch.cumsum(torch.bincount(row, minlength=n_keys), 0).to(torch.int32)
    return ex_rowptr, ids.to(torch.int32).contiguous()


MERGE_MAX_LISTS, MERGE_MAX_N = 64, 256


def cell_means(table, cell_rowptr, cell_col, centroids):
    """pc_cell_means: the centroid update of a Lloyd iteration, in place: centroids[c] = the fp32 mean of the rows
    table[cell_col[i]], i in [cell_rowptr[c], cell_rowptr[c + 1]); a cell without members keeps the centroid it had.  table
    [P, D] fp32, D 128 or 256; cell_rowptr [C + 1] / cell_col int32 as type_csr makes them of an assignment; centroids [C, D]
    fp32.  One fixed summation order per cell, no atomics: the same bits on every run.  An id outside [0, P) is passed over
    (not summed, not counted in the divisor, not reported).  Returns centroids."""
    d = _table_width(table, rows=True)
    _req(centroids, torch.float32, "centroids")
    if centroids.dim() != 2 or centroids.shape[1] != d or centroids.shape[0] < 1:
        raise ValueError(f"centroids: expected [C, {d}] with C >= 1, got shape {tuple(centroids.shape)}")
    c = centroids.shape[0]
    _req(cell_rowptr, torch.int32, "cell_rowptr", (c + 1,))
    _req(cell_col, torch.int32, "cell_col")
    if cell_col.dim() != 1:
        raise ValueError(f"cell_col: expected a 1-D tensor, got shape {tuple(cell_col.shape)}")
    if cell_col.numel() == 0:                             # (every cell empty: one unread entry)
        cell_col = torch.zeros(1, dtype=torch.int32, device=table.device)
    check(_lib.lib().pc_cell_means(_p(table), _p(cell_rowptr), _p(cell_col), c, table.shape[0], d, _p(centroids), _stream()),
          "pc_cell_means")
    return centroids


def cell_means_bf16(table, cell_rowptr, cell_col, centroids):
    """pc_cell_means_bf16: cell_means for the [P, D] torch.bfloat16 copy of a catalogue (catalogue_bf16; a CompactCatalogue's
    .table), in place: centroids[c] = the fp32 mean of the stored rows table[cell_col[i]] widened (exactly) to fp32 -- the
    same lanes, order, tree and division, so the bits of cell_means(table.float(), ...) without the fp32 table ever being
    formed.  cell_rowptr / cell_col / centroids [C, D] fp32, the empty cell and ids outside [0, P) as there.  Returns
    centroids."""
    if isinstance(table, torch.Tensor) and table.dtype == torch.float32:
        raise ValueError("cell_means_bf16: an fp32 table is cell_means's; this function reads the bf16 copy (catalogue_bf16)")
    d = _table_width(table, rows=True, dtype=torch.bfloat16)
    _req(centroids, torch.float32, "centroids")
    if centroids.dim() != 2 or centroids.shape[1] != d or centroids.shape[0] < 1:
        raise ValueError(f"centroids: expected [C, {d}] with C >= 1, got shape {tuple(centroids.shape)}")
    c = centroids.shape[0]
    _req(cell_rowptr, torch.int32, "cell_rowptr", (c + 1,))
    _req(cell_col, torch.int32, "cell_col")
    if cell_col.dim() != 1:
        raise ValueError(f"cell_col: expected a 1-D tensor, got shape {tuple(cell_col.shape)}")
    if cell_col.numel() == 0:                             # (every cell empty: one unread entry)
        cell_col = torch.zeros(1, dtype=torch.int32, device=table.device)
    check(_lib.lib().pc_cell_means_bf16(_p(table), _p(cell_rowptr), _p(cell_col), c, table.shape[0], d, _p(centroids),
                                        _stream()), "pc_cell_means_bf16")
    return centroids


def merge_lists(idx, score):
    """pc_merge_lists: idx [R, L, n] int32 / score [R, L, n] fp32, L lists per row as the grouped retrievals return them (sorted
    under (score descending, product index ascending), -1 / -inf behind the last entry), the lists of a row over disjoint
    products -> (idx [R, n] int32, score [R, n] fp32): the first n of the row's union under the same total order, the scores'
    bits unchanged, -1 / -inf past the end.  1 <= L <= 64, 1 <= n <= 256."""
    r, l, n = _list_pair("merge_lists", idx, score, "[R, L, n]")
    if not 1 <= l <= MERGE_MAX_LISTS:
        raise ValueError(f"merge_lists: L must be in [1, {MERGE_MAX_LISTS}], got {l}")
    if not 1 <= n <= MERGE_MAX_N:
        raise ValueError(f"merge_lists: n must be in [1, {MERGE_MAX_N}], got {n}")
    out_idx, out_sc = _list_out(r, n, idx.device)
    if r == 0:
        return out_idx, out_sc
    check(_lib.lib().pc_merge_lists(_p(idx), _p(score), r, l, n, _p(out_idx), _p(out_sc), _stream()), "pc_merge_lists")
    return out_idx, out_sc


DIVERSIFY_MAX_POOL = 256


def inv_norm(table):
    """pc_inv_norm: scale[p] = 1 / |table[p]|_2 for a [P, D] fp32 device table -> [P] fp32, the per-product factor under which
    diversify_lists' similarity is the cosine; 0 for an all-zero row.  half_sq_norm_bias's fixed summation order, one correctly
    rounded square root and one correctly rounded division: the same bits on every run.  Once per catalogue."""
    return _inv_norm("pc_inv_norm", table, torch.float32)


def inv_norm_bf16(table):
    """pc_inv_norm_bf16: inv_norm for the [P, D] torch.bfloat16 copy of a catalogue (catalogue_bf16) -> [P] fp32: the factors
    of the ROUNDED rows, bit for bit inv_norm(table.float()), without the fp32 table ever being formed."""
    return _inv_norm("pc_inv_norm_bf16", table, torch.bfloat16)


def _inv_norm(name, table, dtype):
    d = _table_width(table, rows=True, dtype=dtype)
    out = torch.empty(table.shape[0], dtype=torch.float32, device=table.device)
    check(getattr(_lib.lib(), name)(_p(table), table.shape[0], d, _p(out), _stream()), name)
    return out


def diversify_lists(idx, score, table, n, lam, scale=None, bad=None):
    """pc_diversify_lists: a greedy maximal-marginal-relevance re-rank of a served pool.  idx [R, m] int32 / score [R, m] fp32,
    1 <= m <= DIVERSIFY_MAX_POOL, as retrieve_list_grouped / retrieve_topk_grouped return them (any order; a slot with id -1 or a
    score that is not finite is no candidate) -> (idx [R, n] int32, score [R, n] fp32): the n products to show in pick order,
    each with its INPUT score, -1 / -inf past the end of a pool with fewer than n candidates.  Round 0 picks the best
    fl(lam * score); every later round the best fl(fl(lam * score_j) - fl((1 - lam) * pen_j)), pen_j the largest similarity of j
    to a product picked so far, under (value descending, product index ascending).  The similarity is the fp32 dot product of
    the two rows of table [P, D] (D 128 or 256) in one fixed order, times fl(scale[a] * scale[b]) with scale [P] fp32
    (inv_norm(table): the cosine); scale=None: the dot product.  lam in [0, 1]: 1 is the pool's own first n, bit for bit.
    An id outside [-1, P) is no candidate, is never read and is counted in `bad` (a [1] int32 device counter the caller passes to
    see the count; added to).  Bitwise deterministic; a permutation of a row's slots changes nothing.  Nothing is read back."""
    return _diversify("diversify_lists", "pc_diversify_lists", torch.float32, idx, score, table, n, lam, scale, bad)


def diversify_lists_bf16(idx, score, table, n, lam, scale=None, bad=None):
    """pc_diversify_lists_bf16: diversify_lists over the [P, D] torch.bfloat16 copy of a catalogue (catalogue_bf16; a
    CompactCatalogue's .table).  The similarity is taken between the ROUNDED rows, and the result is bit for bit
    diversify_lists(idx, score, table.float(), ...): the rows are widened (exactly) as they are gathered and everything behind
    the gather is the same code.  scale [P] fp32 as there (inv_norm_bf16(table): the cosine) or None.  A function of its own:
    diversify_lists refuses a bf16 table."""
    return _diversify("diversify_lists_bf16", "pc_diversify_lists_bf16", torch.bfloat16, idx, score, table, n, lam, scale, bad)


def _diversify(what, name, dtype, idx, score, table, n, lam, scale, bad):
    """diversify_lists / diversify_lists_bf16 behind the choice of the entry: the checks (host side alone), then the call."""
    r, m = _list_pair(what, idx, score, "[R, m]")
    if not 1 <= m <= DIVERSIFY_MAX_POOL:
        raise ValueError(f"{what}: the pool m must be in [1, {DIVERSIFY_MAX_POOL}], got {m}")
    n = int(n)
    if not 1 <= n <= m:
        raise ValueError(f"{what}: n must be in [1, m = {m}], got {n}")
    lam = float(lam)
    if not 0.0 <= lam <= 1.0:                             # (a NaN fails the comparison)
        raise ValueError(f"{what}: lam must be in [0, 1], got {lam}")
    d = _table_width(table, rows=True, dtype=dtype)
    _optional(what, scale, torch.float32, "scale", "[P]", (table.shape[0],))
    _counters(bad=bad)
    out_idx, out_sc = _list_out(r, n, idx.device)
    if r == 0:
        return out_idx, out_sc
    check(getattr(_lib.lib(), name)(_p(idx), _p(score), r, m, _p(table), _p(scale), table.shape[0], d, n, lam, _p(out_idx),
                                    _p(out_sc), _p(bad), _stream()), name)
    return out_idx, out_sc


CAP_LISTS_MAX_POOL = 256


def cap_lists(idx, score, n, group=None, cap=1, row_ban=None, bad=None):
    """pc_cap_lists: at most `cap` products of one product group in a served row, as a post-pass over a pool.  idx [R, m] int32
    / score [R, m] fp32, 1 <= m <= CAP_LISTS_MAX_POOL, as the grouped retrievals return them -- or several of their lists side
    by side -- in any order (a slot with id -1 or a score that is not finite is no candidate) -> (idx [R, n] int32, score [R, n]
    fp32): the first n candidates under (score descending, product index ascending) that the rule keeps, each with its INPUT
    score bits, -1 / -inf past the end.  group [P] int32: the product's group, negative = ungrouped and never capped (ids are
    only compared: any non-negative int32); None: nothing is grouped, and the call is the sort / merge alone.  A grouped
    candidate is kept iff fewer than cap candidates of its group stand in front of it.  row_ban [R] int32 (needs group): a
    non-negative entry names a group none of whose products is a candidate of that row.  An id outside [-1, P) -- without a
    group: a negative id below -1 -- is no candidate, is never used as an index and is counted in `bad` (a [1] int32 device
    counter the caller passes to see the count; added to).  cap >= m or group=None returns the pool's first n: of a grouped
    entry's list its own first n, bit for bit.  Bitwise deterministic; a permutation of a row's slots changes nothing.  Nothing
    is read back."""
    r, m = _list_pair("cap_lists", idx, score, "[R, m]")
    if not 1 <= m <= CAP_LISTS_MAX_POOL:
        raise ValueError(f"cap_lists: the pool m must be in [1, {CAP_LISTS_MAX_POOL}], got {m}")
    n, cap = int(n), int(cap)
    if not 1 <= n <= m:
        raise ValueError(f"cap_lists: n must be in [1, m = {m}], got {n}")
    if cap < 1:
        raise ValueError(f"cap_lists: cap must be at least 1, got {cap}")
    num_products = 2 ** 31 - 1                            # without groups every non-negative id is a candidate
    if group is not None:
        _optional("cap_lists", group, torch.int32, "group", "[P]")
        if group.dim() != 1 or group.shape[0] < 1:
            raise ValueError(f"cap_lists: group must be [P] with at least one product, got {tuple(group.shape)}")
        num_products = group.shape[0]
    if row_ban is not None and group is None:
        raise ValueError("cap_lists: row_ban names a group per row and needs group")
    _optional("cap_lists", row_ban, torch.int32, "row_ban", "[R]", (r,))
    _counters(bad=bad)
    out_idx, out_sc = _list_out(r, n, idx.device)
    if r == 0:
        return out_idx, out_sc
    # (a group holds at most m of a row's slots: every cap >= m is the cap m, whatever fits a C int)
    check(_lib.lib().pc_cap_lists(_p(idx), _p(score), r, m, _p(group), _p(row_ban), num_products, n, min(cap, m), _p(out_idx),
                                  _p(out_sc), _p(bad), _stream()), "pc_cap_lists")
    return out_idx, out_sc


FUSE_LISTS_MAX_POOL, FUSE_LISTS_MAX_N = 1024, 256


def fuse_lists(idx, score, n, combine="sum", source=None, exclude=None, num_products=None, bad=None):
    """pc_fuse_lists: the lists served for the items of a basket fused into one list.  idx [B, S, w] int32 / score [B, S, w]
    fp32, 1 <= S w <= FUSE_LISTS_MAX_POOL: S source rows of w slots per basket, each row what a grouped retrieval returned for
    one basket item (its K type lists side by side), in any order (a slot with id -1 or a score that is not finite is no
    candidate) -> (idx [B, n] int32, score [B, n] fp32, support [B, n] int32), 1 <= n <= min(S w, FUSE_LISTS_MAX_N): the first n
    products of the basket under (fused score descending, product index ascending), -1 / -inf / 0 past the end.  All candidate
    slots of a basket with one id are one product; with its slot scores in descending order s1 >= s2 >= ..., combine="sum":
    f = s1, f = fl(f + s2), ... (sequential fp32, the largest first: the pinned order makes the bits independent of the slot
    order); combine="max": f = s1, a dedupe.  support = the number of slots fused.  source [B, S] int32: the product id of the
    item behind each row, -1 = no item here (the row is dropped); the sources are banned from their basket's list.  exclude =
    (ex_rowptr [P + 1], ex_col) as exclusion_csr returns them (needs source): every id in the rows of a basket's sources is
    banned too, whichever row offered it.  num_products: ids at or above it are bad; taken from ex_rowptr where given, else the
    argument, else 2^31 - 1.  An id or a source outside [-1, num_products) is never used as an index and is counted in `bad`
    (a [1] int32 device counter the caller passes to see the count; added to).  Bitwise deterministic; a permutation of a
    basket's rows (with their sources) or of the slots inside rows changes nothing.  Nothing is read back."""
    b, s, w = _list_pair("fuse_lists", idx, score, "[B, S, w]")
    if not 1 <= s * w <= FUSE_LISTS_MAX_POOL:
        raise ValueError(f"fuse_lists: the pool S * w must be in [1, {FUSE_LISTS_MAX_POOL}], got {s} * {w}")
    n = int(n)
    if not 1 <= n <= min(s * w, FUSE_LISTS_MAX_N):
        raise ValueError(f"fuse_lists: n must be in [1, min(S * w, {FUSE_LISTS_MAX_N}) = {min(s * w, FUSE_LISTS_MAX_N)}], got {n}")
    if combine not in ("sum", "max"):
        raise ValueError(f"fuse_lists: combine must be 'sum' or 'max', got {combine!r}")
    _optional("fuse_lists", source, torch.int32, "source", "[B, S]", (b, s))
    ex_rowptr, ex_col, num_products = _exclusion_pair("fuse_lists", exclude, source, num_products, idx.device)
    _counters(bad=bad)
    out_idx, out_sc, out_sup = _list_out(b, n, idx.device, support=True)
    if b == 0:
        return out_idx, out_sc, out_sup
    check(_lib.lib().pc_fuse_lists(_p(idx), _p(score), _p(source), b, s, w, _p(ex_rowptr), _p(ex_col), num_products, n,
                                   0 if combine == "sum" else 1, _p(out_idx), _p(out_sc), _p(out_sup), _p(bad), _stream()),
          "pc_fuse_lists")
    return out_idx, out_sc, out_sup


FUSE_SESSIONS_MAX_POOL, FUSE_SESSIONS_MAX_N = 1024, 256


def fuse_sessions(idx, score, seg_rowptr, n, combine="sum", source=None, weight=None, exclude=None, num_products=None,
                  max_items=None, bad=None, truncated=None):
    """pc_fuse_sessions: fuse_lists for ragged sessions with a weight per item.  idx [R, w] int32 / score [R, w] fp32,
    1 <= w <= FUSE_SESSIONS_MAX_POOL: row r is what a grouped retrieval returned for item r (its K type lists side by side), in
    any order (a slot with id -1 or a score that is not finite is no candidate); seg_rowptr [B + 1] int32: session b owns the
    rows [seg_rowptr[b], seg_rowptr[b + 1]) -> (idx [B, n] int32, score [B, n] fp32, support [B, n] int32), 1 <= n <=
    FUSE_SESSIONS_MAX_N: the first n products of the session under (fused score descending, product index ascending), -1 /
    -inf / 0 past the end; an empty session is all padding.  Only the LAST L = min(FUSE_SESSIONS_MAX_POOL // w, max_items)
    rows of a session offer candidates (max_items None or 0: no cap); a longer session is counted in `truncated`; every row
    still bans.  weight [R] fp32 (None: every weight is 1): a slot's term is t = fl(weight[r] * score), one rounded fp32
    multiplication formed before anything is added; a row whose weight is not finite and > 0 offers nothing, but its source
    still bans ("already bought"); a term that is not finite is no candidate.  All candidate slots of a session with one id are
    one product; with its terms in descending order t1 >= t2 >= ..., combine="sum": f = t1, f = fl(f + t2), ... (sequential
    fp32, the largest first); combine="max": f = t1.  support = the number of slots fused.  source [R] int32: the product id
    of the item behind each row, -1 = no item (the row offers nothing); the sources of ALL rows are banned from their session's
    list.  exclude = (ex_rowptr [P + 1], ex_col) as exclusion_csr returns them (needs source): every id in the rows of a
    session's sources is banned too, whichever row offered it.  num_products: ids at or above it are bad; taken from ex_rowptr
    where given, else the argument, else 2^31 - 1.  An id of a live row or a source outside [-1, num_products) is never used
    as an index and is counted in `bad` (a [1] int32 device counter the caller passes to see the count; added to), and so is a
    seg_rowptr entry outside [0, R] or below its predecessor, which is clamped.  `truncated`: a [1] int32 device counter,
    added to.  Bitwise deterministic; a permutation of a session's rows (with their sources and weights, among the rows of one
    truncation status) or of the slots inside rows changes nothing.  Nothing is read back."""
    r, w = _list_pair("fuse_sessions", idx, score, "[R, w]")
    if not 1 <= w <= FUSE_SESSIONS_MAX_POOL:
        raise ValueError(f"fuse_sessions: the row width w must be in [1, {FUSE_SESSIONS_MAX_POOL}], got {w}")
    _req(seg_rowptr, torch.int32, "seg_rowptr")
    if seg_rowptr.dim() != 1 or seg_rowptr.numel() < 1:
        raise ValueError(f"fuse_sessions: expected seg_rowptr [B + 1] with B >= 0, got {tuple(seg_rowptr.shape)}")
    b = seg_rowptr.numel() - 1
    n = int(n)
    if not 1 <= n <= FUSE_SESSIONS_MAX_N:
        raise ValueError(f"fuse_sessions: n must be in [1, {FUSE_SESSIONS_MAX_N}], got {n}")
    if combine not in ("sum", "max"):
        raise ValueError(f"fuse_sessions: combine must be 'sum' or 'max', got {combine!r}")
    _optional("fuse_sessions", source, torch.int32, "source", "[R]", (r,))
    _optional("fuse_sessions", weight, torch.float32, "weight", "[R]", (r,))
    ex_rowptr, ex_col, num_products = _exclusion_pair("fuse_sessions", exclude, source, num_products, idx.device)
    max_items = 0 if max_items is None else int(max_items)
    if not 0 <= max_items <= 2 ** 31 - 1:
        raise ValueError(f"fuse_sessions: max_items must be None or in [0, 2^31 - 1] (0: no cap), got {max_items}")
    _counters(bad=bad, truncated=truncated)
    out_idx, out_sc, out_sup = _list_out(b, n, idx.device, support=True)
    if b == 0:
        return out_idx, out_sc, out_sup
    if r == 0:                                            # (no rows: nothing offers and nothing bans; every pointer is null)
        source = weight = ex_rowptr = ex_col = None
    check(_lib.lib().pc_fuse_sessions(_p(idx), _p(score), _p(source), _p(weight), _p(seg_rowptr), r, b, w, max_items,
                                      _p(ex_rowptr), _p(ex_col), num_products, n, 0 if combine == "sum" else 1, _p(out_idx),
                                      _p(out_sc), _p(out_sup), _p(bad), _p(truncated), _stream()), "pc_fuse_sessions")
    return out_idx, out_sc, out_sup


class CompactCatalogue:
    """The bf16 copy of a catalogue as a serving table of its own: everything PCompanionInference needs to serve lists of up
    to RETRIEVE_LIST_MAX_N products per type and diversified lists without the fp32 features (catalogue=CompactCatalogue(...)).
    table: a [P, D] device tensor, D 128 or 256 -- fp32: rounded once here (catalogue_bf16); torch.bfloat16: taken as it is.
      .table     [P, D] torch.bfloat16, contiguous, on the device
      .inv_norm  [P] fp32 = inv_norm_bf16(.table), formed on first use: the cosine's factors
      .half_sq_norm  [P] fp32 = half_sq_norm_bias_bf16(.table), formed on first use: the Euclidean order's terms
    All describe the ROUNDED rows: the cosine and the distance are between the rows that are actually stored.  Ranks
    (rank_grouped_bf16), a bias (retrieve_list_grouped_bf16_biased) and substitutes (inference.CompactSimilarProducts) are
    served from it too, through functions and classes of their own: rank_grouped, the bias= arguments and SimilarProducts
    still take the fp32 table alone."""

    _inv_norm = None
    _half_sq_norm = None

    def __init__(self, table):
        if not isinstance(table, torch.Tensor) or table.dtype not in (torch.float32, torch.bfloat16):
            raise ValueError(f"CompactCatalogue: the table must be a [P, D] float32 or bfloat16 device tensor, got "
                             f"{table.dtype if isinstance(table, torch.Tensor) else type(table).__name__}")
        if table.dim() != 2 or table.shape[0] < 1 or table.shape[1] not in (128, 256):
            raise ValueError(f"CompactCatalogue: the table must be [P >= 1, 128 or 256], got {tuple(table.shape)}")
        if not table.is_cuda or not table.is_contiguous():
            raise ValueError("CompactCatalogue: the table must be a contiguous device tensor")
        self.table = table if table.dtype == torch.bfloat16 else catalogue_bf16(table)

    @property
    def inv_norm(self):
        if self._inv_norm is None:
            self._inv_norm = inv_norm_bf16(self.table)        # once per catalogue
        return self._inv_norm

    @property
    def half_sq_norm(self):
        if self._half_sq_norm is None:
            self._half_sq_norm = half_sq_norm_bias_bf16(self.table)   # once per catalogue
        return self._half_sq_norm


class CellIndex:
    """A k-means cell index over a [P, D] table (build_cell_index): centroids [C, D] fp32, centroid_bias [C] fp32 =
    half_sq_norm_bias(centroids), cell_of [P] int32 = the assignment under THESE centroids, cell_rowptr [C + 1] / cell_col [P]
    int32 = type_csr(cell_of, C), and the integers n_cells, dim, num_products."""

    def __init__(self, centroids, centroid_bias, cell_of, cell_rowptr, cell_col):
        self.centroids, self.centroid_bias, self.cell_of = centroids, centroid_bias, cell_of
        self.cell_rowptr, self.cell_col = cell_rowptr, cell_col
        self.n_cells, self.dim = int(centroids.shape[0]), int(centroids.shape[1])
        self.num_products = int(cell_of.shape[0])


def _assign_cells(table, centroids, centroid_bias=None, chunk_rows=1 << 20):
    """cell_of [P] int32: the nearest centroid of every row of table under Euclidean distance -- the biased grouped retrieval
    with the centroids as the candidates of one type and n = 1, in chunks of chunk_rows rows; the total order (score
    descending, index ascending) gives a tie to the lowest cell.  A bf16 table (build_cell_index_bf16) travels one chunk of
    rows widened (exactly) to fp32 at a time: a row's cell does not depend on its chunk."""
    p, c = table.shape[0], centroids.shape[0]
    dev = table.device
    if centroid_bias is None:
        centroid_bias = half_sq_norm_bias(centroids)
    chunk_rows = min(int(chunk_rows), p)
    zeros = torch.zeros(chunk_rows, dtype=torch.int32, device=dev)
    rowptr = torch.tensor([0, c], dtype=torch.int32, device=dev)
    col = torch.arange(c, dtype=torch.int32, device=dev)
    cell_of = torch.empty(p, dtype=torch.int32, device=dev)
    for lo in range(0, p, chunk_rows):
        hi = min(lo + chunk_rows, p)
        rows = table[lo:hi] if table.dtype == torch.float32 else table[lo:hi].float()
        idx, _ = retrieve_topk_grouped(rows, zeros[:hi - lo], rowptr, col, centroids, 1, bias=centroid_bias)
        cell_of[lo:hi] = idx[:, 0]
        del rows, idx                                     # (one widened chunk at a time)
    return cell_of


def _lloyd(what, table, d, means, n_cells, iters, seed, init, chunk_rows):
    """build_cell_index's argument checks and Lloyd loop over a checked [P, d] table; means: the centroid update of the
    table's element type (cell_means / cell_means_bf16)."""
    p = table.shape[0]
    n_cells, iters, chunk_rows = int(n_cells), int(iters), int(chunk_rows)
    if not 1 <= n_cells <= p:
        raise ValueError(f"{what}: n_cells must be in [1, P = {p}], got {n_cells}")
    if iters < 0:
        raise ValueError(f"{what}: iters must not be negative, got {iters}")
    if chunk_rows < 1:
        raise ValueError(f"{what}: chunk_rows must be positive, got {chunk_rows}")
    if init is not None:
        _req(init, torch.float32, "init")
        if tuple(init.shape) != (n_cells, d):
            raise ValueError(f"{what}: init must be [{n_cells}, {d}], got shape {tuple(init.shape)}")
        centroids = init.clone()
    else:
        gen = torch.Generator(device="cpu")
        gen.manual_seed(int(seed))
        first = torch.randperm(p, generator=gen)[:n_cells].to(table.device)
        centroids = table[first].float().contiguous()     # (fp32 rows as they are; bf16 rows widened)
    for _ in range(iters):
        cell_of = _assign_cells(table, centroids, None, chunk_rows)
        rowptr, col = type_csr(cell_of, n_cells)
        means(table, rowptr, col, centroids)
    bias = half_sq_norm_bias(centroids)
    cell_of = _assign_cells(table, centroids, bias, chunk_rows)
    rowptr, col = type_csr(cell_of, n_cells)
    return CellIndex(centroids, bias, cell_of, rowptr, col)


def build_cell_index(table, n_cells, iters=10, seed=0, init=None, chunk_rows=1 << 20):
    """Lloyd's k-means over table [P, D] fp32 (D 128 or 256) on the device -> CellIndex with 1 <= n_cells <= P cells.
    init: [n_cells, D] fp32 device tensor of starting centroids; None: the rows at the first n_cells entries of
    torch.randperm(P) drawn from a CPU torch.Generator seeded with `seed`.  An iteration is one assignment (_assign_cells: the
    biased grouped retrieval over the centroids, chunk_rows rows at a time) and one update (type_csr of the assignment, then
    cell_means; an empty cell keeps its centroid); the final centroids get one more assignment, so cell_of is always the
    assignment under the stored centroids.  Every step is bitwise deterministic, so equal arguments give equal bits in every
    field.  Nothing is read back to the host but type_csr's range check of the assignment."""
    d = _table_width(table)
    return _lloyd("build_cell_index", table, d, cell_means, n_cells, iters, seed, init, chunk_rows)


def build_cell_index_bf16(catalogue, n_cells, iters=10, seed=0, init=None, chunk_rows=1 << 18):
    """build_cell_index over the bf16 copy of a catalogue alone: catalogue an ops.CompactCatalogue or a contiguous
    [P, 128 | 256] torch.bfloat16 device tensor -> CellIndex (fp32 centroids and centroid_bias, as there: C x D floats).  The
    same Lloyd loop: the assignment is the biased 16-entry retrieval with n = 1 over the fp32 centroids, its query rows ONE
    chunk of at most chunk_rows stored rows widened (exactly) to fp32 at a time -- no fp32 tensor of more than chunk_rows rows
    is ever made (a catalogue of at most chunk_rows rows travels as its one chunk) --; the update is type_csr + cell_means_bf16; the final centroids get one more assignment.  init: [n_cells, D] fp32; None: the
    widened rows at the first n_cells entries of the same CPU torch.randperm(P) seeded with `seed`.  Every field has the bits
    of build_cell_index(catalogue.table.float(), same arguments), for any chunk_rows: a row's assignment does not depend on
    the chunk it travels in, and cell_means_bf16 is cell_means on the widened table bit for bit.  A function of its own:
    build_cell_index refuses a bf16 table."""
    table = catalogue.table if isinstance(catalogue, CompactCatalogue) else catalogue
    if isinstance(table, torch.Tensor) and table.dtype == torch.float32:
        raise ValueError("build_cell_index_bf16: an fp32 table is build_cell_index's; this function reads the bf16 copy "
                         "(catalogue_bf16, CompactCatalogue)")
    d = _table_width(table, dtype=torch.bfloat16)
    return _lloyd("build_cell_index_bf16", table, d, cell_means_bf16, n_cells, iters, seed, init, chunk_rows)
