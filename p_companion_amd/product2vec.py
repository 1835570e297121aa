"""Product2Vec on MI355X -- drop-in for the reference's src/models/product2vec.py.

Same constructor, method names/signatures, batch-dict keys and state_dict keys
(ffn.0.weight ... attention.out_proj.bias, incl. the BatchNorm buffers); every number is
produced by the HIP kernels of libpcompanion_hip.so through the C ABI.  torch.nn
submodules are kept ONLY as parameter containers (so checkpoints interchange and the
default initialisers / RNG consumption are the reference's); their forward() is never
called and there is no CPU fallback.

Two ways in:
  * dense tensors (reference loader compatible): forward(features[, neighbors]) builds
    the autograd graph from two custom Functions (FFN, attention) -> works with
    loss.backward() and any torch optimizer, exactly like the reference module;
  * index batches (anchor_idx / positive_idx / negative_idx / neighbor_idx over a device
    resident feature table): train_model runs the fused step pc_p2v_train_step -- gather,
    4 BatchNorm call groups, attention, loss, whole backward -- with gradients written
    straight into .grad (views of one flat buffer) and, with FusedAdam, one Adam launch.
"""
import logging
from typing import Dict, Optional

import numpy as np
import torch
import torch.nn as nn

from . import ops

import weakref

_STEP_CACHE = weakref.WeakKeyDictionary()        # Product2Vec -> (buffer addresses, tensor dicts, C structs) of train_step_indexed
_FFN_KEYS = ops.P2V_KEYS[:8]
_ATT_KEYS = ops.P2V_KEYS[8:]


class _FFNFunction(torch.autograd.Function):
    """get_initial_embedding on a [R,128] block, training mode (product2vec.py:31-46).
    row_weight / count (key-padding mask only, else None): fp32 [R] with 0 for a padding row and the number of real rows --
    BatchNorm's statistics, running-statistics update and backward sums then span the real rows."""

    @staticmethod
    def forward(ctx, module, x, row_weight, count, *weights):
        params = module._tensor_dict()
        y, sv = ops.ffn_forward_train(params, x, None, x.shape[0], [0], update_running=True, row_weight=row_weight,
                                      counts=None if count is None else [count])
        ctx.module, ctx.sv = module, sv
        ctx.save_for_backward(x)
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        params = ctx.module._tensor_dict()
        grads, dx = ops.ffn_backward(params, x, None, dy.contiguous(), ctx.sv, need_dx=ctx.needs_input_grad[1])
        return (None, dx, None, None) + tuple(grads[k] for k in _FFN_KEYS)


class _AttentionFunction(torch.autograd.Function):
    """apply_attention (product2vec.py:48-68): query [B,D], keys [B,N,D] -> [B,D].  key_pad: None, or the [B,N] key-padding
    mask (True = padding; the backward reads it from the saved state)."""

    @staticmethod
    def forward(ctx, module, query, keys, key_pad, *weights):
        ctx.dropout = module._next_dropout()                 # one fresh mask per forward; the backward regenerates it
        params = module._tensor_dict(ctx.dropout)
        out, sv = ops.attention_forward(params, query, keys, key_pad=key_pad)
        ctx.module, ctx.sv = module, sv
        ctx.save_for_backward(query, keys)
        return out

    @staticmethod
    def backward(ctx, dout):
        query, keys = ctx.saved_tensors
        params = ctx.module._tensor_dict(ctx.dropout)
        grads, dq, dk = ops.attention_backward(params, query, keys, dout.contiguous(), ctx.sv)
        return (None, dq, dk, None) + tuple(grads[k] for k in _ATT_KEYS)


class _NoEvalBackward(torch.autograd.Function):
    """Eval-mode forward (BatchNorm running statistics, no dropout) with gradients enabled.  The reference would
    differentiate through it (product2vec.py:31-46 has no mode switch in autograd); the HIP path implements the
    backward of the TRAINING graph only, so the output carries a node that raises when differentiated -- inference
    code that merely forgot torch.no_grad() keeps working, a fine-tuning / saliency pass fails loudly instead of
    silently receiving no gradient."""

    @staticmethod
    def forward(ctx, y, what, *deps):
        ctx.what = what
        return y.view_as(y)

    @staticmethod
    def backward(ctx, g):
        raise NotImplementedError(
            f"{ctx.what}: backward through the eval-mode forward is not implemented in the HIP path "
            "(call .train(), or wrap inference in torch.no_grad())")


def _guard_eval(y, what, deps):
    deps = [d for d in deps if isinstance(d, torch.Tensor) and d.requires_grad]
    if torch.is_grad_enabled() and deps:
        return _NoEvalBackward.apply(y, what, *deps)
    return y


class _TripletLossFunction(torch.autograd.Function):
    """The loss expression of train_model (product2vec.py:137-154) as one kernel."""

    @staticmethod
    def forward(ctx, a, p, n, margin):
        out = ops.triplet_loss(a, p, n, margin, need_grad=True)
        ctx.save_for_backward(out["da"], out["dp"], out["dn"])
        return out["loss"].reshape(())

    @staticmethod
    def backward(ctx, g):
        da, dp, dn = ctx.saved_tensors
        return da * g, dp * g, dn * g, None


class _FusedDenseLoss(torch.autograd.Function):
    """The whole loop body of train_model (product2vec.py:132-154: four FFN calls, attention, the hinge) on a DENSE
    reference batch as one fused HIP step: the batch's rows are laid end to end as a temporary table
    [anchor B | neighbours B*N | positive B | negatives B*K] addressed by identity indices, so the four calls run as
    the segments of one launch sequence and forward + backward are a single pc_p2v_train_step (every slot its own
    row, zero padding rows included, exactly as the reference computes them).  The parameter gradients are formed
    in forward and handed to autograd in backward (scaled by the incoming gradient)."""

    @staticmethod
    def forward(ctx, module, anchor, positive, negative, neighbors, key_pad, *weights):
        b, k, n = anchor.shape[0], negative.shape[1], neighbors.shape[1]
        dev = anchor.device
        d = anchor.shape[1]
        table = torch.cat([anchor, neighbors.reshape(-1, d), positive, negative.reshape(-1, d)])
        key = (b, n, k, dev)
        idx = module._dense_idx.get(key)
        if idx is None:
            ar = lambda lo, cnt: torch.arange(lo, lo + cnt, dtype=torch.int32, device=dev)
            idx = (ar(0, b), ar(b + b * n, b), ar(2 * b + b * n, b * k).reshape(b, k), ar(b, b * n).reshape(b, n))
            module._dense_idx.clear()
            module._dense_idx[key] = idx
        names = [nm for nm, _ in module.named_parameters()]
        grads = {nm: torch.empty_like(w) for nm, w in zip(names, weights)}
        nbr = idx[3]
        if key_pad is not None:
            # the key-padding mask (config.ATTENTION_KEY_MASK): a padding slot is index -1 of the masked step
            nbr = torch.where(key_pad, torch.full_like(nbr, -1), nbr)
        out = ops.p2v_train_step(module._tensor_dict(module._next_dropout()), grads, table, idx[0], idx[1], idx[2], nbr,
                                 float(module.config.MARGIN), masked=key_pad is not None)
        ctx.grads = [grads[nm] for nm in names]
        return out["loss"].reshape(())

    @staticmethod
    def backward(ctx, g):
        return (None, None, None, None, None, None) + tuple(torch._foreach_mul(ctx.grads, g))      # one multi-tensor launch


class FusedAdam(torch.optim.Optimizer):
    """torch.optim.Adam semantics (defaults of scripts/pretrain_product2vec.py:34) as ONE HIP
    launch over the module's flat parameter buffer.  Opt-in: any torch optimizer works too."""

    def __init__(self, module, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        self.module = module
        super().__init__(list(module.parameters()), dict(lr=lr, betas=betas, eps=eps))
        self._state_ready = False
        # the sharded optimizer (step(shard=True) / a sharded epoch call): (rank, world, floats per slice) as of the latest sharded
        # step, and whether the moments of the OTHER ranks' slices are behind (only this rank's slice is updated)
        self._shard = None
        self._shard_stale = False

    def _ensure(self):
        flat, gflat = self.module.flatten_parameters()
        if not self._state_ready or self.exp_avg.data_ptr() == 0:
            self.exp_avg = ops.alloc(flat.numel(), torch.float32, flat.device, zero=True)
            self.exp_avg_sq = ops.alloc(flat.numel(), torch.float32, flat.device, zero=True)
            self.step_count = torch.zeros(1, dtype=torch.int64, device=flat.device)
            self.scalars = torch.zeros(2, dtype=torch.float32, device=flat.device)
            self._state_ready = True
            # the step number as the HOST knows it: valid while every increment of the device counter went through step()
            # (then the update is ONE launch, pc_adam_step_at); None once a fused step advanced the counter itself
            # (fused_state()) -- the two-launch form then reads the device counter
            self._host_step = 0
            self._device_counter_only = False     # True once the device counter has been advanced behind the host's back
        elif self.exp_avg.numel() != flat.numel() or self.exp_avg.device != flat.device:
            self._follow(flat)
        return flat, gflat

    def _follow(self, flat):
        """The module's flat buffers are no longer the ones the moments were laid out for.  A change of the PADDING only
        (flatten_parameters(pad_multiple=...) behind a load_state_dict(): what GraphedJointStep(shard_optimizer=True) does on
        resume) carries moments, step counter and the host's step number over -- the real prefix is copied, the pad region stays
        zero.  Anything else is an error once the optimizer has stepped or loaded a state: a silent fresh start would run every
        later update with zero moments and the wrong bias corrections."""
        n_real = sum(p.numel() for _, p in self.module._named_flat())
        started = self._host_step != 0                 # (None: the device counter runs on its own -- steps have been taken)
        if self.exp_avg.device != flat.device:
            if started:
                raise RuntimeError(f"FusedAdam: the module moved from {self.exp_avg.device} to {flat.device} after the optimizer "
                                   "had stepped; its moments and step count would be lost (build a new optimizer and "
                                   "load_state_dict() what this one's state_dict() returns)")
            self._state_ready = False
            self._ensure()
            return
        if flat.numel() < n_real or self.exp_avg.numel() < n_real:
            raise RuntimeError(f"FusedAdam: flat buffers of {flat.numel()} floats (moments: {self.exp_avg.numel()}) cannot hold "
                               f"the module's {n_real} parameters")
        if started and self._shard is not None and self._shard_stale:
            raise RuntimeError("FusedAdam: the flat buffers' padding changed while this rank holds current moments for its own "
                               "slice only (sharded optimizer): call gather_state(exchange) on every rank first")
        m, v = self.exp_avg, self.exp_avg_sq
        self.exp_avg = ops.alloc(flat.numel(), torch.float32, flat.device, zero=True)
        self.exp_avg_sq = ops.alloc(flat.numel(), torch.float32, flat.device, zero=True)
        self.exp_avg[:n_real].copy_(m[:n_real])
        self.exp_avg_sq[:n_real].copy_(v[:n_real])
        self._shard, self._shard_stale = None, False              # (the slices are those of the new length from the next step on)

    @torch.no_grad()
    def step(self, closure=None, exchange=None, shard=False):
        """exchange (ops.Exchange, optional): a data-parallel replica's gradient exchange, issued from the same foreign call as
        the update (pc_exchange_adam) -- the flat gradient buffer holds the replicas' mean afterwards (shard=False).
        shard=True: the optimizer sharded over the replicas (pc_exchange_adam_plan: reduce-scatter, Adam on this rank's slice of
        the flat buffers, all-gather of the parameters).  The flat gradient buffer then holds the mean in THIS rank's slice only
        (the other slices are unspecified), and only this rank's slice of the moments is current: gather_state(exchange) before
        state_dict().  The Adam kernel moves 16-byte chunks, so every slice must be a multiple of 4 floats: pad the module's
        flat buffers to a multiple of 4 * world (module.flatten_parameters(pad_multiple=4 * exchange.world) before the first
        step); any other length is refused by every rank before a collective is issued."""
        flat, gflat = self._ensure()
        g = self.param_groups[0]
        if self._host_step is not None and flat.is_cuda and torch.cuda.is_current_stream_capturing():
            # a step that is being CAPTURED (GraphedJointStep mode 'graph' records optimizer.step() inside torch.cuda.graph)
            # must not bake the host's step number into the graph as a kernel argument: every replay would run Adam with
            # the capture-time bias corrections.  The device-counter form (pc_adam_step) is replay-safe; the host stops
            # counting for good (replays advance the device counter without passing through here).
            self._host_step = None
            self._device_counter_only = True
        if self._host_step is not None:
            # (counted once the call has been accepted: a refused update leaves the host where the device counter is)
            t = self._host_step + 1
            if exchange is not None:
                ops.exchange_adam(exchange, flat, gflat, self.exp_avg, self.exp_avg_sq, self.step_count, t,
                                  self.scalars, g["lr"], g["betas"], g["eps"], shard=shard)
                self._sharded_step(exchange, shard, flat.numel())
            else:
                ops.adam_step_at(flat, gflat, self.exp_avg, self.exp_avg_sq, self.step_count, t, g["lr"], g["betas"], g["eps"])
            self._host_step = t
            return
        if exchange is not None:
            ops.exchange_adam(exchange, flat, gflat, self.exp_avg, self.exp_avg_sq, self.step_count, 0, self.scalars, g["lr"],
                              g["betas"], g["eps"], shard=shard)
            self._sharded_step(exchange, shard, flat.numel())
            return
        ops.adam_step(flat, gflat, self.exp_avg, self.exp_avg_sq, self.step_count, self.scalars, g["lr"],
                      g["betas"], g["eps"])

    def _sharded_step(self, exchange, shard, n):
        """Behind a step over an exchange: a sharded one updated this rank's slice of the moments only."""
        if shard:
            world = int(exchange.world)
            self._shard = (int(exchange.rank), world, n // world)
            self._shard_stale = world > 1

    def riding_state(self):
        """For a step that applies this optimizer's update in its own last gradient launch (Product2Vec.train_step_indexed(
        optimizer=...): pc_p2v_train_step_unique_adam): the flat buffers, the hyper-parameters and the step number t of THIS
        update.  Does NOT count the step: the caller reports it with advance(1) once the launch that carries the update has been
        accepted (and must not call step() for it) -- a call refused in between leaves the step number where the device counter
        and the moments are.  None when the host does not know the step number (a captured graph / a fused joint step has
        advanced the device counter on its own): the caller then steps separately."""
        flat, gflat = self._ensure()
        if self._host_step is None or (flat.is_cuda and torch.cuda.is_current_stream_capturing()):
            return None
        g = self.param_groups[0]
        return {"param": flat, "grad": gflat, "exp_avg": self.exp_avg, "exp_avg_sq": self.exp_avg_sq, "step_count": self.step_count,
                "t": self._host_step + 1, "lr": g["lr"], "betas": g["betas"], "eps": g["eps"]}

    def epoch_state(self):
        """What an epoch-in-one-call of a replica (ops.PreparedJointStep.run_epoch_dp) needs: the flat moment buffers, the device
        step counter, the scratch scalars and t_first -- the Adam step number of the epoch's first step when the host knows it,
        else 0 (the device counter decides).  Report the steps the call ran with advance()."""
        self._ensure()
        t_first = self._host_step + 1 if self._host_step is not None else 0
        return self.exp_avg, self.exp_avg_sq, self.step_count, self.scalars, t_first

    def advance(self, steps, exchange=None, shard=False):
        """Report `steps` updates that another call applied over this optimizer's buffers (riding_state() / epoch_state());
        exchange / shard: as given to that call (a sharded epoch leaves only this rank's slice of the moments current)."""
        if self._host_step is not None:
            self._host_step += int(steps)
        if exchange is not None and int(steps) > 0:
            self._sharded_step(exchange, shard, self.exp_avg.numel())

    def zero_grad(self, set_to_none=False):
        _, gflat = self._ensure()
        gflat.zero_()

    def fused_state(self):
        """What a fused training step needs to apply this optimizer's update in its own last kernel
        (ops.joint_fused_step(adam=...)): per-parameter views of the flat moment buffers, the device step counter and
        the hyper-parameters.  The caller must NOT call step() for that iteration."""
        self._ensure()
        self._host_step = None                    # (the fused step advances the device counter: the host no longer knows it)
        self._device_counter_only = True
        m, v, off = {}, {}, 0
        for name, p in self.module._named_flat():
            n = p.numel()
            m[name] = self.exp_avg[off:off + n].view(p.shape)
            v[name] = self.exp_avg_sq[off:off + n].view(p.shape)
            off += n
        g = self.param_groups[0]
        return {"exp_avg": m, "exp_avg_sq": v, "step_count": self.step_count, "lr": g["lr"], "betas": g["betas"],
                "eps": g["eps"]}

    # ------------------------------------------------------------------ checkpoint layout of torch.optim.Adam
    def _slices(self):
        """[(index in param_groups[0]['params'], offset, numel, shape)] of the parameters that live in the flat buffer."""
        self._ensure()
        pos = {id(p): i for i, p in enumerate(self.param_groups[0]["params"])}
        out, off = [], 0
        for _, p in self.module._named_flat():
            out.append((pos[id(p)], off, p.numel(), tuple(p.shape)))
            off += p.numel()
        return out

    def state_dict(self):
        """The dict torch.optim.Adam.state_dict() would return for the same parameters after the same steps
        (train.py:66 saves it as 'optimizer_state_dict'): per-parameter 'step' / 'exp_avg' / 'exp_avg_sq' sliced out
        of the flat moment buffers, parameters without a gradient (the frozen product table, p_companion.py:26-29)
        hold no state, like in torch.  torch.optim.Adam(model.parameters()).load_state_dict() reads it.
        A sharded optimizer (step(shard=True)) holds current moments for this rank's slice only: RuntimeError until
        gather_state(exchange) has brought the other slices in -- zeros are never exported as moments."""
        if self._shard is not None and self._shard_stale:
            rank, world, _ = self._shard
            raise RuntimeError(f"FusedAdam.state_dict(): the optimizer is sharded over {world} replicas and rank {rank} holds "
                               "current moments for its own slice only; call gather_state(exchange) on EVERY rank first "
                               "(a collective: it is not run from here, where one rank may be alone)")
        n = len(self.param_groups[0]["params"])
        group = {"lr": self.param_groups[0]["lr"], "betas": tuple(self.param_groups[0]["betas"]),
                 "eps": self.param_groups[0]["eps"], "weight_decay": 0, "amsgrad": False, "maximize": False,
                 "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                 "decoupled_weight_decay": False, "params": list(range(n))}
        state = {}
        steps = int(self.step_count) if self._state_ready else 0
        if steps > 0:
            for idx, off, m, shape in self._slices():
                state[idx] = {"step": torch.tensor(float(steps)),
                              "exp_avg": self.exp_avg[off:off + m].view(shape).clone(),
                              "exp_avg_sq": self.exp_avg_sq[off:off + m].view(shape).clone()}
        return {"state": state, "param_groups": [group]}

    @torch.no_grad()
    def gather_state(self, exchange):
        """The sharded optimizer's checkpoint collective: all-gather of exp_avg and exp_avg_sq over `exchange` (the one the steps
        ran over), after which every rank holds the whole state and state_dict() works -- until the next sharded step.  EVERY
        rank must call it (at the same point of the program, like a step).  Deliberately not part of state_dict(): a checkpoint
        written by rank 0 alone must not turn into a collective the other ranks never enter.  Nothing to do (and no collective)
        for an optimizer that has not taken a sharded step -- the same on every rank."""
        self._ensure()
        if self._shard is None:
            return
        rank, world, length = self._shard
        if (int(exchange.rank), int(exchange.world)) != (rank, world) or length * world != self.exp_avg.numel():
            raise ValueError(f"FusedAdam.gather_state: the optimizer stepped as rank {rank} of {world} over slices of {length} "
                             f"floats; the exchange is rank {exchange.rank} of {exchange.world}")
        for buf in (self.exp_avg, self.exp_avg_sq):
            if hasattr(exchange, "register"):                      # (a host-driven exchange finds its buffers by address)
                exchange.register(buf)
            exchange.all_gather_(buf)
        self._shard_stale = False

    def load_state_dict(self, state_dict):
        """Accepts torch.optim.Adam's layout (also what state_dict() above emits): a resumed run continues with the
        saved moments and step count.  On a sharded optimizer too: every rank loads the whole state and steps on from its
        own slice."""
        groups = state_dict["param_groups"]
        if len(groups) != 1:
            raise ValueError("FusedAdam: one parameter group expected")
        n = len(self.param_groups[0]["params"])
        if len(groups[0]["params"]) != n:
            raise ValueError("loaded state dict contains a parameter group that doesn't match the size of optimizer's group")
        for k in ("lr", "betas", "eps"):
            if k in groups[0]:
                self.param_groups[0][k] = tuple(groups[0][k]) if k == "betas" else groups[0][k]
        if groups[0].get("weight_decay", 0) or groups[0].get("amsgrad", False) or groups[0].get("maximize", False):
            raise ValueError("FusedAdam implements torch.optim.Adam's defaults only (no weight decay / amsgrad / maximize)")
        order = {pid: i for i, pid in enumerate(groups[0]["params"])}
        state = {order[k] if k in order else k: v for k, v in state_dict["state"].items()}
        slices = self._slices()
        self.exp_avg.zero_(); self.exp_avg_sq.zero_()
        steps = set()
        for idx, off, m, shape in slices:
            st = state.get(idx)
            if st is None:
                continue
            if tuple(st["exp_avg"].shape) != shape:
                raise ValueError(f"FusedAdam.load_state_dict: parameter {idx} has shape {shape}, state has "
                                 f"{tuple(st['exp_avg'].shape)}")
            self.exp_avg[off:off + m].copy_(st["exp_avg"].reshape(-1))
            self.exp_avg_sq[off:off + m].copy_(st["exp_avg_sq"].reshape(-1))
            steps.add(int(float(st["step"])))
        if len(steps) > 1:
            raise ValueError("FusedAdam keeps ONE step count for all parameters; the state holds %s" % sorted(steps))
        loaded = steps.pop() if steps else 0
        self.step_count.fill_(loaded)
        # a prepared fused step (fused_state()) or a captured graph keeps advancing the DEVICE counter: the host's copy would
        # drift from it after the next such step, so it stays out of the picture once that has happened
        self._host_step = None if self._device_counter_only else loaded
        self._shard_stale = False                  # (every slice holds the loaded state)


class _FlatParamsMixin:
    """Parameters as views of one flat fp32 buffer (+ a flat gradient buffer whose views are
    the .grad tensors), so the fused step writes gradients in place and Adam is one launch."""

    _flat_keys = ()

    def _named_flat(self):
        sd = dict(self.named_parameters())
        return [(k, sd[k]) for k in self._flat_keys]

    def flatten_parameters(self, pad_multiple=None):
        """pad_multiple (sticky once given): the flat buffers' length is rounded up to a multiple of it (zeros behind the last
        parameter) -- the sharded optimizer splits them into world equal slices (ops.exchange_adam(shard=True))."""
        if pad_multiple is not None:
            self._flat_pad = max(1, int(pad_multiple))
        pad = getattr(self, "_flat_pad", 1)
        items = self._named_flat()
        flat = getattr(self, "_flat", None)
        ok = flat is not None and flat.device == items[0][1].device and flat.numel() % pad == 0
        if ok:
            off = 0
            for _, p in items:
                if p.data_ptr() != flat.data_ptr() + 4 * off or p.grad is None or \
                        p.grad.data_ptr() != self._gflat.data_ptr() + 4 * off:
                    ok = False
                    break
                off += p.numel()
        if not ok:
            dev = items[0][1].device
            n = sum(p.numel() for _, p in items)
            n = (n + pad - 1) // pad * pad
            flat = ops.alloc(n, torch.float32, dev, zero=True)
            gflat = ops.alloc(n, torch.float32, dev, zero=True)
            off = 0
            for _, p in items:
                m = p.numel()
                flat[off:off + m].copy_(p.data.reshape(-1))
                if p.grad is not None:
                    gflat[off:off + m].copy_(p.grad.reshape(-1))
                p.data = flat[off:off + m].view(p.shape)
                p.grad = gflat[off:off + m].view(p.shape)
                off += m
            self._flat, self._gflat = flat, gflat
        return self._flat, self._gflat


class Product2Vec(nn.Module, _FlatParamsMixin):
    _flat_keys = ops.P2V_KEYS

    def __init__(self, config):
        super().__init__()
        self.config = config
        if config.PRODUCT_EMB_DIM not in (128, 256) or (config.HIDDEN_SIZE, config.NUM_ATTENTION_HEADS) != (ops.H, ops.HEADS):
            raise ValueError("the gfx950 kernels are built for PRODUCT_EMB_DIM = 128 (config.py:8) or 256 (BASELINE "
                             "configs[4]), HIDDEN_SIZE = 256, NUM_ATTENTION_HEADS = 4 (config.py:10-11)")
        self.dim = int(config.PRODUCT_EMB_DIM)
        # parameter containers only -- same construction order as product2vec.py:14-29, so
        # torch.manual_seed(s) yields the reference's initial weights
        self.ffn = nn.Sequential(
            nn.Linear(config.PRODUCT_EMB_DIM, config.HIDDEN_SIZE),
            nn.BatchNorm1d(config.HIDDEN_SIZE),
            nn.Tanh(),
            nn.Linear(config.HIDDEN_SIZE, config.HIDDEN_SIZE),
            nn.Tanh(),
            nn.Linear(config.HIDDEN_SIZE, config.PRODUCT_EMB_DIM))
        self.attention = nn.MultiheadAttention(embed_dim=config.PRODUCT_EMB_DIM,
                                               num_heads=config.NUM_ATTENTION_HEADS,
                                               dropout=config.DROPOUT, batch_first=True)
        self.last_embedding_table = None
        self._dropout_seed, self._dropout_step = None, 0
        self._dense_idx = {}                      # identity index arrays of the fused dense-batch step, by (B, N, K)

    # ------------------------------------------------------------------ plumbing
    def _tensor_dict(self, dropout=None):
        d = dict(self.named_parameters())
        d.update(dict(self.named_buffers()))
        if dropout is not None:
            d[ops.DROPOUT_KEY] = dropout
        return d

    def _next_dropout(self):
        """(p, seed, offset) of the attention-weight dropout of this training-mode forward
        (nn.MultiheadAttention(dropout=config.DROPOUT), product2vec.py:23-28), None when it is off.  The masks are the
        build's own counter-based stream (include/pcompanion_hip.h pc_dropout) -- ATen's cannot be reproduced, so a
        run with DROPOUT > 0 matches the reference in distribution, not bit for bit; the seed is drawn once from
        torch's generator (torch.manual_seed makes runs repeatable), the offset counts forwards."""
        p = float(getattr(self.config, "DROPOUT", 0.0))
        if not self.training or p == 0.0:
            return None
        if self._dropout_seed is None:
            self._dropout_seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        self._dropout_step += 1
        return (p, self._dropout_seed, self._dropout_step - 1)

    def _weights(self, keys):
        d = dict(self.named_parameters())
        return tuple(d[k] for k in keys)

    @staticmethod
    def _dev(t):
        if not t.is_cuda:
            raise TypeError("Product2Vec runs on the GPU only: move inputs to config.DEVICE (no CPU fallback)")
        return t.contiguous().float()

    # ------------------------------------------------------------------ reference surface
    def get_initial_embedding(self, features: torch.Tensor) -> torch.Tensor:
        """Get initial embedding through FFN (product2vec.py:31-46)."""
        if features.dim() == 1:
            return self._ffn(features.unsqueeze(0)).squeeze(0)
        elif features.dim() == 2:
            return self._ffn(features)
        elif features.dim() == 3:
            B, N, D = features.shape
            return self._ffn(features.reshape(-1, D)).reshape(B, N, -1)
        raise ValueError(f"Unexpected input dimension: {features.dim()}")

    def _key_mask_on(self):
        """config.ATTENTION_KEY_MASK, read at call time like MARGIN (a missing attribute means False): the key-padding mask, a
        labelled deviation from the reference -- padding slots are no keys of the attention and stay out of the neighbour
        call's BatchNorm statistics."""
        return bool(getattr(self.config, "ATTENTION_KEY_MASK", False))

    def _ffn(self, x, pad=None):
        """pad (optional, bool [R], True = padding row): training-mode BatchNorm spans the other rows only.  Costs one host read
        of the real-row count (this is the non-fused path).  No real row: the call does not happen (zeros come back, the
        running statistics stay); exactly one: the error BatchNorm raises for one row."""
        x = self._dev(x)
        if self.training:
            row_weight = count = None
            if pad is not None:
                count = int((~pad).sum())
                if count == 0:
                    return torch.zeros(x.shape[0], self.dim, dtype=torch.float32, device=x.device)
                row_weight = (~pad).to(torch.float32).contiguous()
            if (x.shape[0] if count is None else count) == 1:
                raise ValueError(f"Expected more than 1 value per channel when training, got input size {x.shape}")
            if torch.is_grad_enabled():
                return _FFNFunction.apply(self, x, row_weight, count, *self._weights(_FFN_KEYS))
            y, _ = ops.ffn_forward_train(self._tensor_dict(), x, None, x.shape[0], [0], True, row_weight=row_weight,
                                         counts=None if count is None else [count])
            return y
        with torch.no_grad():
            y = ops.ffn_forward_eval(self._tensor_dict(), x, None, x.shape[0])
        return _guard_eval(y, "Product2Vec.get_initial_embedding", [x] + list(self._weights(_FFN_KEYS)))

    def _pad_mask(self, key_padding_mask, b, n):
        m = key_padding_mask
        if not isinstance(m, torch.Tensor) or m.dtype != torch.bool or tuple(m.shape) != (b, n):
            raise ValueError(f"key_padding_mask: expected a bool tensor of shape {(b, n)} (True = padding)")
        return m.to(self._device()).contiguous()

    def apply_attention(self, query: torch.Tensor, key_value: torch.Tensor,
                        key_padding_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Apply attention mechanism with proper reshaping (product2vec.py:48-68).
        key_padding_mask (optional, bool [B,N], True = padding): nn.MultiheadAttention's argument of that name, which the
        reference never passes -- a labelled deviation.  Padding slots are no keys; a sample without a real slot gets
        out_proj.bias (torch gives NaN).  Training and eval mode."""
        if query.dim() == 1:
            query = query.unsqueeze(0).unsqueeze(0)
        elif query.dim() == 2:
            query = query.unsqueeze(1)
        if key_value.dim() == 2:
            key_value = key_value.unsqueeze(0)
        if query.size(1) != 1:
            raise ValueError("the HIP attention kernel handles one query token per sample "
                             "(the only use in product2vec.py:70-81)")
        q2 = self._dev(query[:, 0, :])
        kv = self._dev(key_value)
        kp = None if key_padding_mask is None else self._pad_mask(key_padding_mask, kv.shape[0], kv.shape[1])
        if torch.is_grad_enabled() and self.training:
            out = _AttentionFunction.apply(self, q2, kv, kp, *self._weights(_ATT_KEYS))
        else:
            with torch.no_grad():
                out, _ = ops.attention_forward(self._tensor_dict(self._next_dropout()), q2, kv, key_pad=kp)   # (dropout off in eval)
            if not self.training:
                out = _guard_eval(out, "Product2Vec.apply_attention", [q2, kv] + list(self._weights(_ATT_KEYS)))
        out = out.unsqueeze(1)
        if query.size(0) == 1 and query.size(1) == 1:
            out = out.squeeze(0).squeeze(0)
        elif query.size(1) == 1:
            out = out.squeeze(1)
        return out

    def forward(self, features: torch.Tensor, neighbors: Optional[torch.Tensor] = None,
                key_padding_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Forward pass through Product2Vec model (product2vec.py:70-81).
        key_padding_mask (optional, bool [B,N] for neighbors [B,N,D], True = padding; a labelled deviation, see
        apply_attention): the padding slots are no keys, and in training mode the neighbour call's BatchNorm spans the
        unmasked rows only -- one host read of their count on this non-fused path."""
        embeddings = self.get_initial_embedding(features)
        if neighbors is not None and neighbors.size(0) > 0:
            if key_padding_mask is not None:
                if neighbors.dim() != 3:
                    raise ValueError("key_padding_mask goes with neighbors of shape [B,N,D]")
                B, N, D = neighbors.shape
                kp = self._pad_mask(key_padding_mask, B, N)
                neighbor_embeddings = self._ffn(neighbors.reshape(-1, D), pad=kp.reshape(-1)).reshape(B, N, -1)
                return self.apply_attention(embeddings, neighbor_embeddings, kp)
            neighbor_embeddings = self.get_initial_embedding(neighbors)
            embeddings = self.apply_attention(embeddings, neighbor_embeddings)
        return embeddings

    # ------------------------------------------------------------------ P11
    @torch.no_grad()
    def generate_embedding_table(self, features: torch.Tensor, cv_rowptr, cv_col, chunk_rows=None):
        """Batched device pass of generate_all_embeddings (product2vec.py:83-111), eval mode:
        pass 1 e1 = ffn(x) for every product; pass 2, for products with co-view out-neighbours,
        attention(query = ffn(e1)  [the reference re-applies the FFN to the stored embedding,
        :105-108 -> :73], keys = ffn(neighbour features) = e1[neighbours]) over the product's
        exact neighbour list (no padding in this pass).
        cv_rowptr / cv_col as CUDA int32 tensors: the CSR stays on the device and the export is one chunked call
        (ops.export_embeddings; chunk_rows products per chunk).  As host numpy arrays: products are grouped by degree on
        the host so each group is one rectangular attention launch."""
        if isinstance(cv_rowptr, torch.Tensor) or isinstance(cv_col, torch.Tensor):
            for name, t in (("cv_rowptr", cv_rowptr), ("cv_col", cv_col)):
                if not isinstance(t, torch.Tensor) or not t.is_cuda:
                    raise TypeError(f"generate_embedding_table: {name} must be a CUDA int32 tensor when the CSR is on the "
                                    "device (or both host numpy arrays)")
            was_training = self.training
            self.eval()
            try:
                out = ops.export_embeddings(self._tensor_dict(), self._dev(features), cv_rowptr, cv_col, chunk_rows=chunk_rows)
            finally:
                self.train(was_training)
            self.last_embedding_table = out
            return out
        was_training = self.training
        self.eval()
        params = self._tensor_dict()
        x = self._dev(features)
        P = x.shape[0]
        e1 = ops.ffn_forward_eval(params, x, None, P)
        e2 = ops.ffn_forward_eval(params, e1, None, P)
        out = e1.clone()
        deg = np.diff(cv_rowptr)
        cv_col = np.asarray(cv_col)
        for d in np.unique(deg):
            if d == 0:
                continue
            nodes = np.nonzero(deg == d)[0]
            starts = cv_rowptr[nodes].astype(np.int64)
            nb = cv_col[(starts[:, None] + np.arange(d)[None, :]).reshape(-1)]
            nb_idx = torch.from_numpy(np.ascontiguousarray(nb, np.int32)).to(x.device)
            node_idx = torch.from_numpy(nodes.astype(np.int32)).to(x.device)
            keys = ops.gather_rows(e1, nb_idx).view(len(nodes), int(d), self.dim)
            query = ops.gather_rows(e2, node_idx)
            upd, _ = ops.attention_forward(params, query, keys)
            ops.scatter_rows(out, node_idx, upd)
        self.train(was_training)
        self.last_embedding_table = out
        return out

    def generate_all_embeddings(self, bpg) -> Dict[str, torch.Tensor]:
        """Generate embeddings for all products in the BPG (product2vec.py:83-111).
        Accepts the integer BPG (p_companion_amd.data.IntBPG) or a reference-style
        BehaviorProductGraph (nodes dict + edges['co_view'] set).  Returns Dict[str, Tensor[128]]
        on the CPU like the reference; the device table stays in self.last_embedding_table.
        A DeviceBPG (world = 1) takes the device-CSR export and returns a read-only Mapping keyed P{i:06d} over the device
        table (data.EmbeddingMapping); a sharded one (world > 1) is refused."""
        from .data import DeviceBPG, EmbeddingMapping, IntBPG
        if isinstance(bpg, DeviceBPG):
            # the large-catalogue path: CSR and features stay in HBM; the result is a read-only Mapping over the device
            # table (one row read per lookup) -- a P-entry dict of host tensors is not built
            if bpg.world != 1:
                raise ValueError(f"generate_all_embeddings: this DeviceBPG holds a cyclic 1/{bpg.world} shard of the features "
                                 f"(rank {bpg.rank}); the export needs the whole table on one device -- generate it with world = 1")
            g = bpg.cuda(self._device())
            if "features" not in g:
                raise ValueError("generate_all_embeddings: the DeviceBPG was generated without features")
            table = self.generate_embedding_table(g["features"], g["cv_rowptr"], g["cv_col"])
            return EmbeddingMapping(table)
        if isinstance(bpg, IntBPG):
            ids = [f"P{i:06d}" for i in range(bpg.num_products)]
            feats = bpg.cuda(self._device())["features"]
            rowptr, col = bpg.cv_rowptr, bpg.cv_col
        else:
            ids = list(bpg.nodes.keys())
            pos = {pid: i for i, pid in enumerate(ids)}
            feats = torch.stack([bpg.nodes[p]["features"] for p in ids]).to(self._device())
            lists = [[pos[t] for t in bpg.get_neighbors(p, edge_type="co_view")] for p in ids]
            rowptr = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
            col = np.array([t for l in lists for t in l], np.int32)
        table = self.generate_embedding_table(feats, np.asarray(rowptr), np.asarray(col))
        cpu = table.cpu()
        return {pid: cpu[i] for i, pid in enumerate(ids)}

    def _device(self):
        return next(self.parameters()).device

    # ------------------------------------------------------------------ P9 loop
    def train_step_indexed(self, table, batch, profile=None, sync_reduce=None, optimizer=None):
        """One loop-body iteration (product2vec.py:130-158 minus optimizer.step) on an index
        batch.  Gradients land in .grad (flat-buffer views); returns the device loss tensor.
        sync_reduce: see ops.p2v_train_step (cross-replica BatchNorm statistics for data-parallel runs).
        optimizer (a FusedAdam over this module): product2vec.py:158's optimizer.step() as well -- inside the step's last
        gradient launch where the batch's layout carries it (the device loader's unique-neighbour batches, one process), by the
        optimizer's own launch otherwise.  Either way the caller does NOT call optimizer.step() for this iteration.
        config.ATTENTION_KEY_MASK (read per call): the masked step, see ops.p2v_train_step(masked=True); not with sync_reduce."""
        flat, gflat = self.flatten_parameters()
        # the tensor dicts and the C structs over them are rebuilt only when a buffer they describe has moved (the parameters and
        # gradients are views of the flat buffers; the BatchNorm buffers are checked by address): a module-tree walk and ~25
        # tensor checks per step otherwise stand between a drained device and the step's first launch
        bn = self.ffn[1]
        key = (flat.data_ptr(), gflat.data_ptr(), bn.running_mean.data_ptr(), bn.running_var.data_ptr(),
               bn.num_batches_tracked.data_ptr(), self.dim)
        cache = _STEP_CACHE.get(self)               # (kept beside the module, not in it: ctypes structs do not pickle / deepcopy)
        if cache is None or cache[0] != key:
            params = self._tensor_dict()
            grads = {k: p.grad for k, p in self.named_parameters()}
            st, dev = ops.p2v_struct(params)
            gst, _ = ops.p2v_struct(grads, with_buffers=False)
            cache = _STEP_CACHE[self] = (key, params, grads, (st, gst, dev))
        params, grads, structs = dict(cache[1]), cache[2], cache[3]
        drop = self._next_dropout()
        if drop is not None:
            params[ops.DROPOUT_KEY] = drop
        nbr = batch.get("neighbor_compact", batch.get("neighbor_idx"))      # compact rows when the loader built them
        adam = None
        if optimizer is not None:
            if not hasattr(optimizer, "riding_state") or optimizer.module is not self:
                raise TypeError("train_step_indexed(optimizer=...) takes the FusedAdam built over this module")
            if sync_reduce is None and isinstance(nbr, dict) and "weight" in nbr:
                adam = optimizer.riding_state()
        out = ops.p2v_train_step(params, grads, table, batch["anchor_idx"], batch["positive_idx"],
                                 batch["negative_idx"], nbr, float(self.config.MARGIN), profile=profile,
                                 sync_reduce=sync_reduce, adam=adam, structs=structs, masked=self._key_mask_on())
        if adam is not None:
            optimizer.advance(1)                   # (only now: the step that carried update number adam["t"] has been accepted)
        elif optimizer is not None:
            optimizer.step()
        after = batch.get("_after_step")           # the device loader's look-ahead builder, queued behind this step's launches
        if after is not None:
            after()
        return out["loss"]

    def train_model(self, train_loader, optimizer, num_epochs=10) -> Dict[str, torch.Tensor]:
        """Train Product2Vec model and generate embeddings for all products
        (product2vec.py:113-170).  Index batches take the fused HIP step; dense reference
        batches take the autograd path.  The loss stays on the device; it is read back once
        per epoch for the log line (the reference syncs every step, :162).  With self.record_step_losses = True (or
        config.RECORD_STEP_LOSSES) the per-step losses (what the reference's progress bar averages, :161-163) are kept in self.step_losses [steps]."""
        device = self.config.DEVICE
        logger = logging.getLogger(__name__)
        self.to(device)
        bpg = train_loader.dataset.bpg
        table = None
        history = [] if (getattr(self, "record_step_losses", False) or getattr(self.config, "RECORD_STEP_LOSSES", False)) else None
        # a device index loader hands out batches that are already where the step reads them: iterated directly (the staging
        # wrapper would put a cross-stream wait in front of every step's first kernel)
        direct = bool(getattr(train_loader, "yields_device_batches", False))
        from .data import prefetch_to_device
        for epoch in range(num_epochs):
            self.train()
            total, pending = None, []
            num_batches = 0

            def fold(total, pending):
                # the epoch's loss sum, on the device: one small reduction per 256 steps instead of an add kernel per step
                part = torch.cat(pending).sum().reshape(1)
                return part if total is None else total + part
            # dense batches: next batch's PCIe copy overlaps this step
            for batch in (train_loader if direct else prefetch_to_device(train_loader, device)):
                if not direct:
                    batch = {k: v.to(device) if isinstance(v, torch.Tensor) else v for k, v in batch.items()}
                if "anchor_idx" in batch:
                    if table is None:
                        table = bpg.cuda(device)["features"]
                    if hasattr(optimizer, "riding_state") and optimizer.module is self:
                        loss = self.train_step_indexed(table, batch, optimizer=optimizer)   # zero_grad + backward + step, fused
                    else:
                        loss = self.train_step_indexed(table, batch)                        # zero_grad + backward, fused
                        optimizer.step()
                else:
                    loss = self.dense_loss(batch)
                    optimizer.zero_grad()
                    loss.backward()
                    optimizer.step()
                    loss = loss.detach().reshape(1)
                pending.append(loss.reshape(1))
                if len(pending) == 256:
                    total, pending = fold(total, pending), []
                num_batches += 1
                if history is not None:
                    history.append(loss.detach().reshape(1).clone())
            if pending:
                total = fold(total, pending)
            if num_batches:
                logger.info(f"Epoch {epoch + 1}/{num_epochs}, Loss: {float(total) / num_batches:.4f}")
        if history is not None:
            self.step_losses = torch.cat(history).cpu() if history else torch.zeros(0)
        self.eval()
        return self.generate_all_embeddings(bpg)

    def dense_loss(self, batch):
        """product2vec.py:132-154 on a dense reference batch (anchor/positive/negative[/anchor_neighbors]).
        With config.ATTENTION_KEY_MASK the key-padding mask is the optional batch key anchor_neighbors_mask (bool [B,N], True =
        padding) or, when the key is absent, the all-zero neighbour rows -- exactly what collate_fn appends, so a reference
        loader works unchanged.  Without the flag the key is ignored."""
        nb = batch.get("anchor_neighbors")
        a, p, n = batch["anchor"], batch["positive"], batch["negative"]
        kp = None
        if self._key_mask_on() and nb is not None and nb.dim() == 3 and nb.shape[1] > 0:
            kp = batch.get("anchor_neighbors_mask")
            kp = (nb == 0).all(dim=-1) if kp is None else kp
            kp = self._pad_mask(kp, nb.shape[0], nb.shape[1])
        if (self.training and torch.is_grad_enabled() and nb is not None and nb.dim() == 3 and nb.shape[0] == a.shape[0]
                and nb.shape[1] > 0 and a.dim() == 2 and p.dim() == 2 and n.dim() == 3 and a.shape[0] > 1
                and not any(t.requires_grad for t in (a, p, n, nb))):
            # training on device batches: the fused step (same numbers as the four module calls below, one launch
            # sequence instead of four forward + four backward ones)
            dev = self.ffn[0].weight.device
            f = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()
            return _FusedDenseLoss.apply(self, f(a), f(p), f(n), f(nb), kp, *[w for _, w in self.named_parameters()])
        anchor_emb = self(batch["anchor"], batch.get("anchor_neighbors"), kp)
        positive_emb = self(batch["positive"])
        negative_emb = self(batch["negative"])
        if negative_emb.dim() == 2:
            negative_emb = negative_emb.unsqueeze(1)
        return _TripletLossFunction.apply(anchor_emb.contiguous(), positive_emb.contiguous(),
                                          negative_emb.contiguous(), float(self.config.MARGIN))
