"""Row-sparse Adam over PCompanion's product table (a labelled extension, DESIGN section 5: the reference's table is frozen).

The table stays requires_grad=False: the update goes around autograd on purpose.  PCompanion.train_step(batch, optimizer,
table_optimizer) forms the gradient of the rows the batch reaches -- its query rows -- with ops.joint_query_grad and hands it
here; step() is one ops.sparse_adam_rows call (torch.optim.SparseAdam's update, duplicates summed in batch order, no float
atomics)."""
import torch

from . import ops


class ProductTableAdam:
    """torch.optim.SparseAdam semantics over model.product_embeddings.weight [P, D]: moments and parameter of a row move only in
    a step that names it.  Holds two zeroed [P, D] fp32 moment tables on the table's device -- twice the table again: 10.2 GB at
    10 M x 128 beside the table's 5.1 GB -- and the step count on the host.  One device (world = 1) only."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        weight = model.product_embeddings.weight
        if weight.dim() != 2 or weight.dtype != torch.float32:
            raise ValueError("ProductTableAdam: model.product_embeddings.weight must be a [P, D] float32 table")
        if not 0.0 <= lr or not 0.0 <= eps or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"ProductTableAdam: invalid lr / betas / eps: {lr}, {betas}, {eps}")
        self.model = model
        self.param_groups = [{"lr": lr, "betas": tuple(betas), "eps": eps, "maximize": False, "params": [0]}]
        self._step = 0
        self.exp_avg = self.exp_avg_sq = None

    def _ensure(self):
        weight = self.model.product_embeddings.weight
        if self.exp_avg is None or self.exp_avg.shape != weight.shape or self.exp_avg.device != weight.device:
            if self._step:
                raise RuntimeError("ProductTableAdam: the product table changed shape or device after the optimizer had stepped; "
                                   "build a new optimizer and load_state_dict() what this one's state_dict() returns")
            self.exp_avg = ops.alloc(weight.numel(), torch.float32, weight.device, zero=True).view(weight.shape)
            self.exp_avg_sq = ops.alloc(weight.numel(), torch.float32, weight.device, zero=True).view(weight.shape)
        return weight

    @torch.no_grad()
    def step(self, idx, grad, bad=None):
        """idx [R] int32 rows of the table (duplicates summed in order, -1 skipped), grad [R, D]: one pc_sparse_adam_rows call."""
        weight = self._ensure()
        g = self.param_groups[0]
        t = self._step + 1
        ops.sparse_adam_rows(weight.data, self.exp_avg, self.exp_avg_sq, idx, grad, t, g["lr"], g["betas"], g["eps"], bad=bad)
        self._step = t                       # (counted once the call has been accepted)

    def state_dict(self):
        """torch.optim.SparseAdam's layout: state[0] = {step, exp_avg, exp_avg_sq} once a step has been taken, and param_groups."""
        state = {}
        if self._step > 0:
            state[0] = {"step": self._step, "exp_avg": self.exp_avg.clone(), "exp_avg_sq": self.exp_avg_sq.clone()}
        return {"state": state, "param_groups": [dict(self.param_groups[0])]}

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        groups = state_dict["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != 1:
            raise ValueError("ProductTableAdam: one parameter group of one parameter expected")
        if groups[0].get("maximize", False):
            raise ValueError("ProductTableAdam implements torch.optim.SparseAdam's defaults only (no maximize)")
        for k in ("lr", "betas", "eps"):
            if k in groups[0]:
                self.param_groups[0][k] = tuple(groups[0][k]) if k == "betas" else groups[0][k]
        st = state_dict["state"].get(groups[0]["params"][0], state_dict["state"].get(0))
        self._step = 0
        weight = self._ensure()
        self.exp_avg.zero_(); self.exp_avg_sq.zero_()
        if st is None:
            return
        for name in ("exp_avg", "exp_avg_sq"):
            if tuple(st[name].shape) != tuple(weight.shape):
                raise ValueError(f"ProductTableAdam.load_state_dict: the table has shape {tuple(weight.shape)}, the state's {name} "
                                 f"{tuple(st[name].shape)}")
            getattr(self, name).copy_(st[name])
        self._step = int(float(st["step"]))
