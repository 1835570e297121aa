"""The per-sample loss and metric kernels against float64 at every branch: ops.triplet_loss, ops.joint_loss,
ops.expand_type_grad, ops.hit_rank, ops.cosine_rows and the cosine of ops.eval_batch_stats.  The cases, the references, the
derived bounds and the checkers are row_loss_cases.py's (its header states every bound and every exact expectation);
test_row_loss_bounds_host.py proves on the CPU that the bounds cannot reject a correct kernel and that the inputs reject
wrong ones.  Every op is called twice with other work in between and must return identical bytes; every case prints its
largest error / bound ratio per output.  Needs an MI355X."""
import ctypes
import hashlib
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import row_loss_cases as rl

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return None if t is None else t.detach().cpu().numpy()


def _twice(call):
    """call() -> tuple of tensors / None; the second call, after unrelated work on the device, must give the same bytes"""
    first = [_host(t) for t in call()]
    torch.randn(1 << 18, device="cuda").sum()
    for a, t in zip(first, call()):
        b = _host(t)
        assert (a is None) == (b is None) and (a is None or a.tobytes() == b.tobytes())
    return first


def triplet_run(a, p, n, margin, need_grad):
    from p_companion_amd import ops
    da, dp, dn = _dev(a), _dev(p), _dev(n)
    keys = ("loss", "d_pos", "d_neg") + (("da", "dp", "dn") if need_grad else ())

    def call():
        out = ops.triplet_loss(da, dp, dn, margin, need_grad=need_grad)
        assert set(out) == set(keys)
        return tuple(out[k] for k in keys)
    return dict(zip(keys, _twice(call)))


def joint_run(sims, proj, pos_t, neg_t, pos, neg, margin, alpha, need_grad):
    from p_companion_amd import ops
    args = [_dev(t) for t in (sims, proj, pos_t, neg_t, pos, neg)]
    return tuple(_twice(lambda: ops.joint_loss(*args, margin, alpha, need_grad=need_grad)))


def expand_run(dsv, pos_t, neg_t, t):
    from p_companion_amd import ops
    args = [_dev(dsv), _dev(pos_t), _dev(neg_t)]
    return _twice(lambda: (ops.expand_type_grad(*args, t),))[0]


def cosine_run(x, y):
    from p_companion_amd import ops
    dx, dy = _dev(x), _dev(y)
    return _twice(lambda: (ops.cosine_rows(dx, dy),))[0]


def hit_run(s):
    from p_companion_amd import ops
    ds = _dev(s)
    return _twice(lambda: (ops.hit_rank(ds),))[0]


def _show(what, ratios):
    print(what, "error / bound:", {k: round(v, 4) for k, v in ratios.items()})


@pytest.mark.parametrize("case", rl.TRIPLET_CASES, ids=rl.triplet_id)
def test_triplet_loss_against_float64(case):
    """d_pos, d_neg, the mean and the three gradients inside the derived bounds; the float64 hinge decision on every decided
    sample; exact zeros on the inactive side, on the exact edge (relu'(0) = 0) and for a distance of exactly 0 (the oracle's
    zero row: the kernels select 0 where they would divide by it); need_grad=False gives the same forward bits."""
    _show(rl.triplet_id(case), rl.check_triplet(case, triplet_run))


@pytest.mark.parametrize("case", rl.JOINT_CASES, ids=rl.joint_id)
def test_joint_loss_against_float64(case):
    _show(rl.joint_id(case), rl.check_joint(case, joint_run, expand_run))


@pytest.mark.parametrize("case", rl.EXACT_CASES, ids=lambda c: "D%d-B%d-K%d" % c)
def test_joint_loss_equals_float64_on_dyadic_data(case):
    """losses, dsims_val, dproj and the dense type gradient EQUAL the float64 oracle: zero norms (subgradient 0), both hinges
    at exactly 0 (torch.clamp: subgradient 1), above and below"""
    rl.check_joint_exact(case, joint_run, expand_run)


@pytest.mark.parametrize("shape", rl.HIT_SHAPES, ids=lambda s: "%dx%d" % s)
def test_hit_rank_equals_the_integer_count(shape):
    rl.check_hit_rank(shape, hit_run)


@pytest.mark.parametrize("case", rl.COSINE_CASES, ids=lambda c: "D%d-B%d-K%d" % c)
def test_cosine_rows_against_float64(case):
    _show("cosine D%d-B%d-K%d" % case, {"cos": rl.check_cosine(case, cosine_run)})


@pytest.mark.parametrize("dim", [128, 256])
def test_eval_batch_stats_clamps_each_norm(dim):
    """the clamp rows of cosine_rows through pc_eval_batch_stats at B = K = 1: cos_sum is the same bits"""
    from p_companion_amd import ops
    x, y, want = rl.clamp_rows(dim)
    types = torch.zeros(1, 1, dtype=torch.int32, device="cuda")
    for r in range(2):
        proj, pos = _dev(x[r:r + 1]), _dev(y[r:r + 1])
        got = _twice(lambda: ops.eval_batch_stats(proj, pos, pos, types))
        assert got[1].dtype == np.float32 and got[1].view(np.int32)[0] == want.view(np.int32), (got, want)


def _cfg():
    return SimpleNamespace(PRODUCT_EMB_DIM=128, TYPE_EMB_DIM=64, HIDDEN_SIZE=256, NUM_ATTENTION_HEADS=4, DROPOUT=0.0,
                           MARGIN=1.0, ALPHA=0.8, NUM_COMP_TYPES=3, NUM_TYPES=40, DEVICE=torch.device("cuda"),
                           LEARNING_RATE=1e-3)


def _step_digest(table, batch):
    """three fused Product2Vec steps on one index batch -> a digest of the losses, the parameters and the running variance"""
    from p_companion_amd.product2vec import FusedAdam, Product2Vec
    torch.manual_seed(0)
    m = Product2Vec(_cfg()).to("cuda").train()
    opt = FusedAdam(m, lr=1e-3)
    h = hashlib.sha256()
    for _ in range(3):
        loss = m.train_step_indexed(table, batch)
        opt.step()
        assert bool(torch.isfinite(loss).all())
        h.update(loss.detach().cpu().numpy().tobytes())
    torch.cuda.synchronize()
    h.update(m.flatten_parameters()[0].detach().cpu().numpy().tobytes())
    h.update(m.ffn[1].running_var.cpu().numpy().tobytes())
    return h.hexdigest()


def test_fused_step_gives_one_digest_under_both_loss_settings():
    """A triplet case (D = 128, B = 33, K = 8: a ragged last 16-sample tile) as the feature rows of a fused Product2Vec step,
    with the hinge inside the attention backward's first launch (PC_OPT_FUSED_LOSS = 1, the default) and as its own launch: the
    same digest.  The batch holds the case's p == a sample (identical feature rows; n_0 == a too), its zero rows and its far
    positive.  (The step-level parity with the oracle is test_gpu_streams.py's and test_gpu_p2v_step.py's.)"""
    from p_companion_amd import _lib, ops
    case = (128, 33, 8, 0)
    assert case in rl.TRIPLET_CASES
    a, p, n, rows = rl.triplet_inputs(case)
    b, k = case[1], case[2]
    assert (a[rows["eps"]] == p[rows["eps"]]).all()
    table = _dev(np.concatenate([a, p, n.reshape(b * k, 128)]))
    g = torch.Generator().manual_seed(5)
    nb = torch.randint(-1, table.shape[0], (b, 6), generator=g, dtype=torch.int32)
    batch = {"anchor_idx": torch.arange(b, dtype=torch.int32).cuda(),
             "positive_idx": (b + torch.arange(b, dtype=torch.int32)).cuda(),
             "negative_idx": (2 * b + torch.arange(b * k, dtype=torch.int32)).reshape(b, k).cuda(),
             "neighbor_idx": nb.cuda()}
    batch["neighbor_compact"] = ops.unique_neighbors(batch["neighbor_idx"])
    L = _lib.lib()
    v = ctypes.c_int(-1)
    assert L.pc_get_option(_lib.PC_OPT_FUSED_LOSS, ctypes.byref(v)) == 0 and v.value == 1
    digests = []
    try:
        for on in (1, 0):
            assert L.pc_set_option(_lib.PC_OPT_FUSED_LOSS, on) == 0
            digests.append(_step_digest(table, batch))
            torch.cuda.synchronize()
    finally:
        L.pc_set_option(_lib.PC_OPT_FUSED_LOSS, 1)
    assert digests[0] == digests[1]
