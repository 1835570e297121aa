"""A trainable product table in the joint step (csrc/table_train.hip; a labelled extension): the query rows'
gradient (pc_joint_query_grad) against an fp64 restatement with the per-op autograd route as the yardstick, the row-sparse
Adam (pc_sparse_adam_rows) bit for bit against a numpy fp32 restatement and against torch.optim.SparseAdam, the step
(PCompanion.train_step(table_optimizer=)) against its twin without a trained table and against an fp64 autograd twin, and
train.train with config.TRAIN_PRODUCT_EMBEDDINGS.  Needs an MI355X.

Measured on an MI355X, e = max|dq - ref| / max|ref| against fp64, (B, K, D): this entry / the per-op autograd route
  (1, 1, 128)    4.56e-07 / 4.12e-07
  (5, 3, 128)    3.16e-07 / 3.04e-07
  (67, 4, 128)   4.53e-07 / 4.38e-07
  (130, 3, 256)  5.91e-07 / 5.91e-07
"""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T_Q, P_Q, ALPHA_Q = 7, 23, 0.8
# (B, K, D) -> seed of np.random.default_rng for which query_conditions() holds (found on the CPU)
QUERY_SEEDS = {(1, 1, 128): 0, (5, 3, 128): 2, (67, 4, 128): 0, (130, 3, 256): 0}


def cfg(tmp=None, **over):
    c = SimpleNamespace(PRODUCT_EMB_DIM=128, TYPE_EMB_DIM=64, HIDDEN_SIZE=256, NUM_ATTENTION_HEADS=4, DROPOUT=0.0,
                        MARGIN=1.0, ALPHA=0.8, NUM_COMP_TYPES=3, NUM_TYPES=20, DEVICE=torch.device("cuda"),
                        LEARNING_RATE=1e-3, BATCH_SIZE=256, PRODUCT2VEC_EPOCHS=1, NUM_EPOCHS=1, MODEL_DIR=str(tmp))
    c.__dict__.update(over)
    return c


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


# ------------------------------------------------------------------ 1. the query rows' gradient
def query_inputs(B, K, D, seed):
    rng = np.random.default_rng(seed)
    f = np.float32
    x = dict(table=rng.standard_normal((P_Q, D)).astype(f), ec=rng.standard_normal((T_Q, 64)).astype(f),
             pos=rng.standard_normal((B, D)).astype(f), neg=rng.standard_normal((B, D)).astype(f),
             w_item=(rng.uniform(-1, 1, (D, D)) / math.sqrt(D)).astype(f), b_item=(rng.uniform(-1, 1, D) / math.sqrt(D)).astype(f),
             w_type=(rng.uniform(-1, 1, (D, 64)) / 8).astype(f), b_type=(rng.uniform(-1, 1, D) / 8).astype(f),
             query_idx=rng.integers(0, P_Q, B).astype(np.int32),
             topk=np.stack([rng.permutation(T_Q)[:K] for _ in range(B)]).astype(np.int32))
    return x


def query_ref64(x, margin, alpha):
    """The formulas of the extension in float64: dq [B, D], the hinge arguments l [B, K]."""
    d = {k: (v.astype(np.float64) if v.dtype == np.float32 else v) for k, v in x.items()}
    B, K = d["topk"].shape
    q = d["table"][d["query_idx"]]
    pi = q @ d["w_item"].T + d["b_item"]
    tp = d["ec"][d["topk"]] @ d["w_type"].T + d["b_type"]              # [B, K, D]
    xx = pi[:, None, :] * tp
    dp, dn = xx - d["pos"][:, None, :], xx - d["neg"][:, None, :]
    np_, nn_ = np.sqrt((dp * dp).sum(-1)), np.sqrt((dn * dn).sum(-1))
    l = margin - np_ + nn_
    g = np.where(l > 0, alpha / (B * K), 0.0)
    ip = np.where(np_ > 0, g / np.where(np_ > 0, np_, 1.0), 0.0)
    in_ = np.where(nn_ > 0, g / np.where(nn_ > 0, nn_, 1.0), 0.0)
    dx = -dp * ip[..., None] + dn * in_[..., None]
    dpi = (dx * tp).sum(1)
    return dpi @ d["w_item"], l


def query_conditions(l):
    """No hinge on its edge; for B K >= 4 between a quarter and three quarters of them active."""
    if np.abs(l).min() < 1e-3:
        return False
    return l.size < 4 or 0.25 <= float((l > 0).mean()) <= 0.75


def scratch_model(x, K, D, table):
    """A PCompanion over `table` carrying the case's item branch (the type branch keeps its random initialisation)."""
    from p_companion_amd.p_companion import PCompanion
    c = cfg(PRODUCT_EMB_DIM=D, NUM_TYPES=T_Q, NUM_COMP_TYPES=K, MARGIN=0.0, ALPHA=ALPHA_Q)
    torch.manual_seed(3)
    m = PCompanion(c, torch.from_numpy(table)).to("cuda").train()
    with torch.no_grad():
        m.item_prediction.item_projection.weight.copy_(torch.from_numpy(x["w_item"]))
        m.item_prediction.item_projection.bias.copy_(torch.from_numpy(x["b_item"]))
        m.item_prediction.type_projection.weight.copy_(torch.from_numpy(x["w_type"]))
        m.item_prediction.type_projection.bias.copy_(torch.from_numpy(x["b_type"]))
        m.complementary_type_embeddings.weight.copy_(torch.from_numpy(x["ec"]))
    return m


def new_route(m, x, table=None, query_idx=None, topk=None, bad=None):
    from p_companion_amd import ops
    params = {k: v.detach() for k, v in m.named_parameters()}
    params["product_embeddings.weight"] = torch.from_numpy(x["table"] if table is None else table).cuda()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return ops.joint_query_grad(params, dev(x["query_idx"] if query_idx is None else query_idx),
                                dev(x["topk"] if topk is None else topk), dev(x["pos"]), dev(x["neg"]), 0.0, ALPHA_Q, bad=bad)


def parent_route(x, K, D, monkeypatch):
    """The per-op autograd route as it stands without this extension: _forward_graph + _JointLoss under autograd on a scratch
    model whose table requires a gradient; the query ids are made unique (row b of the scratch table = the row sample b reads),
    so weight.grad[b] is dq[b].  The case's topk stands in for the type branch's."""
    from p_companion_amd import ops
    from p_companion_amd.p_companion import _JointLoss
    B = x["query_idx"].shape[0]
    m = scratch_model(x, K, D, x["table"][x["query_idx"]])
    m.product_embeddings.weight.requires_grad_(True)
    topk = torch.from_numpy(x["topk"]).cuda()
    monkeypatch.setattr(ops, "topk_rows", lambda sims, k, want_values=False: topk)
    qi = torch.arange(B, dtype=torch.int32, device="cuda")
    zi = torch.zeros(B, dtype=torch.int32, device="cuda")
    sims, top, proj = m._forward_graph(qi, zi, K)
    assert top is topk
    loss = _JointLoss.apply(sims.contiguous(), proj.contiguous(), zi, zi, torch.from_numpy(x["pos"]).cuda(),
                            torch.from_numpy(x["neg"]).cuda(), 0.0, ALPHA_Q, 0)
    (grad,) = torch.autograd.grad(loss, [m.product_embeddings.weight])
    monkeypatch.undo()
    return m, grad.cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("B,K,D", sorted(QUERY_SEEDS))
def test_query_gradient_against_fp64(B, K, D, monkeypatch):
    x = query_inputs(B, K, D, QUERY_SEEDS[(B, K, D)])
    ref, l = query_ref64(x, 0.0, ALPHA_Q)
    assert query_conditions(l), "the seed no longer meets the conditions on the inputs"
    m, parent = parent_route(x, K, D, monkeypatch)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = new_route(m, x, bad=bad).cpu().numpy().astype(np.float64)
    assert int(bad) == 0
    dead = ~(l > 0).any(axis=1)
    assert (got[dead] == 0).all(), "a sample without an active hinge has a zero gradient row, exactly"
    assert (ref[dead] == 0).all()
    scale = np.abs(ref).max()
    e_new, e_parent = np.abs(got - ref).max() / scale, np.abs(parent - ref).max() / scale
    print(f"query gradient (B, K, D) = ({B}, {K}, {D}): e(new) = {e_new:.3e}, e(parent route) = {e_parent:.3e}")
    assert e_new <= max(4 * e_parent, 8 * 2.0 ** -24), (e_new, e_parent)


def test_query_gradient_at_a_zero_norm():
    """All weights zero, b_item = 1, b_type = pos of one sample: x = pos exactly there, np = 0 under an active hinge -- the
    positive term vanishes (subgradient 0 at a zero norm) and nothing turns infinite."""
    B, K, D = 5, 3, 128
    x = query_inputs(B, K, D, 1)
    for k in ("w_item", "w_type"):
        x[k] = np.zeros_like(x[k])
    x["b_item"] = np.ones_like(x["b_item"])
    x["b_type"] = x["pos"][2].copy()
    ref, l = query_ref64(x, 0.0, ALPHA_Q)
    assert l[2].min() > 0 and (ref == 0).all()                        # (np = 0, nn > 0: active; W_item = 0: dq = 0 dpi)
    m = scratch_model(x, K, D, x["table"])
    got = new_route(m, x).cpu().numpy()
    assert np.isfinite(got).all() and (got == 0).all()
    # the same sample with W_item = I: dq = dpi, where an unguarded g / np would show as inf / nan
    x["w_item"] = np.eye(D, dtype=np.float32)
    x["b_item"] = np.zeros_like(x["b_item"])
    x["table"][x["query_idx"][2]] = 1.0
    ref, l = query_ref64(x, 0.0, ALPHA_Q)
    assert l[2].min() > 0
    m = scratch_model(x, K, D, x["table"])
    got = new_route(m, x).cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    assert np.abs(got - ref).max() <= 1e-5 * np.abs(ref).max()


def test_query_gradient_ids_out_of_range():
    B, K, D = 67, 4, 128
    x = query_inputs(B, K, D, 2)
    m = scratch_model(x, K, D, x["table"])
    clean = new_route(m, x)
    qi, topk = x["query_idx"].copy(), x["topk"].copy()
    qi[5] = P_Q
    topk[40, 2] = T_Q
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = new_route(m, x, query_idx=qi, topk=topk, bad=bad)
    assert int(bad) == 2
    assert (got[5] == 0).all() and (got[40] == 0).all()
    keep = [b for b in range(B) if b not in (5, 40)]
    assert torch.equal(bits(got[keep]), bits(clean[keep]))
    # negative ids as well, and the counter is added to
    qi[6], topk[41, 0] = -1, -7
    new_route(m, x, query_idx=qi, topk=topk, bad=bad)
    assert int(bad) == 6


# ------------------------------------------------------------------ 2. the row-sparse Adam
def coalesce_in_order(idx, grad, P):
    """(distinct valid ids ascending, their gradient sums: sequential fp32 adds in ascending position, number of bad ids)."""
    valid = (idx >= 0) & (idx < P)
    nbad = int(((idx != -1) & ~valid).sum())
    rows = np.nonzero(valid)[0]
    order = rows[np.argsort(idx[rows], kind="stable")]
    ids = idx[order]
    if ids.size == 0:
        return ids, np.zeros((0, grad.shape[1]), np.float32), nbad
    start = np.nonzero(np.concatenate([[True], ids[1:] != ids[:-1]]))[0]
    length = np.diff(np.concatenate([start, [ids.size]]))
    g = grad[order[start]].copy()
    for j in range(1, int(length.max())):
        seg = np.nonzero(length > j)[0]
        g[seg] = g[seg] + grad[order[start[seg] + j]]               # (float32 + float32: one rounding)
    return ids[start], g, nbad


def sparse_adam_ref(p, m, v, idx, grad, t, lr, b1, b2, eps):
    """The update in numpy float32, one rounding per operation; p, m, v are changed in place.  Returns the bad count."""
    f = np.float32
    u, g, nbad = coalesce_in_order(idx, grad, p.shape[0])
    omb1, omb2, epsf = f(1.0 - b1), f(1.0 - b2), f(eps)
    neg_s = -f(lr * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t))
    mu, vu = m[u], v[u]
    mu = mu + (g - mu) * omb1
    vu = vu + (g * g - vu) * omb2
    den = np.sqrt(vu) + epsf
    p[u] = p[u] + neg_s * (mu / den)
    m[u], v[u] = mu, vu
    assert p.dtype == m.dtype == v.dtype == np.float32
    return nbad


GUARD = 3


def guarded(a):
    """`a` [P, D] between GUARD canary rows on the device: (buffer, the [P, D] view)."""
    buf = torch.full((a.shape[0] + 2 * GUARD, a.shape[1]), 12345.0, dtype=torch.float32, device="cuda")
    buf[GUARD:GUARD + a.shape[0]] = torch.from_numpy(a)
    return buf, buf[GUARD:GUARD + a.shape[0]]


def canaries_intact(buf):
    c = torch.cat([buf[:GUARD], buf[-GUARD:]])
    return bool((c == 12345.0).all())


def adam_case_idx(rng, R, P):
    """R ids: rows of multiplicity exactly 65, 2, 2, 1, 300 and (where R allows) 1500 among random ones, seventeen -1, one id
    at P and one at -2."""
    idx = rng.integers(0, P, R).astype(np.int32)
    if R >= 1000 and P >= 400:
        hot = rng.choice(P, 7, replace=False).astype(np.int32)
        idx[np.isin(idx, hot[:6])] = hot[6]                           # (the six multiplicities are then exact)
        free = rng.permutation(R)
        at = 0
        for u, mult in zip(hot[:6], (65, 2, 2, 1, 300, 1500 if R >= 20_000 else 3)):
            idx[free[at:at + mult]] = u
            at += mult
        idx[free[at:at + 17]] = -1
        idx[free[at + 17]] = P
        idx[free[at + 18]] = -2
    elif R > 4:
        idx[rng.permutation(R)[:3]] = (-1, P, -2)
    return idx


@pytest.mark.parametrize("D", [128, 256])
@pytest.mark.parametrize("R,P", [(1, 50), (1000, 700), (1000, 1), (70_000, 70_000), (70_000, 40_000)])
def test_sparse_adam_bit_for_bit(R, P, D):
    from p_companion_amd import ops
    rng = np.random.default_rng(1000 * D + R + P)
    f = np.float32
    p = rng.standard_normal((P, D)).astype(f)
    m, v = np.zeros((P, D), f), np.zeros((P, D), f)
    (pb, pd), (mb, md), (vb, vd) = guarded(p), guarded(m), guarded(v)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    lr, (b1, b2), eps = 1e-3, (0.9, 0.999), 1e-8
    nbad = 0
    for t in range(1, 6):
        idx = adam_case_idx(rng, R, P)
        if t == 1 and R >= 20_000:
            mult = np.bincount(idx[(idx >= 0) & (idx < P)], minlength=P)
            assert {1, 2, 65, 1500} <= set(mult.tolist())
        grad = (rng.standard_normal((R, D)) * 10.0 ** rng.uniform(-6, 1, (R, 1))).astype(f)
        didx, dgrad = torch.from_numpy(idx).cuda(), torch.from_numpy(grad).cuda()
        if t == 3:
            # the same call from the same state gives the same bits
            twin = [x.clone() for x in (pd, md, vd)]
            ops.sparse_adam_rows(twin[0], twin[1], twin[2], didx, dgrad, t, lr, (b1, b2), eps)
        ops.sparse_adam_rows(pd, md, vd, didx, dgrad, t, lr, (b1, b2), eps, bad=bad)
        if t == 3:
            for a, b in zip(twin, (pd, md, vd)):
                assert torch.equal(bits(a), bits(b))
        nbad += sparse_adam_ref(p, m, v, idx, grad, t, lr, b1, b2, eps)
        # every bit of the three tables: the touched rows follow the restatement, the others keep theirs
        for name, dev, ref in (("exp_avg", md, m), ("exp_avg_sq", vd, v), ("table", pd, p)):
            got = dev.cpu().numpy()
            diff = np.nonzero((got.view(np.int32) != ref.view(np.int32)).any(axis=1))[0]
            assert diff.size == 0, (name, t, diff[:5], got[diff[:1]], ref[diff[:1]])
        assert int(bad) == nbad
    assert nbad > 0 or R == 1
    assert canaries_intact(pb) and canaries_intact(mb) and canaries_intact(vb)


def test_sparse_adam_against_torch_sparse_adam():
    """torch.optim.SparseAdam on the CPU, fed the gradient coalesced in ascending position: the moments are equal bit for bit
    over the steps; the parameters start every step from torch's and are held to |d| <= 2^-22 (|p| + 4 lr) (torch rounds
    the last product differently, by one ulp of the parameter)."""
    from p_companion_amd import ops
    rng = np.random.default_rng(7)
    P, D, R, lr = 200, 128, 300, 1e-3
    w = torch.nn.Parameter(torch.from_numpy(rng.standard_normal((P, D)).astype(np.float32)))
    opt = torch.optim.SparseAdam([w], lr=lr)
    pd = w.detach().clone().cuda()
    md, vd = torch.zeros_like(pd), torch.zeros_like(pd)
    for t in range(1, 8):
        idx = rng.integers(0, P, R).astype(np.int32)
        idx[:40] = idx[40:80]
        grad = (rng.standard_normal((R, D)) * 10.0 ** rng.uniform(-6, 1, (R, 1))).astype(np.float32)
        u, g, _ = coalesce_in_order(idx, grad, P)
        w.grad = torch.sparse_coo_tensor(torch.from_numpy(u.astype(np.int64))[None], torch.from_numpy(g), (P, D))
        pd.copy_(w.detach())
        opt.step()
        ops.sparse_adam_rows(pd, md, vd, torch.from_numpy(idx).cuda(), torch.from_numpy(grad).cuda(), t, lr)
        st = opt.state[w]
        assert torch.equal(bits(md), bits(st["exp_avg"])), t
        assert torch.equal(bits(vd), bits(st["exp_avg_sq"])), t
        d = (pd.cpu() - w.detach()).abs()
        assert bool((d <= 2.0 ** -22 * (w.detach().abs() + 4 * lr)).all()), (t, float(d.max()))
        untouched = np.setdiff1d(np.arange(P), u)
        assert torch.equal(bits(pd[untouched]), bits(w.detach()[untouched]))


# ------------------------------------------------------------------ 3. the step
P_S, T_S, K_S, B_S = 2000, 20, 3, 256


def step_batch(D, seed):
    g = torch.Generator().manual_seed(seed)
    qi = torch.randint(0, P_S, (B_S,), generator=g, dtype=torch.int32)
    qi[:8] = qi[8:16]                                                  # popular queries repeat inside a batch
    return {"query_idx": qi.cuda(), "query_types": torch.randint(0, T_S, (B_S,), generator=g).cuda(),
            "positive_types": torch.randint(0, T_S, (B_S, 1), generator=g).cuda(),
            "negative_types": torch.randint(0, T_S, (B_S, 1), generator=g).cuda(),
            "positive_items": torch.randn(B_S, D, generator=g).cuda(), "negative_items": torch.randn(B_S, D, generator=g).cuda()}


def step_models(D, n, **over):
    from p_companion_amd.p_companion import PCompanion
    c = cfg(PRODUCT_EMB_DIM=D, NUM_TYPES=T_S, NUM_COMP_TYPES=K_S, **over)
    table = torch.randn(P_S, D, generator=torch.Generator().manual_seed(D))
    torch.manual_seed(1)
    models = [PCompanion(c, table).to("cuda").train()]
    st0 = {k: v.detach().clone() for k, v in models[0].state_dict().items()}
    for _ in range(n - 1):
        models.append(PCompanion(c, table).to("cuda").train())
        models[-1].load_state_dict(st0)
    return c, table, models


def pin_scatter_order(monkeypatch, D):
    """At PRODUCT_EMB_DIM = 256 the step is the per-op route, whose nn.Embedding backward (functional._Embedding.backward ->
    ops.scatter_add_rows) adds the rows of one id with float atomics: two runs of the SAME unchanged step differ (measured on an
    MI355X with these shapes: 4 of the 1280 elements of query_type_embeddings.weight after one step, max 6e-8; from the second
    step on every weight), so 'bit for bit against a twin' says nothing there until that order is pinned.  Both models of a
    twin test therefore run with the one op replaced by the same sum in ascending position (numpy, on the host); everything
    else of the step is the code as it stands.  At 128 the step holds no float atomics on these shapes and nothing is replaced."""
    if D == 128:
        return
    from p_companion_amd import ops

    def ordered(table, idx, src):
        t, i, x = table.cpu().numpy(), idx.cpu().numpy(), src.cpu().numpy()
        np.add.at(t, i[i >= 0], x[i >= 0])
        table.copy_(torch.from_numpy(t))

    monkeypatch.setattr(ops, "scatter_add_rows", ordered)


@pytest.mark.parametrize("D", [128, 256])
def test_step_with_a_zero_table_rate_is_the_step_without(D, monkeypatch):
    from p_companion_amd.product2vec import FusedAdam
    from p_companion_amd.table_optim import ProductTableAdam
    pin_scatter_order(monkeypatch, D)
    _, table, (a, b) = step_models(D, 2)
    oa, ob, ta = FusedAdam(a, lr=1e-3), FusedAdam(b, lr=1e-3), ProductTableAdam(a, lr=0.0)
    assert not a.product_embeddings.weight.requires_grad
    for s in range(3):
        batch = step_batch(D, 10 + s)
        la, ka = a.train_step(batch, optimizer=oa, table_optimizer=ta)
        lb, kb = b.train_step(batch)
        ob.step()
        assert torch.equal(bits(la), bits(lb)) and torch.equal(ka, kb), s
        for (k, va), (_, vb) in zip(a.state_dict().items(), b.state_dict().items()):
            assert torch.equal(bits(va), bits(vb)), (s, k)
    assert torch.equal(bits(a.product_embeddings.weight), bits(table.cuda()))
    assert ta.state_dict()["state"][0]["step"] == 3 and a.index_errors() == 0
    assert not a.product_embeddings.weight.requires_grad


@pytest.mark.parametrize("D", [128, 256])
def test_step_moves_exactly_the_query_rows(D, monkeypatch):
    from p_companion_amd.product2vec import FusedAdam
    from p_companion_amd.table_optim import ProductTableAdam
    pin_scatter_order(monkeypatch, D)
    # MARGIN = 100: every hinge is active, so every query row has a gradient
    _, table, (a, b) = step_models(D, 2, MARGIN=100.0)
    oa, ob, ta = FusedAdam(a, lr=1e-3), FusedAdam(b, lr=1e-3), ProductTableAdam(a, lr=1e-3)
    batch = step_batch(D, 20)
    la, ka = a.train_step(batch, optimizer=oa, table_optimizer=ta)
    lb, kb = b.train_step(batch)
    ob.step()
    assert torch.equal(bits(la), bits(lb)) and torch.equal(ka, kb)
    for (k, va), (_, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        if k != "product_embeddings.weight":
            assert torch.equal(bits(va), bits(vb)), k
    assert torch.equal(bits(b.product_embeddings.weight), bits(table.cuda()))
    moved = (bits(a.product_embeddings.weight) != bits(b.product_embeddings.weight)).any(dim=1)
    want = torch.zeros(P_S, dtype=torch.bool)
    want[batch["query_idx"].cpu().long()] = True
    assert torch.equal(moved, want)
    with pytest.raises(TypeError, match="ProductTableAdam"):
        a.train_step(batch, optimizer=oa, table_optimizer=ProductTableAdam(b))
    with pytest.raises(TypeError, match="ProductTableAdam"):
        a.train_step(batch, optimizer=oa, table_optimizer=torch.optim.SparseAdam([torch.nn.Parameter(torch.zeros(2, 2))]))


@pytest.mark.parametrize("D", [128, 256])
def test_three_steps_against_an_fp64_autograd_twin(D):
    """torch.optim.Adam for the weights and torch.optim.SparseAdam for the table over the float64 restatement of the whole
    model, the same batch three times, the table at a rate (0.05) at which its update decides the later losses."""
    from oracle import joint_oracle
    from p_companion_amd.product2vec import FusedAdam
    from p_companion_amd.table_optim import ProductTableAdam
    c, table, (a,) = step_models(D, 1)
    lr_table = 0.05
    oa, ta = FusedAdam(a, lr=1e-3), ProductTableAdam(a, lr=lr_table)
    batch = step_batch(D, 30)
    hb = {k: (v.cpu().double() if v.is_floating_point() else v.cpu().long()) for k, v in batch.items()}
    uq = torch.unique(hb["query_idx"])

    def twin(train_table):
        st = {k: torch.nn.Parameter(v.detach().cpu().double()) for k, v in a.state_dict().items()}
        tbl = st["product_embeddings.weight"]
        adam = torch.optim.Adam([st[k] for k in joint_oracle.TRAINABLE], lr=1e-3)
        sparse = torch.optim.SparseAdam([tbl], lr=lr_table)
        losses = []
        for _ in range(3):
            out = joint_oracle.forward(st, hb["query_idx"], hb["query_types"], K_S)
            loss = joint_oracle.compute_loss(out, hb, float(c.MARGIN), float(c.ALPHA))[0]
            adam.zero_grad()
            tbl.grad = None
            loss.backward()
            losses.append(float(loss.detach()))
            adam.step()
            if train_table:
                tbl.grad = torch.sparse_coo_tensor(uq[None], tbl.grad[uq], tbl.shape)
                sparse.step()
        return losses, tbl.detach()

    want, tbl64 = twin(True)
    frozen, _ = twin(False)
    assert abs(want[2] - frozen[2]) > 1e-3, "the table's update must decide the third loss, or this test shows nothing"
    for s in range(3):
        losses, _ = a.train_step(batch, optimizer=oa, table_optimizer=ta)
        print(f"D = {D} step {s + 1}: loss {float(losses[0]):.7f}, fp64 twin {want[s]:.7f}, frozen twin {frozen[s]:.7f}")
        assert abs(float(losses[0]) - want[s]) <= 1e-4, (s, float(losses[0]), want[s])
    # (Adam's first steps move an element by about lr whatever its gradient's size, so an element whose gradient is lost in
    # fp32 rounding may take the other direction: the touched rows are compared as a fraction, not by their maximum)
    d = (a.product_embeddings.weight.detach().cpu().double() - tbl64)[uq].abs()
    assert float((d <= 1e-3).double().mean()) >= 0.99
    rest = torch.ones(P_S, dtype=torch.bool)
    rest[uq] = False
    assert torch.equal(a.product_embeddings.weight.detach().cpu()[rest], table[rest])


# ------------------------------------------------------------------ 4. the loop
@pytest.mark.parametrize("source,D", [("host", 128), ("device", 128), ("device", 256)])
def test_train_with_the_flag(source, D, tmp_path):
    from p_companion_amd import train as drv
    from p_companion_amd.data import ComplementaryIndexDataset, ComplementaryIndexLoader, generate_device_bpg
    from p_companion_amd.metrics import Metrics
    from p_companion_amd.p_companion import PCompanion
    bpg = generate_device_bpg(P_S, T_S, seed=4, dim=D)
    graph = bpg.to_host() if source == "host" else bpg
    table = torch.randn(P_S, D, generator=torch.Generator().manual_seed(3))

    def loaders():
        return [ComplementaryIndexLoader(ComplementaryIndexDataset(graph, mode, seed=5), 128, shuffle=sh, seed=1)
                for mode, sh in (("train", True), ("val", False))]

    runs = {}
    for flag in (True, False):
        c = cfg(tmp_path / str(flag), PRODUCT_EMB_DIM=D, NUM_TYPES=T_S, NUM_EPOCHS=2, BATCH_SIZE=128, PRODUCT_EMBEDDING_LR=1e-2)
        if flag:
            c.TRAIN_PRODUCT_EMBEDDINGS = True
        tr, va = loaders()
        torch.manual_seed(0)
        # (a device table is taken by PCompanion without a copy: training must leave the caller's tensor pretrained)
        given = table.cuda() if source == "device" else table
        model = drv.train(c, tr, va, given)
        assert torch.equal(bits(given), bits(table))
        assert model.step_losses.numel() == 2 * len(tr) and torch.isfinite(model.step_losses).all()
        assert not model.product_embeddings.weight.requires_grad
        ckpt = torch.load(os.path.join(c.MODEL_DIR, "best_model.pth"), weights_only=False)
        runs[flag] = (c, model, ckpt)
    c, model, ckpt = runs[False]
    assert set(ckpt) == {"epoch", "model_state_dict", "optimizer_state_dict", "metrics"}
    assert torch.equal(bits(model.product_embeddings.weight), bits(table))
    assert torch.equal(bits(ckpt["model_state_dict"]["product_embeddings.weight"]), bits(table))
    c, model, ckpt = runs[True]
    assert set(ckpt) == {"epoch", "model_state_dict", "optimizer_state_dict", "metrics", "table_optimizer_state_dict"}
    ts = ckpt["table_optimizer_state_dict"]
    assert set(ts) == {"state", "param_groups"} and set(ts["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    assert ts["state"][0]["step"] == (ckpt["epoch"] + 1) * len(loaders()[0]) and ts["param_groups"][0]["lr"] == 1e-2
    assert tuple(ts["state"][0]["exp_avg"].shape) == (P_S, D) and not ts["state"][0]["exp_avg"].is_cuda
    saved = ckpt["model_state_dict"]["product_embeddings.weight"]
    assert not torch.equal(saved, table) and torch.isfinite(saved).all()
    assert abs(float(runs[False][1].step_losses[0]) - float(model.step_losses[0])) <= 1e-6       # (step 1 reads the pretrained table either way)
    assert not torch.equal(runs[False][1].step_losses, model.step_losses)
    # a fresh model from the checkpoint is evaluated as the trained one was at that epoch: the evaluation read the updated table
    fresh = PCompanion(c, table).to("cuda")
    fresh.load_state_dict(ckpt["model_state_dict"])
    va = loaders()[1]
    va.epoch, va.step = ckpt["epoch"], ckpt["epoch"] * len(va)
    again = Metrics.evaluate_model(fresh, va, c.DEVICE)
    assert again == model.epoch_metrics[ckpt["epoch"]] == ckpt["metrics"]
    stale = PCompanion(c, table).to("cuda")
    stale.load_state_dict(dict(ckpt["model_state_dict"], **{"product_embeddings.weight": table}))
    va.epoch, va.step = ckpt["epoch"], ckpt["epoch"] * len(va)
    assert Metrics.evaluate_model(stale, va, c.DEVICE) != again


def test_train_refuses_a_sharded_catalogue_with_the_flag(tmp_path):
    from p_companion_amd import train as drv
    from p_companion_amd.data import generate_device_bpg
    bpg = generate_device_bpg(P_S, T_S, seed=1, rank=0, world=2)
    ld = SimpleNamespace(dataset=SimpleNamespace(bpg=bpg))
    with pytest.raises(ValueError, match="world"):
        drv.train(cfg(tmp_path, TRAIN_PRODUCT_EMBEDDINGS=True), ld, ld, torch.zeros(P_S, 128))
