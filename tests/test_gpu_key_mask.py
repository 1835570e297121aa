"""The key-padding mask of Product2Vec's attention and neighbour BatchNorm (a labelled deviation, off by default; DESIGN
section 5): whole steps, the dense attention op and the module surface against a MASKED oracle composed from
oracle.p2v_oracle in FLOAT64.  Needs an MI355X (the oracle-only discrimination check at the top runs on the CPU:
`-m gpu -k test_oracle`).

The masked oracle: `ffn` over the real neighbour rows only (one BatchNorm call of n_real rows, none when the batch is
padding alone), `attention` per sample over that sample's real keys (with the philox_oracle multipliers of those slots,
element (b, h, n) of the [B,HEADS,N] tensor, when dropout is on), a sample without a real key takes the out_proj.bias row;
then triplet_loss and autograd.grad.

Bounds are the step tests' own (tests/test_gpu_p2v_step.py, restated in tests/test_gpu_neighbour_rows.py): loss 2e-6,
anchor_emb 2e-5, running statistics 1e-6, every gradient tensor 2e-6 + 2e-4 max|ref| of ITS fp64 gradient.  ffn.0.bias is
skipped: its gradient is analytically zero.  Each check prints `mask-ratio ...` lines (error / bound)
before it asserts.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import p2v_oracle, philox_oracle

P, K_NEG, MARGIN = 251, 5, 1.0
GRAD_KEYS = tuple(k for k in p2v_oracle.TRAINABLE if k != "ffn.0.bias")
DROPOUT = (0.25, 2 ** 40 + 77, 6)                      # (p, seed, offset)
HUB = (140, 4, (130, 65, 64, 63, 33, 17, 16, 1, 2, 1))  # tests/test_gpu_neighbour_rows.py's `hub` multiplicities


@pytest.fixture(scope="module")
def ops():
    from p_companion_amd import ops as o
    assert torch.cuda.is_available()
    return o


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _state(seed, d=128):
    """init_state with the BatchNorm affine and the attention biases off their (1, 0, 0) initial values."""
    st = p2v_oracle.init_state(seed, d=d)
    st["ffn.1.weight"] = 1.0 + 0.1 * rnd(256, seed=seed + 1)
    st["ffn.1.bias"] = 0.1 * rnd(256, seed=seed + 2)
    st["attention.in_proj_bias"] = 0.05 * rnd(3 * d, seed=seed + 3)
    st["attention.out_proj.bias"] = 0.05 * rnd(d, seed=seed + 4)
    return st


# ------------------------------------------------------------------ neighbour matrices (padding at shuffled positions)
def _random_degrees(b, n, seed, lo, hi):
    rng = np.random.RandomState(seed)
    nb = np.argsort(rng.rand(b, P), axis=1)[:, :n].astype(np.int32)
    deg = rng.randint(lo, hi + 1, size=b)
    nb[np.arange(n)[None, :] >= deg[:, None]] = -1
    for r in range(b):
        nb[r] = nb[r, rng.permutation(n)]
    return nb


def _from_multiplicities(b, n, mult, seed):
    rng = np.random.RandomState(seed)
    ids = np.sort(rng.choice(P, len(mult), replace=False))
    nb = np.full((b, n), -1, np.int32)
    fill = np.zeros(b, np.int64)
    for pid, m in zip(ids, mult):
        who = np.argsort(fill, kind="stable")[:m]
        assert len(who) == m and fill[who].max() < n
        nb[who, fill[who]] = pid
        fill[who] += 1
    for r in range(b):
        nb[r] = nb[r, rng.permutation(n)]
    return nb


def _neighbours(name):
    if name == "deg04":                                            # degrees 0 .. 4: keyless samples among them
        nb = _random_degrees(24, 4, 5, 0, 4)
        deg = (nb >= 0).sum(1)
        assert deg.min() == 0 and deg.max() == 4 and 0 < (nb < 0).sum() < nb.size
        return nb
    if name == "wide9":                                            # the same batch with five more -1 columns, slots reshuffled
        nb = np.concatenate([_neighbours("deg04"), np.full((24, 5), -1, np.int32)], axis=1)
        rng = np.random.RandomState(9)
        for r in range(nb.shape[0]):
            nb[r] = nb[r, rng.permutation(9)]
        return nb
    if name == "n70":                                              # N > 64 (slot map read from memory), N mod 4 = 2
        return _random_degrees(12, 70, 6, 0, 70)
    if name == "no_padding":
        return _random_degrees(24, 4, 7, 4, 4)
    if name == "all_padding":
        return np.full((24, 4), -1, np.int32)
    if name == "one_real":
        nb = np.full((24, 4), -1, np.int32)
        nb[7, 2] = 100
        return nb
    if name == "hub":
        return _from_multiplicities(*HUB, seed=3)
    raise KeyError(name)


def _case(name, d=128):
    return _case_cached(name, int(d))


@functools.lru_cache(maxsize=None)
def _case_cached(name, d):
    """Inputs of one case (shared, never modified).  wide9 shares deg04's triplet: the two widths are one batch."""
    nb = _neighbours(name)
    b = nb.shape[0]
    g = torch.Generator().manual_seed(17)
    batch = {"anchor_idx": torch.randint(0, P, (b,), generator=g, dtype=torch.int32),
             "positive_idx": torch.randint(0, P, (b,), generator=g, dtype=torch.int32),
             "negative_idx": torch.randint(0, P, (b, K_NEG), generator=g, dtype=torch.int32),
             "neighbor_idx": torch.from_numpy(nb)}
    return {"st": _state(11, d), "table": rnd(P, d, seed=1), "batch": batch, "nb": nb}


# ------------------------------------------------------------------ the fp64 oracles
def _drop_mult(b, n):
    p, seed, offset = DROPOUT
    m = philox_oracle.dropout_mask(seed, offset, philox_oracle.STREAM_ATTENTION, b * 4 * n, p)
    return torch.from_numpy(m).view(b, 4, n)


def _masked_attention(a, key_rows, nb, work, mult):
    """Per sample over its real keys; key_rows: the FFN rows of the real slots in slot order (None: no real slot)."""
    b, n = nb.shape
    real = nb >= 0
    first = np.concatenate([[0], np.cumsum(real.sum(1))])
    out = []
    for i in range(b):
        if first[i + 1] == first[i]:
            out.append(work["attention.out_proj.bias"].to(a.dtype))                 # no key: the bias row
            continue
        keys = key_rows[first[i]:first[i + 1]].unsqueeze(0)
        m = None if mult is None else mult[i][:, torch.from_numpy(real[i])].unsqueeze(0).to(a.dtype)
        out.append(p2v_oracle.attention(a[i:i + 1], keys, work, mask=m)[0])
    return torch.stack(out)


def _work(c, dtype):
    st = {k: (v.to(dtype, copy=True) if v.is_floating_point() else v.clone()) for k, v in c["st"].items()}
    leaves = {k: st[k].clone().requires_grad_(True) for k in p2v_oracle.TRAINABLE}
    work = dict(st)
    work.update(leaves)
    return st, leaves, work


def _oracle(name, d=128, dropout=False, masked=True):
    return _oracle_cached(name, int(d), bool(dropout), bool(masked))


@functools.lru_cache(maxsize=None)
def _oracle_cached(name, d, dropout, masked):
    """One step in float64.  masked=False: the reference's semantics (padding rows are keys and BatchNorm rows)."""
    dtype = torch.float64
    c = _case(name, d)
    st, leaves, work = _work(c, dtype)
    tab = torch.cat([c["table"].to(dtype), torch.zeros(1, d, dtype=dtype)])        # index -1: the zero row
    rows = lambda t: tab[t.long()]
    bt, nb = c["batch"], c["nb"]
    b, n = nb.shape
    mult = _drop_mult(b, n) if dropout else None
    a = p2v_oracle.ffn(rows(bt["anchor_idx"]), work, True)
    if masked:
        real = torch.from_numpy(nb.reshape(-1)[nb.reshape(-1) >= 0])
        key_rows = p2v_oracle.ffn(rows(real), work, True) if real.numel() else None
        emb = _masked_attention(a, key_rows, nb, work, mult)
    else:
        keys = p2v_oracle.ffn(rows(bt["neighbor_idx"]).reshape(-1, d), work, True).reshape(b, n, d)
        emb = p2v_oracle.attention(a, keys, work, mask=None if mult is None else mult.to(dtype))
    pos = p2v_oracle.forward(rows(bt["positive_idx"]), None, work, True)
    neg = p2v_oracle.forward(rows(bt["negative_idx"]), None, work, True)
    loss, _, _ = p2v_oracle.triplet_loss(emb, pos, neg, MARGIN)
    # (a batch of padding alone reaches in_proj and out_proj.weight through no path: their gradient is zero)
    grads = torch.autograd.grad(loss, [leaves[k] for k in p2v_oracle.TRAINABLE], allow_unused=True)
    grads = [torch.zeros_like(leaves[k]) if g is None else g for k, g in zip(p2v_oracle.TRAINABLE, grads)]
    return {"loss": float(loss.detach()), "anchor_emb": emb.detach(), "running_mean": st["ffn.1.running_mean"],
            "running_var": st["ffn.1.running_var"], "nbt": int(st["ffn.1.num_batches_tracked"]),
            "grads": dict(zip(p2v_oracle.TRAINABLE, grads))}


def _grad_bound(ref):
    return 2e-6 + 2e-4 * float(ref.abs().max())


def _ratios(got, ref):
    r = {"loss": abs(got["loss"] - ref["loss"]) / 2e-6,
         "emb": float((got["anchor_emb"].double() - ref["anchor_emb"]).abs().max()) / 2e-5 if "anchor_emb" in got else float("nan"),
         "stats": max(float((got[k].double() - ref[k]).abs().max()) for k in ("running_mean", "running_var")) / 1e-6}
    for k in GRAD_KEYS:
        r[k] = float((got["grads"][k].double() - ref["grads"][k]).abs().max()) / _grad_bound(ref["grads"][k])
    return r


def _report(what, r):
    worst = max(GRAD_KEYS, key=lambda k: r[k])
    print(f"mask-ratio {what}: loss {r['loss']:.3f} emb {r['emb']:.3f} stats {r['stats']:.3f} "
          f"grad {r[worst]:.3f} ({worst})")


def _within(what, got, ref, keys=None):
    r = _ratios(got, ref)
    _report(what, r)
    bad = {k: round(v, 3) for k, v in r.items() if (keys is None or k in keys) and not v <= 1.0}
    assert not bad, f"{what}: error / bound above 1: {bad}"
    return r


# ------------------------------------------------------------------ a. the test can tell the modes apart (CPU)
@pytest.mark.parametrize("name,d,dropout", [("deg04", 128, False), ("n70", 128, False), ("hub", 128, False),
                                            ("deg04", 256, False), ("deg04", 128, True), ("wide9", 128, False)])
def test_oracle_unmasked_misses_the_masked_one(name, d, dropout):
    """Every case with padding: the unmasked fp64 oracle is off the masked one by more than 50 x the bound on the loss and
    on at least one gradient tensor (no device involved)."""
    r = _ratios(_oracle(name, d, dropout, masked=False), _oracle(name, d, dropout))
    _report(f"oracle unmasked-vs-masked {name} d{d}{' dropout' if dropout else ''}", r)
    assert r["loss"] > 50.0, r["loss"]
    assert max(r[k] for k in GRAD_KEYS) > 50.0


def test_oracle_modes_agree_without_padding():
    r = _ratios(_oracle("no_padding", masked=False), _oracle("no_padding"))
    assert max(r.values()) < 1e-6, r


def test_oracle_both_widths_are_one_batch():
    """N = 4 and its widening to N = 9 have the same masked oracle (the loss to fp64 rounding: the slots are reshuffled)."""
    r = _ratios(_oracle("wide9"), _oracle("deg04"))
    assert max(r.values()) < 1e-6, r


# ------------------------------------------------------------------ b. device steps
def _dev_batch(c):
    return c["table"].cuda(), {k: v.cuda() for k, v in c["batch"].items()}


def _layout(ops, nb_dev, which):
    return nb_dev if which == "dense" else ops.compact_neighbors(nb_dev) if which == "compact" else ops.unique_neighbors(nb_dev)


def _step(ops, c, table, batch, layout, dropout=False, masked=True, nbt=4):
    params = {k: v.clone().cuda() for k, v in c["st"].items()}
    grads = {k: torch.full_like(params[k], 7.0) for k in ops.P2V_KEYS}            # overwritten, not accumulated into
    if dropout:
        params[ops.DROPOUT_KEY] = DROPOUT
    out = ops.p2v_train_step(params, grads, table, batch["anchor_idx"], batch["positive_idx"], batch["negative_idx"], layout,
                             MARGIN, want_emb=True, masked=masked)
    assert int(params["ffn.1.num_batches_tracked"]) == nbt
    res = {"loss": float(out["loss"]), "anchor_emb": out["anchor_emb"].cpu(), "running_mean": params["ffn.1.running_mean"].cpu(),
           "running_var": params["ffn.1.running_var"].cpu(), "grads": {k: grads[k].cpu() for k in ops.P2V_KEYS}}
    assert all(bool(torch.isfinite(v).all()) for v in list(res["grads"].values()) + [res["anchor_emb"]])
    return res


STEP_CASES = [("deg04", 128, False, ("dense", "compact", "unique")),      # every entry point through ops; keyless samples
              ("n70", 128, False, ("compact", "unique")),
              ("no_padding", 128, False, ("compact", "unique")),
              ("hub", 128, False, ("unique",)),                           # a row with more than 64 slots
              ("deg04", 256, False, ("compact", "unique")),
              ("deg04", 128, True, ("compact", "unique")),
              ("wide9", 128, False, ("compact", "unique"))]


@pytest.mark.parametrize("name,d,dropout,layouts", STEP_CASES,
                         ids=[f"{n}-d{d}{'-dropout' if dr else ''}" for n, d, dr, _ in STEP_CASES])
def test_masked_step_against_the_masked_oracle(ops, name, d, dropout, layouts):
    c = _case(name, d)
    # (dropout: the multipliers are indexed by the slot, so the widths draw differently; every case has its own oracle)
    ref = _oracle(name, d, dropout)
    table, batch = _dev_batch(c)
    for which in layouts:
        layout = _layout(ops, batch["neighbor_idx"], which)
        got = _step(ops, c, table, batch, layout, dropout)
        _within(f"masked {name} d{d}{' dropout' if dropout else ''} {which}", got, ref)
        if which == "unique":                          # the caller's multiplicities are read, never written: one batch, both modes
            assert float(layout["weight"][-1]) == float((c["nb"] < 0).sum())
    if name == "no_padding":                           # ... and the masked step meets the unmasked oracle
        _within("masked no_padding vs the unmasked oracle", got, _oracle(name, d, dropout, masked=False))
    if name == "wide9":                                # both widths meet the same oracle
        _within("masked wide9 vs the N = 4 oracle", got, _oracle("deg04", d))


@pytest.mark.parametrize("name,d,dropout,which", [("deg04", 128, False, "dense"), ("deg04", 128, False, "compact"),
                                                  ("deg04", 128, False, "unique"), ("n70", 128, False, "unique"),
                                                  ("deg04", 128, True, "unique"), ("hub", 128, False, "unique")])
def test_flag_off_is_the_unmasked_step(ops, name, d, dropout, which):
    """The same calls on the same batch objects without the flag still meet the UNMASKED oracle (and miss the masked one)."""
    c = _case(name, d)
    table, batch = _dev_batch(c)
    layout = _layout(ops, batch["neighbor_idx"], which)
    masked = _step(ops, c, table, batch, layout, dropout, masked=True)
    _within(f"masked-first {name} {which}", masked, _oracle(name, d, dropout))
    got = _step(ops, c, table, batch, layout, dropout, masked=False)
    _within(f"flag off {name} {which}", got, _oracle(name, d, dropout, masked=False))
    assert _ratios(got, _oracle(name, d, dropout))["loss"] > 50.0


def test_batch_of_padding_alone(ops):
    """Finite everywhere; the neighbour call did not happen (three BatchNorm calls: running statistics and
    num_batches_tracked as the oracle's without it); the attention gradients are those of the bias-only output."""
    c = _case("all_padding")
    ref = _oracle("all_padding")
    assert ref["nbt"] == 3
    table, batch = _dev_batch(c)
    for which in ("dense", "compact", "unique"):
        got = _step(ops, c, table, batch, _layout(ops, batch["neighbor_idx"], which), nbt=3)
        _within(f"masked all_padding {which}", got, ref)
        assert float(got["grads"]["attention.in_proj_weight"].abs().max()) == 0.0
        assert float(got["grads"]["attention.in_proj_bias"].abs().max()) == 0.0
        assert float(got["grads"]["attention.out_proj.weight"].abs().max()) == 0.0
        assert float(ref["grads"]["attention.out_proj.bias"].abs().max()) > 1e-3
        bias = c["st"]["attention.out_proj.bias"]
        assert torch.equal(got["anchor_emb"], bias.expand_as(got["anchor_emb"]))


def test_one_real_slot_is_a_batchnorm_error(ops):
    c = _case("one_real")
    table, batch = _dev_batch(c)
    for which in ("dense", "compact", "unique"):
        params = {k: v.clone().cuda() for k, v in c["st"].items()}
        grads = {k: torch.zeros_like(params[k]) for k in ops.P2V_KEYS}
        with pytest.raises(ValueError, match="Expected more than 1 value per channel"):
            ops.p2v_train_step(params, grads, table, batch["anchor_idx"], batch["positive_idx"], batch["negative_idx"],
                               _layout(ops, batch["neighbor_idx"], which), MARGIN, masked=True)
        assert int(params["ffn.1.num_batches_tracked"]) == 0


def _adam_close(actual, desired, steps, lr=1e-3, tight=5e-5):
    """tests/test_gpu_p2v_step.py's criterion for parameters behind Adam steps: an update is lr g / (|g| + eps) per step, at
    most lr, and takes the sign of g -- which fp32 cannot pin where |g| is rounding noise.  So: every element within
    1.05 lr steps, and 99.9 % of them within `tight`."""
    d = (actual.double() - desired.double()).abs()
    assert float(d.max()) <= 1.05 * lr * steps
    assert float((d <= tight).double().mean()) >= 0.999


def test_loader_rows_and_riding_adam(ops):
    """The unique layout with loader-made step_rows and the optimizer riding in the step's last launch
    (pc_p2v_train_step_unique_masked): gradients against the masked oracle, parameters after the update against
    p2v_oracle.adam_step over the oracle's gradients."""
    c = _case("deg04")
    ref = _oracle("deg04")
    table, batch = _dev_batch(c)
    uq = ops.unique_neighbors(batch["neighbor_idx"])
    n_dev = torch.tensor([uq["n_unique"]], dtype=torch.int32, device="cuda")
    uq = dict(uq, step_rows=ops.concat_step_rows(batch["anchor_idx"], batch["positive_idx"], batch["negative_idx"],
                                                 uq["nb_rows"], n_dev))
    keys = ops.P2V_KEYS
    shapes = [tuple(c["st"][k].shape) for k in keys]
    sizes = [int(np.prod(s)) for s in shapes]
    offs = np.concatenate([[0], np.cumsum(sizes)])
    flat = torch.cat([c["st"][k].reshape(-1) for k in keys]).cuda()
    gflat, m, v = torch.zeros_like(flat), torch.zeros_like(flat), torch.zeros_like(flat)
    params = {k: flat[offs[i]:offs[i + 1]].view(s) for i, (k, s) in enumerate(zip(keys, shapes))}
    grads = {k: gflat[offs[i]:offs[i + 1]].view(s) for i, (k, s) in enumerate(zip(keys, shapes))}
    for k in ("ffn.1.running_mean", "ffn.1.running_var", "ffn.1.num_batches_tracked"):
        params[k] = c["st"][k].clone().cuda()
    step_count = torch.zeros(1, dtype=torch.int64, device="cuda")
    adam = {"param": flat, "grad": gflat, "exp_avg": m, "exp_avg_sq": v, "step_count": step_count, "t": 1, "lr": 1e-3,
            "betas": (0.9, 0.999), "eps": 1e-8}
    out = ops.p2v_train_step(params, grads, table, batch["anchor_idx"], batch["positive_idx"], batch["negative_idx"], uq, MARGIN,
                             want_emb=True, adam=adam, masked=True)
    got = {"loss": float(out["loss"]), "anchor_emb": out["anchor_emb"].cpu(), "running_mean": params["ffn.1.running_mean"].cpu(),
           "running_var": params["ffn.1.running_var"].cpu(), "grads": {k: grads[k].cpu() for k in keys}}
    _within("masked deg04 unique + step_rows + adam", got, ref)
    assert int(step_count) == 1
    want = {k: c["st"][k].double().clone() for k in p2v_oracle.TRAINABLE}
    p2v_oracle.adam_step(want, ref["grads"], {k: (torch.zeros_like(x), torch.zeros_like(x)) for k, x in want.items()}, 1)
    for k in GRAD_KEYS:
        _adam_close(params[k].cpu(), want[k], 1)


# ------------------------------------------------------------------ c. the dense attention op
def test_dense_attention_op_with_key_pad(ops):
    """ops.attention_forward / attention_backward(key_pad=...), N on both sides of 64, D = 128 and 256, padding rows filled
    with inf / NaN (a padding row is never multiplied in): out, dquery, dkeys and the attention gradients against the masked
    oracle at tests/test_gpu_ops.py::test_attention's tolerances; dkeys of padding slots exactly zero."""
    tol = lambda what, ref: {"out": 3e-6, "dquery": 1e-5, "dkeys": 1e-5}.get(what) or 3e-5 * max(1.0, float(ref.abs().max()))
    names = [k for k in p2v_oracle.TRAINABLE if k.startswith("attention")]
    for b, n, d in ((7, 6, 128), (5, 70, 128), (6, 9, 256)):
        st = _state(11, d)
        rng = np.random.RandomState(n)
        pad = rng.rand(b, n) < 0.4
        pad[1] = True                                              # a sample without a key
        pad[2] = False
        q, kv, dout = rnd(b, d, seed=50), rnd(b, n, d, seed=51), rnd(b, d, seed=52)
        leaves = {k: st[k].double().requires_grad_(True) for k in names}
        qi, ki = q.double().requires_grad_(True), kv.double().requires_grad_(True)
        nb = np.where(pad, -1, 1).astype(np.int32)
        key_rows = ki.reshape(-1, d)[torch.from_numpy(~pad.reshape(-1))]
        out = _masked_attention(qi, key_rows, nb, leaves, None)
        (out * dout.double()).sum().backward()
        ref = {"out": out.detach(), "dquery": qi.grad, "dkeys": ki.grad}
        ref.update({k: leaves[k].grad for k in names})
        dst = {k: v.clone().cuda() for k, v in st.items()}
        poisoned = kv.clone()
        poisoned[torch.from_numpy(pad)] = float("nan")
        poisoned[0][torch.from_numpy(pad[0])] = float("inf")
        kp = torch.from_numpy(pad).cuda()
        o, sv = ops.attention_forward(dst, q.cuda(), poisoned.cuda(), key_pad=kp)
        grads, dq, dk = ops.attention_backward(dst, q.cuda(), poisoned.cuda(), dout.cuda(), sv)
        got = {"out": o.cpu(), "dquery": dq.cpu(), "dkeys": dk.cpu()}
        got.update({k: grads[k].cpu() for k in names})
        assert float(got["dkeys"][torch.from_numpy(pad)].abs().max()) == 0.0
        assert float(sv["probs"].cpu().permute(0, 2, 1)[torch.from_numpy(pad)].abs().max()) == 0.0   # saved probability exactly 0
        assert torch.equal(got["out"][1], st["attention.out_proj.bias"])
        for k, r in ref.items():
            err, t = float((got[k].double() - r).abs().max()), tol(k, r)
            print(f"mask-ratio attention op B={b} N={n} D={d} {k}: {err / t:.3f}")
            assert err <= t, f"{k}: {err:.3e} > {t:.1e}"


# ------------------------------------------------------------------ d. the module surface
def _cfg(d=128, mask=None):
    c = SimpleNamespace(PRODUCT_EMB_DIM=d, TYPE_EMB_DIM=64, HIDDEN_SIZE=256, NUM_ATTENTION_HEADS=4, DROPOUT=0.0, MARGIN=MARGIN,
                        DEVICE=torch.device("cuda:0"), LEARNING_RATE=1e-3)
    if mask is not None:
        c.ATTENTION_KEY_MASK = mask
    return c


def _model(c, cfg):
    from p_companion_amd.product2vec import Product2Vec
    m = Product2Vec(cfg).cuda()
    m.load_state_dict({k: v.clone() for k, v in c["st"].items()})
    return m.train()


def _dense_batch(c):
    """The reference loader's dense batch (collate_fn: zero rows at the padding slots) plus the explicit mask key."""
    tab = torch.cat([c["table"], torch.zeros(1, c["table"].shape[1])])
    bt = c["batch"]
    return {"anchor": tab[bt["anchor_idx"].long()].cuda(), "positive": tab[bt["positive_idx"].long()].cuda(),
            "negative": tab[bt["negative_idx"].long()].cuda(), "anchor_neighbors": tab[bt["neighbor_idx"].long()].cuda(),
            "anchor_neighbors_mask": torch.from_numpy(c["nb"] < 0).cuda()}


def _module_result(m, loss):
    sd = m.state_dict()
    return {"loss": float(loss.detach()), "running_mean": sd["ffn.1.running_mean"].cpu(), "running_var": sd["ffn.1.running_var"].cpu(),
            "grads": {k: p.grad.detach().cpu() for k, p in m.named_parameters()}}


def _forward_oracle(c, training):
    """anchor embedding and the gradients of sum(emb * dout) under the masked semantics (two BatchNorm calls in training)."""
    st, leaves, work = _work(c, torch.float64)
    d = c["table"].shape[1]
    tab = torch.cat([c["table"].double(), torch.zeros(1, d, dtype=torch.float64)])
    bt, nb = c["batch"], c["nb"]
    a = p2v_oracle.ffn(tab[bt["anchor_idx"].long()], work, training)
    real = torch.from_numpy(nb.reshape(-1)[nb.reshape(-1) >= 0])
    emb = _masked_attention(a, p2v_oracle.ffn(tab[real.long()], work, training), nb, work, None)
    dout = rnd(*emb.shape, seed=77).double()
    grads = torch.autograd.grad((emb * dout).sum(), [leaves[k] for k in p2v_oracle.TRAINABLE], allow_unused=True)
    return emb.detach(), dout, dict(zip(p2v_oracle.TRAINABLE, grads)), st


def test_module_forward_with_key_padding_mask():
    """Product2Vec.forward(features, neighbors, key_padding_mask): train mode with autograd through _FFNFunction and
    _AttentionFunction (the neighbour call's BatchNorm over the unmasked rows: its running statistics too), and eval mode."""
    c = _case("deg04")
    db = _dense_batch(c)
    m = _model(c, _cfg())
    emb_ref, dout, gref, st_ref = _forward_oracle(c, True)
    emb = m(db["anchor"], db["anchor_neighbors"], key_padding_mask=db["anchor_neighbors_mask"])
    (emb * dout.float().cuda()).sum().backward()
    e = float((emb.detach().cpu().double() - emb_ref).abs().max()) / 2e-5
    s = max(float((m.state_dict()[k].cpu().double() - st_ref[k]).abs().max()) for k in ("ffn.1.running_mean", "ffn.1.running_var")) / 1e-6
    print(f"mask-ratio module forward train: emb {e:.3f} stats {s:.3f}")
    assert e <= 1.0 and s <= 1.0 and int(m.state_dict()["ffn.1.num_batches_tracked"]) == 2
    for k, p in m.named_parameters():
        if k == "ffn.0.bias":
            continue
        r = float((p.grad.cpu().double() - gref[k]).abs().max()) / _grad_bound(gref[k])
        print(f"mask-ratio module forward train grad {k}: {r:.3f}")
        assert r <= 1.0, (k, r)
    m = _model(c, _cfg()).eval()                                   # (a fresh module: the running statistics of the case)
    emb_ref, _, _, _ = _forward_oracle(c, False)
    with torch.no_grad():
        emb = m(db["anchor"], db["anchor_neighbors"], key_padding_mask=db["anchor_neighbors_mask"])
    e = float((emb.cpu().double() - emb_ref).abs().max()) / 2e-5
    print(f"mask-ratio module forward eval: emb {e:.3f}")
    assert e <= 1.0


@pytest.mark.parametrize("explicit", [True, False], ids=["explicit-mask", "zero-rows"])
def test_dense_loss_with_the_flag(explicit):
    """dense_loss under config.ATTENTION_KEY_MASK: the mask from the batch key, or from the all-zero neighbour rows when the
    key is absent; with the flag off the same batch object still meets the unmasked oracle (the key is ignored)."""
    c = _case("deg04")
    db = _dense_batch(c)
    if not explicit:
        del db["anchor_neighbors_mask"]
    cfg = _cfg(mask=True)
    m = _model(c, cfg)
    loss = m.dense_loss(db)
    loss.backward()
    _within(f"dense_loss masked ({'key' if explicit else 'zero rows'})", _module_result(m, loss), _oracle("deg04"),
            keys=("loss", "stats") + GRAD_KEYS)
    cfg.ATTENTION_KEY_MASK = False                                # read at call time
    m2 = _model(c, cfg)
    loss = m2.dense_loss(db)
    loss.backward()
    _within("dense_loss flag off", _module_result(m2, loss), _oracle("deg04", masked=False), keys=("loss", "stats") + GRAD_KEYS)
    m3 = _model(c, _cfg())                                         # attribute missing: False
    loss = m3.dense_loss(db)
    loss.backward()
    _within("dense_loss no attribute", _module_result(m3, loss), _oracle("deg04", masked=False), keys=("loss", "stats") + GRAD_KEYS)


def test_train_step_indexed_honours_the_flag():
    c = _case("deg04")
    table, batch = _dev_batch(c)
    from p_companion_amd import ops
    batch["neighbor_compact"] = ops.unique_neighbors(batch["neighbor_idx"])
    for flag in (True, False):
        m = _model(c, _cfg(mask=flag))
        loss = m.train_step_indexed(table, batch)
        _within(f"train_step_indexed flag {flag}", _module_result(m, loss), _oracle("deg04", masked=flag),
                keys=("loss", "stats") + GRAD_KEYS)
    m = _model(c, _cfg(mask=True))
    with pytest.raises(ValueError, match="sync_reduce"):
        m.train_step_indexed(table, batch, sync_reduce=lambda t: t)


def _small_bpg():
    """251 products, co-view degrees 0 .. 4, 48 similarity pairs (two batches of 24) whose anchors have a co-view edge."""
    from p_companion_amd.data import IntBPG
    rng = np.random.RandomState(21)
    deg = rng.randint(0, 5, size=P)
    deg[:60] = rng.randint(1, 5, size=60)
    rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    col = np.concatenate([rng.choice(P, k, replace=False) for k in deg]).astype(np.int32)
    anchors = rng.choice(60, 48, replace=False)
    pairs = np.stack([anchors, (anchors + 1 + rng.randint(0, P - 1, size=48)) % P], axis=1).astype(np.int32)
    return IntBPG(features=rnd(P, 128, seed=1).numpy(), type_idx=np.zeros(P, np.int32), category=np.zeros(P, np.int32),
                  cv_rowptr=rowptr, cv_col=col, similarity_pairs=pairs, complementary_pairs=np.zeros((0, 2), np.int32), n_types=1)


def test_two_step_train_model_with_the_flag():
    """train_model over the device loader (unique layout, loader-made rows, riding FusedAdam) with the flag on: two steps against
    the masked oracle stepping with p2v_oracle.adam_step over the very batches the loader builds (a second loader with the
    same seed hands them out).  Step 1's loss at the step bound; step 2's, behind one fp32 Adam update, at the 1e-4 the
    project asks of multi-step losses (tests/test_gpu_p2v_step.py); the parameters by _adam_close over two steps."""
    from p_companion_amd.data import SimilarityIndexLoader
    from p_companion_amd.product2vec import FusedAdam
    bpg = _small_bpg()
    st0 = _state(11)
    seen = []
    for b in SimilarityIndexLoader(bpg, 24, shuffle=False, seed=3, prefetch=False):
        nbc = b["neighbor_compact"]
        nb = nbc["nb_rows"][nbc["slot_row"].long()].cpu().numpy()
        seen.append({"anchor_idx": b["anchor_idx"].cpu(), "positive_idx": b["positive_idx"].cpu(),
                     "negative_idx": b["negative_idx"].cpu(), "nb": nb})
    assert len(seen) == 2 and all((s["nb"] < 0).any() for s in seen)
    # the oracle's two steps
    st = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in st0.items()}
    moments = {k: (torch.zeros_like(st[k]), torch.zeros_like(st[k])) for k in p2v_oracle.TRAINABLE}
    tab = torch.cat([torch.from_numpy(bpg.features).double(), torch.zeros(1, 128, dtype=torch.float64)])
    losses = []
    for t, s in enumerate(seen, 1):
        leaves = {k: st[k].clone().requires_grad_(True) for k in p2v_oracle.TRAINABLE}
        work = dict(st)
        work.update(leaves)
        a = p2v_oracle.ffn(tab[s["anchor_idx"].long()], work, True)
        real = torch.from_numpy(s["nb"].reshape(-1)[s["nb"].reshape(-1) >= 0])
        emb = _masked_attention(a, p2v_oracle.ffn(tab[real.long()], work, True), s["nb"], work, None)
        pos = p2v_oracle.forward(tab[s["positive_idx"].long()], None, work, True)
        neg = p2v_oracle.forward(tab[s["negative_idx"].long()], None, work, True)
        loss, _, _ = p2v_oracle.triplet_loss(emb, pos, neg, MARGIN)
        grads = dict(zip(p2v_oracle.TRAINABLE, torch.autograd.grad(loss, [leaves[k] for k in p2v_oracle.TRAINABLE])))
        with torch.no_grad():
            p2v_oracle.adam_step({k: st[k] for k in p2v_oracle.TRAINABLE}, grads, moments, t)
        losses.append(float(loss))
    cfg = _cfg(mask=True)
    m = _model({"st": st0}, cfg)
    m.record_step_losses = True
    emb = m.train_model(SimilarityIndexLoader(bpg, 24, shuffle=False, seed=3, prefetch=False), FusedAdam(m), num_epochs=1)
    assert len(emb) == P
    got = [float(x) for x in m.step_losses]
    print(f"mask-ratio train_model losses: step 1 {abs(got[0] - losses[0]) / 2e-6:.3f} (x 2e-6), "
          f"step 2 {abs(got[1] - losses[1]) / 1e-4:.3f} (x 1e-4)")
    assert abs(got[0] - losses[0]) <= 2e-6 and abs(got[1] - losses[1]) <= 1e-4
    sd = m.state_dict()
    assert int(sd["ffn.1.num_batches_tracked"]) == 8
    for k in GRAD_KEYS:
        _adam_close(sd[k].cpu(), st[k], 2)
