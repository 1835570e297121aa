"""The key rows' gradient of the unique-neighbour step (attn_dkv_rows_kernel, csrc/attention.hip) at every slot-list
length, the two slot-map forms of the attention core, the padding column sums off the 64-row grid and the LDS bound on
N -- whole steps on hand-built [B,N] neighbour matrices against the oracle evaluated in FLOAT64.  Needs an MI355X (the
oracle-only preconditions at the top run on the CPU: `-m gpu -k test_oracle`).

A case is written as the multiplicities of its neighbour products in ascending id order: the row index of the unique
layout is the rank of the product id, so the tuple fixes the groups of four rows a wave takes and with them the path
(<= 16 slots: 16-lane sort; 17..64 in any row of the group: whole-wave sort; > 64: fp64 in arrival order).

Bounds are the step tests' own (tests/test_gpu_p2v_step.py): loss 2e-6, anchor_emb 2e-5, running statistics 1e-6, every
gradient tensor 2e-6 + 2e-4 max|ref| of ITS fp64 gradient.  ffn.0.bias is skipped: its gradient is analytically zero
(DESIGN section 4).  Each check prints `rows-ratio ...` lines (error / bound) before it asserts.
"""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import p2v_oracle, philox_oracle

P, K_NEG, MARGIN = 251, 5, 1.0
GRAD_KEYS = tuple(k for k in p2v_oracle.TRAINABLE if k != "ffn.0.bias")
FFN_KEYS = tuple(k for k in GRAD_KEYS if k.startswith("ffn."))
DROPOUT = (0.25, 2 ** 40 + 77, 6)                      # case 5: (p, seed, offset)

# multiplicities in ascending product id; `|` in the comments = the groups of four rows one wave takes
MULT = {
    "short_mixed": (24, 4, (17, 16, 2, 1, 15, 3, 5, 1, 1)),                 # whole-wave | 16-lane | lone tail row
    "wave_cut": (24, 4, (1, 2, 3, 16, 15, 5, 1, 1, 17)),                    # 16-lane | 16-lane | whole-wave cut by `rows`
    "hub": (140, 4, (130, 65, 64, 63, 33, 17, 16, 1, 2, 1)),                # fp64 path, both sides of 64 and of 16
}


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


# ------------------------------------------------------------------ neighbour matrices
def _from_multiplicities(b, n, mult, seed):
    """Product i (ascending id) goes into the mult[i] samples with the fewest filled slots, at most once per sample; the
    slots of every sample are then shuffled; the rest is padding."""
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
    assert [int((nb == pid).sum()) for pid in ids] == list(mult)
    return nb


def _random_degrees(b, n, seed, lo, hi):
    """Distinct random products per sample, per-sample degree uniform in lo..hi, padding at random slots."""
    rng = np.random.RandomState(seed)
    nb = np.argsort(rng.rand(b, P), axis=1)[:, :n].astype(np.int32)
    deg = rng.randint(lo, hi + 1, size=b)
    nb[np.arange(n)[None, :] >= deg[:, None]] = -1
    for r in range(b):
        nb[r] = nb[r, rng.permutation(n)]
    return nb


def _neighbours(name):
    if name in MULT:
        b, n, mult = MULT[name]
        return _from_multiplicities(b, n, mult, seed=3)
    if name == "colsum_515":                                       # rider: one 8 x 64-row unrolled trip, then rows 512..514
        return _random_degrees(515, 4, 5, 0, 4)
    if name == "n70":                                              # N > 64 and N mod 4 = 2: the slot map is read from memory
        return _random_degrees(12, 70, 6, 0, 70)
    if name == "no_padding":
        return _random_degrees(24, 4, 7, 4, 4)
    if name == "all_padding":
        return np.full((24, 4), -1, np.int32)
    raise KeyError(name)


def _case(name, d=128):
    """Inputs of one case (shared, never modified): parameters, feature table, index batch.  One cache entry per case,
    however the call spells its arguments."""
    return _case_cached(name, int(d))


@functools.lru_cache(maxsize=None)
def _case_cached(name, d):
    nb = _neighbours(name)
    b = nb.shape[0]
    g = torch.Generator().manual_seed(17)
    batch = {"anchor_idx": torch.randint(0, P, (b,), generator=g, dtype=torch.int32),
             "positive_idx": torch.randint(0, P, (b,), generator=g, dtype=torch.int32),
             "negative_idx": torch.randint(0, P, (b, K_NEG), generator=g, dtype=torch.int32),
             "neighbor_idx": torch.from_numpy(nb)}
    return {"st": _state(11, d), "table": rnd(P, d, seed=1), "batch": batch, "nb": nb}


def _row_slots(nb, row):
    """Slots (b * N + n, ascending) of the unique layout's row `row` = the product with the row-th smallest id."""
    ids = np.unique(nb[nb >= 0])
    return np.flatnonzero(nb.reshape(-1) == ids[row])


# ------------------------------------------------------------------ the fp64 oracle
def _attn_mask(b, n):
    p, seed, offset = DROPOUT
    m = philox_oracle.dropout_mask(seed, offset, philox_oracle.STREAM_ATTENTION, b * 4 * n, p)
    return torch.from_numpy(m).view(b, 4, n)


def _oracle(name, d=128, dropout=False, detach=None, dtype=torch.float64):
    """The step of product2vec.py:126-154 through p2v_oracle's ffn / attention / triplet_loss on `dtype` tensors.
    detach: flat slots whose key rows are cut from the graph between the neighbours' FFN and the attention (the forward
    is unchanged, their gradient is gone).  The result is shared and never modified; one cache entry per evaluation,
    however the call spells its arguments."""
    detach = None if detach is None else tuple(sorted(int(s) for s in detach))
    return _oracle_cached(name, int(d), bool(dropout), detach, dtype)


@functools.lru_cache(maxsize=None)
def _oracle_cached(name, d, dropout, detach, dtype):
    c = _case(name, d)
    # a copy of its own even where `dtype` is the case's: p2v_oracle.ffn updates the running statistics in place
    st = {k: (v.to(dtype, copy=True) if v.is_floating_point() else v.clone()) for k, v in c["st"].items()}
    start = {k: c["st"][k].clone() for k in ("ffn.1.running_mean", "ffn.1.running_var")}
    leaves = {k: st[k].clone().requires_grad_(True) for k in p2v_oracle.TRAINABLE}
    work = dict(st)
    work.update(leaves)
    tab = torch.cat([c["table"].to(dtype), torch.zeros(1, d, dtype=dtype)])        # the padding row, in `dtype`
    rows = lambda t: tab[t.long()]
    bt = c["batch"]
    b, n = bt["neighbor_idx"].shape
    a = p2v_oracle.ffn(rows(bt["anchor_idx"]), work, True)
    keys = p2v_oracle.ffn(rows(bt["neighbor_idx"]).reshape(-1, d), work, True).reshape(b, n, d)
    if detach is not None:
        cut = torch.zeros(b * n, dtype=torch.bool)
        cut[torch.as_tensor(list(detach))] = True
        keys = torch.where(cut.view(b, n, 1), keys.detach(), keys)
    mask = _attn_mask(b, n).to(dtype) if dropout else None
    emb = p2v_oracle.attention(a, keys, work, mask=mask)
    pos = p2v_oracle.forward(rows(bt["positive_idx"]), None, work, True)
    neg = p2v_oracle.forward(rows(bt["negative_idx"]), None, work, True)
    loss, _, _ = p2v_oracle.triplet_loss(emb, pos, neg, MARGIN)
    grads = torch.autograd.grad(loss, [leaves[k] for k in p2v_oracle.TRAINABLE])
    assert int(st["ffn.1.num_batches_tracked"]) == 4
    assert all(torch.equal(c["st"][k], v) for k, v in start.items()), "the case's shared state was modified"
    return {"loss": float(loss.detach()), "anchor_emb": emb.detach(), "running_mean": st["ffn.1.running_mean"],
            "running_var": st["ffn.1.running_var"], "grads": dict(zip(p2v_oracle.TRAINABLE, grads))}


def _grad_bound(ref):
    return 2e-6 + 2e-4 * float(ref.abs().max())


def _ratios(got, ref):
    """error / bound of everything the issue bounds; got: a device step or another oracle evaluation."""
    r = {"loss": abs(got["loss"] - ref["loss"]) / 2e-6,
         "emb": float((got["anchor_emb"].double() - ref["anchor_emb"]).abs().max()) / 2e-5,
         "stats": max(float((got[k].double() - ref[k]).abs().max()) for k in ("running_mean", "running_var")) / 1e-6}
    for k in GRAD_KEYS:
        r[k] = float((got["grads"][k].double() - ref["grads"][k]).abs().max()) / _grad_bound(ref["grads"][k])
    return r


def _report(what, r):
    worst = max(GRAD_KEYS, key=lambda k: r[k])
    print(f"rows-ratio {what}: loss {r['loss']:.3f} emb {r['emb']:.3f} stats {r['stats']:.3f} "
          f"grad {r[worst]:.3f} ({worst})")


def _within(what, got, ref):
    r = _ratios(got, ref)
    _report(what, r)
    bad = {k: round(v, 3) for k, v in r.items() if not v <= 1.0}
    assert not bad, f"{what}: error / bound above 1: {bad}"
    return r


# ------------------------------------------------------------------ a. oracle-only preconditions (CPU)
def _padding_slots(nb, lo, hi):
    n = nb.shape[1]
    return tuple(int(s) for s in np.flatnonzero(nb.reshape(-1) < 0) if lo * n <= s < hi * n)


def _control_slots(control):
    """(case, the slots whose key-row gradient the control loses)."""
    case = {"hub_one_of_64": "hub", "hub_65th_of_65": "hub", "hub_past_64_of_130": "hub", "short_17th_of_17": "short_mixed",
            "short_2nd_of_2": "short_mixed", "colsum_pad_512_514": "colsum_515", "colsum_pad_448_511": "colsum_515"}[control]
    nb = _case(case)["nb"]
    if control == "hub_one_of_64":
        s = _row_slots(nb, 2); assert len(s) == 64
        return case, (int(s[20]),)
    if control == "hub_65th_of_65":
        s = _row_slots(nb, 1); assert len(s) == 65
        return case, (int(s[64]),)
    if control == "hub_past_64_of_130":
        s = _row_slots(nb, 0); assert len(s) == 130
        return case, tuple(int(x) for x in s[64:])
    if control == "short_17th_of_17":
        s = _row_slots(nb, 0); assert len(s) == 17
        return case, (int(s[16]),)
    if control == "short_2nd_of_2":
        s = _row_slots(nb, 2); assert len(s) == 2
        return case, (int(s[1]),)
    if control == "colsum_pad_512_514":                            # the rider's remainder loop: row groups 0..2, one trip
        s = _padding_slots(nb, 512, 515)
    else:                                                          # the last (u = 7) load of the rider's unrolled trip
        s = _padding_slots(nb, 448, 512)
    assert len(s) > 0
    return case, s


CONTROLS = ("hub_one_of_64", "hub_65th_of_65", "hub_past_64_of_130", "short_17th_of_17", "short_2nd_of_2",
            "colsum_pad_512_514", "colsum_pad_448_511")


def _ffn_move(got, ref):
    return max(float((got["grads"][k].double() - ref["grads"][k]).abs().max()) / _grad_bound(ref["grads"][k]) for k in FFN_KEYS)


@pytest.mark.parametrize("control", CONTROLS)
def test_oracle_control_moves_an_ffn_gradient(control):
    """A lost slot cannot hide inside the tolerance: with the key rows of the control's slots detached, the fp64 oracle
    itself moves some ffn.* gradient tensor by >= 10 x that tensor's bound (no device involved)."""
    case, slots = _control_slots(control)
    full, cut = _oracle(case), _oracle(case, detach=slots)
    assert cut["loss"] == full["loss"] and torch.equal(cut["anchor_emb"], full["anchor_emb"])      # the forward is unchanged
    move = _ffn_move(cut, full)
    print(f"rows-control oracle {control}: {len(slots)} slots, ffn gradient moves by {move:.1f} x bound")
    assert move >= 10.0, f"{control}: {move:.2f}"


def test_oracle_fp32_sits_far_inside_the_bounds():
    """The bounds leave the kernels fp32's own room: the oracle in float32 is at a small fraction of them."""
    for case in ("short_mixed", "hub", "colsum_515"):
        r = _ratios(_oracle(case, dtype=torch.float32), _oracle(case))
        _report(f"oracle-fp32 {case}", r)
        assert max(r.values()) < 0.25, r


# ------------------------------------------------------------------ device steps
def _dev_batch(c):
    return c["table"].cuda(), {k: v.cuda() for k, v in c["batch"].items()}


def _layouts(ops, nb_dev, which):
    return {k: (nb_dev if k == "dense" else ops.compact_neighbors(nb_dev) if k == "compact" else ops.unique_neighbors(nb_dev))
            for k in which}


def _step(ops, c, table, batch, layout, dropout=False):
    params = {k: v.clone().cuda() for k, v in c["st"].items()}
    grads = {k: torch.full_like(params[k], 7.0) for k in ops.P2V_KEYS}            # overwritten, not accumulated into
    if dropout:
        params[ops.DROPOUT_KEY] = DROPOUT
    out = ops.p2v_train_step(params, grads, table, batch["anchor_idx"], batch["positive_idx"], batch["negative_idx"], layout,
                             MARGIN, want_emb=True)
    assert int(params["ffn.1.num_batches_tracked"]) == 4
    return {"loss": float(out["loss"]), "anchor_emb": out["anchor_emb"].cpu(), "running_mean": params["ffn.1.running_mean"].cpu(),
            "running_var": params["ffn.1.running_var"].cpu(), "grads": {k: grads[k].cpu() for k in ops.P2V_KEYS}}


def _bit_equal(x, y):
    return (x["loss"] == y["loss"] and torch.equal(x["anchor_emb"], y["anchor_emb"])
            and all(torch.equal(x["grads"][k], y["grads"][k]) for k in x["grads"]))


STEP_CASES = [("short_mixed", 128, False, ("dense", "compact", "unique")),        # 1
              ("wave_cut", 128, False, ("dense", "compact", "unique")),           # 2
              ("hub", 128, False, ("dense", "compact", "unique")),                # 3
              ("hub", 256, False, ("dense", "compact", "unique")),                # 4: attn_dkv_rows_kernel<4>, attn_core_*<16>
              ("hub", 128, True, ("compact", "unique")),                          # 5: pm enters dV; value-bias gradient = third column block
              ("colsum_515", 128, False, ("compact", "unique")),                  # 6
              ("n70", 128, False, ("dense", "compact", "unique")),                # 7
              ("no_padding", 128, False, ("dense", "compact", "unique")),         # 8
              ("all_padding", 128, False, ("dense", "compact", "unique"))]        # 8: no real row, the rider workgroups alone


@pytest.mark.parametrize("name,d,dropout,layouts", STEP_CASES,
                         ids=[f"{n}-d{d}{'-dropout' if dr else ''}" for n, d, dr, _ in STEP_CASES])
def test_step_against_the_fp64_oracle(ops, name, d, dropout, layouts):
    c = _case(name, d)
    ref = _oracle(name, d, dropout)
    table, batch = _dev_batch(c)
    for lname, layout in _layouts(ops, batch["neighbor_idx"], layouts).items():
        got = _step(ops, c, table, batch, layout, dropout)
        _within(f"{name} d{d}{' dropout' if dropout else ''} {lname}", got, ref)
        assert _bit_equal(got, _step(ops, c, table, batch, layout, dropout)), f"{lname}: two runs of one layout differ"
    if name in MULT:                                               # the case is what its comment says it is
        uq = ops.unique_neighbors(batch["neighbor_idx"])
        off = uq["ref_off"].cpu().numpy()
        assert tuple(np.diff(off[:uq["n_unique"] + 1])) == MULT[name][2]


# ------------------------------------------------------------------ b. well-formed but shortened layouts
def _shortened(uq, row, keep):
    """The unique layout with row `row`'s slot list cut to its first `keep` entries (ref_off shifted to match; slot_row,
    weight and nb_rows untouched: the forward and BatchNorm are unchanged, every index stays in range)."""
    off, slot = uq["ref_off"].cpu().numpy().copy(), uq["ref_slot"].cpu().numpy()
    lo, hi = int(off[row]), int(off[row + 1])
    removed = tuple(int(s) for s in slot[lo + keep:hi])
    off[row + 1:] -= hi - lo - keep
    dev = uq["ref_off"].device
    out = dict(uq, ref_off=torch.from_numpy(off).to(dev),
               ref_slot=torch.from_numpy(np.concatenate([slot[:lo + keep], slot[hi:]])).to(dev))
    return out, removed


@pytest.mark.parametrize("control,row,keep", [("hub_past_64_of_130", 0, 64), ("short_17th_of_17", 0, 16), ("short_2nd_of_2", 2, 1)])
def test_shortened_slot_list_is_seen(ops, control, row, keep):
    """The device step on a slot list that lacks entries leaves the bounds against the full fp64 oracle by > 10 x in some
    ffn.* tensor, and sits inside them against the oracle whose detached slots are exactly the removed ones."""
    case, slots = _control_slots(control)
    c = _case(case)
    table, batch = _dev_batch(c)
    short, removed = _shortened(ops.unique_neighbors(batch["neighbor_idx"]), row, keep)
    assert sorted(removed) == sorted(slots)
    got = _step(ops, c, table, batch, short)
    move = _ffn_move(got, _oracle(case))
    print(f"rows-control device {control}: ffn gradient off the full oracle by {move:.1f} x bound")
    assert move > 10.0, f"{control}: {move:.2f}"
    _within(f"{control} vs its detached oracle", got, _oracle(case, detach=slots))


# ------------------------------------------------------------------ c. arrival order
def _permuted(uq, seed):
    off, slot = uq["ref_off"].cpu().numpy(), uq["ref_slot"].cpu().numpy().copy()
    rng = np.random.RandomState(seed)
    for r in range(uq["n_unique"]):
        slot[off[r]:off[r + 1]] = rng.permutation(slot[off[r]:off[r + 1]])
    return dict(uq, ref_slot=torch.from_numpy(slot).to(uq["ref_slot"].device))


@pytest.mark.parametrize("name", ["short_mixed", "wave_cut", "hub"])
def test_arrival_order_of_the_slot_lists(ops, name):
    """The device builder fills ref_slot through integer atomics: a row's list arrives in any order.  Lists of <= 64 slots
    are sorted in the wave, so cases 1 and 2 are bit-equal to the ascending layout; the hub's longer rows are summed in
    fp64 in arrival order and stay within the bounds against the fp64 oracle (bit-equality is printed, not asserted)."""
    c = _case(name)
    table, batch = _dev_batch(c)
    uq = ops.unique_neighbors(batch["neighbor_idx"])
    base = _step(ops, c, table, batch, uq)
    for seed in (101, 102, 103):
        perm = _permuted(uq, seed)
        assert not torch.equal(perm["ref_slot"], uq["ref_slot"])
        got = _step(ops, c, table, batch, perm)
        same = _bit_equal(got, base)
        print(f"rows-order {name} permutation {seed}: bit-equal to the ascending layout: {same}")
        if name == "hub":
            _within(f"hub permuted {seed}", got, _oracle(name))
        else:
            assert same, f"{name}: permutation {seed} changed the result"


# ------------------------------------------------------------------ 9. the LDS bound on N (dense op)
def _attention_case(b, n, st, q, kv, dout, dtype):
    names = [k for k in p2v_oracle.TRAINABLE if k.startswith("attention")]
    leaves = {k: st[k].to(dtype).requires_grad_(True) for k in names}
    qi, ki = q.to(dtype).requires_grad_(True), kv.to(dtype).requires_grad_(True)
    out = p2v_oracle.attention(qi, ki, leaves)
    (out * dout.to(dtype)).sum().backward()
    res = {"out": out.detach(), "dquery": qi.grad, "dkeys": ki.grad}
    res.update({k: leaves[k].grad for k in names})
    return res


def _attention_tol(what, ref):
    """tests/test_gpu_ops.py::test_attention's tolerances."""
    return {"out": 3e-6, "dquery": 1e-5, "dkeys": 1e-5}.get(what) or 3e-5 * max(1.0, float(ref.abs().max()))


def _attention_hip(ops, st, q, kv, dout):
    dst = {k: v.clone().cuda() for k, v in st.items()}
    out, sv = ops.attention_forward(dst, q.cuda(), kv.cuda())
    grads, dq, dk = ops.attention_backward(dst, q.cuda(), kv.cuda(), dout.cuda(), sv)
    res = {"out": out.cpu(), "dquery": dq.cpu(), "dkeys": dk.cpu()}
    res.update({k: grads[k].cpu() for k in p2v_oracle.TRAINABLE if k.startswith("attention")})
    return res


def test_largest_accepted_key_count(ops):
    """8 HEADS N 4 <= 60000 (attn_check): N = 468 is the last key count the attention takes."""
    b, n = 3, 468
    st = _state(11)
    q, kv, dout = rnd(b, 128, seed=50), rnd(b, n, 128, seed=51), rnd(b, 128, seed=52)
    ref = _attention_case(b, n, st, q, kv, dout, torch.float64)
    got = _attention_hip(ops, st, q, kv, dout)
    for k, r in ref.items():
        err, tol = float((got[k].double() - r).abs().max()), _attention_tol(k, r)
        print(f"rows-ratio N=468 {k}: {err / tol:.3f}")
        assert err <= tol, f"{k}: {err:.3e} > {tol:.1e}"


def test_key_count_past_the_lds_bound_is_refused(ops):
    """N = 469: PC_ESHAPE from both entries, before any launch."""
    from p_companion_amd._lib import HipKernelError
    b, n = 3, 469
    dst = {k: v.clone().cuda() for k, v in _state(11).items()}
    q, kv, dout = rnd(b, 128, seed=50).cuda(), rnd(b, n, 128, seed=51).cuda(), rnd(b, 128, seed=52).cuda()
    with pytest.raises(HipKernelError, match="PC_ESHAPE"):
        ops.attention_forward(dst, q, kv)
    z = lambda *s: torch.zeros(*s, device="cuda")
    sv = {"q": z(b, 128), "qt": z(b, 4, 128), "c": z(b, 4, 128), "sp": z(b, 4), "probs": z(b, 4, n), "ctx": z(b, 128)}
    with pytest.raises(HipKernelError, match="PC_ESHAPE"):
        ops.attention_backward(dst, q, kv, dout, sv)


# ------------------------------------------------------------------ 10. peaked softmax (dense op)
PEAK_FACTOR = 100.0        # on the K block of in_proj_weight: the logits of a (sample, head) then span 132.5 .. 268.9


def test_peaked_softmax(ops):
    """Logits spanning more than 100 in every head of every sample (K block x 100: the span is 1.33 .. 2.69 at factor 1, so
    132.5 .. 268.9 over the 8 x 4 heads, asserted below; V and the outputs stay O(1)).  fp32's inherent error grows with
    the logits, so the bound is max(test_attention's tolerance, 4 x the error of the fp32 oracle against the fp64 one) per
    tensor -- 4 for an equally long but different summation order: the absorbed form rounds (Wk_h^T q_h) . y where the
    oracle rounds q_h . (Wk_h y).  The measured ratios are printed (`rows-peak ...`) and recorded in DESIGN section 4."""
    b, n, d = 8, 33, 128
    st = _state(11)
    st["attention.in_proj_weight"] = st["attention.in_proj_weight"].clone()
    st["attention.in_proj_weight"][d:2 * d] *= PEAK_FACTOR
    q, kv, dout = rnd(b, d, seed=50), rnd(b, n, d, seed=51), rnd(b, d, seed=52)
    w, bias = st["attention.in_proj_weight"].double(), st["attention.in_proj_bias"].double()
    qh = (q.double() @ w[:d].T + bias[:d]).view(b, 4, 1, 32) / math.sqrt(32)
    kh = (kv.double() @ w[d:2 * d].T + bias[d:2 * d]).view(b, n, 4, 32).transpose(1, 2)
    logits = (qh * kh).sum(-1)
    span = logits.max(-1).values - logits.min(-1).values
    print(f"rows-peak factor {PEAK_FACTOR}: logit span min {float(span.min()):.1f} max {float(span.max()):.1f}")
    assert float(span.min()) > 100.0
    ref = _attention_case(b, n, st, q, kv, dout, torch.float64)
    f32 = _attention_case(b, n, st, q, kv, dout, torch.float32)
    assert float(ref["out"].abs().max()) < 10.0
    got = _attention_hip(ops, st, q, kv, dout)
    bad = {}
    for k, r in ref.items():
        e_hip, e_f32 = float((got[k].double() - r).abs().max()), float((f32[k].double() - r).abs().max())
        tol = _attention_tol(k, r)
        print(f"rows-peak {k}: hip {e_hip:.3e} fp32-oracle {e_f32:.3e} ratio {e_hip / max(e_f32, 1e-300):.2f} "
              f"fixed tolerance {tol:.1e}")
        if e_hip > max(tol, 4.0 * e_f32):
            bad[k] = (e_hip, e_f32)
    assert not bad, bad
