"""Case lists, input builders, float64 references, bounds and checkers of the per-sample loss and metric kernels:
ops.triplet_loss (triplet_loss16_kernel / triplet_sample16 at D = 128, triplet_loss_kernel<4> at D = 256, hinge_mean_body),
ops.joint_loss / ops.expand_type_grad (joint_loss_kernel<1|2>, joint_loss_reduce_kernel, expand_type_grad_kernel),
ops.hit_rank (hit_rank_kernel) and ops.cosine_rows (cosine_rows_kernel<1|2>).  test_gpu_row_losses.py hands the checkers the
device ops, test_row_loss_bounds_host.py hands them numpy fp32 restatements of the kernels (three summation orders, at HALF of
every bound) and mutated restatements (which must be rejected).  Pure torch / numpy: importable without a GPU.

References.  p2v_oracle.triplet_loss and joint_oracle.type_loss / item_loss on the fp32 inputs widened to float64, autograd for
the gradients, the joint forms mixed as joint_oracle.compute_loss mixes them.  Hyper-parameters enter as the fp32 values the
C ABI passes (margin, alpha), and the pairwise eps as the kernels' constant 1e-6f widened -- 2.5e-14 away from the oracle's
double 1e-6, and the only way a planted distance of exactly 0 is 0 on both sides.

Bounds, u = 2^-24, first-order terms written out, the second-order ones carried by the explicit (1 + ...) factors below and by
the +4 of the norm bound (D^2 u^2 < u / 100 at D = 256).  No coefficient is fitted to a result.

  norm of D terms.  x_i = a_i - p_i + eps: one rounding for the difference, one for the sum, so |x^_i - x_i| <= 2 u |x_i| + u eps
  and | ||x^|| - ||x|| | <= 2 u d + u eps sqrt(D).  D squares (one rounding each, none under an fma) summed in ANY order: relative
  error <= D u of the sum, halved by the square root, plus the root's own rounding: (D/2 + 1) u.  Together
      |d^ - d| <= (D/2 + 4) u d + 2 u eps sqrt(D)                                                        norm_bound()
  (the joint kernels and the cosine subtract once or not at all and add no eps: the same form with eps = 0 covers them).

  d- = (sum_j d-_j) / K: K - 1 additions and one division:  e_neg = mean_j e_j (1 + K u) + K u d-.

  gap = (margin - d+) + d-, two roundings:  errA = e_pos (1 + u) + u |margin - d+|,  e_gap = (errA + e_neg)(1 + u) + u |gap|.
  The joint item gap has the same form; the type gap reads its two operands exactly: e = u |margin - s+| (1 + u) + u |gap|.
  A sample with |gap| > e_gap is DECIDED: every correct evaluation has the sign of the float64 gap.

  gradient element = a sum of terms T = x_i c, c = scale / d.  c^ carries k roundings (1 / B or alpha / (B K), the product K d_j
  of the triplet negatives, the division) and the distance's own error: |c^ / c - 1| <= R = (1 + e_d / (d - e_d)) (1 + u)^k - 1.
  With ex = |x^_i - x_i| and the product's rounding:  e_T = ex c (1 + R)(1 + u) + |x_i| c (R + u + R u).            term_bound()
  n terms added by n - 1 additions in any order: e = sum e_T + ((1 + u)^(n-1) - 1) sum (|T| + e_T).                  sum_bound()
  The triplet da has K + 1 terms, dp and dn one, the joint dproj two.  Where d == 0 exactly (planted) the term is exactly 0:
  torch's norm has subgradient 0 at 0, and the kernels select 0 there.  At a hinge of exactly 0 the oracles differ, and the
  kernels with them: the triplet hinge is F.relu (slope 0 at 0), the joint hinges are torch.clamp(min=0) (slope 1 at 0).

  reduced losses.  hinge_mean_body and joint_loss_reduce_kernel: a thread adds ceil(B / 256) values, eight tree levels, one
  division -- at most (B / 256 + 9) roundings on any value:  e = [sum_b e_b + (B / 256 + 9) u sum_b (l_b + e_b)] / B (/ K).
  (A bound of that fixed tree, not of any order: one sequential fp32 chain over 513 samples already exceeds half of it.)
  The joint item value of a sample is itself a K-term sum (sum_bound), the mixed loss adds four more roundings.

Hinge conditions (asserted by the checkers on the float64 side, for the device and for the host run alike): apart from the
planted exact edge every sample of every case is decided, and in every random case with B >= 32 the active and the inactive
share are both at least 10 %.

NaN inputs are out of scope everywhere.  In particular hit_rank_kernel counts `v > g or (v == g and c < r)`, which a NaN never
satisfies, while torch.topk ranks NaN above everything: the two order NaN scores differently, and no case holds one."""
import contextlib

import numpy as np
import torch

from oracle import joint_oracle, p2v_oracle

U = 2.0 ** -24
F32 = np.float32
EPS32 = F32(1e-6)              # PAIR_EPS / PC_PAIR_EPS of the kernels
EPS = float(EPS32)
CLAMP32 = F32(1e-8)            # the cosine kernels' fmaxf(norm, 1e-8f)
NEVER = 0x7fffffff             # hit_rank of a row without a column of its own


# ------------------------------------------------------------------ bounds
def norm_bound(d, dim, eps=0.0):
    return (dim / 2 + 4) * U * d + 2 * U * eps * np.sqrt(dim)


def scale_error(d, e_d, roundings):
    """R: relative error bound of c^ = scale / d^ against scale / d (0 where d == 0: the term is selected away)"""
    ok = d > 0
    rho = np.where(ok, e_d / np.where(ok, d - e_d, 1.0), 0.0)
    return (1 + rho) * (1 + U) ** roundings - 1


def term_bound(x, ex, c, r):
    return ex * c * (1 + r) * (1 + U) + np.abs(x) * c * (r + U + r * U)


def sum_bound(abs_terms, err_terms, additions):
    """abs_terms / err_terms: sum over the terms of |T| and of e_T"""
    return err_terms + ((1 + U) ** additions - 1) * (abs_terms + err_terms)


def gap_bound(margin, d_pos, e_pos, d_neg, e_neg):
    err_a = e_pos * (1 + U) + U * np.abs(margin - d_pos)
    return (err_a + e_neg) * (1 + U) + U * np.abs(margin - d_pos + d_neg)


def mean_bound(values, errors, batch):
    """sum over the batch through the fixed 256-thread tree, divided once; the caller divides by the count"""
    return errors.sum() + (batch / 256 + 9) * U * (values + errors).sum()


def worst_ratio(got, ref, bound):
    """largest |got - ref| / bound; inf for a NaN, an infinity or an error where the bound is 0"""
    got = np.asarray(got, dtype=np.float64)
    if got.shape != np.shape(ref) or not np.isfinite(got).all():
        return float("inf")
    err = np.abs(got - ref)
    bound = np.broadcast_to(np.asarray(bound, dtype=np.float64), err.shape)
    pos = bound > 0
    r = np.where(pos, err / np.where(pos, bound, 1.0), np.where(err == 0, 0.0, np.inf))
    return float(r.max()) if r.size else 0.0


def _rng(seed):
    return np.random.default_rng(seed)


def _randn(rng, *shape):
    return rng.standard_normal(shape).astype(F32)


# ================================================================== triplet hinge
TRIPLET_B = (1, 3, 4, 5, 15, 16, 17, 33, 67, 255, 256, 257, 300, 513)
PLANTS = ("eps", "dpos0", "neg0", "far", "edge")
# eps    p_b == a_b and n_b0 == a_b: both distances are eps sqrt(D) -- the only place the pairwise eps is visible
# dpos0  a_b = 0, p_b = 1e-6f in every dimension: a - p + eps == 0 exactly, d+ = 0 (oracle: zero dp row, finite da row)
# neg0   the same construction for the last negative of the sample
# far    d+ ~ 100 sqrt(2 D): far on the inactive side, three gradient rows of exact zeros
# edge   d+ ~ d- + 1; the case's margin becomes fp32(d+^ - d-^) of the op's own need_grad=False outputs.  d-/2 <= d+ <= 2 d-,
#        so that difference is exact (Sterbenz), and so is margin - d+^ = -d-^: the op's gap is exactly 0, relu'(0) = 0.


def plant_rows(batch, rot=0):
    """{kind: row}: all five from B = 15 on (spread over the first workgroup and the last sample); below, sample i carries
    PLANTS[(i + rot) % 5]"""
    if batch >= 15:
        return {"eps": 1, "neg0": 2, "far": 5, "edge": 7, "dpos0": batch - 1}
    return {PLANTS[(i + rot) % 5]: i for i in range(min(batch, 5))}


def _triplet_cases():
    cases = []
    for dim, k0 in ((128, 0), (256, 3)):
        for i, b in enumerate(TRIPLET_B):                    # fourteen B in a row: every K of 1..8 per D
            rot = {1: 0, 3: 2, 4: 1}.get(b, 0)
            cases.append((dim, b, (i + k0) % 8 + 1, rot))
        for rot in range(1, 5):                              # B = 1 once per planted kind (rot 0 is in the loop above)
            cases.append((dim, 1, (2 * rot + k0) % 8 + 1, rot))
    return cases


TRIPLET_CASES = _triplet_cases()                             # (D, B, K, rot)
# cases whose first seed left less than 10 % of the samples on one side of the hinge take the next one
TRIPLET_RESEED = {(256, 67, 4, 0): 3, (256, 255, 5, 0): 1}


def triplet_id(case):
    return "D%d-B%d-K%d-rot%d" % case


def triplet_inputs(case):
    dim, b, k, rot = case
    rng = _rng(7000 * dim + 10 * b + k + 100003 * rot + 1000003 * TRIPLET_RESEED.get(case, 0))
    a, p, n = _randn(rng, b, dim), _randn(rng, b, dim), _randn(rng, b, k, dim)
    rows = plant_rows(b, rot)
    for kind, r in rows.items():
        if kind == "eps":
            p[r] = a[r]
            n[r, 0] = a[r]
        elif kind == "dpos0":
            a[r] = 0
            p[r] = EPS32
        elif kind == "neg0":
            a[r] = 0
            p[r] = F32(0.01) * _randn(rng, dim)              # (a near positive: the sample is active even at K = 1, d- = 0)
            n[r, k - 1] = EPS32
        elif kind == "far":
            p[r] = a[r] + 100 * _randn(rng, dim)
        elif kind == "edge":
            d_neg = np.linalg.norm(a[r].astype(np.float64) - n[r] + EPS, axis=-1).mean()
            v = rng.standard_normal(dim)
            p[r] = (a[r] - v / np.linalg.norm(v) * (d_neg + 1.0)).astype(F32)
    return a, p, n, rows


@contextlib.contextmanager
def _oracle_eps(eps):
    old = p2v_oracle.PAIRWISE_EPS
    p2v_oracle.PAIRWISE_EPS = eps
    try:
        yield
    finally:
        p2v_oracle.PAIRWISE_EPS = old


def triplet_reference(a, p, n, margin):
    """float64: loss, d_pos, d_neg, da, dp, dn (p2v_oracle.triplet_loss + autograd) and every bound of the header"""
    b, k, dim = n.shape
    ta, tp, tn = (torch.from_numpy(t).double().requires_grad_(True) for t in (a, p, n))
    with _oracle_eps(EPS):
        loss, d_pos, d_neg = p2v_oracle.triplet_loss(ta, tp, tn, float(margin))
    loss.backward()
    ref = {"loss": float(loss.detach()), "d_pos": d_pos.detach().numpy(), "d_neg": d_neg.detach().numpy(),
           "da": ta.grad.numpy(), "dp": tp.grad.numpy(), "dn": tn.grad.numpy()}
    x = a.astype(np.float64) - p + EPS
    y = a.astype(np.float64)[:, None] - n + EPS
    d, dj = np.linalg.norm(x, axis=-1), np.linalg.norm(y, axis=-1)
    e_d, e_dj = norm_bound(d, dim, EPS), norm_bound(dj, dim, EPS)
    e_neg = e_dj.mean(1) * (1 + k * U) + k * U * ref["d_neg"]
    gap = margin - d + dj.mean(1)
    e_gap = gap_bound(margin, d, e_d, dj.mean(1), e_neg)
    active = gap > 0
    c_pos = np.where(active & (d > 0), 1.0 / (b * np.where(d > 0, d, 1.0)), 0.0)[:, None]
    c_neg = np.where(active[:, None] & (dj > 0), 1.0 / (b * k * np.where(dj > 0, dj, 1.0)), 0.0)[..., None]
    ex, ey = (2 * U * np.abs(x) + U * EPS) * (1 + U), (2 * U * np.abs(y) + U * EPS) * (1 + U)
    e_tp = term_bound(x, ex, c_pos, scale_error(d, e_d, 2)[:, None])
    e_tn = term_bound(y, ey, c_neg, scale_error(dj, e_dj, 3)[..., None])
    e_da = sum_bound(np.abs(x) * c_pos + (np.abs(y) * c_neg).sum(1), e_tp + e_tn.sum(1), k)
    hinge = np.maximum(gap, 0.0)
    bound = {"loss": mean_bound(hinge, e_gap, b) / b, "d_pos": e_d, "d_neg": e_neg, "da": e_da, "dp": e_tp, "dn": e_tn}
    return ref, bound, gap, e_gap


def hinge_shares(gap, e_gap, allowed_undecided=()):
    """(undecided samples outside `allowed_undecided`, active share, inactive share)"""
    und = set(np.nonzero(np.abs(gap) <= e_gap)[0].tolist()) - set(allowed_undecided)
    return sorted(und), float((gap > 0).mean()), float((gap <= 0).mean())


def check_triplet(case, run, frac=1.0):
    """run(a, p, n, margin, need_grad) -> dict of numpy arrays as ops.triplet_loss.  Asserts everything the header states for
    one case; returns the largest error / bound ratio per output."""
    dim, b, k, rot = case
    a, p, n, rows = triplet_inputs(case)
    first = run(a, p, n, 1.0, False)
    assert set(first) == {"loss", "d_pos", "d_neg"}
    margin, edge = F32(1.0), rows.get("edge")
    if edge is not None:
        dp_, dn_ = first["d_pos"][edge], first["d_neg"][edge]
        assert dn_ / 2 <= dp_ <= 2 * dn_ and dp_ > dn_, (dp_, dn_)
        margin = F32(dp_ - dn_)
        assert 0.9 < margin < 1.1
    ref, bound, gap, e_gap = triplet_reference(a, p, n, float(margin))
    # ---- the conditions on the inputs
    undecided, act, inact = hinge_shares(gap, e_gap, () if edge is None else (edge,))
    assert not undecided, (undecided, gap[undecided], e_gap[undecided])
    if b >= 32:
        assert act >= 0.1 and inact >= 0.1, (act, inact)
    for kind, r in rows.items():
        if kind == "far":
            assert gap[r] < -100
        elif kind != "edge":
            assert gap[r] > 0.5                                      # the zero-distance and eps samples are active
    out = run(a, p, n, float(margin), True)
    again = run(a, p, n, float(margin), False)
    for name in ("loss", "d_pos", "d_neg"):                          # the da == NULL branch: the same forward bits
        assert np.array_equal(out[name].view(np.int32), again[name].view(np.int32)), name
    assert np.array_equal(first["d_pos"].view(np.int32), out["d_pos"].view(np.int32))       # (no distance depends on the margin)
    assert np.array_equal(first["d_neg"].view(np.int32), out["d_neg"].view(np.int32))
    # ---- the op's own hinge decision, restated in numpy fp32 from its own distances
    gap32 = (margin - out["d_pos"]) + out["d_neg"]
    assert gap32.dtype == F32
    on = gap32 > 0
    if edge is not None:
        assert gap32[edge] == 0 and not on[edge]
    decided = np.abs(gap) > e_gap
    assert np.array_equal(on[decided], (gap > 0)[decided])
    off_rows = ~on
    for name in ("da", "dp", "dn"):
        g = out[name]
        assert np.isfinite(g).all(), name + ": not finite"
        assert not g[off_rows].any(), name + ": a gradient on the inactive side or on the edge"
    sends = out["dp"].reshape(b, -1).any(1) | out["dn"].reshape(b, -1).any(1)
    assert np.array_equal(sends, on)                                 # every active sample sends a gradient
    if "dpos0" in rows:
        assert first["d_pos"][rows["dpos0"]] == 0 and not out["dp"][rows["dpos0"]].any() and out["da"][rows["dpos0"]].any()
    if "neg0" in rows:
        assert not out["dn"][rows["neg0"], k - 1].any() and out["dp"][rows["neg0"]].any()
    if "eps" in rows:
        assert abs(float(first["d_pos"][rows["eps"]]) - EPS * np.sqrt(dim)) <= frac * norm_bound(EPS * np.sqrt(dim), dim, EPS)
    # ---- against float64 (the edge sample is undecided there: its exact zeros were asserted above)
    keep = np.ones(b, dtype=bool)
    if edge is not None:
        keep[edge] = False
    ratios = {"loss": worst_ratio(out["loss"].reshape(()), ref["loss"], bound["loss"])}
    for name in ("d_pos", "d_neg"):
        ratios[name] = worst_ratio(out[name], ref[name], bound[name])
    for name in ("da", "dp", "dn"):
        ratios[name] = worst_ratio(out[name][keep], ref[name][keep], bound[name][keep])
    bad = {name: r for name, r in ratios.items() if not r <= frac}
    assert not bad, (triplet_id(case), bad)
    return ratios


# ------------------------------------------------------------------ numpy fp32 restatements
ORDERS = ("seq", "rev", "tree")


def _chain(v, idx):
    s = np.zeros(v.shape[:-1], dtype=F32)
    for i in idx:
        s = s + v[..., i]
    return s


def _halve(part):
    while part.shape[-1] > 1:                    # the xor butterfly / the LDS tree: lane l takes lane l + half
        h = part.shape[-1] // 2
        part = part[..., :h] + part[..., h:]
    return part[..., 0]


def lane_layout(kind, dim):
    """[lanes, dims per lane]: the dims a lane adds, in its order.  group16: triplet_sample16 (8 consecutive dims, 16 lanes);
    wave4: triplet_loss_kernel<4> (4 consecutive, 64 lanes); pairs: the joint / cosine kernels (dims 2l, 2l+1 of every 128-wide
    chunk, 64 lanes)"""
    if kind == "group16":
        return np.arange(128).reshape(16, 8)
    if kind == "wave4":
        return np.arange(256).reshape(64, 4)
    ch = np.arange(dim // 128)[None, :, None] * 128
    return (ch + 2 * np.arange(64)[:, None, None] + np.arange(2)[None, None, :]).reshape(64, -1)


def sum32(v, order, layout):
    """fp32 sum over the last axis: sequential, reversed, or per lane and then by halving as the kernels do"""
    assert v.dtype == F32
    dim = v.shape[-1]
    if order == "seq":
        return _chain(v, range(dim))
    if order == "rev":
        return _chain(v, range(dim - 1, -1, -1))
    part = _chain(v[..., layout], range(layout.shape[1]))
    return _halve(part)


def batch_sum32(v):
    """hinge_mean_body / joint_loss_reduce_kernel over a [B] vector: thread t adds b = t, t + 256, ..., then the LDS tree.  The
    order is fixed in the kernels and the (B / 256 + 9) u term is a bound of THIS tree, so the restatements keep it in every
    summation order of the rows."""
    assert v.dtype == F32 and v.ndim == 1
    pad = np.zeros((-v.size) % 256, dtype=F32)
    per_thread = np.concatenate([v, pad]).reshape(-1, 256).T
    return _halve(_chain(per_thread, range(per_thread.shape[1])))


def _guarded_div(num, den, guard):
    if not guard:
        with np.errstate(divide="ignore", invalid="ignore"):
            return (num / den).astype(F32)
    ok = den > 0
    return np.where(ok, num / np.where(ok, den, F32(1)), F32(0)).astype(F32)


TRIPLET_MUTANTS = ("no_eps", "mean_over_k_plus_1", "relu_slope_1_at_0", "dn_sign", "no_zero_guard")


def triplet_restated(order, mutant=None):
    """a run() for check_triplet: the two triplet kernels and the mean in numpy fp32 (every operation one rounding; the device
    may contract a multiply-add, which only removes roundings)"""
    def run(a, p, n, margin, need_grad):
        b, k, dim = n.shape
        lay = lane_layout("group16" if dim == 128 else "wave4", dim)
        eps = F32(0) if mutant == "no_eps" else EPS32
        margin = F32(margin)
        x = (a - p) + eps
        y = (a[:, None] - n) + eps
        d_pos = np.sqrt(sum32(x * x, order, lay))
        dj = np.sqrt(sum32(y * y, order, lay))
        d_neg = _chain(dj, range(k)) / F32(k + 1 if mutant == "mean_over_k_plus_1" else k)
        gap = (margin - d_pos) + d_neg
        loss = batch_sum32(np.where(gap > 0, gap, F32(0))) / F32(b)
        out = {"loss": np.asarray(loss, dtype=F32).reshape(1), "d_pos": d_pos, "d_neg": d_neg}
        if need_grad:
            active = gap >= 0 if mutant == "relu_slope_1_at_0" else gap > 0
            gs = np.where(active, F32(1) / F32(b), F32(0)).astype(F32)
            guard = mutant != "no_zero_guard"
            ip = _guarded_div(gs, d_pos, guard)
            inj = _guarded_div(gs[:, None], F32(k) * dj, guard)
            out["dp"] = x * ip[:, None]
            ga = -out["dp"]
            for j in range(k):
                ga = ga + y[:, j] * inj[:, j, None]
            out["da"] = ga
            out["dn"] = y * inj[..., None] * F32(1 if mutant == "dn_sign" else -1)
            assert all(out[name].dtype == F32 for name in out)
        return out
    return run


# ================================================================== joint hinges
JOINT_PLANTS = ("first_last", "last_first", "same_type", "np_zero", "nn_zero")
# first_last / last_first   (pos_t, neg_t) = (0, T - 1) / (T - 1, 0): the two ends of a row of sims
# same_type                 pos_t == neg_t (column T - 1): the type gap is the margin, dsims_val = (-g, +g), the dense row sums to 0
# np_zero / nn_zero         proj_b0 == pos_b / == neg_b exactly: a zero norm (subgradient 0)
# Sample i of a case carries JOINT_PLANTS[(i + rot) % 5] for i < min(B, 5), and sample B - 1 is a same_type row when B > 5.
# (D, B, K, T, alpha, rot).  T = 1 makes every row a same_type row, so the type hinge has no inactive side: B < 32 only.
JOINT_CASES = [(128, 1, 1, 1, 0.5, 0), (256, 1, 3, 2, 0.8, 1), (128, 1, 2, 65, 0.0, 2), (256, 1, 8, 300, 1.0, 3),
               (128, 1, 3, 2, 0.8, 4), (256, 3, 2, 65, 0.5, 0), (128, 3, 8, 1, 0.8, 2), (256, 4, 1, 300, 0.0, 1),
               (128, 4, 3, 2, 1.0, 3), (128, 5, 2, 300, 0.8, 0), (256, 5, 8, 1, 0.5, 0), (128, 64, 3, 65, 0.8, 0),
               (256, 64, 1, 2, 0.5, 0), (128, 64, 8, 300, 0.0, 0), (256, 257, 2, 300, 1.0, 0), (128, 257, 1, 2, 0.8, 0),
               (256, 257, 3, 65, 0.8, 0), (128, 513, 8, 65, 0.5, 0), (256, 513, 3, 2, 0.0, 0), (256, 513, 8, 300, 0.8, 0),
               (128, 513, 2, 300, 1.0, 0)]
JOINT_MARGIN = 1.0
# cases whose first seeds left an undecided gap (|gap| <= its bound: about one in 3 000 gaps at D = 256) take the next one
JOINT_RESEED = {(256, 257, 2, 300, 1.0, 0): 1, (256, 513, 3, 2, 0.0, 0): 1, (256, 513, 8, 300, 0.8, 0): 3}


def joint_id(case):
    return "D%d-B%d-K%d-T%d-alpha%g-rot%d" % case


def joint_plant_rows(batch, rot=0):
    return {i: JOINT_PLANTS[(i + rot) % 5] for i in range(min(batch, 5))}


def joint_inputs(case):
    dim, b, k, t, alpha, rot = case
    rng = _rng(9000 * dim + 10 * b + k + 31 * t + 100003 * rot + 1000003 * JOINT_RESEED.get(case, 0))
    sims, proj = _randn(rng, b, t), _randn(rng, b, k, dim)
    pos, neg = _randn(rng, b, dim), _randn(rng, b, dim)
    pos_t = rng.integers(0, t, b).astype(np.int32)
    neg_t = rng.integers(0, t, b).astype(np.int32)
    if t == 2:
        neg_t = (1 - pos_t).astype(np.int32)                 # (two columns: keep the same_type rows to the planted ones)
    for i, kind in joint_plant_rows(b, rot).items():
        if kind == "first_last":
            pos_t[i], neg_t[i] = 0, t - 1
        elif kind == "last_first":
            pos_t[i], neg_t[i] = t - 1, 0
        elif kind == "same_type":
            pos_t[i] = neg_t[i] = t - 1
        elif kind == "np_zero":
            proj[i, 0] = pos[i]
        elif kind == "nn_zero":
            proj[i, 0] = neg[i]
    if b > 5:
        pos_t[b - 1] = neg_t[b - 1] = t // 2
    return sims, proj, pos_t, neg_t, pos, neg


def joint_reference(sims, proj, pos_t, neg_t, pos, neg, margin, alpha):
    """float64 (joint_oracle.type_loss / item_loss mixed as compute_loss, autograd): losses [3], dsims_val [B,2] (the gradient
    of the two gathered similarities), the dense d(loss)/d(sims) [B,T] and dproj -- margin and alpha as the fp32 values the
    op receives"""
    b = sims.shape[0]
    margin, alpha = float(F32(margin)), float(F32(alpha))
    ts = torch.from_numpy(sims).double().requires_grad_(True)
    tx = torch.from_numpy(proj).double().requires_grad_(True)
    lp, ln = torch.from_numpy(pos_t.astype(np.int64)), torch.from_numpy(neg_t.astype(np.int64))
    tp_, tn_ = torch.from_numpy(pos).double(), torch.from_numpy(neg).double()
    tl = joint_oracle.type_loss(ts, lp, ln, margin)
    il = joint_oracle.item_loss(tx, tp_, tn_, margin)
    (alpha * il + (1 - alpha) * tl).backward()
    ar = torch.arange(b)
    pair = torch.stack([ts.detach()[ar, lp], ts.detach()[ar, ln]], 1).requires_grad_(True)
    zero, one = torch.zeros(b, dtype=torch.int64), torch.ones(b, dtype=torch.int64)
    ((1 - alpha) * joint_oracle.type_loss(pair, zero, one, margin)).backward()
    return {"losses": np.array([alpha * float(il.detach()) + (1 - alpha) * float(tl.detach()), float(tl.detach()), float(il.detach())]),
            "dsims_val": pair.grad.numpy(), "dense": ts.grad.numpy(), "dproj": tx.grad.numpy()}


def joint_bounds(sims, proj, pos_t, neg_t, pos, neg, margin, alpha):
    """bounds of every output, the item gaps [B,K] and the type gaps [B] with their own bounds"""
    b, k, dim = proj.shape
    margin, alpha = float(F32(margin)), float(F32(alpha))
    ar = np.arange(b)
    sp, sn = sims[ar, pos_t].astype(np.float64), sims[ar, neg_t].astype(np.float64)
    gap_t = margin - sp + sn
    e_gap_t = U * np.abs(margin - sp) * (1 + U) + U * np.abs(gap_t)
    g_t = (1 - alpha) / b                                            # fl(fl(1 - alpha) / B): two roundings
    e_dsv = np.where(gap_t >= 0, ((1 + U) ** 2 - 1) * g_t, 0.0)[:, None] * np.ones((1, 2))
    xp = proj.astype(np.float64) - pos[:, None]
    xn = proj.astype(np.float64) - neg[:, None]
    dp, dn = np.linalg.norm(xp, axis=-1), np.linalg.norm(xn, axis=-1)
    e_dp, e_dn = norm_bound(dp, dim), norm_bound(dn, dim)
    gap_i = margin - dp + dn
    e_gap_i = gap_bound(margin, dp, e_dp, dn, e_dn)
    g_i = np.where(gap_i >= 0, alpha / (b * k), 0.0)                 # one rounding (B K is exact), one more for g / norm
    c_p = np.where(dp > 0, g_i / np.where(dp > 0, dp, 1.0), 0.0)[..., None]
    c_n = np.where(dn > 0, g_i / np.where(dn > 0, dn, 1.0), 0.0)[..., None]
    e_tp = term_bound(xp, U * np.abs(xp), c_p, scale_error(dp, e_dp, 2)[..., None])
    e_tn = term_bound(xn, U * np.abs(xn), c_n, scale_error(dn, e_dn, 2)[..., None])
    e_dproj = sum_bound(np.abs(xp) * c_p + np.abs(xn) * c_n, e_tp + e_tn, 1)
    hinge_i = np.maximum(gap_i, 0.0)
    e_li = sum_bound(hinge_i.sum(1), e_gap_i.sum(1), k - 1)          # part_item[b]: K values added in a row
    hinge_t = np.maximum(gap_t, 0.0)
    tl, il = hinge_t.mean(), hinge_i.mean()
    e_tl = mean_bound(hinge_t, e_gap_t, b) / b
    e_il = mean_bound(hinge_i.sum(1), e_li, b) / (b * k)
    e_mix = alpha * e_il + (1 - alpha) * e_tl
    e_loss = e_mix + ((1 + U) ** 4 - 1) * (alpha * il + (1 - alpha) * tl + e_mix)
    bound = {"losses": np.array([e_loss, e_tl, e_il]), "dsims_val": e_dsv, "dproj": e_dproj}
    return bound, gap_i, e_gap_i, gap_t, e_gap_t


def check_joint(case, run, expand, frac=1.0):
    """run(sims, proj, pos_t, neg_t, pos, neg, margin, alpha, need_grad) -> (losses [3], dsims_val [B,2] | None, dproj | None)
    as ops.joint_loss; expand(dsims_val, pos_t, neg_t, T) -> dense [B,T] as ops.expand_type_grad.  Returns the ratios."""
    dim, b, k, t, alpha, rot = case
    inputs = joint_inputs(case)
    sims, proj, pos_t, neg_t, pos, neg = inputs
    ref = joint_reference(*inputs, JOINT_MARGIN, alpha)
    bound, gap_i, e_gap_i, gap_t, e_gap_t = joint_bounds(*inputs, JOINT_MARGIN, alpha)
    # ---- the conditions on the inputs
    assert not (np.abs(gap_i) <= e_gap_i).any() and not (np.abs(gap_t) <= e_gap_t).any()
    same = pos_t == neg_t
    kinds = set(joint_plant_rows(b, rot).values())
    assert (gap_t[same] == float(F32(JOINT_MARGIN))).all() and (same.any() or (b < 5 and "same_type" not in kinds))
    if b >= 32:
        assert t > 1 and not same.all()
        for gap in (gap_i, gap_t):
            assert (gap > 0).mean() >= 0.1 and (gap < 0).mean() >= 0.1, ((gap > 0).mean(), (gap < 0).mean())
    if "np_zero" in kinds:
        assert (np.abs(proj - pos[:, None]).sum(-1) == 0).any()
    if "nn_zero" in kinds:
        assert (np.abs(proj - neg[:, None]).sum(-1) == 0).any()
    losses, dsv, dproj = run(*inputs, JOINT_MARGIN, alpha, True)
    fwd = run(*inputs, JOINT_MARGIN, alpha, False)
    assert fwd[1] is None and fwd[2] is None
    assert np.array_equal(fwd[0].view(np.int32), losses.view(np.int32))          # need_grad=False: the same three losses
    dense = expand(dsv, pos_t, neg_t, t)
    assert dense.shape == (b, t) and dense.dtype == F32
    # ---- the dense form: exact given dsims_val
    g = dsv[:, 1]
    assert np.array_equal(dsv[:, 0], -g)
    want = np.zeros((b, t), dtype=F32)
    ar = np.arange(b)
    want[ar, neg_t] = g
    want[ar, pos_t] = np.where(same, F32(0), -g)                                 # pos_t == neg_t: -g + g, exactly 0
    assert np.array_equal(dense, want)
    g_type = float(F32(1.0) - F32(alpha)) / b
    assert (g[same] != 0).all() if g_type else not g.any()
    e_dense = np.zeros((b, t))
    e_dense[ar, pos_t] = e_dense[ar, neg_t] = np.where(same, 0.0, bound["dsims_val"][:, 0])
    ratios = {"losses": worst_ratio(losses, ref["losses"], bound["losses"]),
              "dsims_val": worst_ratio(dsv, ref["dsims_val"], bound["dsims_val"]),
              "dense": worst_ratio(dense, ref["dense"], e_dense),
              "dproj": worst_ratio(dproj, ref["dproj"], bound["dproj"])}
    bad = {name: r for name, r in ratios.items() if not r <= frac}
    assert not bad, (joint_id(case), bad)
    return ratios


# ---- exact cases: every intermediate is dyadic, so fp32 and float64 compute the same numbers
# (D, B, K): B K a power of two, alpha = 0.5, margin = 2, sims integer-valued in [-3, 3].  neg_b = pos_b + Q_b and
# proj_bk = pos_b + P_bk with Q, P in {0, +-1}: |Q_b|_0 = m_b, P_bk = Q_b on c of those positions and +-1 on r further ones, so
# |proj - pos|^2 = c + r and |proj - neg|^2 = m - c + r.  EXACT_COMBOS lists (m, |.|^2 of the positive, of the negative); the
# item gap 2 - np + nn takes 4, 2, 0 (np = 4, nn = 2, and np = 2, nn = 0), -4 and -6, np == 0 and nn == 0 among them.
EXACT_CASES = [(128, 64, 1), (256, 64, 2), (128, 64, 4), (256, 64, 8), (128, 512, 1), (256, 512, 2), (256, 512, 4),
               (128, 512, 8)]
EXACT_MARGIN, EXACT_ALPHA, EXACT_T = 2.0, 0.5, 7
EXACT_COMBOS = {0: [(0, 0), (4, 4), (16, 16), (64, 64)], 4: [(0, 4), (4, 4), (4, 0)], 16: [(16, 4)],
                64: [(64, 4), (64, 0), (64, 64)]}
EXACT_GAPS = (4, 2, 0, -4, -6)


def exact_inputs(case):
    dim, b, k = case
    rng = _rng(11 * dim + b + k)
    pos = rng.integers(-3, 4, (b, dim)).astype(F32)
    neg, proj = pos.copy(), np.repeat(pos[:, None], k, axis=1)
    sizes = sorted(EXACT_COMBOS)
    for i in range(b):
        m = sizes[i % 4]
        q = np.zeros(dim, dtype=F32)
        q[:m] = rng.choice([-1, 1], m)
        neg[i] += q
        for j in range(k):
            sq_p, sq_n = EXACT_COMBOS[m][(i // 4 + j) % len(EXACT_COMBOS[m])]
            r = (sq_p + sq_n - m) // 2
            c = sq_p - r
            assert 0 <= c <= m and 0 <= r <= dim - m and c + r == sq_p and m - c + r == sq_n
            pat = np.zeros(dim, dtype=F32)
            pat[:c] = q[:c]
            pat[m:m + r] = rng.choice([-1, 1], r)
            proj[i, j] += pat
    sims = rng.integers(-3, 4, (b, EXACT_T)).astype(F32)
    pos_t = rng.integers(0, EXACT_T, b).astype(np.int32)
    neg_t = rng.integers(0, EXACT_T, b).astype(np.int32)
    pos_t[:4], neg_t[:4] = (0, 0, EXACT_T - 1, 3), (EXACT_T - 1, 1, 0, 3)
    sims[0, 0], sims[0, EXACT_T - 1] = 3, 1                              # type gap exactly 0
    sims[1, 0], sims[1, 1] = 1, 2                                        # 3
    sims[2, EXACT_T - 1], sims[2, 0] = 3, -2                             # -3
    return sims, proj, pos_t, neg_t, pos, neg


def check_joint_exact(case, run, expand):
    dim, b, k = case
    inputs = exact_inputs(case)
    sims, proj, pos_t, neg_t, pos, neg = inputs
    _, gap_i, _, gap_t, _ = joint_bounds(*inputs, EXACT_MARGIN, EXACT_ALPHA)
    assert set(np.unique(gap_i).tolist()) == set(EXACT_GAPS) and (gap_i == np.round(gap_i)).all()
    assert tuple(gap_t[:3]) == (0, 3, -3) and gap_t[3] == EXACT_MARGIN
    assert (np.abs(proj - pos[:, None]).sum(-1) == 0).any() and (np.abs(proj - neg[:, None]).sum(-1) == 0).any()
    ref = joint_reference(*inputs, EXACT_MARGIN, EXACT_ALPHA)
    losses, dsv, dproj = run(*inputs, EXACT_MARGIN, EXACT_ALPHA, True)
    fwd = run(*inputs, EXACT_MARGIN, EXACT_ALPHA, False)
    dense = expand(dsv, pos_t, neg_t, EXACT_T)
    assert np.array_equal(fwd[0].view(np.int32), losses.view(np.int32))
    for name, got in (("losses", losses), ("dsims_val", dsv), ("dproj", dproj), ("dense", dense)):
        assert got.dtype == F32
        # equal as numbers to the float64 result, which fp32 holds exactly (a zero's sign is not a number)
        assert np.array_equal(got.astype(np.float64), ref[name]), (case, name)


JOINT_MUTANTS = ("item_scale_over_b", "type_scale_alpha", "no_zero_guard")


def joint_restated(order, mutant=None):
    def run(sims, proj, pos_t, neg_t, pos, neg, margin, alpha, need_grad):
        b, k, dim = proj.shape
        t = sims.shape[1]
        lay = lane_layout("pairs", dim)
        margin, alpha = F32(margin), F32(alpha)
        ar = np.arange(b)
        lt = (margin - sims[ar, pos_t]) + sims[ar, neg_t]
        xp, xn = proj - pos[:, None], proj - neg[:, None]
        np_, nn_ = np.sqrt(sum32(xp * xp, order, lay)), np.sqrt(sum32(xn * xn, order, lay))
        l = (margin - np_) + nn_
        part_item = _chain(np.where(l > 0, l, F32(0)), range(k))
        tl = batch_sum32(np.where(lt > 0, lt, F32(0))) / F32(b)
        il = batch_sum32(part_item) / (F32(b) * F32(k))
        losses = np.array([alpha * il + (F32(1) - alpha) * tl, tl, il], dtype=F32)
        if not need_grad:
            return losses, None, None
        scale_t = alpha if mutant == "type_scale_alpha" else F32(1) - alpha
        g = np.where(lt >= 0, scale_t / F32(b), F32(0)).astype(F32)
        dsv = np.stack([-g, g], 1)
        den = F32(b) if mutant == "item_scale_over_b" else F32(b) * F32(k)
        gi = np.where(l >= 0, alpha / den, F32(0)).astype(F32)
        guard = mutant != "no_zero_guard"
        ip, in_ = _guarded_div(gi, np_, guard), _guarded_div(gi, nn_, guard)
        dproj = -xp * ip[..., None] + xn * in_[..., None]
        assert dsv.dtype == F32 and dproj.dtype == F32
        return losses, dsv, dproj
    return run


def expand_restated(dsv, pos_t, neg_t, t):
    dense = np.zeros((dsv.shape[0], t), dtype=F32)
    for i in range(dsv.shape[0]):
        dense[i, pos_t[i]] += dsv[i, 0]
        dense[i, neg_t[i]] += dsv[i, 1]
    return dense


# ================================================================== hit_rank
HIT_SHAPES = [(1, 1), (5, 3), (3, 5), (64, 64), (65, 65), (67, 130), (130, 67), (259, 1000)]


def hit_inputs(shape):
    """values in {-2, ..., 2}: ties everywhere; +inf, -inf and -0.0 beside +0.0 planted on and off the diagonal"""
    rows, cols = shape
    rng = _rng(13 * rows + cols)
    s = rng.integers(-2, 3, (rows, cols)).astype(F32)
    if rows >= 5 and cols >= 5:
        s[0, 0], s[0, 3] = np.inf, np.inf                    # the own score is +inf, tied above the diagonal
        s[1, 1], s[1, 0] = -np.inf, -np.inf                  # -inf, tied below
        s[2, 2], s[2, 0], s[2, 4] = 0.0, -0.0, -0.0          # -0.0 == +0.0: a tie on either side
        s[3, 3], s[3, 1] = -0.0, 0.0
        s[4, 0], s[4, 2] = np.inf, -np.inf                   # infinities that are not the own score
    return s


def hit_expected(s):
    rows, cols = s.shape
    want = np.full(rows, NEVER, dtype=np.int64)
    c = np.arange(cols)
    for r in range(min(rows, cols)):
        want[r] = int(((s[r] > s[r, r]) | ((s[r] == s[r, r]) & (c < r))).sum())
    return want


def check_hit_rank(shape, run):
    s = hit_inputs(shape)
    got = run(s)
    assert got.dtype == np.int32 and np.array_equal(got.astype(np.int64), hit_expected(s)), shape


def hit_restated(mutant=None):
    def run(s):
        rows, cols = s.shape
        c, r = np.arange(cols)[None, :], np.arange(rows)[:, None]
        g = s[np.arange(rows), np.minimum(np.arange(rows), cols - 1)][:, None]
        tie = (c <= r) if mutant == "tie_rule_le" else (c < r)
        beat = ((s > g) | ((s == g) & tie)).sum(1)
        return np.where(np.arange(rows) < cols, beat, NEVER).astype(np.int32)
    return run


# ================================================================== cosine_rows
COSINE_CASES = [(128, 1, 1), (256, 1, 3), (128, 5, 3), (256, 5, 1), (128, 67, 1), (256, 67, 3), (128, 5, 8), (256, 67, 8),
                (128, 1, 8)]          # (D, B, K)


def cosine_reference(x, y):
    """float64 dot / (max(|x|, c) max(|y|, c)) with the kernels' clamp constant, and the bound per element: D products and
    their sum in any order, |dot^ - dot| <= ((1 + u)^D - 1) sum |x_i y_i|; each norm as norm_bound; one product of the clamped
    norms and one division"""
    b, k, dim = x.shape
    x64, y64 = x.astype(np.float64), y.astype(np.float64)[:, None]
    dot, mag = (x64 * y64).sum(-1), np.abs(x64 * y64).sum(-1)
    na, nb = np.linalg.norm(x64, axis=-1), np.linalg.norm(y64, axis=-1) * np.ones((1, k))
    ca, cb = np.maximum(na, float(CLAMP32)), np.maximum(nb, float(CLAMP32))
    ref = dot / (ca * cb)
    r = (1 + norm_bound(na, dim) / (ca - norm_bound(na, dim))) * (1 + norm_bound(nb, dim) / (cb - norm_bound(nb, dim))) \
        * (1 + U) ** 2 - 1
    bound = ((1 + U) ** dim - 1) * mag / (ca * cb) * (1 + r) + np.abs(ref) * r
    return ref.reshape(-1), bound.reshape(-1)


def cosine_random_inputs(case):
    dim, b, k = case
    rng = _rng(17 * dim + 5 * b + k)
    x, y = _randn(rng, b, k, dim), _randn(rng, b, dim)
    x *= (10.0 ** rng.uniform(-3, 3, (b, k, 1))).astype(F32) / F32(np.sqrt(dim))       # norms over 1e-3 ... 1e3
    y *= (10.0 ** rng.uniform(-3, 3, (b, 1))).astype(F32) / F32(np.sqrt(dim))
    return x, y


def cosine_exact_inputs(case):
    """entries in {0, +-1} with 4, 16 or 64 non-zeros: integer dot, norms 2, 4, 8 -- and a zero x row and a zero y row"""
    dim, b, k = case
    rng = _rng(19 * dim + 5 * b + k)
    x, y = np.zeros((b, k, dim), dtype=F32), np.zeros((b, dim), dtype=F32)
    for i in range(b):
        perm = rng.permutation(dim)                          # supports cut from one permutation: they overlap
        cnt = (4, 16, 64)[i % 3]
        y[i, perm[:cnt]] = rng.choice([-1, 1], cnt)
        for j in range(k):
            cnt = (4, 16, 64)[(i + j + 1) % 3]
            x[i, j, perm[2 + j:2 + j + cnt]] = rng.choice([-1, 1], cnt)
    x[0, k - 1] = 0
    if b > 1:
        y[b - 1] = 0
    return x, y


def clamp_rows(dim):
    """x = 2^-30 e_0 against y = e_0 and against y = 64 e_0: |x| is below the clamp, the dot is not 0.  Both rows give
    2^-30 / 1e-8f (the second scales numerator and denominator by 64); without the clamp both would give 1, and a clamp of the
    PRODUCT of the norms gives 1 on the second (2^-24 > 1e-8)."""
    x, y = np.zeros((2, 1, dim), dtype=F32), np.zeros((2, dim), dtype=F32)
    x[:, 0, 0] = F32(2.0 ** -30)
    y[0, 0], y[1, 0] = 1, 64
    return x, y, F32(2.0 ** -30) / CLAMP32


def check_cosine(case, run, frac=1.0):
    dim, b, k = case
    x, y = cosine_random_inputs(case)
    ref, bound = cosine_reference(x, y)
    norms = np.linalg.norm(x.astype(np.float64), axis=-1)
    assert 1e-4 < norms.min() and norms.max() < 1e4 and (b * k < 8 or norms.max() / norms.min() > 100)
    ratio = worst_ratio(run(x, y), ref, bound)
    assert ratio <= frac, (case, ratio)
    x, y = cosine_exact_inputs(case)
    ref, _ = cosine_reference(x, y)
    got = run(x, y)
    assert got.dtype == F32 and np.array_equal(got.astype(np.float64), ref.astype(F32).astype(np.float64)), case
    assert got[k - 1] == 0 and (b == 1 or not got[(b - 1) * k:].any())
    assert b * k == 1 or np.abs(got).max() > 0
    x, y, want = clamp_rows(dim)
    got = run(x, y)
    assert got[0].view(np.int32) == want.view(np.int32) and got[1].view(np.int32) == want.view(np.int32), (got, want)
    return ratio


def cosine_restated(order, mutant=None):
    def run(x, y):
        b, k, dim = x.shape
        lay = lane_layout("pairs", dim)
        yy = np.broadcast_to(y[:, None], x.shape)
        dot = sum32(x * yy, order, lay)
        na, nb = np.sqrt(sum32(x * x, order, lay)), np.sqrt(sum32(yy * yy, order, lay))
        if mutant == "clamp_on_product":
            den = np.maximum(na * nb, CLAMP32)
        else:
            den = np.maximum(na, CLAMP32) * np.maximum(nb, CLAMP32)
        out = (dot / den).reshape(-1)
        assert out.dtype == F32
        return out
    return run
