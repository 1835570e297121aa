"""Diversified lists: pc_diversify_lists / ops.diversify_lists (a greedy maximal-marginal-relevance re-rank of a served pool on
the device), pc_inv_norm / ops.inv_norm and PCompanionInference.recommend_diverse_batch.

Three references.  On exact data (a table of integers in [-4, 4], integer scores, lam 0.5 / 0.25, a scale of powers of two)
every quantity of the contract is exact in fp32, so a float64 greedy run in numpy gives the ids and the score bits, ties under
the index tie-break included.  lam = 1 is the pool's own first n, bit for bit.  On Gaussian data with the cosine scale a fresh
greedy run would cascade after one near-tie, so the device is teacher-forced: in every round its own earlier picks are taken
as given, every remaining candidate's value is formed in float64, and the device's pick must reach the float64 maximum within
the sum of the two candidates' allowances -- the forward bound of the contract's operations (DESIGN 7 "Diversified lists",
Numerics):
    e_sim(j, i) = gamma(D / 4 + 4 + [D = 256]) * f_ji * sum_d |e_j[d]| |e_i[d]|,   f = scale[j] scale[i], gamma(k) = k u / (1 - k u)
                  (D / 4 fused multiply-adds and 2 (+1) additions per chain, the product of the factors, the product with it)
    allow_j     = (u |lam s_j| + mu max_i e_sim(j, i) + u mu |pen_j| + u |v_j|) (1 + 4 u),   u = 2^-24
Needs an MI355X."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

P, R = 600, 37
SHAPES = ((1, 1), (5, 5), (16, 10), (17, 17), (64, 16), (65, 10), (200, 200), (256, 32), (256, 256))
DIMS = (128, 256)
U = 2.0 ** -24
CLONES = np.arange(300, 600)               # products with one and the same table row (the exact table)


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(sc):
    return sc.contiguous().view(torch.int32)


def same(got, want):
    return torch.equal(got[0], want[0]) and torch.equal(bits(got[1]), bits(want[1]))


def candidates(ids, sc):
    return (ids >= 0) & (ids < P) & np.isfinite(sc)


def greedy64(idx, score, table, scale, n, lam):
    """The contract in float64 (exact on exact data): (ids [R, n] int32, scores [R, n] fp32)."""
    lam = float(np.float32(lam))
    mu = float(np.float32(1) - np.float32(lam))
    t64 = table.astype(np.float64)
    out_i = np.full((idx.shape[0], n), -1, np.int32)
    out_s = np.full((idx.shape[0], n), -np.inf, np.float32)
    for r in range(idx.shape[0]):
        live = candidates(idx[r], score[r])
        ids = np.where(live, idx[r], 0)
        rows = t64[ids]
        sim = rows @ rows.T
        if scale is not None:
            f = scale.astype(np.float64)[ids]
            sim = sim * np.outer(f, f)
        ls = lam * score[r].astype(np.float64)
        pen = np.full(len(ids), -np.inf)
        for t in range(n):
            if not live.any():
                break
            v = ls if t == 0 else ls - mu * pen
            v = np.where(live, v, -np.inf)
            best = np.nonzero(live & (v == v[live].max()))[0]
            j = best[np.argmin(ids[best])]
            out_i[r, t], out_s[r, t] = ids[j], score[r, j]
            live[j] = False
            pen = np.maximum(pen, sim[:, j])
    return out_i, out_s


def exact_pool(rng, m):
    """Distinct integer-scored products per row; row 0 draws from the clones alone."""
    idx = np.stack([rng.permutation(P)[:m] for _ in range(R)]).astype(np.int32)
    idx[0] = rng.permutation(CLONES)[:m]
    score = rng.integers(-8, 9, (R, m)).astype(np.float32)
    return idx, score


@pytest.fixture(scope="module", params=DIMS, ids=lambda d: f"D{d}")
def exact(request):
    dim = request.param
    rng = np.random.default_rng(500 + dim)
    table = rng.integers(-4, 5, (P, dim)).astype(np.float32)
    table[CLONES] = table[CLONES[0]]
    scale = (2.0 ** rng.integers(-3, 2, P)).astype(np.float32)
    return dim, table, scale, cuda(table), cuda(scale)


# ---- 1. exact data, bit for bit
@pytest.mark.parametrize("m,n", SHAPES)
def test_exact_data_matches_the_float64_greedy_run_bit_for_bit(exact, m, n):
    from p_companion_amd import ops
    dim, table, scale, dtable, dscale = exact
    rng = np.random.default_rng(10 * m + n + dim)
    idx, score = exact_pool(rng, m)
    for lam, sc_h, sc_d in ((0.5, None, None), (0.25, scale, dscale)):
        got = ops.diversify_lists(cuda(idx), cuda(score), dtable, n, lam, scale=sc_d)
        want = greedy64(idx, score, table, sc_h, n, lam)
        assert got[0].shape == (R, n) and got[0].dtype == torch.int32 and got[1].dtype == torch.float32
        assert same(got, (cuda(want[0]), cuda(want[1]))), (lam, sc_h is not None)
    if n == m:                                            # every candidate exactly once
        assert (np.sort(got[0].cpu().numpy(), 1) == np.sort(idx, 1)).all()


# ---- 2. structure: holes, short pools, an empty row, scores that are not finite, ids out of range
@pytest.mark.parametrize("m,n", [(17, 17), (65, 10), (256, 32)])
def test_holes_short_pools_bad_scores_and_bad_ids(exact, m, n):
    from p_companion_amd import ops
    dim, table, scale, dtable, dscale = exact
    rng = np.random.default_rng(77 + m + dim)
    idx, score = exact_pool(rng, m)
    idx[rng.random((R, m)) < 0.2] = -1                    # -1 slots anywhere in the pool
    idx[3] = -1                                           # a row without a candidate
    idx[4, 3:] = -1                                       # fewer than n candidates (n > 3)
    idx[4, :3] = [7, 8, 9]
    idx[5][np.isin(idx[5], (11, 12))] = -1
    idx[6][idx[6] == 13] = -1
    score[5, 0], score[5, m // 2], score[6, m - 1] = np.nan, np.inf, -np.inf
    idx[5, 0], idx[5, m // 2], idx[6, m - 1] = 11, 12, 13      # (candidates but for their scores)
    out_of_range = [P, P + 1000, -2, 2 ** 31 - 1, -2 ** 31]
    for k, x in enumerate(out_of_range):
        idx[7 + k, (3 * k) % m] = x
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = ops.diversify_lists(cuda(idx), cuda(score), dtable, n, 0.5, scale=dscale, bad=bad)
    want = greedy64(idx, score, table, scale, n, 0.5)
    assert same(got, (cuda(want[0]), cuda(want[1])))
    assert int(bad) == len(out_of_range)
    g_i, g_s = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert (g_i[3] == -1).all() and np.isneginf(g_s[3]).all()
    if n > 3:
        assert sorted(g_i[4, :3]) == [7, 8, 9] and (g_i[4, 3:] == -1).all() and np.isneginf(g_s[4, 3:]).all()
    assert 11 not in g_i[5] and 12 not in g_i[5] and 13 not in g_i[6]
    # two calls: the same bits, and the counter is added to
    again = ops.diversify_lists(cuda(idx), cuda(score), dtable, n, 0.5, scale=dscale, bad=bad)
    assert same(again, got) and int(bad) == 2 * len(out_of_range)
    # without a counter the ids are passed over all the same
    assert same(ops.diversify_lists(cuda(idx), cuda(score), dtable, n, 0.5, scale=dscale), got)
    # a row's output does not depend on the other rows of the call
    for lo, hi in ((0, 1), (5, 9), (R - 1, R)):
        part = ops.diversify_lists(cuda(idx[lo:hi]), cuda(score[lo:hi]), dtable, n, 0.5, scale=dscale)
        assert same(part, (got[0][lo:hi], got[1][lo:hi]))
    # no rows
    e_i, e_s = ops.diversify_lists(cuda(idx[:0]), cuda(score[:0]), dtable, n, 0.5)
    assert e_i.shape == (0, n) and e_s.shape == (0, n)


# ---- 3. Gaussian data: lam = 1 and the teacher-forced float64 check
TYPE_SIZES = (400, 150, 50)                # pools of 256: full, short, shorter


@pytest.fixture(scope="module", params=DIMS, ids=lambda d: f"D{d}")
def gauss(request):
    from p_companion_amd import ops
    dim = request.param
    rng = np.random.default_rng(900 + dim)
    table = rng.standard_normal((P, dim)).astype(np.float32)
    type_idx = rng.permutation(np.repeat(np.arange(3), TYPE_SIZES)).astype(np.int32)
    order = np.argsort(type_idx, kind="stable").astype(np.int32)
    rowptr = np.concatenate([[0], np.cumsum(TYPE_SIZES)]).astype(np.int32)
    types = rng.permutation(np.repeat(np.arange(3), (25, 8, 4))).astype(np.int32)
    assert len(types) == R
    proj = rng.standard_normal((R, dim)).astype(np.float32)
    dtable = cuda(table)
    lists = {}

    def pool(m):                                          # retrieve_list_grouped(m), once per m
        if m not in lists:
            lists[m] = ops.retrieve_list_grouped(cuda(proj), cuda(types), cuda(rowptr), cuda(order), dtable, m)
        return lists[m]

    scale = ops.inv_norm(dtable)
    return dim, table, dtable, scale, pool


def shuffled(rng, idx, sc):
    perm = np.argsort(rng.random(idx.shape), 1)
    take = lambda t: cuda(np.take_along_axis(t.cpu().numpy(), perm, 1))
    return take(idx), take(sc)


@pytest.mark.parametrize("m,n", SHAPES)
def test_lam_one_is_the_first_n_of_the_list_as_it_is_and_shuffled(gauss, m, n):
    from p_companion_amd import ops
    dim, table, dtable, scale, pool = gauss
    idx, sc = pool(m)
    want = (idx[:, :n].contiguous(), sc[:, :n].contiguous())
    assert same(ops.diversify_lists(idx, sc, dtable, n, 1.0, scale=scale), want)
    assert same(ops.diversify_lists(idx, sc, dtable, n, 1.0), want)
    s_idx, s_sc = shuffled(np.random.default_rng(m + n), idx, sc)
    assert same(ops.diversify_lists(s_idx, s_sc, dtable, n, 1.0, scale=scale), want)


def teacher_forced(idx, score, picks, table, scale, lam, dim):
    """(rounds, rounds whose pick is not the float64 arg-max, worst shortfall / allowance, violations)"""
    lam = float(np.float32(lam))
    mu = float(np.float32(1) - np.float32(lam))
    k = dim // 4 + 4 + (dim == 256)
    gamma = k * U / (1 - k * U)
    t64, a64 = table.astype(np.float64), np.abs(table).astype(np.float64)
    rounds = off = violations = 0
    worst = 0.0
    for r in range(idx.shape[0]):
        live = candidates(idx[r], score[r])
        ids = np.where(live, idx[r], 0)
        f = np.outer(scale.astype(np.float64)[ids], scale.astype(np.float64)[ids])
        sim = (t64[ids] @ t64[ids].T) * f
        e_sim = gamma * (a64[ids] @ a64[ids].T) * f
        s = score[r].astype(np.float64)
        pen, e_pen = np.full(len(ids), -np.inf), np.zeros(len(ids))
        for t in range(picks.shape[1]):
            if not live.any():
                assert (picks[r, t:] == -1).all()
                break
            v = lam * s if t == 0 else lam * s - mu * pen
            allow = (U * np.abs(lam * s) + (0 if t == 0 else mu * e_pen + U * mu * np.abs(pen) + U * np.abs(v))) * (1 + 4 * U)
            at = np.nonzero(live & (ids == picks[r, t]))[0]
            assert len(at) == 1, (r, t, picks[r, t])      # a remaining candidate, once
            j = at[0]
            vm = np.where(live, v, -np.inf)
            jm = int(np.argmax(vm))
            short = vm[jm] - v[j]
            rounds += 1
            if short > 0:
                off += 1
                ratio = short / (allow[j] + allow[jm])
                worst = max(worst, ratio)
                violations += ratio > 1
            live[j] = False
            pen = np.maximum(pen, sim[:, j])
            e_pen = np.maximum(e_pen, e_sim[:, j])
    return rounds, off, worst, violations


@pytest.mark.parametrize("m,n", SHAPES)
def test_cosine_picks_reach_the_float64_maximum_round_by_round(gauss, m, n):
    from p_companion_amd import ops
    dim, table, dtable, scale, pool = gauss
    idx, sc = pool(m)
    rng = np.random.default_rng(3 * m + n)
    for lam in (0.7, 0.3):
        got = ops.diversify_lists(idx, sc, dtable, n, lam, scale=scale)
        assert same(ops.diversify_lists(*shuffled(rng, idx, sc), dtable, n, lam, scale=scale), got)      # permuted slots
        picks = got[0].cpu().numpy()
        idx_h, sc_h = idx.cpu().numpy(), sc.cpu().numpy()
        # the scores are the picks' input scores
        for r in (0, R // 2, R - 1):
            of = dict(zip(idx_h[r].tolist(), sc_h[r].tolist()))
            assert all(p < 0 or np.float32(of[p]) == s for p, s in zip(picks[r].tolist(), got[1][r].cpu().numpy()))
        rounds, off, worst, violations = teacher_forced(idx_h, sc_h, picks, table, scale.cpu().numpy(), lam, dim)
        print(f"D={dim} m={m} n={n} lam={lam}: {rounds} rounds, {off} not the float64 arg-max, worst shortfall / allowance "
              f"{worst:.3f}")
        assert violations == 0
        assert off <= 0.01 * rounds
        if n == m:
            assert (np.sort(picks, 1) == np.sort(idx_h, 1)).all()


# ---- 4. ops.inv_norm
@pytest.mark.parametrize("dim", DIMS)
def test_inv_norm_against_float64_and_exact_where_it_can_be(dim):
    from p_companion_amd import ops
    rng = np.random.default_rng(40 + dim)
    table = rng.standard_normal((1000, dim)).astype(np.float32)
    table[5] = 0
    table[6] = 0
    table[6, 3] = 4.0                                     # |e|^2 = 16: 1 / 4
    table[7] = 0.25                                       # |e|^2 = D / 16 = 8 or 16 ... a power of four at D = 256 only
    table[8] = 0
    table[8, :4] = [1, -1, 1, 1]                          # |e|^2 = 4
    table[9] = 0
    table[9, dim - 1] = 2.0 ** -7                         # |e|^2 = 4^-7
    got = ops.inv_norm(cuda(table))
    assert torch.equal(bits(ops.inv_norm(cuda(table))), bits(got))
    with np.errstate(divide="ignore"):
        want = 1.0 / np.sqrt((table.astype(np.float64) ** 2).sum(1))
    g = got.cpu().numpy().astype(np.float64)
    keep = np.arange(1000) != 5
    rel = np.abs(g[keep] - want[keep]) / want[keep]
    print(f"inv_norm D={dim}: worst relative error {rel.max():.3e}, bound {(dim + 2) * U:.3e}")
    assert rel.max() <= (dim + 2) * U
    assert g[5] == 0.0
    assert g[6] == 0.25 and g[8] == 0.5 and g[9] == 128.0
    if dim == 256:
        assert g[7] == 0.25
    for rows in (1, 15, 17, 999):                         # every grid: the same bits
        assert torch.equal(bits(ops.inv_norm(cuda(table[:rows]))), bits(got[:rows])), rows


# ---- 5. the C ABI's refusals
def test_c_abi_return_codes():
    from p_companion_amd import _lib
    L = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    m, n, dim = 20, 5, 128
    idx = torch.zeros(R, m, dtype=torch.int32, device="cuda")
    sc = torch.zeros(R, m, device="cuda")
    table = torch.zeros(P + 1, dim, device="cuda")
    out_i = torch.full((R, m), 12345, dtype=torch.int32, device="cuda")
    out_s = torch.full((R, m), 7.0, device="cuda")

    def call(**kw):
        a = dict(idx=p(idx), score=p(sc), rows=R, m=m, table=p(table), scale=None, num_products=P, dim=dim, n=n, lam=0.5,
                 out_idx=p(out_i), out_score=p(out_s), bad=None, stream=st)
        a.update(kw)
        return L.pc_diversify_lists(*a.values())

    for kw in (dict(m=0), dict(m=257), dict(n=0), dict(n=m + 1), dict(dim=64), dict(dim=192), dict(lam=-0.01), dict(lam=1.01),
               dict(lam=float("nan")), dict(rows=-1), dict(num_products=0), dict(idx=None), dict(score=None), dict(table=None),
               dict(out_idx=None), dict(out_score=None), dict(table=ctypes.c_void_p(table.data_ptr() + 4))):
        assert call(**kw) == -2, kw
    assert call(rows=0) == 0 and call(rows=0, idx=None, score=None, out_idx=None, out_score=None) == 0
    torch.cuda.synchronize()
    assert (out_i == 12345).all() and (out_s == 7.0).all()          # nothing was launched
    assert call() == 0 and call(lam=0.0) == 0 and call(lam=1.0) == 0
    norm = torch.empty(P, device="cuda")
    assert L.pc_inv_norm(p(table), P, dim, p(norm), st) == 0
    assert L.pc_inv_norm(None, P, dim, p(norm), st) == -1 and L.pc_inv_norm(p(table), P, dim, None, st) == -1
    assert L.pc_inv_norm(p(table), 0, dim, p(norm), st) == -1 and L.pc_inv_norm(p(table), P, 64, p(norm), st) == -2
    assert L.pc_inv_norm(ctypes.c_void_p(table.data_ptr() + 4), P, dim, p(norm), st) == -2
    torch.cuda.synchronize()


# ---- 6. through PCompanionInference
def test_recommend_diverse_batch():
    from test_gpu_catalogue_eval import cfg
    from p_companion_amd import ops
    from p_companion_amd.data import DeviceBPG, generate_scaled_bpg
    from p_companion_amd.inference import PCompanionInference
    from p_companion_amd.p_companion import PCompanion
    dim = 128
    host = generate_scaled_bpg(20_000, 100, seed=3, dim=dim)
    g = dict(host.cuda())
    g["comp_pairs"] = cuda(host.complementary_pairs.astype(np.int32))
    g["max_degree"] = int(np.diff(host.cv_rowptr).max())
    bpg = DeviceBPG(g, 100, dim)
    c = cfg(100, dim)
    torch.manual_seed(0)
    model = PCompanion(c, torch.randn(bpg.num_products, dim, generator=torch.Generator().manual_seed(11)))
    inf = PCompanionInference(model, c, bpg)
    cv_rowptr, cv_col = host.cv_rowptr, host.cv_col
    q = torch.arange(0, 20_000, 211, dtype=torch.int32)
    mask = torch.rand(20_000, generator=torch.Generator().manual_seed(5)).cuda() < 0.7
    for situation in ("plain", "both"):
        if situation == "both":
            inf.set_exclusions()
            inf.set_eligible(mask)
        for n, pool in ((10, 64), (16, 16), (20, 100)):
            # diversity 0: recommend_batch(n) itself
            want = inf.recommend_batch(q, n)
            got = inf.recommend_diverse_batch(q, n, pool=pool, diversity=0.0)
            assert torch.equal(got[0], want[0]) and same(got[1:], want[1:]), (situation, n, pool)
            # diversity > 0: the composition of recommend_batch(pool) and ops.diversify_lists
            types, p_idx, p_sc = inf.recommend_batch(q, pool)
            b, k, _ = p_idx.shape
            for sim, scale in (("cosine", ops.inv_norm(inf.features)), ("dot", None)):
                got = inf.recommend_diverse_batch(q, n, pool=pool, diversity=0.3, similarity=sim)
                ref = ops.diversify_lists(p_idx.reshape(b * k, pool), p_sc.reshape(b * k, pool), inf.features, n,
                                          1.0 - 0.3, scale=scale)
                assert torch.equal(got[0], types) and got[1].shape == (b, k, n)
                assert same((got[1].reshape(b * k, n), got[2].reshape(b * k, n)), ref), (situation, n, pool, sim)
            idx_h = got[1].cpu().numpy()
            if inf.eligible is not None:
                assert mask[got[1][got[1] >= 0].long()].all()
            if inf.exclusions is not None:
                for i, query in enumerate(q.tolist()):
                    gone = set(cv_col[cv_rowptr[query]:cv_rowptr[query + 1]].tolist()) | {query}
                    assert not set(idx_h[i].reshape(-1).tolist()) & gone, query
        inf.set_exclusions(False)
        inf.set_eligible(None)
    # the diversified lists differ from the relevance order somewhere (the re-rank does something)
    assert not torch.equal(inf.recommend_diverse_batch(q, 10, pool=64, diversity=0.7)[1], inf.recommend_batch(q, 10)[1])
    # a bf16 catalogue: the pool is bounded by what it serves, and the similarity needs the graph's fp32 features
    half = PCompanionInference(model, c, bpg, catalogue=torch.bfloat16)
    with pytest.raises(ValueError, match="fp32 catalogue"):
        half.recommend_diverse_batch(q, 10, pool=17)
    types, p_idx, p_sc = half.recommend_batch(q, 16)
    got = half.recommend_diverse_batch(q, 10, pool=16, diversity=0.3)
    b, k, _ = p_idx.shape
    ref = ops.diversify_lists(p_idx.reshape(b * k, 16), p_sc.reshape(b * k, 16), g["features"], 10, 1.0 - 0.3,
                              scale=ops.inv_norm(g["features"]))
    assert same((got[1].reshape(b * k, 10), got[2].reshape(b * k, 10)), ref)
    no_feat = DeviceBPG({k_: v for k_, v in bpg.arrays.items() if k_ != "features"}, bpg.n_types, bpg.dim)
    given = PCompanionInference(model, c, no_feat, catalogue=half.catalogue.clone())
    with pytest.raises(ValueError, match="without"):
        given.recommend_diverse_batch(q, 10, pool=16)
