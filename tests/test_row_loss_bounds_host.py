"""CPU checks behind tests/test_gpu_row_losses.py (row_loss_cases.py holds the lists, the float64 references, the bounds and
the checkers).  Three things: the case lists cover what they claim; the bounds cannot reject a correct kernel -- numpy fp32
restatements of every kernel in three summation orders (sequential, reversed, per lane and then by halving as the kernels add)
pass every check at HALF of every bound and make the float64 hinge decision on every decided sample; and the inputs can
reject a wrong kernel -- every mutated restatement fails the same checkers on at least one case."""
import numpy as np
import pytest

import row_loss_cases as rl


# ------------------------------------------------------------------ the lists cover what they claim
def test_triplet_cases_cover_every_k_every_batch_residue_and_every_planted_sample():
    for dim in (128, 256):
        cases = [c for c in rl.TRIPLET_CASES if c[0] == dim]
        assert {c[2] for c in cases} == set(range(1, 9))
        assert {c[1] for c in cases} == set(rl.TRIPLET_B)
        per = 16 if dim == 128 else 4                              # samples per workgroup
        bs = {c[1] for c in cases}
        assert {b % per for b in bs} >= ({0, 1, per - 1} if dim == 128 else {0, 1, 3})
        assert any(b < per for b in bs) and any(b > 256 and b % 256 for b in bs) and 256 in bs       # the mean strides by 256
        assert {kind for c in cases if c[1] == 1 for kind in rl.plant_rows(1, c[3])} == set(rl.PLANTS)
        for c in cases:
            rows = rl.plant_rows(c[1], c[3])
            assert len(set(rows.values())) == len(rows) == min(c[1], 5) and max(rows.values()) < c[1]
            if c[1] >= 15:
                assert set(rows) == set(rl.PLANTS) and rows["dpos0"] == c[1] - 1
    for c in rl.TRIPLET_CASES:                                     # the planted rows are what their names say
        a, p, n, rows = rl.triplet_inputs(c)
        x = (a - p) + rl.EPS32
        y = (a[:, None] - n) + rl.EPS32
        if "eps" in rows:
            assert (x[rows["eps"]] == rl.EPS32).all() and (y[rows["eps"], 0] == rl.EPS32).all()
        if "dpos0" in rows:
            assert not x[rows["dpos0"]].any()
        if "neg0" in rows:
            assert not y[rows["neg0"], c[2] - 1].any() and x[rows["neg0"]].any()


def test_joint_cases_cover_the_listed_shapes():
    cs = rl.JOINT_CASES
    assert {c[0] for c in cs} == {128, 256} and {c[2] for c in cs} == {1, 2, 3, 8}
    assert {c[1] for c in cs} == {1, 3, 4, 5, 64, 257, 513} and {c[3] for c in cs} == {1, 2, 65, 300}
    assert {c[4] for c in cs} == {0.0, 0.5, 0.8, 1.0}
    for dim in (128, 256):
        assert {c[4] for c in cs if c[0] == dim} == {0.0, 0.5, 0.8, 1.0}
    assert all(c[1] < 32 for c in cs if c[3] == 1)
    assert {kind for c in cs if c[1] == 1 for kind in rl.joint_plant_rows(1, c[5]).values()} == set(rl.JOINT_PLANTS)
    for c in cs:
        sims, proj, pos_t, neg_t, pos, neg = rl.joint_inputs(c)
        t = c[3]
        assert pos_t.min() >= 0 and neg_t.min() >= 0 and pos_t.max() < t and neg_t.max() < t
        if c[1] >= 5:
            assert {0, t - 1} <= set(pos_t.tolist()) and {0, t - 1} <= set(neg_t.tolist()) and (pos_t == neg_t).any()
    assert {(c[1], c[2]) for c in rl.EXACT_CASES} == {(b, k) for b in (64, 512) for k in (1, 2, 4, 8)}
    assert {c[0] for c in rl.EXACT_CASES} == {128, 256}
    for c in rl.EXACT_CASES:
        sims, proj, pos_t, neg_t, pos, neg = rl.exact_inputs(c)
        assert (sims == np.round(sims)).all()
        for d in (proj - pos[:, None], proj - neg[:, None]):
            assert set(np.unique(d).tolist()) <= {-1.0, 0.0, 1.0}
            assert set(np.unique(np.abs(d).sum(-1)).tolist()) <= {0.0, 4.0, 16.0, 64.0}


def test_hit_rank_and_cosine_cases_cover_the_listed_shapes():
    assert rl.HIT_SHAPES == [(1, 1), (5, 3), (3, 5), (64, 64), (65, 65), (67, 130), (130, 67), (259, 1000)]
    s = rl.hit_inputs((67, 130))
    assert np.isposinf(s).any() and np.isneginf(s).any() and np.signbit(s[s == 0]).any() and not np.signbit(s[s == 0]).all()
    assert not np.isnan(s).any()
    ties = sum(int((s[r] == s[r, r]).sum()) - 1 for r in range(67))
    assert ties > 67                                               # the tie rule decides in most rows
    assert rl.hit_expected(rl.hit_inputs((130, 67)))[67:].tolist() == [rl.NEVER] * 63
    cs = rl.COSINE_CASES
    assert {c[0] for c in cs} == {128, 256} and {c[1] for c in cs} == {1, 5, 67} and {c[2] for c in cs} == {1, 3, 8}
    assert any(c[1] * c[2] % 4 for c in cs)
    for c in cs:
        x, y = rl.cosine_exact_inputs(c)
        assert set(np.unique(x).tolist()) <= {-1.0, 0.0, 1.0} and set(np.unique(y).tolist()) <= {-1.0, 0.0, 1.0}
        assert set(np.abs(x).sum(-1).ravel().tolist()) <= {0.0, 4.0, 16.0, 64.0}
        assert set(np.abs(y).sum(-1).tolist()) <= {0.0, 4.0, 16.0, 64.0}


# ------------------------------------------------------------------ the bounds cannot reject a correct kernel
@pytest.mark.parametrize("order", rl.ORDERS)
def test_restated_triplet_kernels_stay_within_half_of_every_bound(order):
    run = rl.triplet_restated(order)
    worst = {}
    for c in rl.TRIPLET_CASES:
        for name, r in rl.check_triplet(c, run, frac=0.5).items():
            worst[name] = max(worst.get(name, 0.0), r)
    print(order, {k: round(v, 3) for k, v in worst.items()})


@pytest.mark.parametrize("order", rl.ORDERS)
def test_restated_joint_kernels_stay_within_half_of_every_bound(order):
    run = rl.joint_restated(order)
    worst = {}
    for c in rl.JOINT_CASES:
        for name, r in rl.check_joint(c, run, rl.expand_restated, frac=0.5).items():
            worst[name] = max(worst.get(name, 0.0), r)
    print(order, {k: round(v, 3) for k, v in worst.items()})
    for c in rl.EXACT_CASES:
        rl.check_joint_exact(c, run, rl.expand_restated)


@pytest.mark.parametrize("order", rl.ORDERS)
def test_restated_cosine_and_hit_rank_pass(order):
    run = rl.cosine_restated(order)
    print(order, round(max(rl.check_cosine(c, run, frac=0.5) for c in rl.COSINE_CASES), 3))
    for shape in rl.HIT_SHAPES:
        rl.check_hit_rank(shape, rl.hit_restated())


# ------------------------------------------------------------------ the inputs can reject a wrong kernel
def _rejected(check, cases):
    hits = 0
    for c in cases:
        try:
            with np.errstate(all="ignore"):                        # (a mutant without the guard divides by zero on purpose)
                check(c)
        except AssertionError:
            hits += 1
    return hits


@pytest.mark.parametrize("mutant", rl.TRIPLET_MUTANTS)
def test_mutated_triplet_kernel_is_rejected(mutant):
    """eps dropped; d- as sum / (K + 1); relu'(0) = 1; the dn sign flipped; the zero-distance guard removed (NaN)"""
    run = rl.triplet_restated("tree", mutant)
    hits = _rejected(lambda c: rl.check_triplet(c, run), rl.TRIPLET_CASES)
    print(mutant, "rejected on", hits, "of", len(rl.TRIPLET_CASES))
    assert hits >= 1


@pytest.mark.parametrize("mutant", rl.JOINT_MUTANTS)
def test_mutated_joint_kernel_is_rejected(mutant):
    """item gradient scaled alpha / B; type gradient scaled alpha instead of 1 - alpha; the zero-norm guard removed (NaN)"""
    run = rl.joint_restated("tree", mutant)
    hits = _rejected(lambda c: rl.check_joint(c, run, rl.expand_restated), rl.JOINT_CASES)
    hits += _rejected(lambda c: rl.check_joint_exact(c, run, rl.expand_restated), rl.EXACT_CASES)
    print(mutant, "rejected on", hits, "of", len(rl.JOINT_CASES) + len(rl.EXACT_CASES))
    assert hits >= 1


def test_mutated_tie_rule_and_cosine_clamp_are_rejected():
    assert _rejected(lambda s: rl.check_hit_rank(s, rl.hit_restated("tie_rule_le")), rl.HIT_SHAPES) == len(rl.HIT_SHAPES)
    assert _rejected(lambda c: rl.check_cosine(c, rl.cosine_restated("tree", "clamp_on_product")), rl.COSINE_CASES) >= 1
