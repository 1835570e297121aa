"""CPU checks behind tests/test_gpu_small_ops.py: the size and case lists reach the launch edges they are named after,
the Adam bound of small_op_cases.py holds for two correct fp32 evaluations with room and rejects three subtly wrong
ones, the dropout oracle's own mask has the kept fraction it should, and the index-check cases plant every special
value at every place under both allow_pad states."""
import numpy as np
import pytest
import torch

import small_op_cases as so
from oracle import philox_oracle

DEFAULTS, SECOND = so.ADAM_HYPER


# ------------------------------------------------------------------ Adam: the lists cover what they claim
def test_adam_sizes_straddle_the_launch_edges():
    assert {n % 4 for n in so.ADAM_SIZES} == {0, 1, 2, 3}
    assert {1, 2, 3} <= set(so.ADAM_SIZES)                           # no float4 group at all: the tail alone
    assert {n % 4 for n in so.ADAM_SIZES if n > 4} == {0, 1, 2, 3}   # every tail length behind float4 groups
    assert so.adam_launch(1024) == (1, 0, 256) and so.adam_launch(1025) == (2, 1, 1)     # one block | two
    assert so.adam_launch(1023) == (1, 3, 256)                       # the tail thread is the last of a full block
    for n in (1025, 1027, 4099, 65537):                              # the tail thread is alone in its block
        blocks, tail, last = so.adam_launch(n)
        assert n in so.ADAM_SIZES and blocks >= 2 and tail and last == 1
    assert max(so.ADAM_SIZES) <= 70000


def test_adam_case_lists_cover_the_issue():
    assert set(so.ADAM_STEPS) == {1, 2, 1000, 100000}
    assert so.ADAM_HYPER == ((1e-3, 0.9, 0.999, 1e-8), (3e-2, 0.5, 0.9, 1e-6))
    assert len(so.ADAM_FAMILY_MODES) == 13 and ("tiny", "zero") in so.ADAM_FAMILY_MODES
    assert ("tiny", "normal") not in so.ADAM_FAMILY_MODES


def test_adam_families_are_what_they_are_named():
    n = 4099
    p, m, v, g = so.adam_inputs("near_eps", "zero", n)
    root = v.double().sqrt()
    for t in so.ADAM_STEPS:                                          # sqrt(v) / bc2s is of the size of the default eps
        share = root / so.adam_scalars(t, DEFAULTS)[1] / DEFAULTS[3]
        assert 0.5 < float(share.min()) and float(share.max()) < 50
    p, m, v, g = so.adam_inputs("tiny", "zero", n)
    tiny = float(np.finfo(np.float32).tiny)
    assert float(v.max()) < tiny and float(v.min()) > 0 and float((g * g).max()) < tiny and bool((p == 0).all())
    assert float(g.abs().min()) > tiny or float(g.abs().median()) > tiny     # g itself is a normal number
    p, m, v, g = so.adam_inputs("wide", "normal", n)
    assert float(g.abs().quantile(0.95) / g.abs().quantile(0.05)) > 1e6
    p, m, v, g = so.adam_inputs("first", "normal", n)
    assert not m.any() and not v.any() and bool((g != 0).all())
    p, m, v, g = so.adam_inputs("g0_live", "normal", n)
    assert not g.any() and bool((m != 0).all()) and bool((v > 0).all())
    assert not so.dead_elements(m, v, g).any()


@pytest.mark.parametrize("p_mode", so.P_MODES)
def test_dead_mix_interleaves_dead_and_one_of_twelve_groups(p_mode):
    for n in (1023, 1025, 4099):
        p, m, v, g = so.adam_inputs("dead_mix", p_mode, n)
        dead = so.dead_elements(m, v, g)
        groups = n // 4
        assert not dead[4 * groups:].any()
        dg = dead[:4 * groups].view(-1, 4)
        assert bool((dg.all(1) | ~dg.any(1)).all())
        assert bool(dg[0::2].all()) and not dg[1::2].any()           # dead, live, dead, live, ...
        stack = torch.stack([g[:4 * groups].view(-1, 4), m[:4 * groups].view(-1, 4), v[:4 * groups].view(-1, 4)], 1)
        nz = (stack != 0).view(groups, 12)
        assert bool((nz[1::2].sum(1) == 1).all())                    # exactly one of the twelve
        assert set(nz[1::2].int().argmax(1).tolist()) == set(range(12))
        neg0 = lambda x: (x == 0) & torch.signbit(x)
        assert neg0(g)[dead].any() and neg0(m)[dead].any() and neg0(v)[dead].any()
        if p_mode == "zero":
            assert neg0(p)[dead].any()
        if n % 4:
            assert bool((g[4 * groups:] != 0).all())                 # the tail has work to do


# ------------------------------------------------------------------ Adam: the reference is torch's
@pytest.mark.parametrize("family", ["train", "wide", "first"])
def test_adam_ref_is_torch_adam_in_fp64(family):
    p, m, v, g = so.adam_inputs(family, "normal", 1027)
    for t in so.ADAM_STEPS:
        for hyper in so.ADAM_HYPER:
            r = so.adam_ref(p, m, v, g, t, hyper)
            tp, tm, tv = so.adam_torch_fp(p, m, v, g, t, hyper, dtype=torch.float64)
            # (fp64 roundoff of a different but equivalent order of the same expressions)
            assert bool(((tp - r["p"]).abs() <= 1e-14 * (r["p"].abs() + r["delta"].abs())).all())
            assert bool(((tm - r["m"]).abs() <= 1e-14 * (m.double().abs() + g.double().abs())).all())
            assert bool(((tv - r["v"]).abs() <= 1e-14 * r["v"].abs()).all())


# ------------------------------------------------------------------ Adam: the bound cannot reject a correct kernel
ROOM = 0.75            # "with room": a correct evaluation uses at most three quarters of the bound


def _worst(evaluate, n):
    worst = {pm: [0.0, 0.0, 0.0] for pm in so.P_MODES}
    for family, p_mode in so.ADAM_FAMILY_MODES:
        p, m, v, g = so.adam_inputs(family, p_mode, n)
        for t in so.ADAM_STEPS:
            for hyper in so.ADAM_HYPER:
                got = evaluate(p, m, v, g, t, hyper)
                r = so.adam_ratios(*got, p, m, v, g, t, hyper)
                assert max(r) <= ROOM, (family, p_mode, t, hyper, r)
                worst[p_mode] = [max(a, b) for a, b in zip(worst[p_mode], r)]
    return worst


def test_kernel_restatement_stays_inside_the_bound():
    worst = _worst(so.adam_restate, 65537)
    print("SO_RATIO restatement (p, m, v):", {k: [f"{x:.3f}" for x in w] for k, w in worst.items()})


def test_torch_adam_fp32_stays_inside_the_bound():
    worst = _worst(so.adam_torch_fp, 65537)
    print("SO_RATIO torch.optim.Adam fp32 (p, m, v):", {k: [f"{x:.3f}" for x in w] for k, w in worst.items()})


# ------------------------------------------------------------------ Adam: the data bites
BITES = [("eps_inside", "near_eps", 1000, DEFAULTS), ("eps_inside", "near_eps", 1, DEFAULTS),
         ("powf32", "train", 1, DEFAULTS), ("powf32", "train", 2, DEFAULTS),
         ("t_plus_1", "train", 1, DEFAULTS), ("t_plus_1", "first", 1, SECOND),
         ("skip_g0", "g0_live", 1000, DEFAULTS)]


@pytest.mark.parametrize("form,family,t,hyper", BITES, ids=lambda x: str(x))
def test_wrong_forms_miss_the_bound(form, family, t, hyper):
    """A subtly wrong update must be REJECTED on the family named for it: its worst element of p' lies at least twice
    the bound away from the reference (the factors are recorded in small_op_cases.py)."""
    p, m, v, g = so.adam_inputs(family, "zero", 4099)
    right = so.adam_ratios(*so.adam_restate(p, m, v, g, t, hyper), p, m, v, g, t, hyper)
    wrong = so.adam_ratios(*so.adam_restate(p, m, v, g, t, hyper, form=form), p, m, v, g, t, hyper)
    print(f"SO_MISS {form} on {family} t={t} {hyper}: p {wrong[0]:.3g} m {wrong[1]:.3g} v {wrong[2]:.3g} (right: {right[0]:.3f})")
    assert right[0] <= ROOM and wrong[0] >= 2.0


def test_skipping_on_zero_gradient_alone_also_misses_the_moments():
    p, m, v, g = so.adam_inputs("g0_live", "normal", 4099)
    wrong = so.adam_ratios(*so.adam_restate(p, m, v, g, 1, DEFAULTS, form="skip_g0"), p, m, v, g, 1, DEFAULTS)
    assert min(wrong) >= 2.0                                         # p, m and v each


# ------------------------------------------------------------------ hidden dropout
def test_dropout_edge_probabilities():
    f = np.float32
    assert philox_oracle.dropout_threshold(1e-10) == 0               # everything is kept ...
    assert f(1) / (f(1) - f(1e-10)) == f(1)                          # ... and the scale is exactly 1
    hi = 1.0 - 2.0 ** -20
    assert float(f(hi)) == hi and philox_oracle.dropout_threshold(hi) == 2 ** 32 - 2 ** 12
    assert f(1) / (f(1) - f(hi)) == f(2 ** 20)
    assert set(so.DROP_PROBS) == {0.1, 0.5, 0.25, 1e-10, hi}
    for p in so.DROP_REFUSED_P:                                      # what the op sees: the fp32 value
        assert not 0.0 < float(f(p)) < 1.0
    assert min(so.DROP_SEEDS) < 2 ** 32 < max(so.DROP_SEEDS) and min(so.DROP_OFFSETS) < 2 ** 32 < max(so.DROP_OFFSETS)
    assert so.DROP_SIZES == (4, 8, 1020, 1024, 1028, 4 * 4099) and max(so.DROP_SIZES) // 4 <= so.DROP_MAX_GROUPS
    assert all(n % 4 for n in so.DROP_REFUSED_N)


@pytest.mark.parametrize("seed", so.DROP_SEEDS)
@pytest.mark.parametrize("offset", so.DROP_OFFSETS)
def test_oracle_mask_keeps_the_right_fraction(seed, offset):
    n, p = 4 * 4099, 0.1
    mask = so.hidden_mask(seed, offset, n, p)
    scale = np.float32(1) / (np.float32(1) - np.float32(p))
    assert set(np.unique(mask).tolist()) == {0.0, float(scale)}
    kept = int(np.count_nonzero(mask))
    sd = (n * p * (1 - p)) ** 0.5
    print(f"SO_DROP kept {kept} of {n}: {(kept - n * (1 - p)) / sd:+.2f} sd")
    assert abs(kept - n * (1 - p)) <= 4 * sd
    # the high words of seed and offset reach the key and the counter: another mask
    assert not np.array_equal(mask, so.hidden_mask(seed & 0xFFFFFFFF ^ 1, offset, n, p))
    assert not np.array_equal(mask, so.hidden_mask(seed, offset + 1, n, p))
    everything = so.hidden_mask(seed, offset, 1028, 1e-10)
    assert bool((everything == 1.0).all())
    nothing = so.hidden_mask(seed, offset, n, 1.0 - 2.0 ** -20)
    assert set(np.unique(nothing).tolist()) <= {0.0, 2.0 ** 20} and np.count_nonzero(nothing) <= 2


def test_high_words_of_seed_and_offset_matter():
    n = 1028
    low = so.hidden_mask(77, 3, n, 0.5)
    assert not np.array_equal(low, so.hidden_mask((1 << 32) + 77, 3, n, 0.5))
    assert not np.array_equal(low, so.hidden_mask(77, (5 << 32) + 3, n, 0.5))


# ------------------------------------------------------------------ index check
def _all_cases():
    return [(count, rot, so.idx_case(count, rot)) for count in (1, 2, 3, 4) for rot in range(so.IDX_ROTATIONS)]


def test_index_cases_cover_the_issue():
    seen, lengths, longest_at = set(), set(), set()
    for count, rot, jobs in _all_cases():
        assert len(jobs) == count
        ns = [len(a) for a, *_ in jobs]
        assert len(set(ns)) == count                                 # unequal lengths: the grid follows the longest
        longest_at.add((count, ns.index(max(ns))))
        lengths.update(ns)
        for arr, hi, allow_pad, planted in jobs:
            assert arr.dtype == np.int32 and hi > 0
            for place, name in planted.items():
                assert int(arr[so.idx_places(len(arr))[place]]) == so.idx_special(name, hi)
                seen.add((name, place, allow_pad))
    assert lengths == set(so.IDX_LENGTHS)
    for name in so.IDX_SPECIALS:
        for place in so.IDX_PLACES:
            for allow_pad in (False, True):
                assert (name, place, allow_pad) in seen, (name, place, allow_pad)
    for count in (2, 3, 4):                                          # the longest array is not always the first
        assert len({at for c, at in longest_at if c == count}) >= 2
    assert {hi for _, _, jobs in _all_cases() for _, hi, _, _ in jobs} == set(so.IDX_HIS)


def test_index_reference_counts_what_it_should():
    i32 = lambda *xs: np.array(xs, dtype=np.int32)
    assert so.idx_bad_count([(i32(-2, -1, 0, 6, 7, so.I32_MIN, so.I32_MAX), 7, False, {})]) == 5
    assert so.idx_bad_count([(i32(-2, -1, 0, 6, 7, so.I32_MIN, so.I32_MAX), 7, True, {})]) == 4
    assert so.idx_bad_count([(i32(so.I32_MAX - 1, so.I32_MAX), so.I32_MAX, False, {})]) == 1
    assert so.idx_bad_count([(i32(-1), 1, True, {}), (i32(-1), 1, False, {})]) == 1
    counts = [so.idx_bad_count(jobs) for _, _, jobs in _all_cases()]
    assert sum(c > 0 for c in counts) >= len(counts) - 4 and len(set(counts)) > 10       # (a lone legal entry: n = 1)
    for count in (1, 2, 3, 4):
        legal = so.idx_legal_case(count)
        assert so.idx_bad_count(legal) == 0 and any(-1 in a for a, *_ in legal)
