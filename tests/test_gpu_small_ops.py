"""Three exported operations of csrc/misc.hip at every launch edge: dense Adam (ops.adam_step / ops.adam_step_at:
adam_prep_kernel, adam_kernel, adam_at_kernel, pc_adam_update / pc_adam_dead of common.h) one step at a time against
torch's single-tensor Adam in fp64 under a derived per-element bound; the hidden-layer dropout (ops.dropout_hidden,
functional.dropout_hidden) bit for bit against philox_oracle's mask; the index check (ops.check_indices) against an
exact numpy count.  Cases, references and the bound: tests/small_op_cases.py (checked on the CPU by
test_small_op_bounds_host.py).  Needs an MI355X."""
import numpy as np
import pytest
import torch

import small_op_cases as so
from test_gpu_building_blocks import bits_equal
from test_gpu_ops import dev, rnd

pytestmark = pytest.mark.gpu

SENTINEL = -7.25
GUARD = 8                   # floats behind every Adam buffer that no launch may touch


@pytest.fixture(scope="module")
def ops():
    from p_companion_amd import ops as o
    assert torch.cuda.is_available()
    return o


def _guarded(x):
    """(a 16-byte aligned device copy of x, the allocation it lies in: GUARD sentinel floats follow it)"""
    n = x.numel()
    whole = torch.full((n + GUARD,), SENTINEL, device="cuda")
    whole[:n].copy_(x)
    view = whole[:n]
    assert view.data_ptr() % 16 == 0
    return view, whole


def _counter(value):
    return torch.tensor([value], dtype=torch.int64, device="cuda")


# ====================================================================================== Adam
def _adam_once(ops, entry, state, g, t, hyper):
    """one step of `entry` from copies of `state` with guard bands: ([p', m', v'], counter after)"""
    lr, b1, b2, eps = hyper
    bufs = [_guarded(x) for x in state]
    gv, gwhole = _guarded(g)
    if entry == "adam_step":
        cnt = _counter(t - 1)
        ops.adam_step(bufs[0][0], gv, bufs[1][0], bufs[2][0], cnt, torch.zeros(2, device="cuda"), lr=lr, betas=(b1, b2), eps=eps)
    else:
        cnt = _counter(-7)
        ops.adam_step_at(bufs[0][0], gv, bufs[1][0], bufs[2][0], cnt, t, lr=lr, betas=(b1, b2), eps=eps)
    n = g.numel()
    for _, whole in bufs:
        assert bool((whole[n:] == SENTINEL).all()), f"{entry}: wrote behind a buffer of {n}"
    assert bits_equal(gwhole[:n], g) and bool((gwhole[n:] == SENTINEL).all())
    return [view for view, _ in bufs], int(cnt)


def _adam_check(ops, state, g, t, hyper, what):
    """both entries from `state` (fp32 device tensors p, m, v): same bits, counter = t, every element inside the bound
    of one step, dead float4 groups untouched bit for bit.  Returns (new state, ratios)."""
    a, cnt_a = _adam_once(ops, "adam_step", state, g, t, hyper)
    b, cnt_b = _adam_once(ops, "adam_step_at", state, g, t, hyper)
    assert cnt_a == t and cnt_b == t, f"{what}: counters {cnt_a}, {cnt_b}"
    for x, y, nm in zip(a, b, "pmv"):
        assert bits_equal(x, y), f"{what}: adam_step and adam_step_at differ in {nm}"
    ratios = so.adam_ratios(*a, *state, g, t, hyper)
    assert max(ratios) <= 1.0, f"{what}: error / bound (p, m, v) = {ratios}"
    dead = so.dead_elements(state[1], state[2], g)
    if bool(dead.any()):
        for x, x0, nm in zip(a, state, "pmv"):
            assert bits_equal(x[dead], x0[dead]), f"{what}: a dead group's {nm} changed"
    return a, ratios


@pytest.mark.parametrize("family,p_mode", so.ADAM_FAMILY_MODES, ids=lambda x: str(x))
def test_adam_single_step(ops, family, p_mode):
    worst = [0.0, 0.0, 0.0]
    for n in so.ADAM_SIZES:
        p, m, v, g = (dev(x) for x in so.adam_inputs(family, p_mode, n))
        if family == "dead_mix" and n >= 8:
            assert bool(so.dead_elements(m, v, g).any())
        for t in so.ADAM_STEPS:
            for hyper in so.ADAM_HYPER:
                _, r = _adam_check(ops, (p, m, v), g, t, hyper, f"{family}-{p_mode}-n{n}-t{t}-lr{hyper[0]}")
                worst = [max(x, y) for x, y in zip(worst, r)]
    print(f"SO_RATIO adam {family} {p_mode} p {worst[0]:.4f} m {worst[1]:.4f} v {worst[2]:.4f}")


@pytest.mark.parametrize("family", ["train", "near_eps", "tiny", "wide", "first", "g0_live"])
def test_adam_rounds_like_the_fp32_restatement(ops, family):
    """pc_adam_update is written with contraction off so that every form of it rounds alike: one correctly rounded fp32
    operation per step of the expression, the scalars rounded from fp64.  numpy's fp32 arithmetic in the same order gives
    the same bits (subnormals included: `tiny`).  The families without dead groups: the restatement skips nothing."""
    n, p_mode = 4099, "zero" if family == "tiny" else "normal"
    state = so.adam_inputs(family, p_mode, n)
    p, m, v, g = (dev(x) for x in state)
    for t in so.ADAM_STEPS:
        for hyper in so.ADAM_HYPER:
            got, _ = _adam_once(ops, "adam_step", (p, m, v), g, t, hyper)
            want = so.adam_restate(*state, t, hyper)
            for x, y, nm in zip(got, want, "pmv"):
                differ = int((x.cpu().view(torch.int32) != y.view(torch.int32)).sum())
                assert differ == 0, f"{family} t={t} lr={hyper[0]}: {differ} of {n} elements of {nm} differ from the restatement"


def test_adam_live_groups_of_dead_mix_update_every_element(ops):
    """A float4 group with ONE non-zero value among its twelve is not dead: the element that carries the value moves (its
    moment decays or takes the gradient in, by far more than the bound), and only a lone v leaves the parameter alone."""
    n, t, hyper = 4099, 1000, so.ADAM_HYPER[0]
    p, m, v, g = (dev(x) for x in so.adam_inputs("dead_mix", "normal", n))
    (p1, m1, v1), _ = _adam_check(ops, (p, m, v), g, t, hyper, "dead_mix live groups")
    full = n - n % 4
    live = ~so.dead_elements(m, v, g)[:full]
    moved = ((m1[:full] != m[:full]) | (v1[:full] != v[:full])).view(-1, 4).any(1)
    assert bool((moved == live.view(-1, 4).all(1)).all())
    carries_g, carries_m, carries_v = (x[:full] != 0 for x in (g, m, v))
    assert bool((p1[:full] != p[:full])[carries_g | carries_m].all())          # the parameter moves with m'
    assert bool((v1[:full] < v[:full])[carries_v].all()) and bool((p1[:full] == p[:full])[carries_v].all())


@pytest.mark.parametrize("n", [1027, 4099])
def test_adam_chain_of_six_steps(ops, n):
    """adam_step six times on its own output, the device counter running 0 -> 6; every step is judged alone from the
    fp32 state the kernel left, so nothing compounds into the bound"""
    hyper = so.ADAM_HYPER[0]
    p = dev(so.adam_inputs("first", "normal", n)[0])
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    cnt, scal = _counter(0), torch.zeros(2, device="cuda")
    for t in range(1, 7):
        g = dev(so.adam_inputs("train", "normal", n, seed=t)[3])
        before = (p.clone(), m.clone(), v.clone())
        ops.adam_step(p, g, m, v, cnt, scal)
        assert int(cnt) == t
        ratios = so.adam_ratios(p, m, v, *before, g, t, hyper)
        print(f"SO_RATIO adam chain n{n} t{t} p {ratios[0]:.4f} m {ratios[1]:.4f} v {ratios[2]:.4f}")
        assert max(ratios) <= 1.0, f"step {t}: error / bound (p, m, v) = {ratios}"
        ss, bc2s = so.adam_scalars(t, hyper)
        assert bits_equal(scal.cpu(), torch.tensor([ss, bc2s], dtype=torch.float64).float())


def _refusal_state(n):
    return [dev(x) for x in so.adam_inputs("train", "normal", n)]      # p, m, v, g


def _unchanged(tensors, before, cnt, value):
    torch.cuda.synchronize()
    return all(bits_equal(x, y) for x, y in zip(tensors, before)) and int(cnt) == value


@pytest.mark.parametrize("which", range(4), ids=["param", "exp_avg", "exp_avg_sq", "grad"])
@pytest.mark.parametrize("n", [7, 1028])
def test_adam_refuses_a_misaligned_buffer(ops, n, which):
    p, m, v, g = _refusal_state(n)
    bufs = [p, m, v, g]
    base = torch.zeros(n + 4, device="cuda")
    base[1:n + 1].copy_(bufs[which])
    bufs[which] = base[1:n + 1]                                        # starts one float into its allocation
    assert bufs[which].data_ptr() % 16 == 4 and bufs[which].is_contiguous()
    before = [x.clone() for x in bufs]
    cnt = _counter(3)
    p, m, v, g = bufs
    with pytest.raises(ops._lib.HipKernelError):
        ops.adam_step(p, g, m, v, cnt, torch.zeros(2, device="cuda"))
    assert _unchanged(bufs, before, cnt, 3)                            # (the counter too: nothing was launched)
    with pytest.raises(ops._lib.HipKernelError):
        ops.adam_step_at(p, g, m, v, cnt, 4)
    assert _unchanged(bufs, before, cnt, 3)
    assert not base[0].item() and not base[n + 1:].any()


@pytest.mark.parametrize("which", range(4), ids=["param", "exp_avg", "exp_avg_sq", "grad"])
def test_adam_refuses_sizes_that_differ(ops, which):
    n = 1028
    bufs = _refusal_state(n)
    bufs[which] = bufs[which][:n - 4].clone()
    before = [x.clone() for x in bufs]
    cnt = _counter(3)
    p, m, v, g = bufs
    with pytest.raises(ValueError):
        ops.adam_step(p, g, m, v, cnt, torch.zeros(2, device="cuda"))
    with pytest.raises(ValueError):
        ops.adam_step_at(p, g, m, v, cnt, 4)
    assert _unchanged(bufs, before, cnt, 3)


@pytest.mark.parametrize("t", [0, -1])
def test_adam_step_at_refuses_step_zero(ops, t):
    bufs = _refusal_state(1027)
    before = [x.clone() for x in bufs]
    cnt = _counter(3)
    p, m, v, g = bufs
    with pytest.raises(ops._lib.HipKernelError):
        ops.adam_step_at(p, g, m, v, cnt, t)
    assert _unchanged(bufs, before, cnt, 3)


# ====================================================================================== hidden dropout
@pytest.mark.parametrize("p", so.DROP_PROBS, ids=lambda p: f"p{p:.7g}")
@pytest.mark.parametrize("offset", so.DROP_OFFSETS)
@pytest.mark.parametrize("seed", so.DROP_SEEDS)
def test_dropout_hidden_is_the_oracle_mask(ops, seed, offset, p):
    for n in so.DROP_SIZES:
        x = so.drop_input(n)
        mask = so.hidden_mask(seed, offset, n, p)
        y = ops.dropout_hidden(dev(x), (p, seed, offset)).cpu()
        assert bits_equal(y, so.drop_expected(x, mask)), f"n = {n}"
        if p == 1e-10:
            assert bits_equal(y, x)                                    # threshold 0, scale exactly 1
        if p > 0.99:
            kept = y != 0
            assert int(kept.sum()) <= 2 and bits_equal(y[kept], x[kept] * 2.0 ** 20)


def test_dropout_hidden_keeps_the_right_fraction(ops):
    n, p, seed, offset = 4 * 4099, 0.1, so.DROP_SEEDS[1], so.DROP_OFFSETS[1]
    y = ops.dropout_hidden(torch.ones(n, device="cuda"), (p, seed, offset)).cpu()
    assert bits_equal(y, torch.from_numpy(so.hidden_mask(seed, offset, n, p).copy()))
    kept = int((y != 0).sum())
    assert abs(kept - n * (1 - p)) <= 4 * (n * p * (1 - p)) ** 0.5


def test_dropout_hidden_mask_follows_the_flat_index(ops):
    B, d = 129, (0.25, so.DROP_SEEDS[0], so.DROP_OFFSETS[1])
    x = dev(so.drop_input(B * 32, seed=1)).view(B, 32)
    y = ops.dropout_hidden(x, d)
    assert y.shape == (B, 32)
    assert bits_equal(y.view(-1), ops.dropout_hidden(x.view(-1), d))
    assert bits_equal(y.view(-1).cpu(), so.drop_expected(x.view(-1).cpu(), so.hidden_mask(d[1], d[2], B * 32, d[0])))


def test_functional_dropout_hidden_forward_and_backward(ops):
    from p_companion_amd import functional
    B, (p, seed, offset) = 129, (0.5, so.DROP_SEEDS[1], so.DROP_OFFSETS[0])
    d = (p, seed, offset)
    x = dev(so.drop_input(B * 32, seed=2)).view(B, 32).requires_grad_(True)
    w = dev(rnd(B, 32, seed=3))
    y = functional.dropout_hidden(x, d)
    assert bits_equal(y.detach(), ops.dropout_hidden(x.detach(), d))
    (y * w).sum().backward()
    assert bits_equal(x.grad, ops.dropout_hidden(w, d))                # w * mask, the same bits as the op on w
    mask = so.hidden_mask(seed, offset, B * 32, p)
    assert bits_equal(x.grad.view(-1).cpu(), so.drop_expected(w.view(-1).cpu(), mask))
    again = functional.dropout_hidden(x, (p, seed, offset + 1)).detach()
    assert not bits_equal(again, y.detach())                           # a fresh mask per offset
    assert bits_equal(again.view(-1).cpu(), so.drop_expected(x.detach().view(-1).cpu(),
                                                            so.hidden_mask(seed, offset + 1, B * 32, p)))


@pytest.mark.parametrize("n", so.DROP_REFUSED_N)
def test_dropout_hidden_refuses_sizes_off_the_group(ops, n):
    with pytest.raises(ops._lib.HipKernelError):
        ops.dropout_hidden(torch.ones(n, device="cuda"), (0.1, 1, 0))


@pytest.mark.parametrize("p", so.DROP_REFUSED_P, ids=lambda p: f"p{p:.10g}")
def test_dropout_hidden_refuses_probabilities_outside_0_1(ops, p):
    with pytest.raises(ValueError):
        ops.dropout_hidden(torch.ones(8, device="cuda"), (p, 1, 0))


# ====================================================================================== index check
def _bad(value=5):
    return torch.tensor([value], dtype=torch.int32, device="cuda")


def _jobs(case):
    return [(dev(arr), hi, allow_pad) for arr, hi, allow_pad, _ in case]


@pytest.mark.parametrize("count", [1, 2, 3, 4])
def test_check_indices_counts_exactly(ops, count):
    for rot in range(so.IDX_ROTATIONS):
        case = so.idx_case(count, rot)
        want = so.idx_bad_count(case)
        jobs, bad = _jobs(case), _bad(5)
        ops.check_indices(jobs, bad)
        assert int(bad) == 5 + want, f"rotation {rot}: lengths {[len(a) for a, *_ in case]}"      # added to, not stored
        ops.check_indices(jobs, bad)
        assert int(bad) == 5 + 2 * want                                # two calls accumulate
        for (arr, *_), (t, *_) in zip(case, jobs):
            assert np.array_equal(t.cpu().numpy(), arr)                # the arrays are only read


@pytest.mark.parametrize("count", [1, 2, 3, 4])
def test_check_indices_leaves_the_counter_on_legal_input(ops, count):
    case = so.idx_legal_case(count)
    assert so.idx_bad_count(case) == 0
    bad = _bad(5)
    ops.check_indices(_jobs(case), bad)
    assert int(bad) == 5


def test_check_indices_refusals(ops):
    ok = dev(np.zeros(4, dtype=np.int32))
    bad = _bad(5)
    with pytest.raises(ValueError):
        ops.check_indices([], bad)
    with pytest.raises(ValueError):
        ops.check_indices([(ok, 3, False)] * 5, bad)
    for hi in (0, -1):
        with pytest.raises(ops._lib.HipKernelError):
            ops.check_indices([(ok, 3, False), (ok, hi, True)], bad)
    torch.cuda.synchronize()
    assert int(bad) == 5
