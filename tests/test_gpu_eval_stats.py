"""ops.eval_batch_stats (pc_eval_batch_stats: metrics.py:88-109 without the [B*K, B] score matrix) against float64.

The hit counts have no free tolerance.  A device score is the exact-fp32 matrix instruction's k-ordered fmaf chain
(v_mfma_f32_16x16x4_f32), whose error against the exact dot product is at most n u sum|x_i y_i| <= D 2^-24 |x| |y|.  A row's
rank compares TWO such numbers (g_r and s_rc), so with S the float64 scores of the eligible rows and

    eps_r = D * 2^-23 * |proj_r|_2 * max_c |y_c|_2

a column c != r with S_rc > S_rr + eps_r beats row r for sure, one with S_rc < S_rr - eps_r does not for sure, and
the columns in between (amb_r of them) may go either way: lo_r <= beat_r <= lo_r + amb_r, and for every k the device's
hits_k must lie in [#{r: lo_r + amb_r < k}, #{r: lo_r < k}].  The inputs are asserted to make this a real check: the lower end
is at least B / 10 for every k and the interval at most 2 wide.  Needs an MI355X."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def make_inputs(B, K, D, seed):
    """proj, targets standard normal; for every even r < B the target of eligible row r is pulled towards proj_r by
    z_r in [2, 4.5] standard deviations of a score, which spreads the true ranks around the three thresholds."""
    g = torch.Generator().manual_seed(seed)
    proj = torch.randn(B, K, D, generator=g)
    targets = torch.randn(B, D, generator=g)
    z = 2.0 + 2.5 * torch.rand(B, generator=g)
    rows = proj.reshape(B * K, D)[:B]
    pull = z[:, None] * rows / rows.norm(dim=1, keepdim=True)
    even = (torch.arange(B) % 2 == 0)[:, None]
    targets = targets + torch.where(even, pull, torch.zeros_like(pull))
    return proj.contiguous(), targets.contiguous()


def hit_intervals(proj, targets):
    """[(lower, upper)] for k = 1, 3, min(10, B) from float64 scores (any device)."""
    B, K, D = proj.shape
    x = proj.reshape(B * K, D)[:B].double()
    y = targets.double()
    S = x @ y.T
    diag = S.diagonal().clone()
    eps = D * 2.0 ** -23 * x.norm(dim=1) * y.norm(dim=1).max()
    off = ~torch.eye(B, dtype=torch.bool, device=S.device)
    lo = ((S > (diag + eps)[:, None]) & off).sum(1)
    amb = (((S - diag[:, None]).abs() <= eps[:, None]) & off).sum(1)
    out = []
    for k in (1, 3, min(10, B)):
        kk = min(k, B)
        out.append((int((lo + amb < kk).sum()), int((lo < kk).sum())))
    return out


SHAPES = [(4096, 3, 128), (4096, 3, 256), (1000, 3, 128), (133, 3, 128), (203, 3, 128), (203, 3, 256), (256, 1, 128),
          (300, 4, 256), (7, 3, 128), (7, 1, 256)]


@pytest.mark.parametrize("B,K,D", SHAPES)
@pytest.mark.parametrize("seed", [0, 1])
def test_hit_counts_lie_in_the_float64_interval(B, K, D, seed):
    from p_companion_amd import ops
    proj, targets = make_inputs(B, K, D, seed)
    proj, targets = proj.cuda(), targets.cuda()
    iv = hit_intervals(proj, targets)
    for lower, upper in iv:                                           # the check cannot pass vacuously
        assert lower >= B / 10 and upper - lower <= 2, (iv, B)
    types = torch.arange(K, dtype=torch.int32, device="cuda").repeat(B, 1).contiguous()
    stats, _ = ops.eval_batch_stats(proj, targets, targets, types)
    s = stats.cpu().tolist()
    print(f"B={B} K={K} D={D} seed={seed}: hits {s[:3]} intervals {iv}")
    for got, (lower, upper) in zip(s[:3], iv):
        assert lower <= got <= upper, (s, iv)
    assert s[3] == K and s[4] == B


def _exact_counts(x, y):
    """beat_r and hits for integer-valued operands (every product and sum exact in fp32 and in int64)."""
    B = y.shape[0]
    S = x[:B].long() @ y.long().T
    g = S.diagonal()
    c, r = torch.arange(B)[None, :], torch.arange(B)[:, None]
    beat = ((S > g[:, None]) | ((S == g[:, None]) & (c < r))).sum(1)
    return beat, [int((beat < min(k, B)).sum()) for k in (1, 3, min(10, B))]


@pytest.mark.parametrize("B,K,D", [(500, 3, 128), (203, 4, 256), (64, 1, 128), (7, 3, 256)])
def test_exact_ties_go_to_the_lower_index(B, K, D):
    """Small integers make every score exact, so the counts must EQUAL the integer restatement -- with natural ties and
    with planted ones: exact copies of targets[r] at a column below r (beats: the lower index wins a tie) and above r (does
    not); the row never counts itself."""
    from p_companion_amd import ops
    g = torch.Generator().manual_seed(B + D)
    proj = torch.randint(-3, 4, (B, K, D), generator=g).float()
    targets = torch.randint(-3, 4, (B, D), generator=g).float()
    r = B // 2
    targets[r] = proj.reshape(B * K, D)[r] * 2                        # row r's own score is its largest by far ...
    targets[1] = targets[r]                                           # ... tied by a copy below r
    targets[B - 1] = targets[r]                                       # ... and one above
    beat, want = _exact_counts(proj.reshape(B * K, D), targets)
    assert int(beat[r]) == 1                                          # the copy below only
    types = torch.zeros(B, K, dtype=torch.int32, device="cuda")
    stats, _ = ops.eval_batch_stats(proj.cuda(), targets.cuda(), targets.cuda(), types)
    assert stats.cpu().tolist()[:3] == want


@pytest.mark.parametrize("B,K,D", [(300, 3, 128), (70, 2, 256), (7, 3, 128)])
def test_identical_targets_rank_by_index(B, K, D):
    """All columns tie with the row's own score: beat_r = r, so exactly min(k, B) rows hit at k."""
    from p_companion_amd import ops
    g = torch.Generator().manual_seed(3)
    proj = torch.randn(B, K, D, generator=g).cuda()
    targets = torch.randn(1, D, generator=g).repeat(B, 1).contiguous().cuda()
    types = torch.zeros(B, K, dtype=torch.int32, device="cuda")
    stats, _ = ops.eval_batch_stats(proj, targets, targets, types)
    assert stats.cpu().tolist()[:3] == [1, min(3, B), min(10, B)]


def test_distinct_columns():
    from p_companion_amd import ops
    B, D = 50, 128
    g = torch.Generator().manual_seed(0)
    t = torch.randn(B, D, generator=g).cuda()

    def distinct(types):
        k = types.shape[1]
        proj = torch.zeros(B, k, D, device="cuda")
        got = int(ops.eval_batch_stats(proj, t, t, types.to(torch.int32).contiguous().cuda())[0][3])
        assert got == np.unique(types.numpy(), axis=1).shape[1]       # metrics.py:29-42
        return got

    col = torch.randint(0, 1000, (B, 1), generator=g)
    other = torch.randint(1000, 2000, (B, 1), generator=g)
    assert distinct(col.repeat(1, 3)) == 1
    assert distinct(torch.cat([col, other, col], 1)) == 2
    assert distinct(torch.cat([col, other, col + 5000], 1)) == 3
    one_row = col.clone()
    one_row[B - 1] += 1                                               # differs from `col` in the last row only
    assert distinct(torch.cat([col, one_row, col], 1)) == 2
    assert distinct(torch.cat([col, one_row, other, one_row], 1)) == 3
    assert distinct(col) == 1
    wide = torch.cat([col, other, col, one_row, other, col + 1, one_row, col], 1)         # K = 8: 4 distinct
    assert distinct(wide) == 4
    assert distinct(torch.randint(-5, 5, (B, 4), generator=g)) == 4


@pytest.mark.parametrize("B,K,D", [(4096, 3, 128), (203, 4, 256), (7, 1, 128)])
def test_cos_sum_against_float64(B, K, D):
    from p_companion_amd import ops
    g = torch.Generator().manual_seed(9)
    proj = torch.randn(B, K, D, generator=g)
    pos = torch.randn(B, D, generator=g)
    proj[0] = 0.0                                                     # zero rows: the eps path
    pos[min(3, B - 1)] = 0.0
    targets = torch.randn(B, D, generator=g)
    types = torch.zeros(B, K, dtype=torch.int32, device="cuda")
    _, cs = ops.eval_batch_stats(proj.cuda(), targets.cuda(), pos.cuda(), types)
    want = torch.nn.functional.cosine_similarity(proj.double(), pos.double()[:, None, :].expand(B, K, D), dim=2).sum()
    print(f"cos_sum B={B} K={K} D={D}: device {float(cs):.9g} float64 {float(want):.9g}")
    assert abs(float(cs) - float(want)) <= B * K * 1e-6


def test_two_calls_give_identical_bytes():
    from p_companion_amd import ops
    proj, targets = make_inputs(1000, 3, 128, 5)
    proj, targets = proj.cuda(), targets.cuda()
    types = torch.randint(0, 4, (1000, 3), dtype=torch.int32).cuda()
    a = ops.eval_batch_stats(proj, targets, targets, types)
    a = (a[0].clone(), a[1].clone())
    torch.randn(1 << 20, device="cuda")                               # (other work in between)
    b = ops.eval_batch_stats(proj, targets, targets, types)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def test_refusals():
    from p_companion_amd import ops
    z = torch.zeros(16, 3, 128, device="cuda")
    t = torch.zeros(16, 128, device="cuda")
    ty = torch.zeros(16, 3, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        ops.eval_batch_stats(torch.zeros(16, 3, 64, device="cuda"), t[:, :64].contiguous(), t[:, :64].contiguous(), ty)
    with pytest.raises(ValueError):
        ops.eval_batch_stats(z, t[:8].contiguous(), t, ty)
    with pytest.raises(TypeError):
        ops.eval_batch_stats(z, t, t, ty.long())
    with pytest.raises(ValueError):
        ops.eval_batch_stats(torch.zeros(16, 9, 128, device="cuda"), t, t, torch.zeros(16, 9, dtype=torch.int32, device="cuda"))
