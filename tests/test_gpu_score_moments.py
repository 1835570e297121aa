"""Score moments (pc_score_moments_grouped / pc_score_moments_grouped_bf16; ops.score_moments_grouped, ops.standardise_scores;
PCompanionInference.score_moments and normalise="zscore").  Needs an MI355X.

The reference is never the code under test: float64 over the score bits the existing list entry returned, float64 dot products
under a derived bound, or exact integers.  u = 2^-24 throughout.

THE ACCUMULATION BOUND (checks (a), (b), (d)).  A sum of n fp32 terms t_i, added in any order, is a tree with at most n - 1
additions of two non-zero operands (adding a zero is exact), so a term passes at most n - 1 roundings and
    |fl(sum t_i) - sum t_i|  <=  ((1 + u)^(n-1) - 1) sum|t_i|  <=  n u sum|t_i|
to first order; where n (n - 1) u > 1 (n > 4096) the second inequality still holds for this kernel, because a term there passes
at most ceil(n / 64) + 4 + 3 + 63 < n / 2 additions (its lane's chunks, the 16-lane butterfly, the waves, the slices).  The
squares: s2 = fma(d, d, s2) rounds once per addition and the product not at all; the issue's allowance of one more rounding per
term is kept, (n + 1) u sum d^2.

(a) starts from the list's own score bits s (fp32) and the pivot's g: d = fl32(s - g) is the device's own subtraction, bit for
bit, so  |s1 - sum d| <= n u sum|d|  and  |s2 - sum d^2| <= (n + 1) u sum d^2  with the sums in float64 -- the chain's rounding
is on neither side.

(b) starts from float64 dot products s64 with the per-score allowance a_p of tests/test_gpu_nearest.py (fp32: (D + 2) u
sum_d|q_d e_pd|) and tests/test_gpu_rank_bf16.py (bf16: (3 D + 4) u ...), |s_p - s64_p| <= a_p.  With x_p = s64_p - s64_g (g the
pivot), the device's d_p = fl(s_p - g) = x_p + eta_p with |eta_p| <= h_p = a_p + a_g + u (|x_p| + a_p + a_g), |d_p| <= |x_p| + h_p.
  mean:  g + S1 / n in exact arithmetic is (1/n) sum s_p: the pivot's own error cancels.  So
         |mean - mu| <= m + u (|xbar| + a_g + m) + u (|mu| + m),   m = (sum a_p + (n + 1) u sum(|x_p| + h_p)) / n
         (the chain; one rounding per subtraction and the accumulation; the division; the final addition).
  std:   sigma^2 = (1/n) sum x_p^2 - xbar^2 for any pivot.  |sum d_p^2 - sum x_p^2| <= sum(2 |x_p| h_p + h_p^2) = E2, the
         accumulation adds (n + 1) u sum(|x_p| + h_p)^2, the division u times the quotient: eA.  m1 = fl(S1 / n) misses xbar by
         em = ES1 / n + u (|xbar| + ES1 / n), ES1 = sum h_p + n u sum(|x_p| + h_p); its square misses xbar^2 by
         eB = 2 |xbar| em + em^2 + u (|xbar| + em)^2.  The subtraction: ev = eA + eB + u (sigma^2 + eA + eB).  The square root:
         |sqrt(v) - sigma| <= min(ev / sigma, sqrt(ev)), and one more rounding.
Both bounds carry a factor 1 + 2^-10 for the second-order terms dropped above.  Nothing in them comes from the device.

Figures of one MI355X run (worst |error| / bound; gate: <= 1), printed again by every run:  (a) s1 0.31, s2 0.33;  (b) mean
0.0084, std 0.0021 over all rows, slices, tables and both D;  (d) std 0.0001 (fp32 table), the uncentred fp32 form 0.9 .. 23.9
times the bound, outside it on 39 of 40 rows (bf16 table, whose bound is four times wider: 33 of 40);  (f) with set_eligible
0.0019.

The catalogue of (a), (b): tests/test_gpu_where_rank.py's -- 20 000 products, type 0 above 10 000 (many chunks, real slices),
type 6 about 3 000, types of about 300, type 7 of 40, types 3 and 4 of 3, type 5 the 30 tied copies (of THREE rows: its scores
take three values, so its s1 / s2 are not zero; the all-alike type of (e) is one row copied 30 times), empty types; 203 rows, a
partial last tile, 1 to 4 row groups per tile, rows of type -1 and T."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_nearest as f32ref
import test_gpu_rank_bf16 as bf16ref
from test_gpu_nearest import dev
from test_gpu_retrieval_grouped import host_csr, mixed_catalogue, mixed_rows, upload

U = 2.0 ** -24
SLICES = (0, 1, 2, 64)
SLACK = 1 + 2.0 ** -10
FIELDS = ("count", "mean", "std", "pivot", "s1", "s2")


def catalogue(dim):
    """tests/test_gpu_where_rank.py's catalogue and rows, from the same generators"""
    type_idx, features, T = mixed_catalogue(20_000, dim, seed=dim)
    type_idx[type_idx >= 30] = 6
    seven = np.nonzero(type_idx == 7)[0]
    type_idx[seven[40:]] = 6
    sizes = np.bincount(type_idx, minlength=T)
    assert sizes[0] > 10_000 and 2_500 < sizes[6] < 3_600 and sizes[7] == 40 and 200 < sizes[8] < 400
    assert sizes[3] == sizes[4] == 3 and sizes[5] == 30 and sizes[1] == sizes[2] == sizes[35] == 0
    types = mixed_rows(203, T, seed=dim)
    types[(types >= 30) & (types < T)] = 6
    types[8:12] = 7
    assert types[0] == -1 and types[1] == T
    proj = np.random.default_rng(7).standard_normal((203, dim)).astype(np.float32)
    return type_idx, features, T, types, proj


def view(t, r):
    """(cand ascending, s64, allowance) of row r of a table fixture"""
    if hasattr(t, "rounded"):
        return bf16ref.view(t, r, None)
    return f32ref.row_view(t, r, np.zeros(t.P, np.float32))


def moment_reference(s64, allow):
    """(mu, sigma, bound on |mean - mu|, bound on |std - sigma|) of one row from its float64 scores and per-score allowances, the
    pivot first: the module docstring's derivation, line by line."""
    n = len(s64)
    ag = allow[0]
    x = s64 - s64[0]
    mu, sigma, xbar = s64.mean(), s64.std(), x.mean()
    h = allow + ag + U * (np.abs(x) + allow + ag)
    absd = np.abs(x) + h
    m = (allow.sum() + (n + 1) * U * absd.sum()) / n
    b_mean = m + U * (abs(xbar) + ag + m) + U * (abs(mu) + m)
    es2 = (2 * np.abs(x) * h + h * h).sum() + (n + 1) * U * (absd ** 2).sum()
    e_a = es2 / n + U * ((x * x).sum() + es2) / n
    es1 = h.sum() + n * U * absd.sum()
    em = es1 / n + U * (abs(xbar) + es1 / n)
    e_b = 2 * abs(xbar) * em + em * em + U * (abs(xbar) + em) ** 2
    ev = e_a + e_b
    ev += U * (sigma ** 2 + ev)
    es = min(ev / sigma, np.sqrt(ev)) if sigma > 0 else np.sqrt(ev)
    return mu, sigma, b_mean * SLACK, (es + U * (sigma + es)) * SLACK


def references(t, R):
    """Per row: count, mu, sigma and the two bounds (zeros for a row without candidates); the pivot is the type's first
    candidate, which is the lowest product id (the CSR is in ascending node order)."""
    ref = SimpleNamespace(count=np.zeros(R, np.int64), mu=np.zeros(R), sigma=np.zeros(R), b_mean=np.zeros(R), b_std=np.zeros(R))
    for r in range(R):
        cand, s64, allow = view(t, r)
        if len(cand):
            assert cand[0] == cand.min()
            ref.count[r] = len(cand)
            ref.mu[r], ref.sigma[r], ref.b_mean[r], ref.b_std[r] = moment_reference(s64, allow)
    return ref


def moments(t, slices=0, col=None, bad=None):
    from p_companion_amd import ops
    return ops.score_moments_grouped(t.dproj, t.dtypes, t.rowptr, t.col if col is None else col, t.table, slices=slices, bad=bad)


def host(m):
    return SimpleNamespace(bad=int(m.bad), **{f: getattr(m, f).cpu().numpy() for f in FIELDS})


def same_bits(a, b):
    return all(torch.equal(getattr(a, f).view(torch.int32), getattr(b, f).view(torch.int32)) for f in FIELDS)


def tables(dim, type_idx, features, T, types, proj):
    return SimpleNamespace(dim=dim, R=len(types), T=T, types=types, type_idx=type_idx,
                           fp32=f32ref.fixture_from(dim, type_idx, features, T, types, proj),
                           bf16=bf16ref.fixture_from(dim, type_idx, features, T, types, proj))


@pytest.fixture(scope="module", params=[128, 256], ids=lambda d: f"D{d}")
def mixed(request):
    m = tables(request.param, *catalogue(request.param))
    m.fp32.ref, m.bf16.ref = references(m.fp32, m.R), references(m.bf16, m.R)
    return m


EDGE_SIZES = (0, 1, 2, 15, 16, 17, 63, 64, 65, 129)
EDGE_ROWS = {9: 65, 8: 64, 7: 17, 6: 16, 5: 1}              # type -> rows of it: tiles of 65, 64, 17, 16 and 1 rows
TIED = len(EDGE_SIZES)                                        # the all-alike type: one row copied 30 times


@pytest.fixture(scope="module", params=[128, 256], ids=lambda d: f"D{d}")
def edges(request):
    """Types of 0, 1, 2, 15, 16, 17, 63, 64, 65 and 129 products and one of 30 copies of one row; 65, 64, 17, 16 rows and one row
    of one type (at D = 256 a tile holds 32 rows: two tiles, and two and one row), two rows of every other type, a row of type -1
    and one of type T."""
    dim = request.param
    rng = np.random.default_rng(100 + dim)
    T = TIED + 1
    type_idx = np.concatenate([np.full(n, t, np.int32) for t, n in enumerate(EDGE_SIZES)] + [np.full(30, TIED, np.int32)])
    type_idx = type_idx[rng.permutation(len(type_idx))]
    features = rng.standard_normal((len(type_idx), dim)).astype(np.float32)
    tied = np.nonzero(type_idx == TIED)[0]
    features[tied] = features[tied[0]]
    types = np.concatenate([[-1, T]] + [np.full(EDGE_ROWS.get(t, 2), t, np.int32) for t in range(T)]).astype(np.int32)
    types[2:] = types[2:][rng.permutation(len(types) - 2)]
    proj = rng.standard_normal((len(types), dim)).astype(np.float32)
    return tables(dim, type_idx, features, T, types, proj)


def check_against_the_lists(m, t, got, most=256):
    """(a) for every row whose type holds at most `most` products; returns the worst error / bound seen (s1, s2)"""
    from p_companion_amd import ops
    idx, sc = ops.retrieve_list_grouped(t.dproj, t.dtypes, t.rowptr, t.col, t.table, 256)
    idx, sc = idx.cpu().numpy(), sc.cpu().numpy()
    rowptr, col = t.rowptr.cpu().numpy(), t.col.cpu().numpy()
    worst, rows = [0.0, 0.0], 0
    for r, ty in enumerate(m.types):
        n = int(rowptr[ty + 1] - rowptr[ty]) if 0 <= ty < m.T else 0
        if n == 0:
            assert got.count[r] == 0 and not any(getattr(got, f)[r] for f in FIELDS[1:]), r
            continue
        if n > most:
            continue
        rows += 1
        assert got.count[r] == n and (idx[r, :n] >= 0).all() and (idx[r, n:] == -1).all(), r
        first = np.nonzero(idx[r, :n] == col[rowptr[ty]])[0]
        assert len(first) == 1
        g = sc[r, first[0]]
        assert got.pivot[r].view(np.int32) == g.view(np.int32), f"row {r}: the pivot is not the list's score of the first candidate"
        d = (sc[r, :n] - g).astype(np.float32).astype(np.float64)             # fl32(s - g): the device's own subtraction
        for k, (have, want, bound) in enumerate(((got.s1[r], d.sum(), n * U * np.abs(d).sum()),
                                                 (got.s2[r], (d * d).sum(), (n + 1) * U * (d * d).sum()))):
            err = abs(float(have) - want)
            assert err <= bound, f"row {r} (type {ty}, n {n}): s{k + 1} off by {err:.3e}, bound {bound:.3e}"
            if bound:
                worst[k] = max(worst[k], err / bound)
        # the derived values are the contract's arithmetic on s1 / s2, one fp32 rounding per operation
        f = np.float32
        m1 = f(got.s1[r]) / f(n)
        assert got.mean[r].view(np.int32) == f(f(g) + m1).view(np.int32), r
        var = f(f(got.s2[r]) / f(n)) - f(m1 * m1)
        assert got.std[r].view(np.int32) == np.sqrt(np.maximum(f(var), f(0))).astype(f).view(np.int32), r
    assert rows >= 10
    return worst


# ---- (a) small types against the list's own bits
@pytest.mark.parametrize("table", ["fp32", "bf16"])
def test_small_types_against_the_lists_own_score_bits(mixed, table):
    """The rows of types 3, 4 (3 products), 5 (30: copies of three rows) and 7 (40); the edge sizes are (e)'s."""
    t = getattr(mixed, table)
    worst = check_against_the_lists(mixed, t, host(moments(t)))
    print(f"(a) D{mixed.dim} {table}: worst s1 {worst[0]:.4f}, s2 {worst[1]:.4f} of the bound")


# ---- (b) every row against float64 dot products, every slices
@pytest.mark.parametrize("table", ["fp32", "bf16"])
def test_every_row_against_float64_for_every_slices(mixed, table):
    t = getattr(mixed, table)
    ref = t.ref
    worst = [0.0, 0.0]
    for slices in SLICES:
        got = host(moments(t, slices))
        assert got.bad == 1                                                   # the row of type T, and only it
        assert (got.count == ref.count).all()
        none = ref.count == 0
        assert none[0] and none[1] and none[2] and none[3]                    # type -1, type T, the empty types 1 and 2
        for f in FIELDS:
            assert (getattr(got, f)[none] == 0).all(), f
        live = ~none
        e_mean, e_std = np.abs(got.mean - ref.mu), np.abs(got.std - ref.sigma)
        bad = np.nonzero(live & ((e_mean > ref.b_mean) | (e_std > ref.b_std)))[0]
        assert not len(bad), (f"slices {slices}, rows {bad[:5]}: mean off by {e_mean[bad[:5]]} (bound {ref.b_mean[bad[:5]]}), "
                              f"std off by {e_std[bad[:5]]} (bound {ref.b_std[bad[:5]]})")
        worst[0] = max(worst[0], (e_mean[live] / ref.b_mean[live]).max())
        worst[1] = max(worst[1], (e_std[live] / ref.b_std[live]).max())
    print(f"(b) D{mixed.dim} {table}: worst mean {worst[0]:.4f}, std {worst[1]:.4f} of the bound")


# ---- (c) exact data
def test_exact_data_is_the_exact_integers_for_every_slices_table_and_candidate_order(mixed):
    """Features in {-1, 0, 1} and sparse queries in {-1, 0, 1}: every score, difference, square and partial sum is an integer
    below 2^24 (asserted), on the bf16 table too, so pivot, s1 and s2 are the exact integers whatever the order of the sums."""
    dim, T, types, type_idx = mixed.dim, mixed.T, mixed.types, mixed.type_idx
    rng = np.random.default_rng(41)
    features = rng.integers(-1, 2, (len(type_idx), dim)).astype(np.float32)
    proj = (rng.integers(-1, 2, (len(types), dim)) * (rng.random((len(types), dim)) < 0.25)).astype(np.float32)
    rowptr, col, table = upload(type_idx, features, T)
    hrow, hcol = host_csr(type_idx, T)
    want = {f: np.zeros(len(types), np.int64) for f in ("count", "pivot", "s1", "s2")}
    fi, pi = features.astype(np.int64), proj.astype(np.int64)
    for r, ty in enumerate(types):
        if not 0 <= ty < T or hrow[ty] == hrow[ty + 1]:
            continue
        s = fi[hcol[hrow[ty]:hrow[ty + 1]]] @ pi[r]
        d = s - s[0]
        assert np.abs(d).sum() < 2 ** 24 and (d * d).sum() < 2 ** 24 and np.abs(s).max() < 2 ** 24
        want["count"][r], want["pivot"][r], want["s1"][r], want["s2"][r] = len(s), s[0], d.sum(), (d * d).sum()
    assert want["s2"].max() > 2 ** 17 and (want["count"] > 10_000).any()      # sums of many terms, not of a handful
    # type_col permuted inside each type, its first entry in place: the same pivot, other lanes and slices for the rest
    perm = hcol.copy()
    for ty in range(T):
        lo, hi = hrow[ty], hrow[ty + 1]
        if hi - lo > 2:
            perm[lo + 1:hi] = perm[lo + 1:hi][rng.permutation(hi - lo - 1)]
    assert (perm != hcol).sum() > 10_000
    base = None
    for tab, c in ((table, col), (table.to(torch.bfloat16), col), (table, dev(perm)), (table.to(torch.bfloat16), dev(perm))):
        t = SimpleNamespace(dproj=dev(proj), dtypes=dev(types), rowptr=rowptr, col=c, table=tab)
        for slices in SLICES:
            m = moments(t, slices)
            got = host(m)
            for f in ("count", "pivot", "s1", "s2"):
                assert (getattr(got, f).astype(np.float64) == want[f]).all(), (f, tab.dtype, slices)
            base = base or m
            assert same_bits(m, base), (tab.dtype, slices)                    # mean and std too: the same bits everywhere


# ---- (d) off-centre scores
@pytest.mark.parametrize("table", ["fp32", "bf16"])
def test_off_centre_scores_keep_their_spread(table):
    """A type of 5 000 rows = a common offset of length 2^10 plus unit noise, 40 queries along the offset: |mean| / std is about
    2^10 for every row.  std meets (b)'s bound.  The uncentred form sum s^2 - (sum s)^2 / n on the SAME data -- numpy fp32 over
    the float64 scores rounded to fp32, accumulated one candidate after another as one accumulator would -- misses it: at
    |mean| / std = 2^10 the two sums agree in their first 20 bits and fp32 has 24.  (numpy's pairwise np.sum of the same terms
    is printed beside it, not asserted: its last-bit luck decides.)"""
    dim, n, R = 128, 5_000, 40
    rng = np.random.default_rng(17)
    unit = np.ones(dim) / np.sqrt(dim)
    features = (1024.0 * unit + rng.standard_normal((n + 1_000, dim))).astype(np.float32)
    type_idx = np.zeros(n + 1_000, np.int32)
    type_idx[n:] = 1
    features[n:] = rng.standard_normal((1_000, dim))
    alpha = rng.uniform(0.5, 2.0, R)
    proj = (alpha[:, None] * (unit + 0.02 * rng.standard_normal((R, dim)) / np.sqrt(dim))).astype(np.float32)
    types = np.zeros(R, np.int32)
    make = bf16ref.fixture_from if table == "bf16" else f32ref.fixture_from
    t = make(dim, type_idx, features, 2, types, proj)
    ref = references(t, R)
    ratio = np.abs(ref.mu) / ref.sigma
    assert (ratio > 2 ** 9.5).all() and (ratio < 2 ** 10.5).all()
    got = host(moments(t))
    e_std, e_mean = np.abs(got.std - ref.sigma), np.abs(got.mean - ref.mu)
    assert (e_std <= ref.b_std).all() and (e_mean <= ref.b_mean).all(), (e_std / ref.b_std).max()
    print(f"(d) {table}: worst std {(e_std / ref.b_std).max():.4f}, mean {(e_mean / ref.b_mean).max():.4f} of the bound; "
          f"relative std error {(e_std / ref.sigma).max():.2e}, bound {(ref.b_std / ref.sigma).max():.2e}")
    f = np.float32
    naive, pairwise = np.zeros(R), np.zeros(R)
    for r in range(R):
        s = view(t, r)[1].astype(f)                                           # the same data: the reference's scores in fp32
        a, b = np.cumsum(s * s, dtype=f)[-1], np.cumsum(s, dtype=f)[-1]
        naive[r] = np.sqrt(max(f(f(a) - f(f(b * b) / f(n))) / f(n), 0))
        a, b = (s * s).sum(dtype=f), s.sum(dtype=f)
        pairwise[r] = np.sqrt(max(f(f(a) - f(f(b * b) / f(n))) / f(n), 0))
    miss = np.abs(naive - ref.sigma) / ref.b_std
    print(f"(d) {table}: the uncentred fp32 form misses the bound by a factor {miss.min():.1f} .. {miss.max():.1f} "
          f"(pairwise np.sum: {(np.abs(pairwise - ref.sigma) / ref.b_std).max():.1f})")
    # The uncentred error is a random walk of about n / 2 roundings of size ulp(n mean^2) / sqrt(12): about n sigma^2 itself, a
    # relative error of the variance of order 1 against a bound of a few per cent -- so a row lands inside the bound by chance
    # about one time in twenty on the fp32 table and, under the bf16 table's four times wider bound, about one time in five.
    # Three rows in four must miss.
    assert (miss > 1).mean() >= 0.75, "the data does not bite: the uncentred form is inside the bound"


# ---- (e) edges
@pytest.mark.parametrize("table", ["fp32", "bf16"])
def test_type_sizes_and_rows_per_type_at_every_edge(edges, table):
    from p_companion_amd import ops
    t = getattr(edges, table)
    m = moments(t)
    got = host(m)
    check_against_the_lists(edges, t, got)
    assert got.bad == 1                                                       # the row of type T; the row of type -1 is skipped
    assert edges.types[0] == -1 and edges.types[1] == edges.T
    for r in (0, 1, *np.nonzero(edges.types == 0)[0]):                        # type -1, type T, the empty type
        assert got.count[r] == 0 and not any(getattr(got, f)[r] for f in FIELDS[1:]), r
    one = np.nonzero(edges.types == 1)[0]                                     # the one-product type
    assert len(one) and (got.count[one] == 1).all() and (got.std[one] == 0).all() and (got.s1[one] == 0).all()
    assert (got.mean[one].view(np.int32) == got.pivot[one].view(np.int32)).all()
    tied = np.nonzero(edges.types == TIED)[0]                                 # 30 copies of one row: every score the pivot's bits
    assert len(tied) and (got.count[tied] == 30).all() and (got.s1[tied] == 0).all() and (got.s2[tied] == 0).all()
    assert (got.std[tied] == 0).all()
    # what is served for such a slot standardises to 0, padding stays -inf
    idx, sc = ops.retrieve_list_grouped(t.dproj, t.dtypes, t.rowptr, t.col, t.table, 4)
    z = ops.standardise_scores(sc, m.mean[:, None], m.std[:, None], m.count[:, None]).cpu().numpy()
    for r in (*one, *tied):
        live = idx[r].cpu().numpy() >= 0
        assert live.any() and (z[r][live] == 0).all() and np.isneginf(z[r][~live]).all(), r
    assert np.isneginf(z[0]).all() and np.isneginf(z[1]).all()
    two = np.nonzero(edges.types == 2)[0][0]                                  # a live slot: finite, and not all zero
    assert np.isfinite(z[two][:2]).all() and (z[two][:2] != 0).any() and np.isneginf(z[two][2:]).all()
    for slices in SLICES:                                                     # run to run, the same bits
        assert same_bits(moments(t, slices), moments(t, slices)), slices
    bad = torch.full((1,), 5, dtype=torch.int32, device="cuda")              # the caller's counter is added to
    assert moments(t, bad=bad).bad is bad and int(bad) == 6


@pytest.mark.parametrize("table", ["fp32", "bf16"])
def test_run_to_run_the_same_bits_on_the_large_catalogue(mixed, table):
    t = getattr(mixed, table)
    for slices in SLICES:
        assert same_bits(moments(t, slices), moments(t, slices)), slices


# ---- (f) the methods
def cfg(n_types, dim):
    return SimpleNamespace(PRODUCT_EMB_DIM=dim, TYPE_EMB_DIM=64, HIDDEN_SIZE=256, NUM_ATTENTION_HEADS=4, DROPOUT=0.0, MARGIN=1.0,
                           ALPHA=0.8, NUM_COMP_TYPES=3, NUM_TYPES=n_types, DEVICE=torch.device("cuda"), LEARNING_RATE=1e-3,
                           BATCH_SIZE=256, NUM_EPOCHS=1)


@pytest.fixture(scope="module")
def served():
    from p_companion_amd import ops
    from p_companion_amd.data import DeviceBPG, generate_scaled_bpg
    from p_companion_amd.inference import CompactInference, PCompanionInference
    from p_companion_amd.p_companion import PCompanion
    dim, products, n_types = 128, 2000, 8
    bpg_host = generate_scaled_bpg(products, n_types, seed=3, dim=dim)
    g = dict(bpg_host.cuda())
    g["comp_pairs"] = dev(bpg_host.complementary_pairs.astype(np.int32))
    g["max_degree"] = int(np.diff(bpg_host.cv_rowptr).max())
    bpg = DeviceBPG(g, n_types, dim)
    c = cfg(n_types, dim)
    torch.manual_seed(0)
    model = PCompanion(c, torch.randn(products, dim, generator=torch.Generator().manual_seed(11)))
    kinds = {"fp32": PCompanionInference(model, c, bpg),
             "bf16": PCompanionInference(model, c, bpg, catalogue=torch.bfloat16),
             "compact": CompactInference(model, c, bpg, catalogue=ops.CompactCatalogue(g["features"]))}
    rng = np.random.default_rng(12)
    q = torch.from_numpy(rng.integers(0, products, 37).astype(np.int32))
    return SimpleNamespace(kinds=kinds, model=model, cfg=c, bpg=bpg, features=g["features"], products=products, n_types=n_types,
                           type_idx=bpg_host.type_idx.astype(np.int32), q=q, rng=rng,
                           group=dev((np.arange(products) // 3).astype(np.int32)))


def bits(*tensors):
    return [t.view(torch.int32) if t.dtype == torch.float32 else t for t in tensors]


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and torch.equal(x, y) for x, y in zip(bits(*a), bits(*b)))


def pool_by_hand(inf, q, n):
    """recommend_batch's raw pool, standardised by hand against score_moments"""
    from p_companion_amd import ops
    types, idx, sc = inf.recommend_batch(q, n)
    t2, count, mean, std = inf.score_moments(q)
    assert torch.equal(types, t2) and count.dtype == torch.int32 and count.shape == types.shape == mean.shape == std.shape
    return types, idx, sc, ops.standardise_scores(sc, mean[..., None], std[..., None], count[..., None])


def methods_by_hand(s, inf):
    """page, capped, basket and session with normalise="zscore" against the post-passes applied by hand to the standardised pool;
    normalise=None against the call without the keyword"""
    from p_companion_amd import ops
    q, p = s.q, s.products
    k = s.cfg.NUM_COMP_TYPES
    b = len(q)
    # recommend_batch: the ids of the raw call, ops.standardise_scores of its scores
    types, idx, sc, z = pool_by_hand(inf, q, 8)
    got = inf.recommend_batch(q, 8, normalise="zscore")
    assert same(got, (types, idx, z))
    assert not torch.equal(z, sc) and torch.equal(torch.isneginf(z), idx < 0)
    assert same(inf.recommend_batch(q, 8, normalise=None), (types, idx, sc))
    # page
    types, idx, sc, z = pool_by_hand(inf, q, 4)
    want = ops.cap_lists(idx.reshape(b, -1), z.reshape(b, -1), 10, s.group, 1)
    got = inf.recommend_page_batch(q, 10, per_type=4, group=s.group, cap=1, normalise="zscore")
    assert same(got[:2], want) and torch.equal(got[2], inf._served_types(want[0]))
    assert same(inf.recommend_page_batch(q, 10, per_type=4, normalise=None), inf.recommend_page_batch(q, 10, per_type=4))
    # capped
    types, idx, sc, z = pool_by_hand(inf, q, 16)
    want = ops.cap_lists(idx.reshape(b * k, -1), z.reshape(b * k, -1), 5, s.group, 2)
    got = inf.recommend_capped_batch(q, 5, group=s.group, cap=2, pool=16, normalise="zscore")
    assert torch.equal(got[0], types) and same((got[1].reshape(b * k, 5), got[2].reshape(b * k, 5)), want)
    assert same(inf.recommend_capped_batch(q, 5, group=s.group, cap=2, pool=16, normalise=None),
                inf.recommend_capped_batch(q, 5, group=s.group, cap=2, pool=16))
    # basket (with a padding slot) and session (ragged, weighted)
    basket = q[:36].reshape(12, 3).clone()
    basket[::4, 2] = -1
    flat = basket.reshape(-1).clamp(0, p - 1)
    types, idx, sc, z = pool_by_hand(inf, flat, 8)
    for combine in ("sum", "max"):
        want = ops.fuse_lists(idx.reshape(12, 3, -1), z.reshape(12, 3, -1), 10, combine, source=basket.cuda(),
                              exclude=inf.exclusions, num_products=p)
        got = inf.recommend_basket_batch(basket, 10, per_item=8, combine=combine, normalise="zscore")
        assert same(got[:2] + got[3:], want) and torch.equal(got[2], inf._served_types(want[0])), combine
    assert same(inf.recommend_basket_batch(basket, 10, per_item=8, normalise=None), inf.recommend_basket_batch(basket, 10, per_item=8))
    items = q[:30].contiguous()
    ptr = torch.tensor([0, 3, 3, 4, 9, 15, 30], dtype=torch.int32)
    weight = torch.from_numpy(np.random.default_rng(5).choice(np.array([0.25, 0.5, 1.0, 2.0], np.float32), 30))
    types, idx, sc, z = pool_by_hand(inf, items, 8)
    want = ops.fuse_sessions(idx.reshape(30, -1), z.reshape(30, -1), ptr.cuda(), 10, "sum", source=items.cuda(), weight=weight.cuda(),
                             exclude=inf.exclusions, num_products=p, max_items=None)
    got = inf.recommend_session_batch(items, ptr, 10, per_item=8, weight=weight, normalise="zscore")
    assert same(got[:2] + got[3:], want) and torch.equal(got[2], inf._served_types(want[0]))
    assert same(inf.recommend_session_batch(items, ptr, 10, per_item=8, weight=weight, normalise=None),
                inf.recommend_session_batch(items, ptr, 10, per_item=8, weight=weight))
    assert inf._normalise is None


@pytest.mark.parametrize("kind", ["fp32", "bf16", "compact"])
def test_the_methods_serve_the_post_passes_of_the_standardised_pool(served, kind):
    from p_companion_amd import ops
    s, inf = served, served.kinds[kind]
    # score_moments is ops.score_moments_grouped on the model's own rows, over the table the object serves from
    q = s.q.cuda()
    out = inf.model({"query_idx": q, "query_types": inf.type_idx[q.long()]})
    types = out["complementary_types"]
    proj = out["projected_embeddings"].contiguous().reshape(types.numel(), -1)
    table = inf.features if kind == "fp32" else inf.catalogue
    assert table.dtype == (torch.float32 if kind == "fp32" else torch.bfloat16)
    m = ops.score_moments_grouped(proj, types.to(torch.int32).reshape(-1).contiguous(), inf.type_rowptr, inf.type_col, table)
    got = inf.score_moments(s.q)
    assert torch.equal(got[0], types)
    assert same(got[1:], (m.count.reshape(types.shape), m.mean.reshape(types.shape), m.std.reshape(types.shape)))
    assert int(m.bad) == 0 and (m.count > 0).all() and (m.std > 0).all()
    methods_by_hand(s, inf)
    with pytest.raises(ValueError, match="normalise must be None or 'zscore'"):
        inf.recommend_page_batch(s.q, normalise="minmax")


@pytest.mark.parametrize("kind", ["fp32", "bf16", "compact"])
def test_with_set_eligible_the_moments_are_the_eligible_products(served, kind):
    """The moments run over the installed CSR: against (b)'s float64 reference over the ELIGIBLE products of each slot's type."""
    s, inf = served, served.kinds[kind]
    mask = torch.from_numpy(np.random.default_rng(9).random(s.products) < 0.6)
    inf.set_eligible(mask.cuda())
    inf.set_exclusions()
    try:
        methods_by_hand(s, inf)
        types, count, mean, std = (t.cpu().numpy() for t in inf.score_moments(s.q))
        q = s.q.cuda()
        out = inf.model({"query_idx": q, "query_types": inf.type_idx[q.long()]})
        proj = out["projected_embeddings"].reshape(types.size, -1).double().cpu().numpy()
        rows = (inf.features if kind == "fp32" else inf.catalogue.float()).double().cpu().numpy()
        scale = (s.cfg.PRODUCT_EMB_DIM + 2 if kind == "fp32" else 3 * s.cfg.PRODUCT_EMB_DIM + 4) * U
        keep = mask.numpy()
        worst = 0.0
        for r, ty in enumerate(types.reshape(-1)):
            cand = np.nonzero((s.type_idx == ty) & keep)[0]                   # ascending: the first is the CSR's first
            assert count.reshape(-1)[r] == len(cand) > 1
            s64, allow = rows[cand] @ proj[r], scale * (np.abs(rows[cand]) @ np.abs(proj[r]))
            mu, sigma, b_mean, b_std = moment_reference(s64, allow)
            e = max(abs(mean.reshape(-1)[r] - mu) / b_mean, abs(std.reshape(-1)[r] - sigma) / b_std)
            assert e <= 1, (r, ty, e)
            worst = max(worst, e)
        print(f"(f) {kind}, eligible: worst {worst:.4f} of the bound")
    finally:
        inf.set_eligible(None)
        inf.set_exclusions(False)


def test_the_standardised_page_does_not_follow_a_rescaled_type(served):
    """The rows of ONE type of the catalogue times 8 (a power of two: every score of that type, its pivot, mean and std scale
    exactly, and z keeps its bits).  The raw page follows the loud type -- its head is that type's wherever 8 x its best score
    beats the other slots' -- and changes; the standardised page is the same ids and the same bits before and after, and is
    not the raw page."""
    s, inf = served, served.kinds["fp32"]
    q = s.q
    types = inf.recommend_batch(q, 4)[0].cpu().numpy()
    loud = int(np.bincount(types.reshape(-1), minlength=s.n_types).argmax())  # the type most queries predict
    has = (types == loud).any(1)
    assert has.sum() >= 5
    scaled = s.features.clone()
    scaled[torch.from_numpy(s.type_idx == loud).cuda()] *= 8
    louder = copy.copy(inf)
    louder.features = scaled
    raw0, raw8 = inf.recommend_page_batch(q, 10, per_type=4), louder.recommend_page_batch(q, 10, per_type=4)
    z0 = inf.recommend_page_batch(q, 10, per_type=4, normalise="zscore")
    z8 = louder.recommend_page_batch(q, 10, per_type=4, normalise="zscore")
    assert same(z0, z8)                                                       # ids, scores and types, bit for bit
    assert not torch.equal(raw0[0], raw8[0])                                  # the raw page follows the rescaling
    assert not torch.equal(z8[0], raw8[0])                                    # and the standardised page is not the raw one
    # the raw page's head after the rescaling: the loud type's wherever its best raw score beats the other slots' best
    _, idx, sc = louder.recommend_batch(q, 4)
    best = sc[:, :, 0].cpu().numpy()
    slot = (types == loud).argmax(1)
    rows = np.nonzero(has)[0]
    wins = np.array([r for r in rows if best[r, slot[r]] > np.delete(best[r], slot[r]).max()], np.int64)
    assert len(wins) >= 1
    assert (raw8[2].cpu().numpy()[wins, 0] == loud).all()
    moved = (raw0[2].cpu().numpy()[wins, 0] != loud).sum()
    share = lambda page: float((page[2].cpu().numpy()[rows] == loud).mean())
    print(f"(f) type {loud} x 8 over {len(rows)} queries: raw heads moved {moved}; share of the page raw {share(raw0):.2f} -> "
          f"{share(raw8):.2f}, standardised {share(z0):.2f} -> {share(z8):.2f}")
    assert share(raw8) > share(raw0) and share(z8) == share(z0)
