"""The grouped retrieval and rank with a per-product term on the score (pc_retrieve_topk_grouped_biased,
pc_rank_grouped_biased, pc_half_sq_norm_bias) and inference.SimilarProducts on top of them.  Needs an MI355X.

The reference is float64 numpy in this file: s64(r, p) = <q_r, e_p> + float64(bias_fp32[p]) with the DEVICE's bias array, so the
bias kernel's own error is tested separately.  The allowance of one entry is the forward-error bound of the device's score --
D products, D - 1 additions of the chain and the one addition of the bias, every partial sum bounded by the sum of the terms'
magnitudes:  |s - s64| <= (D + 2) 2^-24 (sum_d |q_d e_pd| + |b_p|).  A flat 1e-5 is not usable: with the half-norm bias s cancels
to near zero for far candidates while its terms are about 150 in size.  A returned index that differs from the reference's at
its rank is accepted only where the two products' float64 scores lie within the sum of their two allowances (the device can
order them either way only then); there is no cap on the number of such rows, every one of them is held to that bound."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_retrieval_grouped import mixed_catalogue, mixed_rows, upload

U = 2.0 ** -24


def build_ref(type_idx, features, types, proj, T):
    """Per type with rows: (cand ascending, rows, dot [C, Rt] float64, adot [C, Rt] = sum_d |q_d e_d|); where[r] = (t, column)."""
    per_type, where = {}, {}
    f64, p64 = features.astype(np.float64), proj.astype(np.float64)
    for t in np.unique(types):
        if not 0 <= t < T:
            continue
        cand = np.nonzero(type_idx == t)[0]
        if cand.size == 0:
            continue
        rows = np.nonzero(types == t)[0]
        per_type[int(t)] = (cand, rows, f64[cand] @ p64[rows].T, np.abs(f64[cand]) @ np.abs(p64[rows]).T)
        for j, r in enumerate(rows):
            where[int(r)] = (int(t), j)
    return per_type, where


def row_view(m, r, bias):
    """(cand, s64, allowance) of row r under `bias` (fp32 numpy, as the device holds it); empty for a row without candidates."""
    if r not in m.where:
        return np.zeros(0, np.int64), np.zeros(0), np.zeros(0)
    t, j = m.where[r]
    cand, _, dot, adot = m.per_type[t]
    b = bias.astype(np.float64)[cand]
    return cand, dot[:, j] + b, (m.dim + 2) * U * (adot[:, j] + np.abs(b))


def ordered(cand, s64):
    """positions of cand under (score descending, product index ascending)"""
    return np.lexsort((cand, -s64))


def check_biased(m, idx, sc, bias, n, excluded=None, exact=False):
    """Every row against the float64 reference (module docstring); exact: ids equal and scores the reference's fp32 bits."""
    for r in range(len(m.types)):
        cand, s64, allow = row_view(m, r, bias)
        if excluded is not None and len(excluded.get(r, ())):
            keep = ~np.isin(cand, excluded[r])
            cand, s64, allow = cand[keep], s64[keep], allow[keep]
        o = ordered(cand, s64)[:n]
        k = len(o)
        assert (idx[r, k:] == -1).all() and np.isneginf(sc[r, k:]).all(), r
        got = idx[r, :k]
        if exact:
            assert (got == cand[o]).all(), f"row {r}: {got} != {cand[o]}"
            assert (sc[r, :k].view(np.int32) == s64[o].astype(np.float32).view(np.int32)).all(), r
            continue
        assert len(set(got.tolist())) == k and np.isin(got, cand).all(), r
        pos = np.searchsorted(cand, got)                                          # (cand ascending)
        err = np.abs(sc[r, :k].astype(np.float64) - s64[pos])
        assert (err <= allow[pos]).all(), f"row {r}: score error {err.max():.3e} above the allowance {allow[pos].min():.3e}"
        diff = got != cand[o]
        if diff.any():
            gap = np.abs(s64[pos][diff] - s64[o][diff])
            assert (gap <= allow[pos][diff] + allow[o][diff]).all(), f"row {r}: index mismatch, float64 gap {gap.max():.3e}"
        if k > 1:
            tie = sc[r, 1:k] == sc[r, :k - 1]
            assert (got[1:][tie] > got[:-1][tie]).all(), f"row {r}: equal scores not in ascending product order"


def fixture_from(dim, type_idx, features, T, types, proj):
    per_type, where = build_ref(type_idx, features, types, proj, T)
    rowptr, col, table = upload(type_idx, features, T)
    return SimpleNamespace(dim=dim, P=len(type_idx), type_idx=type_idx, features=features, T=T, types=types, proj=proj,
                           per_type=per_type, where=where, rowptr=rowptr, col=col, table=table,
                           dproj=torch.from_numpy(proj).cuda(), dtypes=torch.from_numpy(types).cuda(),
                           dcand=torch.from_numpy(type_idx).cuda())


@pytest.fixture(scope="module", params=[128, 256])
def mixed(request):
    """16 000 products, 203 rows: type 0 splits into three slices, the last tile of the heavy type is partial, rows of type -1,
    T and of the empty types, types of 3 products, the tied type 5."""
    from p_companion_amd import ops
    dim = request.param
    type_idx, features, T = mixed_catalogue(16_000, dim, seed=dim)
    assert (type_idx == 0).sum() > 8192                       # three slices at RG_SLICE_MIN = 4096
    types = mixed_rows(203, T, seed=dim)
    proj = np.random.default_rng(7).standard_normal((203, dim)).astype(np.float32)
    m = fixture_from(dim, type_idx, features, T, types, proj)
    m.bias = {"random": torch.from_numpy((np.random.default_rng(3).standard_normal(m.P) * 10).astype(np.float32)).cuda(),
              "half_norm": ops.half_sq_norm_bias(m.table)}
    m.hbias = {k: v.cpu().numpy() for k, v in m.bias.items()}
    return m


@pytest.fixture(scope="module")
def exact():
    """Integer features and queries in [-4, 4] at D = 128: every dot product, -|e|^2 / 2 and their sum is exact in fp32 and
    float64 alike.  2 000 products: type 0 holds 1 100 (two 64-row tiles of rows), the 59 others about 15 each."""
    dim, P, T, R = 128, 2_000, 60, 150
    rng = np.random.default_rng(31)
    type_idx = rng.integers(1, T, P).astype(np.int32)
    type_idx[:1100] = 0
    features = rng.integers(-4, 5, (P, dim)).astype(np.float32)
    features[5] = features[3]                                 # exact ties inside type 0
    features[9] = features[3]
    types = rng.integers(0, T, R).astype(np.int32)
    types[:70] = 0
    types[70:74] = [-1, T, 7, 7]
    proj = rng.integers(-4, 5, (R, dim)).astype(np.float32)
    return fixture_from(dim, type_idx, features, T, types, proj)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- the bias kernel
@pytest.mark.parametrize("dim", [128, 256])
def test_half_sq_norm_bias_against_float64_and_for_every_grid(dim):
    """Relative error at most D 2^-24 (all terms have one sign); the same bits whatever the number of rows in the launch (the
    grid is sized by it; 70 001 rows are more than one pass of the largest grid) and run to run."""
    from p_companion_amd import ops
    P = 70_001
    table = torch.from_numpy(np.random.default_rng(dim).standard_normal((P, dim)).astype(np.float32)).cuda()
    got = ops.half_sq_norm_bias(table)
    want = -0.5 * (table.cpu().numpy().astype(np.float64) ** 2).sum(1)
    rel = np.abs(got.cpu().numpy().astype(np.float64) - want) / np.abs(want)
    print(f"half_sq_norm_bias D={dim}: worst relative error {rel.max():.3e}, bound {dim * U:.3e}")
    assert got.dtype == torch.float32 and tuple(got.shape) == (P,) and (rel <= dim * U).all()
    assert torch.equal(ops.half_sq_norm_bias(table).view(torch.int32), got.view(torch.int32))
    for rows in (1, 15, 17, 4097):
        assert torch.equal(ops.half_sq_norm_bias(table[:rows].contiguous()).view(torch.int32), got[:rows].view(torch.int32)), rows
    z = torch.zeros(3, dim, device="cuda")
    z[1, dim - 1] = 3.0
    assert ops.half_sq_norm_bias(z).cpu().tolist() == [0.0, -4.5, 0.0]


# ---- 1. parity
@pytest.mark.parametrize("kind", ["random", "half_norm"])
@pytest.mark.parametrize("n", [1, 10, 16])
def test_parity_with_the_float64_reference(mixed, n, kind):
    from p_companion_amd import ops
    m = mixed
    idx, sc = ops.retrieve_topk_grouped(m.dproj, m.dtypes, m.rowptr, m.col, m.table, n, bias=m.bias[kind])
    idx, sc = idx.cpu().numpy(), sc.cpu().numpy()
    check_biased(m, idx, sc, m.hbias[kind], n)
    # the special rows: types -1 / n_types / empty give nothing, short types give what they have
    assert (idx[:4] == -1).all() and np.isneginf(sc[:4]).all()
    assert (idx[4:6, :min(n, 3)] >= 0).all() and (idx[4:6, 3:] == -1).all()


# ---- 2. zero bias
def excl_triple(m, seed=0):
    """One key per row: lists of 0 to 5 products of the row's own type."""
    rng = np.random.default_rng(seed)
    lists = []
    for r in range(len(m.types)):
        cand = row_view(m, r, np.zeros(m.P, np.float32))[0]
        lists.append(np.sort(rng.choice(cand, min(len(cand), int(rng.integers(0, 6))), replace=False)) if len(cand) else cand)
    return lists


def as_csr(lists):
    rowptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
    col = (np.concatenate(lists) if len(lists) else np.zeros(0)).astype(np.int32)
    return dev(rowptr), dev(col)


def test_zero_bias_is_the_unbiased_entry_bit_for_bit(mixed):
    from p_companion_amd import ops
    m = mixed
    zero = torch.zeros(m.P, device="cuda")
    lists = excl_triple(m)
    key = torch.arange(len(m.types), dtype=torch.int32, device="cuda")
    targets = dev(np.random.default_rng(2).integers(0, m.P, len(m.types)).astype(np.int32))
    for exclude in (None, (key,) + as_csr(lists)):
        a_i, a_s = ops.retrieve_topk_grouped(m.dproj, m.dtypes, m.rowptr, m.col, m.table, 16, exclude=exclude)
        b_i, b_s = ops.retrieve_topk_grouped(m.dproj, m.dtypes, m.rowptr, m.col, m.table, 16, exclude=exclude, bias=zero)
        assert torch.equal(a_i, b_i) and torch.equal(a_s.view(torch.int32), b_s.view(torch.int32))
        ct = None if exclude is None else m.dcand
        a_r, a_b = ops.rank_grouped(m.dproj, m.dtypes, targets, m.rowptr, m.col, m.table, exclude=exclude, cand_type=ct)
        b_r, b_b = ops.rank_grouped(m.dproj, m.dtypes, targets, m.rowptr, m.col, m.table, exclude=exclude, cand_type=ct, bias=zero)
        assert torch.equal(a_r, b_r) and torch.equal(a_b, b_b)


# ---- 3. exact data
def test_exact_data_equals_the_reference_ties_included(exact):
    from p_companion_amd import ops
    m = exact
    bias = np.random.default_rng(4).integers(-50, 51, m.P).astype(np.float32)
    bias[[3, 5, 9]] = 7.0                                     # the copied rows stay tied
    for n in (1, 10, 16):
        idx, sc = ops.retrieve_topk_grouped(m.dproj, m.dtypes, m.rowptr, m.col, m.table, n, bias=dev(bias))
        check_biased(m, idx.cpu().numpy(), sc.cpu().numpy(), bias, n, exact=True)


def test_exact_data_with_the_half_norm_bias_is_the_float64_l2_order(exact):
    from p_companion_amd import ops
    m = exact
    hb = ops.half_sq_norm_bias(m.table)
    assert (hb.cpu().numpy().astype(np.float64) == -0.5 * (m.features.astype(np.float64) ** 2).sum(1)).all()
    idx, sc = ops.retrieve_topk_grouped(m.dproj, m.dtypes, m.rowptr, m.col, m.table, 16, bias=hb)
    idx = idx.cpu().numpy()
    check_biased(m, idx, sc.cpu().numpy(), hb.cpu().numpy(), 16, exact=True)
    f64, p64 = m.features.astype(np.float64), m.proj.astype(np.float64)
    for r in m.where:
        cand = np.nonzero(m.type_idx == m.types[r])[0]
        d2 = ((p64[r][None, :] - f64[cand]) ** 2).sum(1)       # brute force, exact in float64
        want = cand[np.lexsort((cand, d2))][:16]
        assert (idx[r, :len(want)] == want).all(), r


@pytest.mark.parametrize("which", ["exact", "mixed"])
def test_the_score_is_one_fp32_addition_after_the_chain(which, exact, mixed):
    """s = fl(d + b) bit for bit, d read from the unbiased entry on types of at most 16 products, where every candidate is
    returned.  An accumulator that started at the bias would round differently at every step of the chain."""
    from p_companion_amd import ops
    m = exact if which == "exact" else mixed
    bias = (np.random.default_rng(6).standard_normal(m.P) * 10).astype(np.float32)
    d_i, d_s = ops.retrieve_topk_grouped(m.dproj, m.dtypes, m.rowptr, m.col, m.table, 16)
    s_i, s_s = ops.retrieve_topk_grouped(m.dproj, m.dtypes, m.rowptr, m.col, m.table, 16, bias=dev(bias))
    d_i, d_s, s_i, s_s = (x.cpu().numpy() for x in (d_i, d_s, s_i, s_s))
    seen = 0
    for r, (t, _) in m.where.items():
        cand = m.per_type[t][0]
        if len(cand) > 16:
            continue
        k = len(cand)
        assert sorted(d_i[r, :k].tolist()) == sorted(s_i[r, :k].tolist()) == cand.tolist()
        d = dict(zip(d_i[r, :k].tolist(), d_s[r, :k]))
        want = np.array([np.float32(d[p]) + bias[p] for p in s_i[r, :k]], np.float32)
        assert (s_s[r, :k].view(np.int32) == want.view(np.int32)).all(), r
        seen += k
    assert seen >= 6


# ---- 4. determinism
def test_bitwise_run_to_run_across_slices_and_candidate_order(mixed):
    from p_companion_amd import ops
    m = mixed
    b = m.bias["half_norm"]
    run = lambda col, s: ops.retrieve_topk_grouped(m.dproj, m.dtypes, m.rowptr, col, m.table, 16, slices=s, bias=b)
    i0, s0 = run(m.col, 0)
    for s in (0, 1, 2, 64):
        i, sc = run(m.col, s)
        assert torch.equal(i, i0) and torch.equal(sc.view(torch.int32), s0.view(torch.int32)), s
    rowptr, col = m.rowptr.cpu().numpy(), m.col.cpu().numpy().copy()
    rng = np.random.default_rng(5)
    for t in range(m.T):
        rng.shuffle(col[rowptr[t]:rowptr[t + 1]])
    i, sc = run(dev(col), 0)
    assert torch.equal(i, i0) and torch.equal(sc.view(torch.int32), s0.view(torch.int32))


# ---- 5. exclusions
def test_exclusion_lists_against_the_reference(mixed):
    from p_companion_amd import ops
    m = mixed
    kind = "half_norm"
    R = len(m.types)
    rng = np.random.default_rng(8)
    lists = excl_triple(m, seed=9)
    heavy = np.nonzero(m.types == 0)[0]
    cand, s64, _ = row_view(m, heavy[0], m.hbias[kind])
    top = cand[ordered(cand, s64)]
    lists[heavy[0]] = np.sort(np.concatenate([top[:20], rng.choice(top[40:], 20, replace=False)]))      # longer than 16: its head
    lists[heavy[1]] = np.zeros(0, np.int64)                                                            # an empty list
    for r in heavy[2:40]:                                                                              # the served head struck out
        c, s, _ = row_view(m, r, m.hbias[kind])
        lists[r] = np.sort(c[ordered(c, s)][:int(rng.integers(1, 12))])
    key = np.arange(R, dtype=np.int32)
    key[heavy[40]] = -1                                                                                # no list
    key[heavy[41]], key[heavy[42]] = R + 3, -5                                                         # out of range
    excluded = {r: lists[r] for r in range(R) if 0 <= key[r] < R}
    rowptr, col = as_csr(lists)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    idx, sc = ops.retrieve_topk_grouped(m.dproj, m.dtypes, m.rowptr, m.col, m.table, 16, exclude=(dev(key), rowptr, col),
                                        bad=bad, bias=m.bias[kind])
    assert bad.item() == 2
    idx, sc = idx.cpu().numpy(), sc.cpu().numpy()
    check_biased(m, idx, sc, m.hbias[kind], 16, excluded=excluded)
    assert not np.isin(idx[heavy[0]], lists[heavy[0]]).any()
    # the rows without a list are served as the unfiltered call serves them
    f_i, f_s = ops.retrieve_topk_grouped(m.dproj, m.dtypes, m.rowptr, m.col, m.table, 16, bias=m.bias[kind])
    for r in (heavy[1], heavy[40], heavy[41], heavy[42]):
        assert (f_i[r].cpu().numpy() == idx[r]).all() and (f_s[r].cpu().numpy() == sc[r]).all(), r


# ---- 6. rank
def rank_case(m, kind, seed):
    """Targets: a member of the served list, any product of the row's type, and (for the filtered call) products of another
    type; lists as in the exclusion test, some of which hold the target."""
    rng = np.random.default_rng(seed)
    R = len(m.types)
    targets = np.zeros(R, np.int32)
    for r in range(R):
        cand, s64, _ = row_view(m, r, m.hbias[kind])
        if not len(cand):
            targets[r] = rng.integers(0, m.P)
        elif r % 3 == 0:
            targets[r] = cand[ordered(cand, s64)][rng.integers(0, min(len(cand), 24))]
        else:
            targets[r] = rng.choice(cand)
    return targets


@pytest.mark.parametrize("kind", ["random", "half_norm"])
def test_rank_below_16_exactly_when_the_list_holds_the_target_there(mixed, kind):
    from p_companion_amd import ops
    m = mixed
    R = len(m.types)
    targets = rank_case(m, kind, seed=12)
    lists = excl_triple(m, seed=13)
    in_list = [r for r in range(R) if r % 7 == 0 and r in m.where]
    for r in in_list:
        lists[r] = np.unique(np.concatenate([lists[r], [targets[r]]]))
    other = [r for r in range(R) if r % 7 == 1 and r in m.where]
    t2 = targets.copy()
    for r in other:
        t2[r] = np.nonzero(m.type_idx != m.types[r])[0][r]
    key = torch.arange(R, dtype=torch.int32, device="cuda")
    for exclude, tg in ((None, targets), ((key,) + as_csr(lists), t2)):
        i16, _ = ops.retrieve_topk_grouped(m.dproj, m.dtypes, m.rowptr, m.col, m.table, 16, exclude=exclude, bias=m.bias[kind])
        ct = None if exclude is None else m.dcand
        ranks = []
        for s in (0, 1, 2, 64):
            rank, bad = ops.rank_grouped(m.dproj, m.dtypes, dev(tg), m.rowptr, m.col, m.table, slices=s, exclude=exclude,
                                         cand_type=ct, bias=m.bias[kind])
            ranks.append(rank)
            assert torch.equal(rank, ranks[0]), s
            assert bad.item() == 1                            # the row of type T
        rank, i16 = ranks[0].cpu().numpy(), i16.cpu().numpy()
        for r in range(R):
            if r not in m.where:                              # types -1 and T: no rank; an empty type: nothing in front
                typed = 0 <= m.types[r] < m.T
                assert rank[r] == (0 if typed and exclude is None else -1), r
                continue
            if exclude is not None and (tg[r] in lists[r] or m.type_idx[tg[r]] != m.types[r]):
                assert rank[r] == -1, r                       # in the row's list, or no candidate of the row's type
                continue
            assert rank[r] >= 0, r
            if rank[r] < 16:
                assert i16[r, rank[r]] == tg[r], r
            else:
                assert tg[r] not in i16[r], r
        served = rank[[r for r in range(R) if r in m.where]]
        assert ((served >= 0) & (served < 16)).sum() > 20 and (served >= 16).sum() > 20
        if exclude is not None:
            assert all(rank[r] == -1 for r in in_list + other)


def test_rank_on_exact_data_equals_the_float64_count(exact):
    from p_companion_amd import ops
    m = exact
    hb = ops.half_sq_norm_bias(m.table)
    m.hbias = {"half_norm": hb.cpu().numpy()}
    targets = rank_case(m, "half_norm", seed=14)
    targets[:3] = [3, 5, 9]                                   # the tied copies: the product index decides
    rank, bad = ops.rank_grouped(m.dproj, m.dtypes, dev(targets), m.rowptr, m.col, m.table, bias=hb)
    rank = rank.cpu().numpy()
    assert bad.item() == 1
    for r in range(len(m.types)):
        if r not in m.where:
            assert rank[r] == (0 if 0 <= m.types[r] < m.T else -1), r
            continue
        cand, s64, _ = row_view(m, r, m.hbias["half_norm"])
        y = targets[r]
        g = s64[np.searchsorted(cand, y)]
        assert rank[r] == ((s64 > g) | ((s64 == g) & (cand < y))).sum(), r


# ---- 7. error codes
def test_error_codes_through_ctypes():
    from p_companion_amd import _lib
    L = _lib.lib()
    R, T, P = 4, 2, 4
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device="cuda")
    a = dict(proj=torch.zeros(R, 256, device="cuda"), types=i32(0, 0, 1, 1), row_key=i32(0, 1, -1, 0), rows=R,
             type_rowptr=i32(0, 2, 4), type_col=i32(0, 1, 2, 3), table=torch.zeros(P, 256, device="cuda"),
             bias=torch.zeros(P, device="cuda"), n_types=T, ex_rowptr=i32(0, 1, 1), ex_col=i32(0), n_keys=2, n=10, dim=128,
             slices=0, out_idx=torch.empty(R, 16, dtype=torch.int32, device="cuda"), out_score=torch.empty(R, 16, device="cuda"),
             bad_count=torch.zeros(1, dtype=torch.int32, device="cuda"),
             ws=torch.empty(L.pc_retrieve_topk_grouped_biased_workspace_bytes(R, T, 16, 64), dtype=torch.uint8, device="cuda"))
    a["ws_bytes"] = a["ws"].numel()
    a["stream"] = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    conv = lambda v: ctypes.c_void_p(v.data_ptr()) if torch.is_tensor(v) else v
    none = dict(row_key=None, ex_rowptr=None, ex_col=None, n_keys=0)

    def retrieve(**kw):
        return L.pc_retrieve_topk_grouped_biased(*[conv(v) for v in {**a, **kw}.values()])

    assert retrieve() == 0 and retrieve(dim=256, n=16, slices=64) == 0 and retrieve(**none) == 0
    assert retrieve(**none, bad_count=None) == 0
    torch.cuda.synchronize()
    for name in ("proj", "types", "type_rowptr", "type_col", "table", "bias", "out_idx", "out_score", "ws", "ex_rowptr", "ex_col",
                 "bad_count"):
        assert retrieve(**{name: None}) == -1, name                                # PC_EINVAL
    assert retrieve(rows=0) == -1 and retrieve(n_types=0) == -1 and retrieve(n_keys=-1) == -1
    assert retrieve(row_key=None) == -1 and retrieve(**{**none, "n_keys": 2}) == -1
    assert retrieve(**{**none, "ex_col": a["ex_col"]}) == -1
    for kw in (dict(n=0), dict(n=17), dict(dim=64), dict(dim=192), dict(slices=-1), dict(slices=65)):
        assert retrieve(**kw) == -2 and retrieve(**kw, **none) == -2, kw           # PC_ESHAPE
    assert retrieve(ws_bytes=L.pc_retrieve_topk_grouped_biased_workspace_bytes(R, T, 10, 0) - 1) == -3      # PC_EWORKSPACE
    assert L.pc_retrieve_topk_grouped_biased_workspace_bytes(R, T, 17, 0) == 0

    b = dict(proj=a["proj"], types=a["types"], targets=i32(1, 0, 3, 2), row_key=a["row_key"], rows=R,
             type_rowptr=a["type_rowptr"], type_col=a["type_col"], table=a["table"], bias=a["bias"], n_types=T, num_products=P,
             ex_rowptr=a["ex_rowptr"], ex_col=a["ex_col"], n_keys=2, cand_type=i32(0, 0, 1, 1), dim=128, slices=0,
             rank_out=torch.empty(R, dtype=torch.int32, device="cuda"), bad_count=a["bad_count"], ws=a["ws"],
             ws_bytes=a["ws_bytes"], stream=a["stream"])
    rnone = dict(none, cand_type=None)

    def rank(**kw):
        return L.pc_rank_grouped_biased(*[conv(v) for v in {**b, **kw}.values()])

    assert rank() == 0 and rank(dim=256, slices=64) == 0 and rank(**rnone) == 0
    torch.cuda.synchronize()
    for name in ("proj", "types", "targets", "type_rowptr", "type_col", "table", "bias", "rank_out", "bad_count", "ws", "row_key",
                 "ex_rowptr", "ex_col", "cand_type"):
        assert rank(**{name: None}) == -1, name
    assert rank(rows=0) == -1 and rank(n_types=0) == -1 and rank(num_products=0) == -1 and rank(n_keys=-1) == -1
    assert rank(**{**rnone, "cand_type": b["cand_type"]}) == -1 and rank(**{**rnone, "n_keys": 1}) == -1
    for kw in (dict(dim=64), dict(dim=192), dict(slices=-1), dict(slices=65)):
        assert rank(**kw) == -2 and rank(**kw, **rnone) == -2, kw
    assert rank(ws_bytes=L.pc_rank_grouped_biased_workspace_bytes(R, T, 0) - 1) == -3
    assert L.pc_rank_grouped_biased_workspace_bytes(R, T, 65) == 0

    out = torch.empty(P, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    assert L.pc_half_sq_norm_bias(p(a["table"]), P, 256, p(out), a["stream"]) == 0
    assert L.pc_half_sq_norm_bias(None, P, 256, p(out), a["stream"]) == -1
    assert L.pc_half_sq_norm_bias(p(a["table"]), P, 256, None, a["stream"]) == -1
    assert L.pc_half_sq_norm_bias(p(a["table"]), 0, 256, p(out), a["stream"]) == -1
    assert L.pc_half_sq_norm_bias(p(a["table"]), P, 64, p(out), a["stream"]) == -2
    torch.cuda.synchronize()


# ---- 8. SimilarProducts
@pytest.fixture(scope="module")
def catalogue():
    from p_companion_amd.data import generate_device_bpg
    bpg = generate_device_bpg(20_000, 20, seed=3, world=1, with_complementary=False)
    g = bpg.cuda()
    q = np.random.default_rng(1).choice(bpg.num_products, 256, replace=False).astype(np.int32)
    return SimpleNamespace(bpg=bpg, table=g["features"], f64=g["features"].cpu().numpy().astype(np.float64),
                           type_idx=g["type_idx"].cpu().numpy(), q=q)


@pytest.mark.parametrize("scope", ["type", "catalogue"])
def test_similar_products(catalogue, scope):
    from p_companion_amd.inference import SimilarProducts
    c = catalogue
    sp = SimilarProducts(c.table, c.bpg, scope=scope)
    n, D, P = 10, c.f64.shape[1], c.f64.shape[0]
    idx, dist = sp.similar_batch(torch.from_numpy(c.q), n)
    assert idx.dtype == torch.int32 and dist.dtype == torch.float32 and tuple(idx.shape) == tuple(dist.shape) == (len(c.q), n)
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    b64 = sp.bias.cpu().numpy().astype(np.float64)
    assert (idx != c.q[:, None]).all() and (idx >= 0).all()
    assert (dist[:, 1:] >= dist[:, :-1]).all()
    for j, qi in enumerate(c.q):
        cand = np.nonzero(c.type_idx == c.type_idx[qi])[0] if scope == "type" else np.arange(P)
        cand = cand[cand != qi]
        s64 = c.f64[cand] @ c.f64[qi] + b64[cand]
        allow = (D + 2) * U * (np.abs(c.f64[cand]) @ np.abs(c.f64[qi]) + np.abs(b64[cand]))
        o = ordered(cand, s64)[:n]
        got = idx[j]
        assert np.isin(got, cand).all() and len(set(got.tolist())) == n
        pos = np.searchsorted(cand, got)
        diff = got != cand[o]
        assert (np.abs(s64[pos][diff] - s64[o][diff]) <= allow[pos][diff] + allow[o][diff]).all(), j
        d64 = np.sqrt(((c.f64[qi][None, :] - c.f64[got] + 1e-6) ** 2).sum(1))
        np.testing.assert_allclose(dist[j], d64, rtol=1e-4, atol=0)

    # rank_pairs against similar_batch: the served products stand at their positions; the query itself and a product outside
    # the scope have no rank
    anchors = np.repeat(c.q[:64], n)
    slot, rank = sp.rank_pairs(torch.from_numpy(anchors), torch.from_numpy(idx[:64].reshape(-1).copy()))
    assert (slot.cpu().numpy() == 0).all() and (rank.cpu().numpy().reshape(64, n) == np.arange(n)[None, :]).all()
    slot, rank = sp.rank_pairs(torch.from_numpy(c.q), torch.from_numpy(c.q))
    assert (slot.cpu().numpy() == 0).all() and (rank.cpu().numpy() == -1).all()
    far = np.array([np.nonzero(c.type_idx != c.type_idx[qi])[0][0] for qi in c.q], np.int32)
    slot, rank = sp.rank_pairs(torch.from_numpy(c.q), torch.from_numpy(far))
    if scope == "type":
        assert (slot.cpu().numpy() == -1).all() and (rank.cpu().numpy() == -1).all()
    else:
        assert (slot.cpu().numpy() == 0).all() and (rank.cpu().numpy() >= 0).all()

    # evaluate_pairs: the same metrics in numpy from the ranks
    rng = np.random.default_rng(5)
    pairs = np.stack([rng.integers(0, P, 3000), rng.integers(0, P, 3000)], 1).astype(np.int32)
    pairs[:640, 0], pairs[:640, 1] = anchors, idx[:64].reshape(-1)
    res = sp.evaluate_pairs(pairs, ks=(1, 3, 10, 100), chunk=1000)
    slot, rank = (x.cpu().numpy() for x in sp.rank_pairs(torch.from_numpy(pairs[:, 0].copy()), torch.from_numpy(pairs[:, 1].copy())))
    ranked = rank >= 0
    want = {"pairs": 3000, "type_hit": (slot >= 0).mean(), "mrr": np.where(ranked, 1.0 / (np.maximum(rank, 0) + 1.0), 0.0).sum() / 3000,
            "median_rank": float(np.median(rank[ranked]))}
    for k in (1, 3, 10, 100):
        want[f"hit@{k}"] = (ranked & (rank < k)).mean()
    assert set(res) == set(want) and res["pairs"] == 3000 and res["hit@10"] >= 640 / 3000
    for k, v in want.items():
        assert abs(res[k] - v) <= 1e-12 * max(1.0, abs(v)), k

    # set_eligible: only eligible products are served, and an ineligible target has no rank
    mask = torch.from_numpy(np.random.default_rng(6).random(P) < 0.7).cuda()
    sp.set_eligible(mask)
    e_idx, _ = sp.similar_batch(torch.from_numpy(c.q), n)
    e_idx = e_idx.cpu().numpy()
    hm = mask.cpu().numpy()
    assert hm[e_idx[e_idx >= 0]].all() and (e_idx != c.q[:, None]).all()
    slot, rank = sp.rank_pairs(torch.from_numpy(anchors), torch.from_numpy(idx[:64].reshape(-1).copy()))
    gone = ~hm[idx[:64].reshape(-1)]
    assert gone.any() and (rank.cpu().numpy()[gone] == -1).all() and (slot.cpu().numpy()[gone] == -1).all()
    assert (rank.cpu().numpy()[~gone] >= 0).all()
    sp.set_eligible(None)
    again, _ = sp.similar_batch(torch.from_numpy(c.q), n)
    assert (again.cpu().numpy() == idx).all()
    with pytest.raises(ValueError, match="16"):
        sp.similar_batch(torch.from_numpy(c.q), 17)
