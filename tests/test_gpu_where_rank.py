"""Ranks under a per-query attribute predicate (pc_rank_grouped_where / pc_rank_grouped_bf16_where; ops.rank_grouped_where;
rank_targets_where / evaluate_catalogue_where, rank_pairs_where / evaluate_pairs_where).  Needs an MI355X.

Every comparison is exact, and the reference is never the code under test: the existing rank entries over a CSR rebuilt in numpy
from the passing products, the existing filtered list entries (rank < 256 exactly when the list holds the target there), or a
numpy count.  The one bounded check is the float64 band of tests/test_gpu_nearest.py (fp32: (D + 2) 2^-24 per entry) and
tests/test_gpu_rank_bf16.py (bf16: (3 D + 4) 2^-24), with those files' allowances as they are, over the passing products.

The catalogue: 20 000 products -- type 0 above 10 000 (many chunks, real slices), type 6 about 3 000, the other random types
about 300, type 7 cut to 40, types 3 and 4 of 3 products, type 5 the 30 tied copies, types 1, 2 and 30..39 empty -- and 203 rows
(a partial last tile, 1 to 4 row groups per tile, rows of type -1 and T), dealt round-robin over the eight predicates of
tests/test_gpu_where_list.py, so that every 16-row group mixes them."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_gpu_nearest as f32ref
import test_gpu_rank_bf16 as bf16ref
from test_gpu_nearest import as_csr, dev, ordered
from test_gpu_retrieval_grouped import mixed_catalogue, mixed_rows
from test_gpu_where_list import BIT31, INF, PREDICATES, _Graph, passes

N = 256
SLICES = (0, 1, 2, 64)
LIST_LENGTHS = bf16ref.LIST_LENGTHS
G = len(PREDICATES)
KINDS = ("none", "random", "half_norm")


def catalogue(dim):
    type_idx, features, T = mixed_catalogue(20_000, dim, seed=dim)
    type_idx[type_idx >= 30] = 6                              # a 3 000-product type; types 30..39 are empty now
    seven = np.nonzero(type_idx == 7)[0]
    type_idx[seven[40:]] = 6                                  # a 40-product type
    sizes = np.bincount(type_idx, minlength=T)
    assert sizes[0] > 10_000 and 2_500 < sizes[6] < 3_600 and sizes[7] == 40 and 200 < sizes[8] < 400
    assert sizes[3] == sizes[4] == 3 and sizes[5] == 30 and sizes[1] == sizes[2] == sizes[35] == 0
    types = mixed_rows(203, T, seed=dim)
    types[(types >= 30) & (types < T)] = 6                   # (the row of type T stays)
    types[8:12] = 7
    assert types[0] == -1 and types[1] == T
    proj = np.random.default_rng(7).standard_normal((203, dim)).astype(np.float32)
    return type_idx, features, T, types, proj


@pytest.fixture(scope="module", params=[128, 256], ids=lambda d: f"D{d}")
def mixed(request):
    """Both tables of one catalogue with their float64 references, the attributes, a predicate per row."""
    from p_companion_amd import ops
    dim = request.param
    type_idx, features, T, types, proj = catalogue(dim)
    R, P = len(types), len(type_idx)
    m = SimpleNamespace(dim=dim, R=R, P=P, T=T, type_idx=type_idx, types=types,
                        fp32=f32ref.fixture_from(dim, type_idx, features, T, types, proj),
                        bf16=bf16ref.fixture_from(dim, type_idx, features, T, types, proj))
    rnd = dev((np.random.default_rng(3).standard_normal(P) * 10).astype(np.float32))
    m.fp32.bias = {"none": None, "random": rnd, "half_norm": ops.half_sq_norm_bias(m.fp32.table)}
    m.bf16.bias = {"none": None, "random": rnd, "half_norm": ops.half_sq_norm_bias_bf16(m.bf16.table)}
    for t in (m.fp32, m.bf16):
        t.hbias = {k: None if v is None else v.cpu().numpy() for k, v in t.bias.items()}
    rng = np.random.default_rng(5)
    m.value = rng.random(P).astype(np.float32)
    m.flags = rng.integers(-2 ** 31, 2 ** 31, P).astype(np.int32)
    # the predicate of row r: PREDICATES[r % 8]; the eighth a band whose ends are values of two products of the row's type
    m.pred = np.arange(R) % G
    m.ends = np.zeros((T + 1, 2), np.float32)                 # per type (row T: the rows without a type)
    m.ends[:] = (0.25, 0.5)
    for t in range(T):
        v = np.sort(m.value[type_idx == t])
        if len(v):
            m.ends[t] = (v[len(v) // 4], v[(3 * len(v)) // 4])
    lo, hi, need, deny = np.zeros(R, np.float32), np.zeros(R, np.float32), np.zeros(R, np.int32), np.zeros(R, np.int32)
    for r in range(R):
        lo[r], hi[r], need[r], deny[r] = row_pred(m, r)
    m.lo, m.hi, m.need, m.deny = lo, hi, need, deny
    m.dvalue, m.dflags = dev(m.value), dev(m.flags)
    m.where = ops.RowWhere(value=m.dvalue, flags=m.dflags, lo=dev(lo), hi=dev(hi), need=dev(need), deny=dev(deny))
    m.ok = np.stack([passes(m.value, m.flags, lo[r], hi[r], need[r], deny[r]) for r in range(R)])      # [R, P]
    share = [m.ok[r][type_idx == 0].mean() for r in range(G, 2 * G)]
    assert share[0] == 1 and share[1] == 0 and 0.4 < share[2] < 0.6 and 0.002 < share[3] < 0.03 and 0.4 < share[7] < 0.6
    assert all(0.05 < s < 0.6 for s in share[4:7])
    return m


def row_pred(m, r):
    p = PREDICATES[r % G]
    if p is not None:
        return p
    t = m.types[r] if 0 <= m.types[r] < m.T else m.T
    return (m.ends[t, 0], m.ends[t, 1], 0, 0)


def view(t, r, hbias):
    """(cand ascending, s64, allowance) of row r of table fixture t under its bias (None: none)"""
    if hasattr(t, "rounded"):
        return bf16ref.view(t, r, hbias)
    return f32ref.row_view(t, r, np.zeros(t.P, np.float32) if hbias is None else hbias)


def make_targets(m, t, hbias, seed):
    """Per predicate in turn: a member of the head of the passing order, any passing product, any product of the type -- and
    for every fifth row of a predicate a product that fails it (where one does)."""
    rng = np.random.default_rng(seed)
    targets = np.zeros(m.R, np.int32)
    for r in range(m.R):
        cand, s64, _ = view(t, r, hbias)
        if not len(cand):
            targets[r] = rng.integers(0, m.P)
            continue
        ok = m.ok[r][cand]
        turn = r // G
        if turn % 5 == 4 and (~ok).any():
            targets[r] = rng.choice(cand[~ok])
        elif turn % 3 == 2 or not ok.any():
            targets[r] = rng.choice(cand)
        elif turn % 3 == 0:
            head = cand[ok][ordered(cand[ok], s64[ok])]
            targets[r] = head[rng.integers(0, min(len(head), 300))]
        else:
            targets[r] = rng.choice(cand[ok])
    return targets


def served_lists(m, t, bias, exclude=None, where=None):
    from p_companion_amd import ops
    i, _ = ops.retrieve_list_grouped_where(t.dproj, t.dtypes, t.rowptr, t.col, t.table, N, where or m.where, exclude=exclude,
                                           bias=bias)
    return i.cpu().numpy()


def rank_where(m, t, targets, bias=None, exclude=None, slices=0, where=None, bad=None, col=None):
    from p_companion_amd import ops
    return ops.rank_grouped_where(t.dproj, t.dtypes, dev(targets), t.rowptr, t.col if col is None else col, t.table,
                                  where or m.where, slices=slices, exclude=exclude, bad=bad, bias=bias,
                                  cand_type=None if exclude is None else t.dcand)


def twin(t, proj, types, targets, rowptr, col, bias=None, exclude=None, cand_type=None):
    """the unfiltered rank entry of the table"""
    from p_companion_amd import ops
    fn = ops.rank_grouped_bf16 if hasattr(t, "rounded") else ops.rank_grouped
    return fn(proj, types, targets, rowptr, col, t.table, bias=bias, exclude=exclude, cand_type=cand_type)


def lists_of(m, t, targets, seed):
    """tests/test_gpu_rank_bf16.py's lists (lengths 0, 1, 15, 16, 17, 40; every fifth with a product of another type); every
    seventh row's list holds its target."""
    lists = bf16ref.exclusion_lists(m.bf16, seed)
    for r in range(0, m.R, 7):
        if r in t.where:
            lists[r] = np.unique(np.concatenate([lists[r], [targets[r]]]))
    return lists


# ---- 1. rank <-> list
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("table", ["fp32", "bf16"])
def test_rank_below_256_exactly_when_the_filtered_list_holds_the_target_there(mixed, table, kind):
    m, t = mixed, getattr(mixed, table)
    bias = t.bias[kind]
    targets = make_targets(m, t, t.hbias[kind], seed=12)
    lists = lists_of(m, t, targets, seed=13)
    assert {len(x) for x in lists} >= set(LIST_LENGTHS)
    # the lists hold entries that fail their row's predicate, and entries that pass
    fails = [int((~m.ok[r][lists[r]]).sum()) for r in range(m.R)]
    holds = [int(m.ok[r][lists[r]].sum()) for r in range(m.R)]
    assert sum(f > 0 for f in fails) > 50 and sum(h > 0 for h in holds) > 50
    key = torch.arange(m.R, dtype=torch.int32, device="cuda")
    for exclude in (None, (key,) + as_csr(lists)):
        served = served_lists(m, t, bias, exclude)
        rank, bad = rank_where(m, t, targets, bias, exclude)
        assert rank.dtype == torch.int32 and bad.item() == 1          # the row of type T
        rank = rank.cpu().numpy()
        seen = {"in": 0, "out": 0, "fail": 0, "listed": 0}
        for r in range(m.R):
            y = targets[r]
            if r not in t.where:                              # types -1 and T: no rank; an empty type: nothing in front
                typed = 0 <= m.types[r] < m.T
                assert rank[r] == (0 if typed and exclude is None and m.ok[r][y] else -1), r
                continue
            if not m.ok[r][y]:
                assert rank[r] == -1 and y not in served[r], r            # the target fails its own predicate
                seen["fail"] += 1
                continue
            if exclude is not None and y in lists[r]:
                assert rank[r] == -1 and y not in served[r], r
                seen["listed"] += 1
                continue
            assert rank[r] >= 0, r
            if rank[r] < N:
                assert served[r, rank[r]] == y, r
                seen["in"] += 1
            else:
                assert y not in served[r], r
                seen["out"] += 1
        assert seen["in"] >= 30 and seen["out"] >= 8 and seen["fail"] >= 20, seen
        assert exclude is None or seen["listed"] >= 5, seen


# ---- 2. a rebuilt CSR per predicate
@pytest.mark.parametrize("kind", ["none", "half_norm"])
@pytest.mark.parametrize("table", ["fp32", "bf16"])
def test_the_mixed_call_equals_the_existing_rank_over_each_predicates_csr(mixed, table, kind):
    m, t = mixed, getattr(mixed, table)
    bias = t.bias[kind]
    targets = make_targets(m, t, t.hbias[kind], seed=22)
    lists = lists_of(m, t, targets, seed=23)
    key = torch.arange(m.R, dtype=torch.int32, device="cuda")
    ex = (key,) + as_csr(lists)
    got = {False: rank_where(m, t, targets, bias)[0].cpu().numpy(), True: rank_where(m, t, targets, bias, ex)[0].cpu().numpy()}
    want = {False: np.full(m.R, -7, np.int32), True: np.full(m.R, -7, np.int32)}
    for g in range(G):
        rows = np.nonzero(m.pred == g)[0]
        # one mask serves the rows of a predicate: the eighth's ends go by the product's own type
        if PREDICATES[g] is None:
            mask = passes(m.value, m.flags, m.ends[m.type_idx, 0], m.ends[m.type_idx, 1], 0, 0)
        else:
            mask = passes(m.value, m.flags, *PREDICATES[g])
        for r in rows:
            if r in t.where:
                c = t.per_type[t.where[r][0]][0]
                assert (mask[c] == m.ok[r][c]).all()
        if not mask.any():
            want[False][rows] = want[True][rows] = -1
            continue
        kept = np.nonzero(mask)[0].astype(np.int32)
        order = kept[np.argsort(m.type_idx[kept], kind="stable")]
        rowptr = np.concatenate([[0], np.cumsum(np.bincount(m.type_idx[kept], minlength=m.T))]).astype(np.int32)
        cand_type = np.where(mask, m.type_idx, -1).astype(np.int32)
        sub = lambda x: x[torch.from_numpy(rows).cuda()].contiguous()
        args = (t, sub(t.dproj), sub(t.dtypes), dev(targets[rows]), dev(rowptr), dev(order))
        plain = twin(*args, bias=bias)[0].cpu().numpy()
        ok_y = m.ok[rows, targets[rows]]
        want[False][rows] = np.where(ok_y, plain, -1)         # (the twin without lists does not look at the target's type)
        want[True][rows] = twin(*args, bias=bias, exclude=(dev(np.arange(len(rows), dtype=np.int32)),) + as_csr([lists[r] for r in rows]),
                                cand_type=dev(cand_type))[0].cpu().numpy()
        assert (want[True][rows][~ok_y] == -1).all()
    for filt in (False, True):
        assert (got[filt] == want[filt]).all(), (filt, np.nonzero(got[filt] != want[filt])[0][:10])
        assert (got[filt][~m.ok[np.arange(m.R), targets]] == -1).all()
    assert (got[False] > 0).sum() > 60 and (got[True] > 0).sum() > 60


# ---- 3. the null filter
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("table", ["fp32", "bf16"])
def test_a_filter_that_passes_everything_is_the_unfiltered_entry(mixed, table, kind):
    from p_companion_amd import ops
    m, t = mixed, getattr(mixed, table)
    bias = t.bias[kind]
    targets = make_targets(m, t, t.hbias[kind], seed=32)
    lists = lists_of(m, t, targets, seed=33)
    key = torch.arange(m.R, dtype=torch.int32, device="cuda")
    inf = lambda x: dev(np.full(m.R, x, np.float32))
    zero = dev(np.zeros(m.R, np.int32))
    wheres = (ops.RowWhere(), ops.RowWhere(value=m.dvalue, lo=inf(-INF), hi=inf(INF)),
              ops.RowWhere(flags=m.dflags, need=zero), ops.RowWhere(flags=m.dflags),
              ops.RowWhere(value=m.dvalue, flags=m.dflags, lo=inf(-INF), hi=inf(INF), need=zero, deny=zero))
    for exclude in (None, (key,) + as_csr(lists)):
        want, wbad = twin(t, t.dproj, t.dtypes, dev(targets), t.rowptr, t.col, bias=bias, exclude=exclude,
                          cand_type=None if exclude is None else t.dcand)
        for w in wheres:
            rank, bad = rank_where(m, t, targets, bias, exclude, where=w)
            assert torch.equal(rank, want) and bad.item() == wbad.item() == 1
    assert (want.cpu().numpy() >= 0).sum() > 100


# ---- 4. the predicate's edges, on integer-valued data
@pytest.mark.parametrize("dim", [128, 256])
def test_edge_values_on_a_hand_made_type(dim):
    """One type of 150 products (and a second of 50) with integer features and queries in [-4, 4]: every score is exact in both
    chains and in float64, so the rank is an exact numpy count.  Values: NaN, +-inf, -0.0, 0.0 and small integers; flags with
    bit 31.  Products 3, 5 and 9 are copies of one row: the target 9 is tied with 3 and 5."""
    from p_companion_amd import ops
    rng = np.random.default_rng(dim)
    P, T = 200, 2
    type_idx = np.zeros(P, np.int32)
    type_idx[150:] = 1
    feats = rng.integers(-4, 5, (P, dim)).astype(np.float32)
    feats[5] = feats[9] = feats[3]
    value = rng.integers(-3, 4, P).astype(np.float32)
    value[[0, 1, 2, 4]] = [np.nan, np.inf, -np.inf, -0.0]
    value[6], value[7] = 0.0, -0.0
    value[3], value[5], value[9] = 3.0, 1.0, 1.0             # 3 fails a band [0, 2]; 5 and 9 pass it
    flags = rng.integers(0, 16, P).astype(np.int32)
    flags[10:40] |= BIT31
    nan = np.float32(np.nan)
    preds = [(-INF, INF, 0, 0), (nan, INF, 0, 0), (-INF, nan, 0, 0), (nan, nan, 0, 0), (0.0, 2.0, 0, 0), (-0.0, 0.0, 0, 0),
             (0.0, -0.0, 0, 0), (1.0, 1.0, 0, 0), (-1.0, 1.0, 0, 0), (-INF, -INF, 0, 0), (INF, INF, 0, 0), (-INF, 0.0, 0, 0),
             (-INF, INF, int(BIT31), 0), (-INF, INF, 0, int(BIT31)), (-INF, INF, int(BIT31) | 1, 2), (0.0, 2.0, 1, int(BIT31)),
             (2.0, 1.0, 0, 0), (-INF, INF, 5, 5)]
    tg = [9, 5, 3, 6, 7, 20, 60, 149]
    rows = [(p, y) for p in preds for y in tg] + [((0.0, 2.0, 0, 0), 160), ((-INF, INF, 0, 0), 1)]      # 160: another type
    R = len(rows)
    lo, hi, need, deny = (np.array([p[k] for p, _ in rows], dt) for k, dt in enumerate((np.float32, np.float32, np.int32, np.int32)))
    targets = np.array([y for _, y in rows], np.int32)
    types = np.zeros(R, np.int32)
    proj = rng.integers(-4, 5, (R, dim)).astype(np.float32)
    ib = rng.integers(-50, 51, P).astype(np.float32)
    ib[[3, 5, 9]] = 7.0
    rowptr, col = dev(np.array([0, 150, 200], np.int32)), dev(np.arange(P, dtype=np.int32))
    where = ops.RowWhere(value=dev(value), flags=dev(flags), lo=dev(lo), hi=dev(hi), need=dev(need), deny=dev(deny))
    lists = [np.unique(rng.choice(150, LIST_LENGTHS[r % 6], replace=False)) for r in range(R)]
    key = torch.arange(R, dtype=torch.int32, device="cuda")
    table32 = dev(feats)
    s64 = feats[:150].astype(np.float64) @ proj.astype(np.float64).T                  # [150, R], exact
    cand = np.arange(150)
    for table in (table32, table32.to(torch.bfloat16)):
        for bias in (None, ib):
            s = s64 + (0 if bias is None else bias[:150, None].astype(np.float64))
            for exclude in (None, (key,) + as_csr(lists)):
                rank, bad = ops.rank_grouped_where(dev(proj), dev(types), dev(targets), rowptr, col, table, where,
                                                   bias=None if bias is None else dev(bias), exclude=exclude,
                                                   cand_type=None if exclude is None else dev(type_idx))
                rank = rank.cpu().numpy()
                assert bad.item() == 0
                for r in range(R):
                    y = targets[r]
                    ok = passes(value[:150], flags[:150], lo[r], hi[r], need[r], deny[r])
                    if exclude is not None:
                        ok = ok & ~np.isin(cand, lists[r])
                    if y >= 150:
                        # another type's product: a twin without lists counts against its score; with lists it is no candidate
                        if exclude is not None or not passes(value[y:y + 1], flags[y:y + 1], lo[r], hi[r], need[r], deny[r])[0]:
                            assert rank[r] == -1, r
                        continue
                    if not passes(value[y:y + 1], flags[y:y + 1], lo[r], hi[r], need[r], deny[r])[0] or \
                            (exclude is not None and y in lists[r]):
                        assert rank[r] == -1, (r, rows[r])
                        continue
                    g = s[y, r]
                    assert rank[r] == (ok & ((s[:, r] > g) | ((s[:, r] == g) & (cand < y)))).sum(), (r, rows[r])
    # what the table of predicates is there for
    p = lambda pr: passes(value[:150], flags[:150], *pr)
    assert p(preds[0]).sum() == 149 and not p(preds[1]).any() and not p(preds[2]).any() and not p(preds[3]).any()      # NaN
    assert p(preds[5]).sum() == p(preds[6]).sum() == (value[:150] == 0).sum() >= 3 and p(preds[5])[[4, 6, 7]].all()     # -0.0 == 0.0
    assert p(preds[7])[[5, 9]].all() and not p(preds[7])[3] and p(preds[9])[2] and p(preds[10])[1] and not p(preds[16]).any()
    assert p(preds[12]).sum() == 30 and p(preds[13]).sum() == 119 and not p(preds[17]).any()      # (119: product 0's value is NaN)
    assert p(preds[4])[[5, 9]].all() and not p(preds[4])[3]   # the target 9 under [0, 2]: 5 precedes it, 3 is not counted


# ---- 5. determinism
@pytest.mark.parametrize("table,kind", [("fp32", "none"), ("fp32", "half_norm"), ("bf16", "random")])
def test_same_ranks_for_every_slicing_candidate_order_row_order_and_call(mixed, table, kind):
    from p_companion_amd import ops
    m, t = mixed, getattr(mixed, table)
    bias = t.bias[kind]
    targets = make_targets(m, t, t.hbias[kind], seed=52)
    lists = lists_of(m, t, targets, seed=53)
    key = torch.arange(m.R, dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(54)
    col = t.col.cpu().numpy().copy()
    rp = t.rowptr.cpu().numpy()
    for c in range(m.T):
        col[rp[c]:rp[c + 1]] = rng.permutation(col[rp[c]:rp[c + 1]])
    perm = rng.permutation(m.R)
    dperm = torch.from_numpy(perm).cuda()
    pw = ops.RowWhere(value=m.dvalue, flags=m.dflags, lo=dev(m.lo[perm]), hi=dev(m.hi[perm]), need=dev(m.need[perm]),
                      deny=dev(m.deny[perm]))
    for exclude in (None, (key,) + as_csr(lists)):
        first = rank_where(m, t, targets, bias, exclude)[0]
        for s in SLICES:
            assert torch.equal(rank_where(m, t, targets, bias, exclude, slices=s)[0], first), s
        assert torch.equal(rank_where(m, t, targets, bias, exclude)[0], first)
        assert torch.equal(rank_where(m, t, targets, bias, exclude, slices=2, col=dev(col))[0], first)
        pex = None if exclude is None else (key[dperm].contiguous(),) + exclude[1:]
        got, _ = ops.rank_grouped_where(t.dproj[dperm].contiguous(), t.dtypes[dperm].contiguous(), dev(targets[perm]), t.rowptr,
                                        t.col, t.table, pw, exclude=pex, bias=bias,
                                        cand_type=None if exclude is None else t.dcand)
        assert torch.equal(got, first[dperm])
        assert (first.cpu().numpy() > 0).sum() > 60


# ---- 6. the float64 band over the passing products
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("table", ["fp32", "bf16"])
def test_every_rank_lies_in_the_float64_band_of_the_passing_products(mixed, table, kind):
    m, t = mixed, getattr(mixed, table)
    targets = make_targets(m, t, t.hbias[kind], seed=62)
    rank = rank_where(m, t, targets, t.bias[kind])[0].cpu().numpy()
    held = 0
    for r in t.where:
        cand, s64, a = view(t, r, t.hbias[kind])
        ok = m.ok[r][cand]
        j = np.searchsorted(cand, targets[r])
        if not ok[j]:
            assert rank[r] == -1, r
            continue
        lo = (ok & (s64 > s64[j] + a + a[j])).sum()
        hi = (ok & (s64 >= s64[j] - a - a[j])).sum() - 1      # (the target itself lies inside its own band)
        assert lo <= rank[r] <= hi, f"row {r}: rank {rank[r]} outside [{lo}, {hi}]"
        held += 1
    assert held > 100


# ---- 7. the C ABI
@pytest.mark.parametrize("table", ["fp32", "bf16"])
def test_error_codes_through_ctypes_leave_the_outputs_untouched(mixed, table):
    from p_companion_amd import _lib
    m, t = mixed, getattr(mixed, table)
    L = _lib.lib()
    name = "pc_rank_grouped_bf16_where" if table == "bf16" else "pc_rank_grouped_where"
    fn = getattr(L, name)
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    targets = make_targets(m, t, None, seed=72)
    lists = lists_of(m, t, targets, seed=73)
    key = torch.arange(m.R, dtype=torch.int32, device="cuda")
    ex_rowptr, ex_col = as_csr(lists)
    out = torch.full((m.R,), 12345, dtype=torch.int32, device="cuda")
    bad = torch.full((1,), 5, dtype=torch.int32, device="cuda")
    ws = torch.empty(getattr(L, name + "_workspace_bytes")(m.R, m.T, 0), dtype=torch.uint8, device="cuda")
    dtg = dev(targets)
    w = m.where
    parts = dict(value=w.value, lo=w.lo, hi=w.hi, flags=w.flags, need=w.need, deny=w.deny)

    def call(keep, keyed=True, **kw):
        st = None if keep is None else ctypes.byref(_lib.RowWhere(**{k: parts[k].data_ptr() for k in keep}))
        a = dict(proj=p(t.dproj), types=p(t.dtypes), targets=p(dtg), row_key=p(key) if keyed else None, rows=m.R,
                 type_rowptr=p(t.rowptr), type_col=p(t.col), table=p(t.table), bias=None, n_types=m.T, num_products=m.P,
                 ex_rowptr=p(ex_rowptr) if keyed else None, ex_col=p(ex_col) if keyed else None,
                 n_keys=m.R if keyed else 0, cand_type=p(t.dcand) if keyed else None, dim=m.dim, slices=0, rank_out=p(out),
                 bad_count=p(bad), where=st, ws=p(ws), ws_bytes=ws.numel(),
                 stream=ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        a.update(kw)
        return fn(*a.values())

    full = tuple(parts)
    for keyed in (True, False):
        assert call(None, keyed) == -1                                                   # a null where
        for keep in (("lo",), ("hi",), ("lo", "hi"), ("value",), ("value", "lo"), ("value", "hi"), ("need",), ("deny",),
                     ("need", "deny"), ("value", "lo", "hi", "need"), ("flags", "need", "hi"), ("value", "flags", "need", "deny")):
            assert call(keep, keyed) == -1, keep                                         # PC_EINVAL: the pairing rules
        assert call(full, keyed, dim=64) == -2 and call(full, keyed, slices=65) == -2
        assert call(full, keyed, ws_bytes=ws.numel() - 1) == -3 and call(full, keyed, table=None) == -1
        assert call(full, keyed, rank_out=None) == -1 and call(full, keyed, num_products=0) == -1
        assert call(("need",), keyed, dim=64) == -1                                      # the pointers before the shapes
    assert call(full, True, cand_type=None) == -1 and call(full, False, cand_type=p(t.dcand)) == -1    # lists without cand_type
    assert call(full, True, ex_col=None) == -1 and call(full, True, row_key=None) == -1
    torch.cuda.synchronize()
    assert (out == 12345).all() and int(bad) == 5
    # and the calls that are in order are served, the counter added to
    for keyed in (True, False):
        assert call(full, keyed) == 0
        torch.cuda.synchronize()
        want, _ = rank_where(m, t, targets, None, (key, ex_rowptr, ex_col) if keyed else None)
        assert torch.equal(out, want)
    assert int(bad) == 7                                      # 5 + the row of type T, twice


@pytest.mark.parametrize("table", ["fp32", "bf16"])
def test_bad_keys_and_targets_are_counted_as_in_the_twin(mixed, table):
    m, t = mixed, getattr(mixed, table)
    targets = make_targets(m, t, None, seed=82)
    lists = lists_of(m, t, targets, seed=83)
    typed = [r for r in range(m.R) if r in t.where]
    targets[typed[:3]] = [-1, m.P, 2 ** 31 - 1]               # out of range: -1 and counted
    key = np.arange(m.R, dtype=np.int32)
    key[typed[3:7]] = [m.R, m.R + 1000, -2, 2 ** 31 - 1]      # no list, counted
    ex = (dev(key),) + as_csr(lists)
    bad, twin_bad = (torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(2))
    rank, _ = rank_where(m, t, targets, None, ex, bad=bad, where=type(m.where)())
    from p_companion_amd import ops
    fn = ops.rank_grouped_bf16 if table == "bf16" else ops.rank_grouped
    want, _ = fn(t.dproj, t.dtypes, dev(targets), t.rowptr, t.col, t.table, exclude=ex, cand_type=t.dcand, bad=twin_bad)
    assert torch.equal(rank, want) and int(bad) == int(twin_bad) == 1 + 3 + 4        # the row of type T, the targets, the keys
    assert (rank[torch.tensor(typed[:3]).cuda()] == -1).all()
    rank2, _ = rank_where(m, t, targets, None, ex, bad=bad)
    assert int(bad) == 16 and (rank2[torch.tensor(typed[:3]).cuda()] == -1).all()          # (added to)
    got = rank2.cpu().numpy()
    for r in typed[3:7]:                                      # a bad key is no list: the rank without one
        if m.ok[r][targets[r]]:
            assert got[r] >= 0


# ---- 8. the complement methods
@pytest.fixture(scope="module")
def complements():
    from test_gpu_catalogue_eval import cfg, trained_model
    from test_gpu_retrieval_list import _graph
    from p_companion_amd.data import ComplementaryIndexDataset
    dim, products = 128, 20_000
    bpg = _graph("int", dim)
    c = cfg(100, dim)
    gen = torch.Generator().manual_seed(21)
    value = (torch.rand(products, generator=gen) * 100 + 1).cuda()
    flags = torch.randint(-2 ** 31, 2 ** 31, (products,), generator=gen, dtype=torch.int64).to(torch.int32).cuda()
    ds = ComplementaryIndexDataset(bpg, "test", seed=2)
    pairs = torch.from_numpy(np.ascontiguousarray(ds.pairs[ds.pairs[:, 2] == 1][:, :2], dtype=np.int32)).cuda()
    return SimpleNamespace(bpg=bpg, c=c, model=trained_model(bpg, c), value=value, flags=flags, ds=ds, pairs=pairs)


@pytest.mark.parametrize("catalogue", ["fp32", "compact"])
def test_rank_targets_where_and_evaluate_catalogue_where(complements, catalogue):
    from p_companion_amd import ops
    from p_companion_amd.inference import CompactInference, PCompanionInference
    from p_companion_amd.metrics import Metrics
    v = complements
    if catalogue == "compact":
        feats = v.bpg.cuda()["features"]
        inf = CompactInference(v.model, v.c, v.bpg, catalogue=ops.CompactCatalogue(ops.catalogue_bf16(feats)))
    else:
        inf = PCompanionInference(v.model, v.c, v.bpg)
    # the pairs: those whose type a slot predicts (up to 1 200 of them) among 300 whose type none does
    typed_all = inf.rank_targets(v.pairs[:, 0].contiguous(), v.pairs[:, 1].contiguous())[0] >= 0
    sel = torch.cat([torch.nonzero(typed_all).reshape(-1)[:1200], torch.nonzero(~typed_all).reshape(-1)[:300]]).sort().values
    q, y = v.pairs[sel, 0].contiguous(), v.pairs[sel, 1].contiguous()
    b = len(q)
    assert int(typed_all[sel].sum()) >= 100
    f = lambda x: torch.full((b,), x, dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="no per-product attributes"):
        inf.rank_targets_where(q, y, lo=f(0.0))
    inf.set_attributes(value=v.value, flags=v.flags)
    with pytest.raises(ValueError, match="at least one of"):
        inf.rank_targets_where(q, y)
    need = torch.full((b,), 1, dtype=torch.int32, device="cuda")
    mask = (v.value >= 20.0) & (v.value <= 60.0) & ((v.flags & 1) == 1)
    for exclusions in (False, True):
        if exclusions:
            inf.set_exclusions()
        # a shared predicate: rank_targets under set_eligible(its mask)
        inf.set_eligible(mask)
        want = inf.rank_targets(q, y)
        inf.set_eligible(None)
        got = inf.rank_targets_where(q, y, lo=f(20.0), hi=f(60.0), need=need)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), exclusions
        assert int((got[1] >= 0).sum()) >= 10 and int(((got[0] >= 0) & (got[1] < 0)).sum()) >= 10
        take = torch.arange(b, device="cuda") % 3 != 0
        s3, r3 = inf.rank_targets_where(q, y, lo=f(20.0), hi=f(60.0), need=need, take=take)
        assert torch.equal(s3, torch.where(take, got[0], -1)) and torch.equal(r3, torch.where(take, got[1], -1))
    # per-query bands, exclusions installed: rank < 256 exactly when recommend_where_batch holds the target there
    lo, hi = inf.band_around(q)
    slot, rank = inf.rank_targets_where(q, y, lo=lo, hi=hi)
    types, idx, _ = inf.recommend_where_batch(q, N, lo=lo, hi=hi)
    ty = inf.type_idx[y.long()].long()
    match = types == ty[:, None]
    assert torch.equal(slot.long(), torch.where(match.any(1), match.int().argmax(1), -1))
    lists = idx[torch.arange(b, device="cuda"), slot.clamp(min=0).long()]               # [B, 256]
    held = lists == y[:, None]
    pos = torch.where(held.any(1), held.int().argmax(1), -1)
    typed = slot >= 0
    assert torch.equal(rank[~typed], torch.full_like(rank[~typed], -1))
    inside = typed & (rank >= 0) & (rank < N)
    assert torch.equal(pos[inside].int(), rank[inside]) and not held[typed & ~inside].any()
    passing = (lo <= v.value[y.long()]) & (v.value[y.long()] <= hi)
    assert (rank[typed & ~passing] == -1).all() and int((typed & ~passing).sum()) > 5 and int(inside.sum()) > 20
    # evaluate_catalogue_where against the metrics of the ranks the served lists give
    ks = (1, 3, 10, 100, 256)
    predicate = lambda qi: dict(zip(("lo", "hi"), inf.band_around(qi)))
    got = inf.evaluate_catalogue_where(v.ds, predicate, ks=ks, chunk=4096)
    assert list(got) == ["pairs", "type_hit"] + [f"hit@{k}" for k in ks] + ["mrr", "median_rank", "filtered_targets"]
    assert inf.evaluate_catalogue_where(v.ds, predicate, ks=ks, chunk=100_000) == got
    aq, ay = v.pairs[:, 0].contiguous(), v.pairs[:, 1].contiguous()
    slots, ranks = [], []
    for s in range(0, len(aq), 4096):
        cq, cy = aq[s:s + 4096], ay[s:s + 4096]
        clo, chi = inf.band_around(cq)
        ctypes_, cidx, _ = inf.recommend_where_batch(cq, N, lo=clo, hi=chi)
        cm = ctypes_ == inf.type_idx[cy.long()].long()[:, None]
        cs = torch.where(cm.any(1), cm.int().argmax(1), -1)
        ch = cidx[torch.arange(len(cq), device="cuda"), cs.clamp(min=0)] == cy[:, None]
        slots.append(cs.int())
        ranks.append(torch.where(ch.any(1) & (cs >= 0), ch.int().argmax(1), -1).int())
    ref = Metrics.catalogue_metrics(torch.cat(slots), torch.cat(ranks), ks)
    assert got["pairs"] == ref["pairs"] == len(aq) and got["type_hit"] == ref["type_hit"] > 0
    for k in ks:
        assert got[f"hit@{k}"] == ref[f"hit@{k}"], k
    assert got["hit@256"] > 0
    # filtered_targets in numpy: in the query's exclusion list, or failing its own band
    ex_rowptr, ex_col = (x.cpu().numpy() for x in inf.exclusions)
    hq, hy, hv = aq.cpu().numpy(), ay.cpu().numpy(), v.value.cpu().numpy()
    hlo, hhi = (x.cpu().numpy() for x in inf.band_around(aq))
    out = ~passes(hv[hy], np.zeros_like(hy), hlo, hhi, 0, 0)
    out |= np.array([hy[i] in ex_col[ex_rowptr[hq[i]]:ex_rowptr[hq[i] + 1]] for i in range(len(hq))])
    assert got["filtered_targets"] == int(out.sum()) > 0
    inf.set_exclusions(False)
    inf.set_attributes()


def test_a_bare_bf16_catalogue_stays_refused(complements):
    from p_companion_amd.inference import PCompanionInference
    v = complements
    inf = PCompanionInference(v.model, v.c, v.bpg, catalogue=torch.bfloat16).set_attributes(value=v.value)
    q = v.pairs[:8, 0].contiguous()
    lo = torch.zeros(8, device="cuda")
    with pytest.raises(ValueError, match="the rank kernels read the fp32 catalogue"):
        inf.rank_targets_where(q, q, lo=lo)
    with pytest.raises(ValueError, match="the rank kernels read the fp32 catalogue"):
        inf.evaluate_catalogue_where(v.ds, lambda qi: dict(lo=lo))


# ---- 9. the substitute methods
@pytest.mark.parametrize("cls", ["SimilarProducts", "CompactSimilarProducts"])
@pytest.mark.parametrize("scope", ["type", "catalogue"])
def test_rank_pairs_where_and_evaluate_pairs_where(scope, cls):
    from p_companion_amd import inference, ops
    from p_companion_amd.metrics import Metrics
    products, dim, n_types = 3000, 128, 6
    rng = np.random.default_rng(41)
    type_idx = rng.integers(0, n_types, products).astype(np.int32)
    table = dev(rng.standard_normal((products, dim)).astype(np.float32))
    if cls == "CompactSimilarProducts":
        table = ops.catalogue_bf16(table)
    sp = getattr(inference, cls)(table, _Graph(type_idx, n_types), scope=scope)
    value = dev((rng.random(products) * 100 + 1).astype(np.float32))
    flags = dev(rng.integers(-2 ** 31, 2 ** 31, products).astype(np.int32))
    a = torch.arange(0, products, 7, dtype=torch.int32)
    b = len(a)
    # targets: the anchor's own neighbours at mixed depths, any product, the anchor itself
    sp.set_attributes(value=value, flags=flags)
    lo, hi = sp.band_around(a, 0.5, 2.0)
    deny = torch.full((b,), int(BIT31) | 1, dtype=torch.int32, device="cuda")
    idx, _ = sp.similar_where_batch(a, N, lo=lo, hi=hi, deny=deny)
    depth = torch.from_numpy(rng.integers(0, N, b)).cuda()
    y = idx[torch.arange(b, device="cuda"), depth]
    anywhere = torch.from_numpy(rng.integers(0, products, b).astype(np.int32)).cuda()
    y = torch.where((y < 0) | (torch.arange(b, device="cuda") % 3 == 0), anywhere, y)
    y[::50] = a.cuda()[::50]
    with pytest.raises(ValueError, match="at least one of"):
        sp.rank_pairs_where(a, y)
    slot, rank = sp.rank_pairs_where(a, y, lo=lo, hi=hi, deny=deny)
    plain_slot, _ = sp.rank_pairs(a, y)
    assert torch.equal(slot, plain_slot)                      # a target that fails keeps its slot
    held = idx == y[:, None]
    pos = torch.where(held.any(1), held.int().argmax(1), -1)
    inside = (rank >= 0) & (rank < N)
    assert torch.equal(pos[inside].int(), rank[inside]) and not held[~inside].any()
    vy, fy = value[y.long()], flags[y.long()]
    ok = (lo <= vy) & (vy <= hi) & ((fy & (int(BIT31) | 1)) == 0)
    assert (rank[~ok] == -1).all() and (rank[::50] == -1).all() and int(inside.sum()) > 50 and int((~ok).sum()) > 20
    assert int(((rank >= N)).sum()) > 5 or scope == "type"
    # a shared predicate: rank_pairs under set_eligible(its mask)
    f = lambda x: torch.full((b,), x, dtype=torch.float32, device="cuda")
    sp.set_eligible((value >= 30.0) & (value <= 70.0))
    want = sp.rank_pairs(a, y)
    sp.set_eligible(None)
    got = sp.rank_pairs_where(a, y, lo=f(30.0), hi=f(70.0))
    assert torch.equal(got[0], plain_slot) and torch.equal(got[1], want[1])
    # evaluate_pairs_where: the metrics of the ranks the served lists give, for k <= 256
    ks = (1, 3, 10, 100, 256)
    pairs = torch.stack([a.cuda(), y], 1)
    predicate = lambda q: dict(zip(("lo", "hi"), sp.band_around(q, 0.5, 2.0)), deny=torch.full((len(q),), int(BIT31) | 1, dtype=torch.int32, device="cuda"))
    res = sp.evaluate_pairs_where(pairs, predicate, ks=ks, chunk=100)
    ref = Metrics.catalogue_metrics(slot, torch.where(held.any(1), pos, -1).int(), ks)
    assert res["pairs"] == b and res["type_hit"] == ref["type_hit"] and all(res[f"hit@{k}"] == ref[f"hit@{k}"] for k in ks)
    assert res == Metrics.catalogue_metrics(slot, rank, ks) and res["hit@256"] > 0
