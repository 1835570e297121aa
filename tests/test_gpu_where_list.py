"""Per-query attribute filters: pc_retrieve_list_grouped_where and its bf16 / biased twins (ops.retrieve_list_grouped_where with
an ops.RowWhere), PCompanionInference.recommend_where_batch and SimilarProducts / CompactSimilarProducts.similar_where_batch.
Needs an MI355X.

Every comparison is bit for bit -- ids as they are, scores as int32 patterns -- and the reference is never the code under
test: it is the EXISTING unfiltered entry (retrieve_list_grouped, its bf16 table, _biased, _bf16_biased) over a CSR rebuilt from
the products that pass a predicate, as set_eligible rebuilds it, one call per predicate; the predicate itself is evaluated in
numpy (fp32 compares, 32-bit masks).  The catalogue, rows, keys and exclusion lists are tests/test_gpu_retrieval_list.py's
(12 350 products in types of 9000 / 3000 / 300 / 40 / 10 / 0, row counts around the 16-row tile, rows of type -1 and T, NS
across both buffer-size thresholds, D = 128 and 256); the rows are dealt round-robin over eight predicates, so every 16-row
tile mixes them."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_retrieval_list import N_KEYS, NS, P, T, _graph, bits, cat, cuda, same      # noqa: F401  (cat: a fixture)

ENTRIES = ("fp32", "bf16", "biased", "bf16_biased")
BIT31 = np.int32(-2 ** 31)
INF = np.float32(np.inf)
# (lo, hi, need, deny) per predicate; None: filled in by the fixture (the ends that are products' own values)
PREDICATES = [(-INF, INF, 0, 0),                                          # 0 all-pass
              (0.6, 0.4, 0, 0),                                           # 1 lo > hi: nothing
              (0.25, 0.75, 0, 0),                                         # 2 about half
              (0.5, 0.51, 0, 0),                                          # 3 about 1 %
              (-INF, INF, int(BIT31) | 1, 0),                             # 4 need alone (bit 31 among the bits)
              (-INF, INF, 0, int(BIT31) | 4),                             # 5 deny alone
              (0.1, 0.9, 2, int(BIT31)),                                  # 6 band + need + deny
              None]                                                       # 7 a band whose ends are products' values
G = len(PREDICATES)


def passes(value, flags, lo, hi, need, deny):
    """The contract in numpy: two fp32 compares and two 32-bit masks."""
    lo, hi, need, deny = np.float32(lo), np.float32(hi), np.int32(need), np.int32(deny)
    with np.errstate(invalid="ignore"):
        return (lo <= value) & (value <= hi) & ((flags & need) == need) & ((flags & deny) == 0)


def old_entry(m, entry, proj, types, rowptr, col, n, exclude=None, bad=None):
    from p_companion_amd import ops
    table = m.table16 if "bf16" in entry else m.table
    args = (proj, types, rowptr, col, table)
    if entry == "biased":
        return ops.retrieve_list_grouped_biased(*args, m.bias, n, exclude=exclude, bad=bad)
    if entry == "bf16_biased":
        return ops.retrieve_list_grouped_bf16_biased(*args, m.bias, n, exclude=exclude, bad=bad)
    return ops.retrieve_list_grouped(*args, n, exclude=exclude, bad=bad)


def new_entry(m, entry, n, where, filt=False, slices=0, col=None, rows=None, bad=None, key=None):
    from p_companion_amd import ops
    pick = (lambda t: t) if rows is None else (lambda t: t[rows].contiguous())
    exclude = ((pick(m.dkey) if key is None else key,) + m.ex) if filt else None
    return ops.retrieve_list_grouped_where(pick(m.dproj), pick(m.dtypes), m.rowptr, m.col if col is None else col,
                                           m.table16 if "bf16" in entry else m.table, n, where, slices=slices, exclude=exclude,
                                           bad=bad, bias=m.bias if "biased" in entry else None)


@pytest.fixture(scope="module")
def wcat(cat):
    """tests/test_gpu_retrieval_list.py's catalogue with a value and flags per product and a predicate per row."""
    from p_companion_amd import ops
    m = cat
    rng = np.random.default_rng(77 + m.dim)
    value = rng.random(P).astype(np.float32)
    lo3, hi3 = np.float32(PREDICATES[3][0]), np.float32(PREDICATES[3][1])
    in3 = (value >= lo3) & (value <= hi3)
    value[in3 & (m.type_idx == 3)] = np.float32(0.52)         # the 1 % band leaves the 40-product type with nothing
    flags = rng.integers(-2 ** 31, 2 ** 31, P).astype(np.int32)
    t0 = m.by(0)
    ends = np.sort(value[t0])[[3000, 4000]]                   # predicate 7: from one product's value to another's, inclusive
    preds = [p if p is not None else (ends[0], ends[1], 0, 0) for p in PREDICATES]
    masks = [passes(value, flags, *p) for p in preds]
    count = lambda g, t: int((masks[g] & (m.type_idx == t)).sum())
    assert masks[0].all() and not masks[1].any() and 0.45 * P < masks[2].sum() < 0.55 * P
    assert 60 < count(3, 0) < 128 and 10 <= count(3, 1) < 64 and 1 <= count(3, 2) < 10 and count(3, 3) == 0
    assert 0.2 * P < masks[4].sum() < 0.3 * P and 0.2 * P < masks[5].sum() < 0.3 * P and 0.15 * P < masks[6].sum() < 0.25 * P
    assert count(7, 0) == 1001 and masks[7][t0[np.argsort(value[t0])[[3000, 4000]]]].all()      # both ends pass
    g_of = (np.arange(m.R) % G).astype(np.int64)              # round-robin: every 16-row tile mixes the predicates
    col = lambda j, dt: np.array([preds[g][j] for g in g_of], dt)
    lo, hi, need, deny = col(0, np.float32), col(1, np.float32), col(2, np.int64).astype(np.int32), col(3, np.int64).astype(np.int32)
    w = SimpleNamespace(**vars(m))
    w.value, w.flags, w.preds, w.masks, w.g_of = value, flags, preds, masks, g_of
    w.lo, w.hi, w.need, w.deny = lo, hi, need, deny
    w.dvalue, w.dflags = cuda(value), cuda(flags)
    w.where = ops.RowWhere(w.dvalue, w.dflags, cuda(lo), cuda(hi), cuda(need), cuda(deny))
    w.table16 = ops.catalogue_bf16(m.table)
    w.bias = cuda((np.random.default_rng(3).standard_normal(P) * 10).astype(np.float32))
    # the CSR of each predicate's passing products, as set_eligible builds it
    w.csr = []
    type_dev = cuda(m.type_idx)
    for g in range(G):
        ids = torch.nonzero(cuda(masks[g])).reshape(-1).to(torch.int32)
        if ids.numel() == 0:                                  # (no candidate anywhere: every type empty, one unread column)
            w.csr.append((torch.zeros(T + 1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")))
            continue
        rowptr, local = ops.type_csr(type_dev[ids.long()].contiguous(), T)
        w.csr.append((rowptr, ids[local.long()].contiguous()))
    w.wanted = {}
    return w


def reference(w, entry, n, filt):
    """The existing entry over each predicate's CSR, its rows in their places: [R, n], computed once per (entry, filt) at 256
    (a list is the head of the longer list: tests/test_gpu_retrieval_list.py's references are cut the same way)."""
    if (entry, filt) not in w.wanted:
        idx = torch.empty(w.R, 256, dtype=torch.int32, device="cuda")
        sc = torch.empty(w.R, 256, dtype=torch.float32, device="cuda")
        for g in range(G):
            sel = cuda(np.nonzero(w.g_of == g)[0])
            exclude = ((w.dkey[sel].contiguous(),) + w.ex) if filt else None
            idx[sel], sc[sel] = old_entry(w, entry, w.dproj[sel].contiguous(), w.dtypes[sel].contiguous(), *w.csr[g], 256,
                                          exclude=exclude)
        w.wanted[entry, filt] = (idx, sc)
    idx, sc = w.wanted[entry, filt]
    return idx[:, :n].contiguous(), sc[:, :n].contiguous()


# ---- 1. against the existing entry
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("filt", [False, True], ids=["plain", "excluding"])
@pytest.mark.parametrize("n", NS)
def test_one_call_equals_the_existing_entry_over_each_predicates_csr(wcat, n, filt, entry):
    w = wcat
    got, want = new_entry(w, entry, n, w.where, filt), reference(w, entry, n, filt)
    assert got[0].shape == (w.R, n) and got[0].dtype == torch.int32 and got[1].dtype == torch.float32
    assert torch.equal(got[0], want[0]), (n, torch.nonzero((got[0] != want[0]).any(1)).reshape(-1)[:10].tolist())
    assert torch.equal(bits(got[1]), bits(want[1])), n


# ---- 2. the null filter
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("n", [40, 200])
def test_a_filter_that_passes_everything_is_the_unfiltered_entry(wcat, n, entry):
    from p_companion_amd import ops
    w = wcat
    full = lambda x, dt: torch.full((w.R,), x, dtype=dt, device="cuda")
    zero = full(0, torch.int32)
    wheres = (ops.RowWhere(), ops.RowWhere(w.dvalue, w.dflags, full(-np.inf, torch.float32), full(np.inf, torch.float32), zero, zero),
              ops.RowWhere(value=w.dvalue, lo=full(-np.inf, torch.float32), hi=full(np.inf, torch.float32)),
              ops.RowWhere(flags=w.dflags), ops.RowWhere(flags=w.dflags, deny=zero))
    for filt in (False, True):
        want = old_entry(w, entry, w.dproj, w.dtypes, w.rowptr, w.col, n, exclude=((w.dkey,) + w.ex) if filt else None)
        for i, where in enumerate(wheres):
            assert same(new_entry(w, entry, n, where, filt), want), (filt, i)


# ---- 3. the predicate itself
@pytest.mark.parametrize("entry", ["fp32", "bf16_biased"])
@pytest.mark.parametrize("filt", [False, True], ids=["plain", "excluding"])
@pytest.mark.parametrize("n", [10, 64, 256])
def test_every_served_id_passes_and_every_row_is_as_long_as_it_can_be(wcat, n, filt, entry):
    w = wcat
    idx, sc = (x.cpu().numpy() for x in new_entry(w, entry, n, w.where, filt))
    lengths = set()
    for r in range(w.R):
        t, g = w.types[r], w.g_of[r]
        got = idx[r][idx[r] >= 0]
        k = len(got)
        assert (idx[r, :k] >= 0).all() and (idx[r, k:] == -1).all() and np.isneginf(sc[r, k:]).all() and np.isfinite(sc[r, :k]).all()
        assert len(set(got.tolist())) == k
        if not 0 <= t < T:
            assert k == 0, r
            continue
        ok = w.masks[g] & (w.type_idx == t)
        if filt and w.key[r] >= 0:
            ok[np.asarray(w.lists[w.key[r]], np.int64)] = False
        assert ok[got].all(), (r, g)
        assert passes(w.value[got], w.flags[got], w.lo[r], w.hi[r], w.need[r], w.deny[r]).all(), (r, g)
        assert k == min(n, int(ok.sum())), (r, g, k, int(ok.sum()))
        assert (np.diff(sc[r, :k]) <= 0).all()
        lengths.add(k)
    assert 0 in lengths and n in lengths and len(lengths) >= 3


# ---- 4. edge values
def test_edge_values_on_a_hand_made_type():
    """One type of 12 products whose score under every row is the product's own first feature (5, 4, 4, 3, 2, 1, 0.5, ...): a
    NaN value is never served, a NaN bound serves nothing, both ends of a band are served, -0.0 == 0.0, bit 31 works in need
    and in deny, and a product tied in score with a failing lower id is served first."""
    from p_companion_amd import ops
    score = np.array([5, 4, 4, 3, 2, 1, 0.5, 0.25, 0.125, 0.0625, 0.03125, 0.015625], np.float32)
    value = np.array([np.nan, 1, 2, 3, -0.0, 0.0, 10, 11, 12, 13, 14, 15], np.float32)
    flags = np.array([BIT31 | 1, 0, BIT31, 1, 0, 3, BIT31 | 2, 0, BIT31, 1, 0, 7], np.int32)
    nan, inf = np.float32(np.nan), INF
    rows = [  # (lo, hi, need, deny) -> the served ids in order
        ((1, 3, 0, 0), [1, 2, 3]),                            # value == lo and value == hi are served; the NaN product is not
        ((nan, 3, 0, 0), []), ((1, nan, 0, 0), []), ((nan, nan, 0, 0), []),
        ((0.0, 0.0, 0, 0), [4, 5]), ((-0.0, -0.0, 0, 0), [4, 5]),
        ((-inf, inf, 0, 0), list(range(1, 12))),              # every non-NaN value
        ((-inf, inf, int(BIT31), 0), [2, 6, 8]), ((-inf, inf, 0, int(BIT31)), [1, 3, 4, 5, 7, 9, 10, 11]),
        ((-inf, inf, int(BIT31) | 2, 0), [6]), ((-inf, inf, 1, int(BIT31)), [3, 5, 9, 11]),
        ((2, 3, 0, 0), [2, 3]),                               # 1 and 2 tie at score 4; 1 fails: 2 leads
        ((3, 1, 0, 0), []), ((inf, inf, 0, 0), []), ((10, 15, 1, 2), [9]),
    ]
    flag_rows = [((0, 0), list(range(12))), ((int(BIT31), 0), [0, 2, 6, 8]), ((0, int(BIT31)), [1, 3, 4, 5, 7, 9, 10, 11]),
                 ((int(BIT31) | 1, 0), [0]), ((-1, 0), []), ((0, -1), [1, 4, 7, 10])]
    for (lo, hi, need, deny), ids in rows:                    # the table above agrees with the contract in numpy
        assert np.nonzero(passes(value, flags, lo, hi, need, deny))[0].tolist() == ids
    for dim in (128, 256):
        feats = np.zeros((12, dim), np.float32)
        feats[:, 0] = score
        table = cuda(feats)
        tables = {"fp32": table, "bf16": ops.catalogue_bf16(table)}         # (the scores are exact in bf16 too)
        rowptr, col = cuda(np.array([0, 12], np.int32)), cuda(np.arange(12, dtype=np.int32))
        zero_bias = torch.zeros(12, device="cuda")

        def serve(preds, n, which, bias, **parts):
            r = len(preds)
            proj = np.zeros((r, dim), np.float32)
            proj[:, 0] = 1
            return ops.retrieve_list_grouped_where(cuda(proj), torch.zeros(r, dtype=torch.int32, device="cuda"), rowptr, col,
                                                   tables[which], n, ops.RowWhere(**parts), bias=zero_bias if bias else None)

        for n in (12, 40, 100):
            for which in ("fp32", "bf16"):
                for bias in (False, True):
                    p = [x for x, _ in rows]
                    arr = lambda j, dt: cuda(np.array([x[j] for x in p]).astype(dt))
                    idx, sc = serve(p, n, which, bias, value=cuda(value), flags=cuda(flags), lo=arr(0, np.float32),
                                    hi=arr(1, np.float32), need=arr(2, np.int32), deny=arr(3, np.int32))
                    idx, sc = idx.cpu().numpy(), sc.cpu().numpy()
                    for r, (_, ids) in enumerate(rows):
                        assert idx[r, :len(ids)].tolist() == ids and (idx[r, len(ids):] == -1).all(), (dim, n, which, bias, r)
                        assert (sc[r, :len(ids)] == score[ids]).all() and np.isneginf(sc[r, len(ids):]).all()
                    # flags alone: no band, so the NaN product is a candidate like the others
                    p = [x for x, _ in flag_rows]
                    idx, _ = serve(p, n, which, bias, flags=cuda(flags), need=cuda(np.array([x[0] for x in p], np.int32)),
                                   deny=cuda(np.array([x[1] for x in p], np.int32)))
                    idx = idx.cpu().numpy()
                    for r, (_, ids) in enumerate(flag_rows):
                        assert idx[r, :len(ids)].tolist() == ids and (idx[r, len(ids):] == -1).all(), (dim, n, which, bias, r)


# ---- 5. invariance
@pytest.mark.parametrize("entry", ["fp32", "bf16_biased"])
@pytest.mark.parametrize("n", [40, 200])
def test_same_bits_for_every_slicing_candidate_order_row_order_and_call(wcat, n, entry):
    from p_companion_amd import ops
    w = wcat
    rowptr = w.rowptr.cpu().numpy()
    col = w.col.cpu().numpy().copy()
    rng = np.random.default_rng(9)
    for t in range(T):
        rng.shuffle(col[rowptr[t]:rowptr[t + 1]])
    perm = rng.permutation(w.R)
    dperm = cuda(perm)
    where_p = ops.RowWhere(w.dvalue, w.dflags, *(cuda(a[perm]) for a in (w.lo, w.hi, w.need, w.deny)))
    for filt in (False, True):
        want = reference(w, entry, n, filt)
        for c, s in ((None, 1), (None, 7), (None, 0), (None, 0), (cuda(col), 0), (cuda(col), 5)):
            assert same(new_entry(w, entry, n, w.where, filt, slices=s, col=c), want), (filt, s, c is not None)
        got = new_entry(w, entry, n, where_p, filt, rows=dperm)
        assert same(got, (want[0][dperm], want[1][dperm])), filt


# ---- 6. refusals
@pytest.mark.parametrize("entry", ENTRIES)
def test_error_codes_through_ctypes_leave_the_outputs_untouched(wcat, entry):
    from p_companion_amd import _lib
    w = wcat
    L = _lib.lib()
    name = {"fp32": "pc_retrieve_list_grouped_where", "bf16": "pc_retrieve_list_grouped_bf16_where",
            "biased": "pc_retrieve_list_grouped_biased_where", "bf16_biased": "pc_retrieve_list_grouped_bf16_biased_where"}[entry]
    fn = getattr(L, name)
    n = 100
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    out_i = torch.full((w.R, n), 12345, dtype=torch.int32, device="cuda")
    out_s = torch.full((w.R, n), 7.0, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = torch.empty(getattr(L, name + "_workspace_bytes")(w.R, T, n, 0), dtype=torch.uint8, device="cuda")
    parts = dict(value=w.where.value, lo=w.where.lo, hi=w.where.hi, flags=w.where.flags, need=w.where.need, deny=w.where.deny)

    def call(keep, keyed=True, **kw):
        st = None if keep is None else ctypes.byref(_lib.RowWhere(**{k: parts[k].data_ptr() for k in keep}))
        a = dict(proj=p(w.dproj), types=p(w.dtypes), row_key=p(w.dkey) if keyed else None, rows=w.R, type_rowptr=p(w.rowptr),
                 type_col=p(w.col), table=p(w.table16 if "bf16" in entry else w.table))
        if "biased" in entry:
            a["bias"] = p(w.bias)
        a.update(n_types=T, ex_rowptr=p(w.ex[0]) if keyed else None, ex_col=p(w.ex[1]) if keyed else None,
                 n_keys=N_KEYS if keyed else 0, n=n, dim=w.dim, slices=0, out_idx=p(out_i), out_score=p(out_s),
                 bad_count=p(bad) if keyed else None, where=st, ws=p(ws), ws_bytes=ws.numel(),
                 stream=ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        a.update(kw)
        return fn(*a.values())

    for keyed in (True, False):
        assert call(None, keyed) == -1                                                   # a null where
        for keep in (("lo",), ("hi",), ("lo", "hi"), ("value",), ("value", "lo"), ("value", "hi"), ("need",), ("deny",),
                     ("need", "deny"), ("value", "lo", "hi", "need"), ("flags", "need", "hi"), ("value", "flags", "need", "deny")):
            assert call(keep, keyed) == -1, keep                                         # PC_EINVAL: the pairing rules
        full = tuple(parts)
        assert call(full, keyed, n=257) == -2 and call(full, keyed, dim=64) == -2 and call(full, keyed, slices=65) == -2
        assert call(full, keyed, ws_bytes=ws.numel() - 1) == -3 and call(full, keyed, table=None) == -1
        assert call(("need",), keyed, n=257) == -1                                       # the pointers before the shapes
    torch.cuda.synchronize()
    assert (out_i == 12345).all() and (out_s == 7.0).all() and int(bad) == 0
    # and the calls that are in order are served: flags with one mask, a band alone, everything
    for keep, keyed in ((("flags", "need"), True), (("flags", "deny"), False), (("value", "lo", "hi"), True), (tuple(parts), True)):
        assert call(keep, keyed) == 0, keep
    torch.cuda.synchronize()
    assert same((out_i, out_s), reference(w, entry, n, True)) and int(bad) == 0


def test_a_bad_exclusion_key_is_counted_as_in_the_twin(wcat):
    w = wcat
    n = 64
    key = w.key.copy()
    free = np.nonzero(w.key == -1)[0]
    key[free[:4]] = [N_KEYS, N_KEYS + 1000, -2, 2 ** 31 - 1]
    for entry in ENTRIES:
        bad, twin_bad = (torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(2))
        got = new_entry(w, entry, n, w.where, True, key=cuda(key), bad=bad)
        old_entry(w, entry, w.dproj, w.dtypes, w.rowptr, w.col, n, exclude=(cuda(key),) + w.ex, bad=twin_bad)
        assert same(got, reference(w, entry, n, True)) and int(bad) == int(twin_bad) == 4, entry
        new_entry(w, entry, 200, w.where, True, key=cuda(key), bad=bad)
        assert int(bad) == 8                                                             # (added to)


# ---- 7. the methods
@pytest.fixture(scope="module")
def served():
    from test_gpu_catalogue_eval import cfg
    from p_companion_amd.p_companion import PCompanion
    dim, products = 128, 20_000
    bpg = _graph("device", dim)
    c = cfg(100, dim)
    torch.manual_seed(0)
    table = torch.randn(products, dim, generator=torch.Generator().manual_seed(11))
    gen = torch.Generator().manual_seed(21)
    value = (torch.rand(products, generator=gen) * 100 + 1).cuda()
    flags = torch.randint(-2 ** 31, 2 ** 31, (products,), generator=gen, dtype=torch.int64).to(torch.int32).cuda()
    return SimpleNamespace(bpg=bpg, c=c, model=PCompanion(c, table), value=value, flags=flags,
                           q=torch.arange(0, products, 197, dtype=torch.int32))


@pytest.mark.parametrize("catalogue", ["fp32", "compact"])
def test_recommend_where_batch(served, catalogue):
    from p_companion_amd import ops
    from p_companion_amd.inference import PCompanionInference
    v = served
    kw = {}
    if catalogue == "compact":
        kw["catalogue"] = ops.CompactCatalogue(ops.catalogue_bf16(v.bpg.cuda()["features"]))
    inf = PCompanionInference(v.model, v.c, v.bpg, **kw)
    q, b = v.q, len(v.q)
    f = lambda x: torch.full((b,), x, dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="no per-product attributes"):
        inf.recommend_where_batch(q, 10, lo=f(0.0))
    assert inf.set_attributes(value=v.value, flags=v.flags) is inf
    with pytest.raises(ValueError, match="at least one of"):
        inf.recommend_where_batch(q, 10)
    # band_around is its formula
    lo, hi = inf.band_around(q)
    vq = v.value[q.cuda().long()]
    assert torch.equal(lo, vq * 0.5) and torch.equal(hi, vq * 2.0) and lo.dtype == torch.float32 and lo.is_cuda
    lo3, hi3 = inf.band_around(q, 0.9, 1.25)
    assert torch.equal(lo3, vq * 0.9) and torch.equal(hi3, vq * 1.25)

    def eligible(mask, n):
        inf.set_eligible(mask)
        out = inf.recommend_batch(q, n)
        inf.set_eligible(None)
        return out

    def equal(got, want):
        return torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(bits(got[2]), bits(want[2]))

    for exclusions in (False, True):
        if exclusions:
            inf.set_exclusions()
        for n in (10, 100):
            # one shared band: recommend_batch under set_eligible(mask of the band)
            want = eligible((v.value >= 20.0) & (v.value <= 60.0), n)
            got = inf.recommend_where_batch(q, n, lo=f(20.0), hi=f(60.0))
            assert got[1].shape == want[1].shape == (b, v.c.NUM_COMP_TYPES, n) and equal(got, want), (exclusions, n)
            assert equal(inf.recommend_where_batch(q, n, hi=f(60.0)), eligible(v.value <= 60.0, n))         # one-sided
            # shared masks, and masks with a band
            need, deny = (torch.full((b,), x, dtype=torch.int32, device="cuda") for x in (5, int(BIT31) | 8))
            mask = ((v.flags & 5) == 5) & ((v.flags & (int(BIT31) | 8)) == 0)
            assert equal(inf.recommend_where_batch(q, n, need=need, deny=deny), eligible(mask, n))
            assert equal(inf.recommend_where_batch(q, n, lo=f(20.0), need=need), eligible((v.value >= 20.0) & ((v.flags & 5) == 5), n))
        # per-query bands: the per-band calls, query by query
        n = 40
        types, idx, sc = inf.recommend_where_batch(q, n, lo=lo, hi=hi)
        for j in range(0, b, 9):
            mask = (v.value >= lo[j]) & (v.value <= hi[j])
            want = eligible(mask, n)
            assert equal((types[j], idx[j], sc[j]), (want[0][j], want[1][j], want[2][j])), (exclusions, j)
            assert (idx[j] >= 0).any() and mask[idx[j][idx[j] >= 0].long()].all()
    inf.set_exclusions(False)
    inf.set_attributes()
    assert inf.attributes is None


def test_a_bare_bf16_catalogue_is_served_up_to_16_and_refused_at_17(served):
    from p_companion_amd.inference import PCompanionInference
    v = served
    inf = PCompanionInference(v.model, v.c, v.bpg, catalogue=torch.bfloat16).set_attributes(value=v.value)
    b = len(v.q)
    lo, hi = (torch.full((b,), x, dtype=torch.float32, device="cuda") for x in (20.0, 60.0))
    types, idx, sc = inf.recommend_where_batch(v.q, 16, lo=lo, hi=hi)
    inf.set_eligible((v.value >= 20.0) & (v.value <= 60.0))
    want = inf.recommend_batch(v.q, 16)
    inf.set_eligible(None)
    assert torch.equal(types, want[0]) and torch.equal(idx, want[1]) and torch.equal(bits(sc), bits(want[2]))
    assert idx.shape == (b, v.c.NUM_COMP_TYPES, 16) and (idx >= 0).any()
    with pytest.raises(ValueError, match="at most 16"):
        inf.recommend_where_batch(v.q, 17, lo=lo, hi=hi)


class _Graph:
    """What SimilarProducts reads of a graph: the products' types."""

    def __init__(self, type_idx, n_types):
        self.type_idx, self.n_types, self.num_products = type_idx, n_types, len(type_idx)

    def cuda(self, device=None):
        return {"type_idx": cuda(self.type_idx)}


@pytest.mark.parametrize("cls", ["SimilarProducts", "CompactSimilarProducts"])
@pytest.mark.parametrize("scope", ["type", "catalogue"])
def test_similar_where_batch_equals_similar_list_batch_under_the_same_eligibility(scope, cls):
    from p_companion_amd import inference, ops
    products, dim, n_types = 3000, 128, 6
    rng = np.random.default_rng(41)
    type_idx = rng.integers(0, n_types, products).astype(np.int32)
    table = cuda(rng.standard_normal((products, dim)).astype(np.float32))
    if cls == "CompactSimilarProducts":
        table = ops.catalogue_bf16(table)
    sp = getattr(inference, cls)(table, _Graph(type_idx, n_types), scope=scope)
    value = cuda((rng.random(products) * 100 + 1).astype(np.float32))
    flags = cuda(rng.integers(-2 ** 31, 2 ** 31, products).astype(np.int32))
    q = torch.arange(0, products, 61, dtype=torch.int32)
    b = len(q)
    f = lambda x: torch.full((b,), x, dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError, match="no per-product attributes"):
        sp.similar_where_batch(q, 10, lo=f(0.0))
    sp.set_attributes(value=value, flags=flags)
    with pytest.raises(ValueError, match="at least one of"):
        sp.similar_where_batch(q, 10)

    def eligible(mask, n):
        sp.set_eligible(mask)
        out = sp.similar_list_batch(q, n)
        sp.set_eligible(None)
        return out

    for n in (10, 100):
        got = sp.similar_where_batch(q, n, lo=f(30.0), hi=f(70.0))
        assert got[0].shape == (b, n) and same(got, eligible((value >= 30.0) & (value <= 70.0), n)), n
        deny = torch.full((b,), int(BIT31) | 1, dtype=torch.int32, device="cuda")
        assert same(sp.similar_where_batch(q, n, hi=f(70.0), deny=deny),
                    eligible((value <= 70.0) & ((flags & (int(BIT31) | 1)) == 0), n)), n
    # cheaper substitutes, query by query: hi = the query's own value
    lo, hi = sp.band_around(q, 0.0, 1.0)
    assert torch.equal(hi, value[q.cuda().long()]) and torch.equal(lo, value[q.cuda().long()] * 0.0)
    idx, dist = sp.similar_where_batch(q, 40, lo=lo, hi=hi)
    assert not (idx == q.cuda()[:, None]).any()               # the query passes its own band and stays excluded
    for j in range(0, b, 7):
        want = eligible((value >= lo[j]) & (value <= hi[j]), 40)
        assert same((idx[j], dist[j]), (want[0][j], want[1][j])), j
    e_i, e_d = sp.similar_where_batch(q[:0], 5, lo=f(0.0)[:0])
    assert e_i.shape == (0, 5) and e_d.shape == (0, 5)


def test_the_cell_index_does_not_serve_the_filter():
    from p_companion_amd.inference import IndexedSimilarProducts
    with pytest.raises(NotImplementedError):
        object.__new__(IndexedSimilarProducts).similar_where_batch(torch.zeros(2, dtype=torch.int32), 10)
