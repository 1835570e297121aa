"""Long substitute lists: pc_retrieve_list_grouped_biased / ops.retrieve_list_grouped_biased (up to 256 products per (query,
type) under the score fl(<q, e_p> + bias[p])) and SimilarProducts / IndexedSimilarProducts.similar_list_batch and
similar_capped_list_batch on top of it.  Needs an MI355X.

The references are never the code under test: the EXISTING 16-entry biased entry, peeled (tests/test_gpu_retrieval_list.py's
scheme: what has been served so far is the next call's exclusion set), compared bit for bit -- ids as they are, scores as int32
patterns; the unbiased list entry for the claim "one fp32 addition after the chain"; and float64 numpy with
tests/test_gpu_nearest.py's per-entry allowance (D + 2) 2^-24 (sum_d |q_d e_pd| + |b_p|), the forward-error bound of D products,
D - 1 additions of the chain and the one addition of the bias.  The catalogue is tests/test_gpu_retrieval_list.py's shape
(12 350 products in types of 9000 / 3000 / 300 / 40 / 10 / 0, row counts around the 16-row tile, exclusion lists of 0 / 1 / 15 /
16 / 17 / 33 entries, a whole type and a row's own top 64), its lengths NS cover both buffer-size thresholds."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_nearest import check_biased, dev, exact, mixed, ordered, row_view      # noqa: F401  (exact, mixed: fixtures)
from test_gpu_retrieval_list import (LENGTHS, N_KEYS, NS, P, ROW_COUNTS, SIZES, T, TILE, bits, csr_of, cuda, ex_csr, padded,
                                     same)

KINDS = ("half_norm", "random")


def peel(m, kind, n, own=None):
    """The first n of every row from the 16-entry biased entry alone: ceil(n / 16) calls, each excluding what the earlier ones
    served (and `own` [R, w], the row's own list, -1 = nothing)."""
    from p_companion_amd import ops
    rows = m.R
    row_key = torch.arange(rows, dtype=torch.int32, device="cuda")
    idx, sc = [], []
    for _ in range((n + 15) // 16):
        parts = ([own] if own is not None else []) + idx
        exclude = None
        if parts:
            served = torch.cat(parts, 1).contiguous()
            rp = (torch.arange(rows + 1, device="cuda") * served.shape[1]).to(torch.int32)
            exclude = (row_key,) + ops.exclusion_csr(rp, served.reshape(-1), include_self=False, num_products=P)
        i, s = ops.retrieve_topk_grouped(m.dproj, m.dtypes, m.rowptr, m.col, m.table, 16, exclude=exclude, bias=m.bias[kind])
        idx.append(i)
        sc.append(s)
    return torch.cat(idx, 1)[:, :n].contiguous(), torch.cat(sc, 1)[:, :n].contiguous()


@pytest.fixture(scope="module", params=[128, 256], ids=lambda d: f"D{d}")
def cat(request):
    """tests/test_gpu_retrieval_list.py's catalogue, rows and keys, with two biases and the peeled references under each."""
    from p_companion_amd import ops
    dim = request.param
    rng = np.random.default_rng(2000 + dim)
    type_idx = rng.permutation(np.repeat(np.arange(T), SIZES)).astype(np.int32)
    by = lambda t: np.nonzero(type_idx == t)[0]
    features = rng.standard_normal((P, dim)).astype(np.float32)
    t0 = by(0)
    a1, b1 = t0[100], t0[2000]                                 # b1 is a copy of a1: tied under the half-norm bias
    features[b1] = features[a1]
    types = np.concatenate([np.repeat(np.arange(T), ROW_COUNTS), [-1, -1, T]]).astype(np.int32)
    types = types[rng.permutation(len(types))]
    R = len(types)
    proj = rng.standard_normal((R, dim)).astype(np.float32)
    rows_of = lambda t: np.nonzero(types == t)[0]
    r0 = rows_of(0)
    proj[r0[1:4]] = 3 * features[a1]                           # three rows whose nearest products are the tied pair
    key = ((np.arange(R) % N_KEYS) - 1).astype(np.int32)       # -1, 0..7 spread over the rows
    key[r0[0]] = 7                                             # its list is its own unfiltered top 64 (half-norm bias)
    key[rows_of(3)[:3]] = [6, 0, 6]                            # key 6 covers the whole 40-product type
    key[rows_of(4)[:2]] = [4, -1]
    rowptr, col = csr_of(type_idx)
    table = cuda(features)
    bias = {"half_norm": ops.half_sq_norm_bias(table),
            "random": cuda((np.random.default_rng(3).standard_normal(P) * 10).astype(np.float32))}
    m = SimpleNamespace(dim=dim, R=R, type_idx=type_idx, features=features, proj=proj, types=types, key=key, by=by,
                        rows_of=rows_of, tied=(a1, b1), rowptr=rowptr, col=col, table=table, dproj=cuda(proj), dtypes=cuda(types),
                        dkey=cuda(key), cand_type=cuda(type_idx), bias=bias)
    m.want = {kind: peel(m, kind, 256) for kind in KINDS}      # the unfiltered references, once
    top = m.want["half_norm"][0].cpu().numpy()
    assert sorted(top[r0[1], :2].tolist()) == [a1, b1] and top[r0[1], 0] == a1      # (the tie goes to the lower id)

    def fill(first, length, pool):
        out = list(dict.fromkeys(int(x) for x in first))[:length]
        for x in pool:
            if len(out) >= length:
                break
            if int(x) not in out:
                out.append(int(x))
        assert len(out) == length
        return sorted(out)

    heads = lambda k: [x for r in np.nonzero(key == k)[0] for x in top[r, :3] if x >= 0]      # what the key's rows serve first
    lists = {0: [], 8: []}
    for k in (1, 2, 3, 4, 5):
        lists[k] = fill(heads(k), LENGTHS[k], rng.permutation(P))
    lists[6] = fill(by(3), 45, list(by(2)[:3]) + heads(6))
    lists[7] = sorted(int(x) for x in top[r0[0], :64])
    assert len(lists[7]) == 64 and all(len(lists[k]) == n for k, n in LENGTHS.items())
    m.lists, m.ex = lists, ex_csr(lists)
    m.own = padded(lists, key)
    m.want_filtered = {kind: peel(m, kind, 256, own=m.own) for kind in KINDS}       # the filtered references, once
    return m


def served(m, kind, n, filt=False, slices=0, col=None, bad=None):
    from p_companion_amd import ops
    ex = ((m.dkey,) + m.ex) if filt else None
    return ops.retrieve_list_grouped_biased(m.dproj, m.dtypes, m.rowptr, m.col if col is None else col, m.table, m.bias[kind], n,
                                            slices=slices, exclude=ex, bad=bad)


def reference(m, kind, n, filt):
    i, s = (m.want_filtered if filt else m.want)[kind]
    return i[:, :n].contiguous(), s[:, :n].contiguous()


# ---- 1. every length against the peeled lists
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("filt", [False, True], ids=["plain", "excluding"])
@pytest.mark.parametrize("n", NS)
def test_lists_equal_the_peeled_16_entry_biased_lists(cat, n, filt, kind):
    m = cat
    got, want = served(m, kind, n, filt), reference(m, kind, n, filt)
    assert got[0].shape == (m.R, n) and got[0].dtype == torch.int32 and got[1].dtype == torch.float32
    assert torch.equal(got[0], want[0]), (n, torch.nonzero((got[0] != want[0]).any(1)).reshape(-1)[:10].tolist())
    assert torch.equal(bits(got[1]), bits(want[1])), n
    idx = got[0].cpu().numpy()
    if filt:
        for r in range(m.R):
            assert not set(idx[r].tolist()) & set(m.lists[m.key[r]] if m.key[r] >= 0 else []), r
    # entries past the end of a short type and rows without a type: -1 / -inf
    sc = got[1].cpu().numpy()
    for r in m.rows_of(4):
        k = 10 - (len(set(m.by(4).tolist()) & set(m.lists[m.key[r]])) if filt and m.key[r] >= 0 else 0)
        assert (idx[r, :k] >= 0).all() and (idx[r, k:] == -1).all() and np.isneginf(sc[r, k:]).all(), r
    nowhere = np.nonzero((m.types == 5) | (m.types == -1) | (m.types == T))[0]
    assert len(nowhere) == 4 and (idx[nowhere] == -1).all() and np.isneginf(sc[nowhere]).all()


def test_the_references_are_what_they_are_meant_to_be(cat):
    """The fixture's own claims: the bias changes the order, the filter bites, the row that lists its own top 64 is served
    positions 64.., the fully excluded type is empty."""
    from p_companion_amd import ops
    m = cat
    plain = ops.retrieve_list_grouped(m.dproj, m.dtypes, m.rowptr, m.col, m.table, 16)[0]
    for kind in KINDS:
        unf, fil = m.want[kind][0].cpu().numpy(), m.want_filtered[kind][0].cpu().numpy()
        assert (unf[:, :16] != plain.cpu().numpy()).any(1).sum() >= 60
        assert (unf[:, :16] != fil[:, :16]).any(1).sum() >= 10
        r3 = m.rows_of(3)
        assert (fil[r3[0]] == -1).all() and (fil[r3[2]] == -1).all() and (fil[r3[1], :40] >= 0).all() and (fil[r3[1], 40:] == -1).all()
    r0 = m.rows_of(0)
    unf, fil = m.want["half_norm"][0].cpu().numpy(), m.want_filtered["half_norm"][0].cpu().numpy()
    assert (fil[r0[0], :192] == unf[r0[0], 64:]).all()


# ---- 2. the 16-entry's own bits
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [1, 10, 16])
def test_short_lists_are_the_16_entry_biased_entrys_bits(cat, n, kind):
    from p_companion_amd import ops
    m = cat
    assert same(served(m, kind, n), ops.retrieve_topk_grouped(m.dproj, m.dtypes, m.rowptr, m.col, m.table, n, bias=m.bias[kind]))
    assert same(served(m, kind, n, True), ops.retrieve_topk_grouped(m.dproj, m.dtypes, m.rowptr, m.col, m.table, n,
                                                                    exclude=(m.dkey,) + m.ex, bias=m.bias[kind]))


# ---- 3. zero bias
@pytest.mark.parametrize("n", [40, 200])
def test_zero_bias_is_the_unbiased_list_bit_for_bit(cat, n):
    from p_companion_amd import ops
    m = cat
    zero = torch.zeros(P, device="cuda")
    for exclude in (None, (m.dkey,) + m.ex):
        a = ops.retrieve_list_grouped(m.dproj, m.dtypes, m.rowptr, m.col, m.table, n, exclude=exclude)
        b = ops.retrieve_list_grouped_biased(m.dproj, m.dtypes, m.rowptr, m.col, m.table, zero, n, exclude=exclude)
        assert same(a, b), exclude is not None


# ---- 4. one addition
@pytest.mark.parametrize("kind", KINDS)
def test_the_score_is_one_fp32_addition_after_the_list_chain(cat, kind):
    """s = fl(d + b) bit for bit, d read from the unbiased list entry where both lists hold every candidate: the types of 40 and
    10 products, and type 0 cut to 256 products (four chunks, the rows in three tiles).  An accumulator that
    started at the bias would round differently at every step of the chain."""
    from p_companion_amd import ops
    m = cat
    rowptr = m.rowptr.cpu().numpy().copy()
    col = m.col.cpu().numpy().copy()
    cut = len(m.by(0)) - 256
    col = np.concatenate([col[:256], col[rowptr[1]:]])
    rowptr[1:] -= cut
    rowptr, col = cuda(rowptr.astype(np.int32)), cuda(col.astype(np.int32))
    d_i, d_s = ops.retrieve_list_grouped(m.dproj, m.dtypes, rowptr, col, m.table, 256)
    s_i, s_s = ops.retrieve_list_grouped_biased(m.dproj, m.dtypes, rowptr, col, m.table, m.bias[kind], 256)
    d_i, d_s, s_i, s_s = (x.cpu().numpy() for x in (d_i, d_s, s_i, s_s))
    hb = m.bias[kind].cpu().numpy()
    seen = 0
    for t, k in ((0, 256), (3, 40), (4, 10)):
        for r in m.rows_of(t):
            assert sorted(d_i[r, :k].tolist()) == sorted(s_i[r, :k].tolist()) and (s_i[r, :k] >= 0).all(), r
            d = dict(zip(d_i[r, :k].tolist(), d_s[r, :k]))
            want = np.array([np.float32(d[p]) + hb[p] for p in s_i[r, :k]], np.float32)
            assert (s_s[r, :k].view(np.int32) == want.view(np.int32)).all(), r
            seen += k
    assert seen >= 256 * (2 * TILE + 1)


# ---- 5. slices, candidate order, repeat calls, the rows' company
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [40, 200])
def test_same_bits_for_every_slicing_candidate_order_and_call(cat, n, kind):
    m = cat
    rowptr = m.rowptr.cpu().numpy()
    col = m.col.cpu().numpy().copy()
    rng = np.random.default_rng(9)
    for t in range(T):
        rng.shuffle(col[rowptr[t]:rowptr[t + 1]])
    for filt in (False, True):
        want = reference(m, kind, n, filt)
        for c, s in ((None, 1), (None, 7), (None, 64), (None, 0), (None, 0), (cuda(col), 0), (cuda(col), 5)):
            assert same(served(m, kind, n, filt, slices=s, col=c), want), (filt, s, c is not None)


@pytest.mark.parametrize("n", [40, 200])
def test_subsets_of_the_rows_are_served_the_same_lists(cat, n):
    """Other tile fillings than the fixture's: two full tiles of one type and one row of another, every type's first row, a type's
    rows in reverse."""
    from p_companion_amd import ops
    m = cat
    kind = "half_norm"
    want_i, want_s = reference(m, kind, n, True)
    for rows in (np.concatenate([m.rows_of(0)[:2 * TILE], m.rows_of(1)[:1]]), np.array([m.rows_of(t)[0] for t in range(T)]),
                 m.rows_of(0)[::-1].copy()):
        sel = cuda(rows.astype(np.int64))
        got = ops.retrieve_list_grouped_biased(m.dproj[sel].contiguous(), m.dtypes[sel].contiguous(), m.rowptr, m.col, m.table,
                                               m.bias[kind], n, exclude=(m.dkey[sel].contiguous(),) + m.ex)
        assert same(got, (want_i[sel], want_s[sel])), len(rows)


# ---- 6. exact data
@pytest.mark.parametrize("n", [200, 256])
def test_exact_data_with_the_half_norm_bias_is_the_float64_l2_order(exact, n):
    """Integer features and queries: every product, the bias and their sum are exact in fp32, so the list is the float64 order,
    ties by ascending id, and the scores are the float64 values' fp32 bits."""
    from p_companion_amd import ops
    m = exact
    hb = ops.half_sq_norm_bias(m.table)
    assert (hb.cpu().numpy().astype(np.float64) == -0.5 * (m.features.astype(np.float64) ** 2).sum(1)).all()
    idx, sc = ops.retrieve_list_grouped_biased(m.dproj, m.dtypes, m.rowptr, m.col, m.table, hb, n)
    idx = idx.cpu().numpy()
    check_biased(m, idx, sc.cpu().numpy(), hb.cpu().numpy(), n, exact=True)
    f64, p64 = m.features.astype(np.float64), m.proj.astype(np.float64)
    long_rows = 0
    for r in m.where:
        cand = np.nonzero(m.type_idx == m.types[r])[0]
        d2 = ((p64[r][None, :] - f64[cand]) ** 2).sum(1)       # brute force, exact in float64
        want = cand[np.lexsort((cand, d2))][:n]
        assert (idx[r, :len(want)] == want).all(), r
        long_rows += len(want) == n
    assert long_rows >= 70


# ---- 7. mixed data against float64
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [100, 256])
def test_parity_with_the_float64_reference(mixed, n, kind):
    """tests/test_gpu_nearest.py's check at list length: every score within its entry's allowance, a differing id only where the
    two float64 scores lie within the sum of the two allowances -- no cap on such rows --, equal scores by ascending id."""
    from p_companion_amd import ops
    m = mixed
    idx, sc = ops.retrieve_list_grouped_biased(m.dproj, m.dtypes, m.rowptr, m.col, m.table, m.bias[kind], n)
    idx, sc = idx.cpu().numpy(), sc.cpu().numpy()
    check_biased(m, idx, sc, m.hbias[kind], n)
    assert (idx[:4] == -1).all() and np.isneginf(sc[:4]).all()                    # types -1 / n_types / empty
    assert (idx[4:6, :3] >= 0).all() and (idx[4:6, 3:] == -1).all()               # types of 3 products


# ---- 8. the rank
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("filt", [False, True], ids=["plain", "excluding"])
def test_position_k_of_a_list_is_the_product_of_biased_rank_k(cat, filt, kind):
    """Every position of every list (0, 15, 16 and n - 1 among them) is the product whose rank_grouped(bias=) is that position,
    and 200 (row, product) pairs from beyond the lists rank at n or behind, or -1 where the row's list holds them."""
    from p_companion_amd import ops
    m = cat
    n = 100
    b = m.bias[kind]
    idx, _ = served(m, kind, n, filt)
    kw = dict(exclude=(m.dkey.repeat_interleave(n).contiguous(),) + m.ex, cand_type=m.cand_type) if filt else {}
    there = (idx >= 0).reshape(-1)
    types = torch.where(there, m.dtypes.repeat_interleave(n), torch.full_like(there, -1, dtype=torch.int32)).contiguous()
    rank, bad = ops.rank_grouped(m.dproj.repeat_interleave(n, 0).contiguous(), types, idx.clamp(min=0).reshape(-1).contiguous(),
                                 m.rowptr, m.col, m.table, bias=b, **kw)
    want = torch.where(there, torch.arange(n, dtype=torch.int32, device="cuda").repeat(m.R), torch.full_like(rank, -1))
    assert int(bad) == 0 and torch.equal(rank, want), torch.nonzero(rank != want).reshape(-1)[:10].tolist()
    assert int(there.sum()) > 60 * n
    rng = np.random.default_rng(5)
    got = idx.cpu().numpy()
    rows = rng.choice(np.nonzero(np.isin(m.types, (0, 1, 2)))[0], 200)
    prods = np.array([rng.choice(np.setdiff1d(m.by(m.types[r]), got[r])) for r in rows], np.int32)
    sel = cuda(rows.astype(np.int64))
    kw = dict(exclude=(m.dkey[sel].contiguous(),) + m.ex, cand_type=m.cand_type) if filt else {}
    rank, bad = ops.rank_grouped(m.dproj[sel].contiguous(), m.dtypes[sel].contiguous(), cuda(prods), m.rowptr, m.col, m.table,
                                 bias=b, **kw)
    rank = rank.cpu().numpy()
    out = np.array([filt and m.key[r] >= 0 and int(p) in m.lists[m.key[r]] for r, p in zip(rows, prods)])
    assert int(bad) == 0 and (rank[out] == -1).all() and (rank[~out] >= n).all()


# ---- 9. refusals
def test_error_codes_through_ctypes():
    """Every refusal returns its code before anything is launched: the outputs and the counter stay as they were."""
    from p_companion_amd import _lib
    L = _lib.lib()
    R, T2, P2 = 4, 2, 4
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device="cuda")
    a = dict(proj=torch.zeros(R, 256, device="cuda"), types=i32(0, 0, 1, 1), row_key=i32(0, 1, -1, 0), rows=R,
             type_rowptr=i32(0, 2, 4), type_col=i32(0, 1, 2, 3), table=torch.zeros(P2, 256, device="cuda"),
             bias=torch.zeros(P2, device="cuda"), n_types=T2, ex_rowptr=i32(0, 1, 1), ex_col=i32(0), n_keys=2, n=100, dim=128,
             slices=0, out_idx=torch.full((R, 256), 12345, dtype=torch.int32, device="cuda"),
             out_score=torch.full((R, 256), 7.0, device="cuda"), bad_count=torch.zeros(1, dtype=torch.int32, device="cuda"),
             ws=torch.empty(L.pc_retrieve_list_grouped_biased_workspace_bytes(R, T2, 256, 64), dtype=torch.uint8, device="cuda"))
    a["ws_bytes"] = a["ws"].numel()
    a["stream"] = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    conv = lambda v: ctypes.c_void_p(v.data_ptr()) if torch.is_tensor(v) else v
    none = dict(row_key=None, ex_rowptr=None, ex_col=None, n_keys=0)

    def retrieve(**kw):
        return L.pc_retrieve_list_grouped_biased(*[conv(v) for v in {**a, **kw}.values()])

    for name in ("proj", "types", "type_rowptr", "type_col", "table", "bias", "out_idx", "out_score", "ws", "ex_rowptr", "ex_col",
                 "bad_count"):
        assert retrieve(**{name: None}) == -1, name                                # PC_EINVAL
    assert retrieve(**none, bias=None) == -1
    assert retrieve(rows=0) == -1 and retrieve(n_types=0) == -1 and retrieve(n_keys=-1) == -1
    assert retrieve(row_key=None) == -1 and retrieve(**{**none, "n_keys": 2}) == -1          # lists without keys
    assert retrieve(**{**none, "ex_col": a["ex_col"]}) == -1 and retrieve(**{**none, "ex_rowptr": a["ex_rowptr"]}) == -1
    for kw in (dict(n=0), dict(n=257), dict(dim=64), dict(dim=192), dict(slices=-1), dict(slices=65)):
        assert retrieve(**kw) == -2 and retrieve(**kw, **none) == -2, kw           # PC_ESHAPE
    assert retrieve(bias=None, n=257) == -1                                        # the pointers before the shapes
    for n in (16, 17, 100, 256):
        need = L.pc_retrieve_list_grouped_biased_workspace_bytes(R, T2, n, 0)
        assert need == L.pc_retrieve_list_grouped_workspace_bytes(R, T2, n, 0) > 0
        assert retrieve(n=n, ws_bytes=need - 1) == -3 and retrieve(n=n, ws_bytes=need - 1, **none) == -3      # PC_EWORKSPACE
    assert L.pc_retrieve_list_grouped_biased_workspace_bytes(R, T2, 257, 0) == 0
    torch.cuda.synchronize()
    assert (a["out_idx"] == 12345).all() and (a["out_score"] == 7.0).all() and int(a["bad_count"]) == 0
    # and the calls that are in order are served
    assert retrieve() == 0 and retrieve(dim=256, n=256, slices=64) == 0 and retrieve(**none) == 0
    assert retrieve(**none, bad_count=None) == 0
    torch.cuda.synchronize()
    last = a["out_idx"].reshape(-1)[:R * 100].view(R, 100)                        # (the last call's [R, n])
    assert (last[:, :2].cpu().numpy() == [[0, 1], [0, 1], [2, 3], [2, 3]]).all() and (last[:, 2:] == -1).all()


# ---- 10. SimilarProducts.similar_list_batch
class _Graph:
    """What SimilarProducts reads of a graph: the products' types."""

    def __init__(self, type_idx, n_types):
        self.type_idx, self.n_types, self.num_products = type_idx, n_types, len(type_idx)

    def cuda(self, device=None):
        return {"type_idx": dev(self.type_idx)}


@pytest.mark.parametrize("scope", ["type", "catalogue"])
def test_similar_list_batch_on_exact_data(exact, scope):
    from p_companion_amd.inference import SimilarProducts
    m = exact
    sp = SimilarProducts(m.table, _Graph(m.type_idx, m.T), scope=scope)
    assert SimilarProducts.MAX_LIST == 256
    rng = np.random.default_rng(17)
    q = np.concatenate([[3, 5, 9], 10 + rng.choice(m.P - 10, 61, replace=False)]).astype(np.int32)      # (3, 5, 9: identical rows)
    n = 100
    f64 = m.features.astype(np.float64)

    def want_of(qi, eligible=None, keep_self=False):
        cand = np.nonzero(m.type_idx == m.type_idx[qi])[0] if scope == "type" else np.arange(m.P)
        if not keep_self:
            cand = cand[cand != qi]
        if eligible is not None:
            cand = cand[eligible[cand]]
        d2 = ((f64[qi][None, :] - f64[cand]) ** 2).sum(1)      # exact in float64
        return cand[np.lexsort((cand, d2))][:n]

    def check(idx, dist, **kw):
        assert idx.dtype == torch.int32 and dist.dtype == torch.float32 and tuple(idx.shape) == tuple(dist.shape) == (len(q), n)
        idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
        short = 0
        for j, qi in enumerate(q):
            want = want_of(qi, **kw)
            k = len(want)
            assert (idx[j, :k] == want).all() and (idx[j, k:] == -1).all() and np.isposinf(dist[j, k:]).all(), (j, qi)
            d64 = np.sqrt(((f64[qi][None, :] - f64[want] + 1e-6) ** 2).sum(1))
            np.testing.assert_allclose(dist[j, :k], d64, rtol=1e-4, atol=0)
            short += k < n
        return idx, short

    tq = torch.from_numpy(q)
    idx, dist = sp.similar_list_batch(tq, n)
    idx_h, short = check(idx, dist)
    assert (idx_h != q[:, None]).all() and (short > 10) == (scope == "type")      # the types of about 15 products
    # n <= 16: similar_batch's ids and distances bit for bit
    for k in (1, 10, 16):
        assert same(sp.similar_list_batch(tq, k), sp.similar_batch(tq, k)), k
    # the distances do not depend on the chunking: chunks of 7, 1 and all queries
    for budget in (7 * 4 * n * m.dim, 1, 1 << 40):
        sp.DIST_BYTES = budget
        assert same(sp.similar_list_batch(tq, n), (idx, dist)), budget
    del sp.DIST_BYTES
    # eligibility, and no exclusion set: the query leads its own list
    mask = np.random.default_rng(6).random(m.P) < 0.7
    sp.set_eligible(dev(mask))
    check(*sp.similar_list_batch(tq, n), eligible=mask)
    sp.set_eligible(None)
    sp.set_exclusions(False)
    i2, _ = check(*sp.similar_list_batch(tq, n), keep_self=True)
    assert (i2[3:, 0] == q[3:]).all() and (i2[:3, 0] == 3).all()
    sp.set_exclusions()
    assert same(sp.similar_list_batch(tq, n), (idx, dist))
    e_i, e_d = sp.similar_list_batch(tq[:0], 33)
    assert e_i.shape == (0, 33) and e_d.shape == (0, 33) and e_i.dtype == torch.int32 and e_d.dtype == torch.float32
    for bad in (0, 257, -1):
        with pytest.raises(ValueError, match="1 to 256"):
            sp.similar_list_batch(tq, bad)


# ---- 11. the limit lifted
@pytest.fixture(scope="module")
def varianted():
    """tests/test_gpu_cap_lists.py::test_similar_capped_batch's table, groups and queries: every product in four variants."""
    from p_companion_amd.data import generate_device_bpg
    from p_companion_amd.inference import IndexedSimilarProducts, SimilarProducts
    products, dim = 2000, 128
    bpg = generate_device_bpg(products, 8, seed=3, world=1, with_complementary=False)
    gen = torch.Generator().manual_seed(9)
    centres = torch.randn(products // 4, dim, generator=gen)
    table = (centres.repeat_interleave(4, dim=0) + 1e-3 * torch.randn(products, dim, generator=gen)).cuda().contiguous()
    group = (torch.arange(products, dtype=torch.int32) // 4).cuda()
    q = torch.arange(0, products, 37, dtype=torch.int32).cuda()
    return SimpleNamespace(group=group, q=q, own=group[q.long()], exact=SimilarProducts(table, bpg, scope="catalogue"),
                           indexed=IndexedSimilarProducts(table, bpg, n_cells=8, nprobe=8, iters=3, seed=1))


@pytest.mark.parametrize("which", ["exact", "indexed"])
def test_a_pool_of_64_fills_the_capped_lists_a_pool_of_16_leaves_short(varianted, which):
    from p_companion_amd import ops
    v = varianted
    sp, q, group, own = getattr(v, which), v.q, v.group, v.own
    idx16, _ = sp.similar_capped_batch(q, 10, group=group)
    assert ((idx16 >= 0).sum(1) < 10).any()                   # the limit this test is about: lists of 10 from a pool of 16
    idx, dist = sp.similar_capped_list_batch(q, 10, group=group, pool=64)
    assert idx.shape == (len(q), 10) and idx.dtype == torch.int32 and dist.dtype == torch.float32
    assert (idx >= 0).all() and torch.isfinite(dist).all()    # ten for every query
    g = group[idx.long()]
    assert not (g == own[:, None]).any()                      # none of the query's own variants
    assert all(len(set(row)) == 10 for row in g.cpu().tolist())                   # one product per group
    assert (dist[:, 1:] >= dist[:, :-1]).all()
    # the rule, applied here to the pool
    p_idx, p_dist = sp.similar_list_batch(q, 64)
    w_idx, w_near = ops.cap_lists(p_idx, -p_dist, 10, group, 1, row_ban=own.contiguous())
    assert same((idx, dist), (w_idx, -w_near))
    # own_group and cap 2, no group, the widest pool, the defaults
    i2, d2 = sp.similar_capped_list_batch(q, 10, group=group, cap=2, own_group=True, pool=64)
    w_idx, w_near = ops.cap_lists(p_idx, -p_dist, 10, group, 2)
    assert same((i2, d2), (w_idx, -w_near)) and (group[i2[:, :2].long()] == own[:, None]).all()
    w_idx, w_near = ops.cap_lists(p_idx, -p_dist, 10)
    assert same(sp.similar_capped_list_batch(q, 10, pool=64), (w_idx, -w_near))
    i3, d3 = sp.similar_capped_list_batch(q, 40, group=group, pool=256)
    p256 = sp.similar_list_batch(q, 256)
    w_idx, w_near = ops.cap_lists(p256[0], -p256[1], 40, group, 1, row_ban=own.contiguous())
    assert same((i3, d3), (w_idx, -w_near)) and (i3 >= 0).all()
    assert same(sp.similar_capped_list_batch(q, group=group), (idx, dist))        # n = 10, pool = 64
    e_i, e_d = sp.similar_capped_list_batch(q[:0], 5, group=group)
    assert e_i.shape == (0, 5) and e_d.shape == (0, 5)


# ---- 12. the index
@pytest.mark.parametrize("n", [40, 256])
def test_probing_every_cell_is_the_parents_list_bit_for_bit(varianted, n):
    from p_companion_amd.inference import SimilarProducts
    v = varianted
    want = v.exact.similar_list_batch(v.q, n)
    assert same(v.indexed.similar_list_batch(v.q, n, nprobe=8), want)
    assert same(v.indexed.similar_list_batch(v.q, n), want)                       # (the constructor's nprobe)
    assert same(SimilarProducts.similar_list_batch(v.indexed, v.q, n), want)      # the parent's method on the indexed object
    # fewer cells: the parent's order restricted to the probed cells' products
    got, _ = v.indexed.similar_list_batch(v.q, n, nprobe=2)
    cells = v.indexed.probe_cells(v.q, 2)
    cell_of = v.indexed.index.cell_of
    full = v.exact.similar_list_batch(v.q, 256)[0]
    for j in range(len(v.q)):
        inside = (cell_of[full[j].long()][:, None] == cells[j][None, :]).any(1)
        keep = full[j][inside][:n]
        # (the parent's 256 nearest cover the head of the restricted list only as far as they reach)
        assert torch.equal(got[j, :len(keep)], keep), j
    with pytest.raises(ValueError, match="nprobe"):
        v.indexed.similar_list_batch(v.q, n, nprobe=9)
