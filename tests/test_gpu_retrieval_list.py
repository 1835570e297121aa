"""Long lists: pc_retrieve_list_grouped / ops.retrieve_list_grouped (up to 256 products per (query, type)) and
PCompanionInference.recommend_batch above 16.

The oracle is the EXISTING code, peeled: ops.retrieve_topk_grouped(n = 16) gives positions 0..15; what has been served so far
(united with the row's own list in the filtered variant) goes through ops.exclusion_csr as a per-row exclusion set
(row_key = arange(R)), and the next call gives the next 16.  A (row, product) score has the same bits wherever it is computed
and every selection is under one total order, so the concatenation, cut to n, is compared bit for bit: ids as they are, scores
as int32 patterns.  The one tolerance is the float64 band of tests/test_gpu_rank_grouped.py, 2 (1e-5 + 1e-5 |g|), taken from
that file.  Needs an MI355X."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

P = 12_350
SIZES = (9000, 3000, 300, 40, 10, 0)       # three automatic slices, one slice, both sides of n = 256 with a chunk to spare,
T = len(SIZES)                             # shorter than most n, shorter than 16, empty
TILE = 16                                  # the list kernel's tile height
ROW_COUNTS = (2 * TILE + 1, 2 * TILE - 1, TILE + 1, TILE - 1, TILE, 1)      # rows per type (1 and 2 * TILE: test_subsets)
N_KEYS = 9                                 # keys 0..7 carry lists, key 8 is not used by a row
LENGTHS = {0: 0, 1: 1, 2: 15, 3: 16, 4: 17, 5: 33}      # key 6: a whole 40-product type; key 7: a row's own top 64
NS = (1, 16, 17, 63, 64, 65, 128, 255, 256) + (32, 33, 96, 97)          # (and both sides of the kernel's two buffer-size thresholds)


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(sc):
    return sc.contiguous().view(torch.int32)


def same(got, want):
    return torch.equal(got[0], want[0]) and torch.equal(bits(got[1]), bits(want[1]))


def csr_of(type_idx):
    order = np.argsort(type_idx, kind="stable").astype(np.int32)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(type_idx, minlength=T))]).astype(np.int32)
    return cuda(rowptr), cuda(order)


def padded(lists, keys):
    """[R, longest] int32 on the device: row r holds the list of keys[r], -1 past its end (and for key -1)"""
    width = max(len(v) for v in lists.values())
    out = np.full((len(keys), width), -1, np.int32)
    for r, k in enumerate(keys):
        if k >= 0:
            out[r, :len(lists[k])] = lists[k]
    return cuda(out)


def peel(proj, types, rowptr, col, table, n, own=None):
    """The first n of every row from the 16-entry alone: ceil(n / 16) calls, each excluding what the earlier ones served (and
    `own` [R, w], the row's own list, -1 = nothing)."""
    from p_companion_amd import ops
    rows = proj.shape[0]
    row_key = torch.arange(rows, dtype=torch.int32, device="cuda")
    idx, sc = [], []
    for _ in range((n + 15) // 16):
        parts = ([own] if own is not None else []) + idx
        if parts:
            served = torch.cat(parts, 1).contiguous()
            rp = (torch.arange(rows + 1, device="cuda") * served.shape[1]).to(torch.int32)
            ex = ops.exclusion_csr(rp, served.reshape(-1), include_self=False, num_products=P)      # (drops the -1 entries)
            i, s = ops.retrieve_topk_grouped(proj, types, rowptr, col, table, 16, exclude=(row_key,) + ex)
        else:
            i, s = ops.retrieve_topk_grouped(proj, types, rowptr, col, table, 16)
        idx.append(i)
        sc.append(s)
    return torch.cat(idx, 1)[:, :n].contiguous(), torch.cat(sc, 1)[:, :n].contiguous()


def ex_csr(lists):
    rowptr = np.concatenate([[0], np.cumsum([len(lists[k]) for k in range(N_KEYS)])]).astype(np.int32)
    col = np.concatenate([np.asarray(lists[k], np.int64) for k in range(N_KEYS)] + [np.zeros(0, np.int64)]).astype(np.int32)
    return cuda(rowptr), cuda(col)


@pytest.fixture(scope="module", params=[128, 256], ids=lambda d: f"D{d}")
def cat(request):
    dim = request.param
    rng = np.random.default_rng(1000 + dim)
    type_idx = rng.permutation(np.repeat(np.arange(T), SIZES)).astype(np.int32)
    by = lambda t: np.nonzero(type_idx == t)[0]
    features = rng.standard_normal((P, dim)).astype(np.float32)
    t0 = by(0)
    a1, b1, a2, b2 = t0[100], t0[2000], t0[300], t0[3000]      # a < b: b is a copy of a (the exclusions fixture's tied pairs)
    features[b1], features[b2] = features[a1], features[a2]
    types = np.concatenate([np.repeat(np.arange(T), ROW_COUNTS), [-1, -1, T]]).astype(np.int32)
    types = types[rng.permutation(len(types))]
    R = len(types)
    proj = rng.standard_normal((R, dim)).astype(np.float32)
    rows_of = lambda t: np.nonzero(types == t)[0]
    r0 = rows_of(0)
    proj[r0[1:4]] = features[a1] + features[a2]                # three rows look at both tied pairs: the four head their lists
    key = ((np.arange(R) % N_KEYS) - 1).astype(np.int32)       # -1, 0..7 spread over the rows
    key[r0[0]] = 7                                             # its list is its own unfiltered top 64
    key[r0[1:4]] = 2
    key[rows_of(3)[:3]] = [6, 0, 6]                            # key 6 covers the whole 40-product type
    key[rows_of(4)[:2]] = [4, -1]
    rowptr, col = csr_of(type_idx)
    table, dproj, dtypes = cuda(features), cuda(proj), cuda(types)
    m = SimpleNamespace(dim=dim, R=R, type_idx=type_idx, features=features, proj=proj, types=types, key=key, by=by,
                        rows_of=rows_of, tied=(a1, b1, a2, b2), rowptr=rowptr, col=col, table=table, dproj=dproj, dtypes=dtypes,
                        dkey=cuda(key), cand_type=cuda(type_idx))
    m.want = peel(dproj, dtypes, rowptr, col, table, 256)      # the unfiltered reference, once
    top = m.want[0].cpu().numpy()

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
    for k in (1, 3, 4, 5):
        lists[k] = fill(heads(k), LENGTHS[k], rng.permutation(P))
    lists[2] = fill([a1, b2], 15, [x for x in heads(2) + list(rng.permutation(P)) if x not in (b1, a2)])
    lists[6] = fill(by(3), 45, list(by(2)[:3]) + heads(6))
    lists[7] = sorted(int(x) for x in top[r0[0], :64])
    assert len(lists[7]) == 64 and all(len(lists[k]) == n for k, n in LENGTHS.items())
    m.lists, m.ex = lists, ex_csr(lists)
    m.own = padded(lists, key)
    m.want_filtered = peel(dproj, dtypes, rowptr, col, table, 256, own=m.own)      # the filtered reference, once
    return m


def served(m, n, filt=False, slices=0, col=None, key=None, bad=None):
    from p_companion_amd import ops
    ex = ((m.dkey if key is None else key,) + m.ex) if filt else None
    return ops.retrieve_list_grouped(m.dproj, m.dtypes, m.rowptr, m.col if col is None else col, m.table, n, slices=slices,
                                     exclude=ex, bad=bad)


def reference(m, n, filt):
    i, s = m.want_filtered if filt else m.want
    return i[:, :n].contiguous(), s[:, :n].contiguous()


# ---- 1. every length against the peeled lists
@pytest.mark.parametrize("filt", [False, True], ids=["plain", "excluding"])
@pytest.mark.parametrize("n", NS)
def test_lists_equal_the_peeled_16_entry_lists(cat, n, filt):
    m = cat
    got, want = served(m, n, filt), reference(m, n, filt)
    assert got[0].shape == (m.R, n) and got[0].dtype == torch.int32 and got[1].dtype == torch.float32
    assert torch.equal(got[0], want[0]), (n, torch.nonzero((got[0] != want[0]).any(1)).reshape(-1)[:10].tolist())
    assert torch.equal(bits(got[1]), bits(want[1])), n
    if filt:
        idx = got[0].cpu().numpy()
        for r in range(m.R):
            assert not set(idx[r].tolist()) & set(m.lists[m.key[r]] if m.key[r] >= 0 else []), r


def test_the_references_are_what_they_are_meant_to_be(cat):
    """The fixture's own claims: the filter bites, the row that lists its own top 64 is served positions 64.., the fully
    excluded type is empty, the tied pairs head the three rows that look at them."""
    m = cat
    unf, fil = m.want[0].cpu().numpy(), m.want_filtered[0].cpu().numpy()
    assert (unf[:, :16] != fil[:, :16]).any(1).sum() >= 10
    r0, r3 = m.rows_of(0), m.rows_of(3)
    assert (fil[r0[0], :192] == unf[r0[0], 64:]).all()
    assert (fil[r3[0]] == -1).all() and (fil[r3[2]] == -1).all() and (fil[r3[1], :40] >= 0).all() and (fil[r3[1], 40:] == -1).all()
    a1, b1, a2, b2 = m.tied
    for r in r0[1:4]:
        assert sorted(unf[r, :4].tolist()) == sorted([a1, b1, a2, b2]) and list(unf[r, :4]).index(a1) + 1 == list(unf[r, :4]).index(b1)
        assert set(fil[r, :2].tolist()) == {b1, a2}            # a1 and b2 are in key 2's list


# ---- 2. the 16-entries' own bits
@pytest.mark.parametrize("n", [1, 10, 16])
def test_short_lists_are_the_16_entries_bits(cat, n):
    from p_companion_amd import ops
    m = cat
    assert same(served(m, n), ops.retrieve_topk_grouped(m.dproj, m.dtypes, m.rowptr, m.col, m.table, n))
    assert same(served(m, n, True), ops.retrieve_topk_grouped(m.dproj, m.dtypes, m.rowptr, m.col, m.table, n,
                                                              exclude=(m.dkey,) + m.ex))


# ---- 3. slices, candidate order, repeat calls, the rows' company
@pytest.mark.parametrize("n", [40, 200])
def test_same_bits_for_every_slicing_candidate_order_and_call(cat, n):
    m = cat
    rowptr = m.rowptr.cpu().numpy()
    col = m.col.cpu().numpy().copy()
    rng = np.random.default_rng(9)
    for t in range(T):
        rng.shuffle(col[rowptr[t]:rowptr[t + 1]])
    for filt in (False, True):
        want = reference(m, n, filt)
        for c, s in ((None, 1), (None, 7), (None, 64), (None, 0), (None, 0), (cuda(col), 0), (cuda(col), 5)):
            assert same(served(m, n, filt, slices=s, col=c), want), (filt, s, c is not None)


def test_subsets_of_the_rows_are_served_the_same_lists(cat):
    """Other tile fillings than the fixture's: two full tiles of one type, one row of another, every row alone in its type."""
    from p_companion_amd import ops
    m = cat
    n = 100
    want_i, want_s = reference(m, n, True)
    for rows in (np.concatenate([m.rows_of(0)[:2 * TILE], m.rows_of(1)[:1]]), np.array([m.rows_of(t)[0] for t in range(T)]),
                 m.rows_of(0)[::-1].copy()):
        sel = cuda(rows.astype(np.int64))
        got = ops.retrieve_list_grouped(m.dproj[sel].contiguous(), m.dtypes[sel].contiguous(), m.rowptr, m.col, m.table, n,
                                        exclude=(m.dkey[sel].contiguous(),) + m.ex)
        assert same(got, (want_i[sel], want_s[sel])), len(rows)


# ---- 4. adversarial arrival order
@pytest.mark.parametrize("order", ["ascending", "descending", "mixed"])
def test_sorted_candidate_streams(cat, order):
    """Type 0 with table[p] = alpha u, alpha ascending in type_col order, and one tile of rows beta u.  beta > 0: every
    candidate beats the threshold -- every chunk fills the buffer, the most compactions possible; beta < 0: no survivor after
    the first ones; both signs in one tile."""
    from p_companion_amd import ops
    m = cat
    rng = np.random.default_rng(77)
    u = rng.standard_normal(m.dim).astype(np.float32)
    feats = m.features.copy()
    ids = m.by(0)                                              # ascending ids: the order of type_col inside the type
    feats[ids] = (1 + np.arange(len(ids), dtype=np.float32) / 4096)[:, None] * u[None, :]
    beta = rng.uniform(0.5, 2.0, TILE).astype(np.float32)
    if order == "descending":
        beta = -beta
    if order == "mixed":
        beta[::2] *= -1
    proj, types = cuda(beta[:, None] * u[None, :]), torch.zeros(TILE, dtype=torch.int32, device="cuda")
    table = cuda(feats)
    want = peel(proj, types, m.rowptr, m.col, table, 256)
    first = want[0][:, 0].cpu().numpy()
    assert ((first == ids[-1]) == (beta > 0)).all() and ((first == ids[0]) == (beta < 0)).all()
    for n in (64, 256):
        for s in (0, 1):
            got = ops.retrieve_list_grouped(proj, types, m.rowptr, m.col, table, n, slices=s)
            assert same(got, (want[0][:, :n].contiguous(), want[1][:, :n].contiguous())), (n, s)


# ---- 5. ties
def test_a_type_of_identical_products_is_served_by_ascending_id(cat):
    from p_companion_amd import ops
    m = cat
    feats = m.features.copy()
    ids = m.by(2)
    assert len(ids) == 300
    feats[ids] = feats[ids[0]]
    table = cuda(feats)
    rows = cuda(m.rows_of(2).astype(np.int64))
    proj, types = m.dproj[rows].contiguous(), m.dtypes[rows].contiguous()
    first = torch.tensor([[int(ids[0])]], dtype=torch.int32, device="cuda").expand(len(rows), 1).contiguous()
    none = torch.full_like(first, -1)
    ex = lambda own: (torch.arange(len(rows), dtype=torch.int32, device="cuda"),) + ops.exclusion_csr(
        torch.arange(len(rows) + 1, dtype=torch.int32, device="cuda"), own.reshape(-1), include_self=False, num_products=P)
    for n in (17, 256):
        idx, sc = ops.retrieve_list_grouped(proj, types, m.rowptr, m.col, table, n)
        assert (idx.cpu().numpy() == ids[None, :n]).all(), n
        assert (bits(sc) == bits(sc)[:, :1]).all()
        assert same((idx, sc), peel(proj, types, m.rowptr, m.col, table, n))
        for own, lo in ((first, 1), (none, 0)):
            idx, sc = ops.retrieve_list_grouped(proj, types, m.rowptr, m.col, table, n, exclude=ex(own))
            assert (idx.cpu().numpy() == ids[None, lo:lo + n]).all(), (n, lo)


# ---- 6. the rank
@pytest.mark.parametrize("filt", [False, True], ids=["plain", "excluding"])
def test_position_k_of_a_list_is_the_product_of_rank_k(cat, filt):
    from p_companion_amd import ops
    m = cat
    n = 100
    idx, _ = served(m, n, filt)
    kw = dict(exclude=(m.dkey.repeat_interleave(n).contiguous(),) + m.ex, cand_type=m.cand_type) if filt else {}
    there = (idx >= 0).reshape(-1)
    types = torch.where(there, m.dtypes.repeat_interleave(n), torch.full_like(there, -1, dtype=torch.int32)).contiguous()
    rank, bad = ops.rank_grouped(m.dproj.repeat_interleave(n, 0).contiguous(), types, idx.clamp(min=0).reshape(-1).contiguous(),
                                 m.rowptr, m.col, m.table, **kw)
    want = torch.where(there, torch.arange(n, dtype=torch.int32, device="cuda").repeat(m.R), torch.full_like(rank, -1))
    assert int(bad) == 0 and torch.equal(rank, want), torch.nonzero(rank != want).reshape(-1)[:10].tolist()
    assert int(there.sum()) > 60 * n
    # 200 (row, product) pairs from outside the lists: behind them, or kept out
    rng = np.random.default_rng(5)
    got = idx.cpu().numpy()
    rows = rng.choice(np.nonzero(np.isin(m.types, (0, 1, 2)))[0], 200)
    prods = np.array([rng.choice(np.setdiff1d(m.by(m.types[r]), got[r])) for r in rows], np.int32)
    sel = cuda(rows.astype(np.int64))
    kw = dict(exclude=(m.dkey[sel].contiguous(),) + m.ex, cand_type=m.cand_type) if filt else {}
    rank, bad = ops.rank_grouped(m.dproj[sel].contiguous(), m.dtypes[sel].contiguous(), cuda(prods), m.rowptr, m.col, m.table, **kw)
    rank = rank.cpu().numpy()
    out = np.array([filt and m.key[r] >= 0 and int(p) in m.lists[m.key[r]] for r, p in zip(rows, prods)])
    assert int(bad) == 0 and (rank[out] == -1).all() and (rank[~out] >= n).all()


# ---- 7. float64
@pytest.mark.parametrize("filt", [False, True], ids=["plain", "excluding"])
def test_lists_against_float64_scores(cat, filt):
    """Every candidate whose float64 score exceeds the float64 n-th best by more than the band is served, and none that is
    below it by more than the band."""
    m = cat
    n = 100
    got = served(m, n, filt)[0].cpu().numpy()
    f64, p64 = m.features.astype(np.float64), m.proj.astype(np.float64)
    checked = 0
    for r in range(m.R):
        t = m.types[r]
        cand = m.by(t) if 0 <= t < T else np.zeros(0, np.int64)
        if filt and m.key[r] >= 0:
            cand = np.setdiff1d(cand, m.lists[m.key[r]])
        mine = got[r][got[r] >= 0]
        assert len(mine) == min(n, len(cand)) and len(set(mine.tolist())) == len(mine) and np.isin(mine, cand).all(), r
        if len(cand) <= n:
            continue
        s = f64[cand] @ p64[r]
        g = np.sort(s)[-n]
        band = 2 * (1e-5 + 1e-5 * abs(g))
        assert np.isin(cand[s > g + band], mine).all(), r
        assert not np.isin(cand[s < g - band], mine).any(), r
        checked += 1
    assert checked >= 3 * TILE


# ---- 8. padding and refusals
def test_padding_range_and_error_codes(cat):
    from p_companion_amd import _lib
    m = cat
    n = 64
    idx, sc = served(m, n)
    idx_h, sc_h = idx.cpu().numpy(), sc.cpu().numpy()
    for r in m.rows_of(4):                                     # 10 products
        assert (idx_h[r, :10] >= 0).all() and (idx_h[r, 10:] == -1).all() and np.isneginf(sc_h[r, 10:]).all()
        assert sorted(idx_h[r, :10].tolist()) == m.by(4).tolist() and np.isfinite(sc_h[r, :10]).all()
    nowhere = np.nonzero((m.types == 5) | (m.types == -1) | (m.types == T))[0]
    assert len(nowhere) == 4 and (idx_h[nowhere] == -1).all() and np.isneginf(sc_h[nowhere]).all()
    # keys out of range: served as -1, counted
    want = served(m, n, True)
    key = m.key.copy()
    free = np.nonzero(m.key == -1)[0]
    key[free[:4]] = [N_KEYS, N_KEYS + 1000, -2, 2 ** 31 - 1]
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert same(served(m, n, True, key=cuda(key), bad=bad), want) and int(bad) == 4
    assert same(served(m, 200, True, key=cuda(key), bad=bad), reference(m, 200, True)) and int(bad) == 8      # (added to)
    # a workspace one byte short: PC_EWORKSPACE, nothing written
    L = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out_i = torch.full((m.R, 256), 12345, dtype=torch.int32, device="cuda")
    out_s = torch.full((m.R, 256), 7.0, device="cuda")
    bad.zero_()
    for n in (17, 256):
        need = L.pc_retrieve_list_grouped_workspace_bytes(m.R, T, n, 0)
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        for keyed in (True, False):
            args = [p(m.dproj), p(m.dtypes), p(m.dkey) if keyed else None, m.R, p(m.rowptr), p(m.col), p(m.table), T,
                    p(m.ex[0]) if keyed else None, p(m.ex[1]) if keyed else None, N_KEYS if keyed else 0, n, m.dim, 0, p(out_i),
                    p(out_s), p(bad) if keyed else None, p(ws), need - 1, st]
            assert L.pc_retrieve_list_grouped(*args) == -3
            args[11] = 257
            assert L.pc_retrieve_list_grouped(*args) == -2
    torch.cuda.synchronize()
    assert (out_i == 12345).all() and (out_s == 7.0).all() and int(bad) == 0


# ---- 9. through PCompanionInference
def _graph(kind, dim):
    from p_companion_amd.data import DeviceBPG, generate_scaled_bpg
    host = generate_scaled_bpg(20_000, 100, seed=3, dim=dim)
    if kind == "int":
        return host
    g = dict(host.cuda())
    g["comp_pairs"] = cuda(host.complementary_pairs.astype(np.int32))
    g["max_degree"] = int(np.diff(host.cv_rowptr).max())
    return DeviceBPG(g, 100, dim)


@pytest.mark.parametrize("kind,dim", [("device", 128), ("int", 256)])
def test_recommend_batch_serves_100_per_type(kind, dim):
    from test_gpu_catalogue_eval import cfg
    from p_companion_amd import ops
    from p_companion_amd.inference import PCompanionInference
    from p_companion_amd.p_companion import PCompanion
    bpg = _graph(kind, dim)
    c = cfg(100, dim)
    torch.manual_seed(0)
    table = torch.randn(bpg.num_products, dim, generator=torch.Generator().manual_seed(11))
    inf = PCompanionInference(PCompanion(c, table), c, bpg)
    assert inf.grouped == (kind == "device")
    g = bpg.cuda()
    cv_rowptr, cv_col = g["cv_rowptr"].cpu().numpy(), g["cv_col"].cpu().numpy()
    q = torch.arange(0, 20_000, 97, dtype=torch.int32)
    b, k, n = len(q), c.NUM_COMP_TYPES, 100
    out = inf.model({"query_idx": q.cuda(), "query_types": inf.type_idx[q.cuda().long()]})
    proj = out["projected_embeddings"].contiguous().reshape(b * k, -1)
    row_types = out["complementary_types"].to(torch.int32).reshape(-1).contiguous()
    row_key = q.cuda().repeat_interleave(k).contiguous()
    mask = torch.rand(20_000, generator=torch.Generator().manual_seed(5)).cuda() < 0.7
    with pytest.raises(ValueError, match="256"):
        inf.recommend_batch(q, 257)

    for situation in ("plain", "exclusions", "eligible", "both"):
        if situation in ("exclusions", "both"):
            inf.set_exclusions()
        if situation in ("eligible", "both"):
            inf.set_eligible(mask)
        types, idx, sc = inf.recommend_batch(q, n)
        assert idx.shape == (b, k, n) and sc.shape == (b, k, n) and idx.dtype == torch.int32 and sc.dtype == torch.float32
        assert torch.equal(types, out["complementary_types"])
        exclude = (row_key,) + inf.exclusions if inf.exclusions is not None else None
        want = ops.retrieve_list_grouped(proj, row_types, inf.type_rowptr, inf.type_col, inf.features, n, exclude=exclude)
        assert same((idx.reshape(b * k, n), sc.reshape(b * k, n)), want), situation
        idx_h = idx.cpu().numpy()
        assert (idx_h[:, :, 16:] >= 0).sum() > 0.5 * idx_h[:, :, 16:].size      # (about 200 products per type, 140 eligible)
        if inf.eligible is not None:
            assert mask[idx[idx >= 0].long()].all()
        if inf.exclusions is not None:
            for i, query in enumerate(q.tolist()):
                gone = set(cv_col[cv_rowptr[query]:cv_rowptr[query + 1]].tolist()) | {query}
                assert not set(idx_h[i].reshape(-1).tolist()) & gone, query
        # the first 16 are recommend_batch(q, 16)'s
        _, idx16, sc16 = inf.recommend_batch(q, 16)
        if kind == "device" or inf.exclusions is not None:     # the grouped search: the same bits
            assert torch.equal(idx[:, :, :16], idx16) and torch.equal(bits(sc[:, :, :16]), bits(sc16)), situation
        else:
            # the per-row kernel sums in another order: the same scores within the band, and the same id wherever the
            # neighbouring scores are further away than the band
            live = idx16 >= 0
            assert torch.equal(live, idx[:, :, :16] >= 0)
            s = torch.nan_to_num(sc[:, :, :17].double(), neginf=-1e30)          # (-inf: past the end of a short type)
            band = 2 * (1e-5 + 1e-5 * s.abs())
            assert ((sc16.double() - s[:, :, :16]).abs() <= band[:, :, :16])[live].all()
            gap_next = ((s[:, :, :16] - s[:, :, 1:17]) > 2 * band[:, :, :16]) & live
            gap_prev = torch.ones_like(gap_next)
            gap_prev[:, :, 1:] = gap_next[:, :, :-1]
            clear = gap_next & gap_prev
            assert torch.equal(idx[:, :, :16][clear], idx16[clear]) and int(clear.sum()) > 0.9 * int(live.sum())
        inf.set_exclusions(False)
        inf.set_eligible(None)
