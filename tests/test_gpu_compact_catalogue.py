"""Long and diversified lists from the bf16 catalogue alone: pc_retrieve_list_grouped_bf16 (ops.retrieve_list_grouped on a bf16
table), pc_diversify_lists_bf16 / pc_inv_norm_bf16 (ops.diversify_lists_bf16, ops.inv_norm_bf16), ops.CompactCatalogue and
PCompanionInference(catalogue=ops.CompactCatalogue(...)).

Every reference is the EXISTING code.  A long bf16 list is the 16-entry bf16 entry peeled (tests/test_gpu_retrieval_list.py's
peel over the bf16 table: the chain is that entry's, so ids and score bits are compared as they are); on small integers, where
every partial sum is exact, it is the fp32 list entry on the widened table; against float64 it is check_rows of
tests/test_gpu_retrieval_grouped.py at its own TOL = 1e-5, as tests/test_gpu_retrieval_bf16.py uses it.  A diversified list
over the bf16 table is ops.diversify_lists on table.float(), bit for bit: widening is exact.  The catalogue, the rows and the
exclusion lists are test_gpu_retrieval_list.py's, restated over a table rounded to bf16.  Needs an MI355X."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_retrieval_grouped import TOL, check_rows, grouped_reference
from test_gpu_retrieval_list import (LENGTHS, N_KEYS, P, ROW_COUNTS, SIZES, T, TILE, bits, csr_of, cuda, ex_csr, padded, peel,
                                     same)

assert TOL == 1e-5 and P == 12_350 and SIZES == (9000, 3000, 300, 40, 10, 0) and ROW_COUNTS == (33, 31, 17, 15, 16, 1)
assert LENGTHS == {0: 0, 1: 1, 2: 15, 3: 16, 4: 17, 5: 33}

NS = (1, 16, 17, 32, 33, 63, 64, 65, 96, 97, 128, 255, 256)


# ---- the catalogue: test_gpu_retrieval_list.py's `cat`, the table rounded to bf16 and every reference over that table
@pytest.fixture(scope="module", params=[128, 256], ids=lambda d: f"D{d}")
def cat(request):
    from p_companion_amd import ops
    dim = request.param
    rng = np.random.default_rng(2000 + dim)
    type_idx = rng.permutation(np.repeat(np.arange(T), SIZES)).astype(np.int32)
    by = lambda t: np.nonzero(type_idx == t)[0]
    features = rng.standard_normal((P, dim)).astype(np.float32)
    t0 = by(0)
    a1, b1, a2, b2 = t0[100], t0[2000], t0[300], t0[3000]      # b is a copy of a: exactly tied scores
    features[b1], features[b2] = features[a1], features[a2]
    types = np.concatenate([np.repeat(np.arange(T), ROW_COUNTS), [-1, -1, T]]).astype(np.int32)
    types = types[rng.permutation(len(types))]
    R = len(types)
    proj = rng.standard_normal((R, dim)).astype(np.float32)
    rows_of = lambda t: np.nonzero(types == t)[0]
    r0 = rows_of(0)
    proj[r0[1:4]] = features[a1] + features[a2]
    key = ((np.arange(R) % N_KEYS) - 1).astype(np.int32)
    key[r0[0]] = 7
    key[r0[1:4]] = 2
    key[rows_of(3)[:3]] = [6, 0, 6]                            # key 6 covers the whole 40-product type
    key[rows_of(4)[:2]] = [4, -1]
    rowptr, col = csr_of(type_idx)
    table = ops.catalogue_bf16(cuda(features))
    rounded = table.float().cpu().numpy()
    dproj, dtypes = cuda(proj), cuda(types)
    m = SimpleNamespace(dim=dim, R=R, type_idx=type_idx, rounded=rounded, proj=proj, types=types, key=key, by=by,
                        rows_of=rows_of, rowptr=rowptr, col=col, table=table, dproj=dproj, dtypes=dtypes, dkey=cuda(key))
    m.want = peel(dproj, dtypes, rowptr, col, table, 256)      # the unfiltered reference, once: 16 calls of the bf16 16-entry
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

    heads = lambda k: [x for r in np.nonzero(key == k)[0] for x in top[r, :3] if x >= 0]
    lists = {0: [], 8: []}
    for k in (1, 3, 4, 5):
        lists[k] = fill(heads(k), LENGTHS[k], rng.permutation(P))
    lists[2] = fill([a1, b2], 15, [x for x in heads(2) + list(rng.permutation(P)) if x not in (b1, a2)])
    lists[6] = fill(by(3), 45, list(by(2)[:3]) + heads(6))
    lists[7] = sorted(int(x) for x in top[r0[0], :64])
    assert [len(lists[k]) for k in range(6)] == [0, 1, 15, 16, 17, 33] and set(by(3)) <= set(lists[6])
    m.lists, m.ex = lists, ex_csr(lists)
    m.own = padded(lists, key)
    m.want_filtered = peel(dproj, dtypes, rowptr, col, table, 256, own=m.own)      # the filtered reference, once
    return m


def served(m, n, filt=False, slices=0, col=None, key=None, bad=None, table=None, proj=None):
    from p_companion_amd import ops
    ex = ((m.dkey if key is None else key,) + m.ex) if filt else None
    return ops.retrieve_list_grouped(m.dproj if proj is None else proj, m.dtypes, m.rowptr, m.col if col is None else col,
                                     m.table if table is None else table, n, slices=slices, exclude=ex, bad=bad)


def reference(m, n, filt):
    i, s = m.want_filtered if filt else m.want
    return i[:, :n].contiguous(), s[:, :n].contiguous()


# ---- 1. the 16-entry bf16 entry's own bits
@pytest.mark.parametrize("n", [1, 10, 16])
def test_short_lists_are_the_bf16_16_entries_bits(cat, n):
    from p_companion_amd import ops
    m = cat
    assert same(served(m, n), ops.retrieve_topk_grouped(m.dproj, m.dtypes, m.rowptr, m.col, m.table, n))
    assert same(served(m, n, True), ops.retrieve_topk_grouped(m.dproj, m.dtypes, m.rowptr, m.col, m.table, n,
                                                              exclude=(m.dkey,) + m.ex))


# ---- 2. every length against the peeled bf16 lists
@pytest.mark.parametrize("filt", [False, True], ids=["plain", "excluding"])
@pytest.mark.parametrize("n", NS)
def test_lists_equal_the_peeled_bf16_16_entry_lists(cat, n, filt):
    m = cat
    got, want = served(m, n, filt), reference(m, n, filt)
    assert got[0].shape == (m.R, n) and got[0].dtype == torch.int32 and got[1].dtype == torch.float32
    assert torch.equal(got[0], want[0]), (n, torch.nonzero((got[0] != want[0]).any(1)).reshape(-1)[:10].tolist())
    assert torch.equal(bits(got[1]), bits(want[1])), n
    idx = got[0].cpu().numpy()
    if not filt:
        for r in m.rows_of(4):                                 # 10 products: -1 / -inf past the end
            assert (idx[r, :10] >= 0).all() and (idx[r, 10:] == -1).all() and torch.isneginf(got[1][r, 10:]).all()
    else:
        for r in range(m.R):
            assert not set(idx[r].tolist()) & set(m.lists[m.key[r]] if m.key[r] >= 0 else []), r
        r3 = m.rows_of(3)
        assert (idx[r3[0]] == -1).all() and (idx[r3[2]] == -1).all()              # the whole type is in key 6's list


# ---- 3. small integers: the fp32 list entry on the widened table, bit for bit
@pytest.mark.parametrize("n", [40, 200])
def test_small_integers_equal_the_fp32_list_entry_bit_for_bit(cat, n):
    from p_companion_amd import ops
    m = cat
    rng = np.random.default_rng(31 + m.dim)
    table = ops.catalogue_bf16(cuda(rng.integers(-3, 4, (P, m.dim)).astype(np.float32)))
    proj = cuda(rng.integers(-3, 4, (m.R, m.dim)).astype(np.float32))
    assert torch.equal(table.float().to(torch.bfloat16), table)
    for filt in (False, True):
        got = served(m, n, filt, table=table, proj=proj)
        want = served(m, n, filt, table=table.float(), proj=proj)
        assert same(got, want), filt
        live = got[1][got[0] >= 0]
        assert (live == live.round()).all() and live.abs().max() > 50             # integers, and not all of them zero


# ---- 4. slices, candidate order, repeat calls
@pytest.mark.parametrize("n", [40, 200])
def test_same_bits_for_every_slicing_candidate_order_and_call(cat, n):
    m = cat
    rowptr = m.rowptr.cpu().numpy()
    col = m.col.cpu().numpy().copy()
    rng = np.random.default_rng(9)
    for t in range(T):
        rng.shuffle(col[rowptr[t]:rowptr[t + 1]])
    assert (col != m.col.cpu().numpy()).sum() > 1000
    for filt in (False, True):
        want = reference(m, n, filt)
        for c, s in ((None, 0), (None, 1), (None, 3), (None, 64), (None, 0), (cuda(col), 0), (cuda(col), 3)):
            assert same(served(m, n, filt, slices=s, col=c), want), (filt, s, c is not None)


# ---- 5. float64 over the rounded table
def test_lists_of_200_against_float64_over_the_rounded_table(cat):
    m = cat
    n = 200
    idx, sc = served(m, n)
    ref = grouped_reference(m.proj, m.types, m.type_idx, m.rounded, n)
    check_rows(idx.cpu().numpy(), sc.cpu().numpy(), ref, m.proj, m.rounded, m.type_idx, m.types, n)
    assert sum(len(r[0]) == n for r in ref) >= 4 * TILE


# ---- 6. ties
def test_a_type_of_identical_rows_is_served_by_ascending_id(cat):
    from p_companion_amd import ops
    m = cat
    ids = m.by(2)
    assert len(ids) == 300
    table = m.table.clone()
    table[cuda(ids.astype(np.int64))] = table[int(ids[0])].clone()
    rows = cuda(m.rows_of(2).astype(np.int64))
    proj, types = m.dproj[rows].contiguous(), m.dtypes[rows].contiguous()
    for n in (17, 256):
        idx, sc = ops.retrieve_list_grouped(proj, types, m.rowptr, m.col, table, n)
        assert (idx.cpu().numpy() == ids[None, :n]).all(), n
        assert (bits(sc) == bits(sc)[:, :1]).all()


# ---- 7. keys out of range
def test_a_key_out_of_range_is_served_without_a_list_and_counted(cat):
    m = cat
    key = m.key.copy()
    free = np.nonzero(m.key == -1)[0]
    key[free[:4]] = [N_KEYS, N_KEYS + 1000, -2, 2 ** 31 - 1]
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert same(served(m, 64, True, key=cuda(key), bad=bad), reference(m, 64, True)) and int(bad) == 4
    assert same(served(m, 200, True, key=cuda(key), bad=bad), reference(m, 200, True)) and int(bad) == 8      # (added to)


# ---- 8. the list entry's refusals
def test_list_entry_return_codes(cat):
    from p_companion_amd import _lib
    m = cat
    L = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out_i = torch.full((m.R, 256), 12345, dtype=torch.int32, device="cuda")
    out_s = torch.full((m.R, 256), 7.0, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    need = L.pc_retrieve_list_grouped_bf16_workspace_bytes(m.R, T, 256, 0)
    assert need == L.pc_retrieve_list_grouped_workspace_bytes(m.R, T, 256, 0) > 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    names = ("proj types row_key rows type_rowptr type_col table n_types ex_rowptr ex_col n_keys n dim slices out_idx out_score "
             "bad_count ws ws_bytes stream").split()

    def call(keyed, **kw):
        a = dict(zip(names, [p(m.dproj), p(m.dtypes), p(m.dkey) if keyed else None, m.R, p(m.rowptr), p(m.col), p(m.table), T,
                             p(m.ex[0]) if keyed else None, p(m.ex[1]) if keyed else None, N_KEYS if keyed else 0, 256, m.dim, 0,
                             p(out_i), p(out_s), p(bad) if keyed else None, p(ws), need, st]))
        a.update(kw)
        return L.pc_retrieve_list_grouped_bf16(*a.values())

    for keyed in (False, True):
        for name in ("proj", "types", "type_rowptr", "type_col", "table", "out_idx", "out_score", "ws"):
            assert call(keyed, **{name: None}) == -1, name
        assert call(keyed, rows=0) == -1 and call(keyed, n_types=0) == -1
        for kw in (dict(n=0), dict(n=257), dict(dim=64), dict(slices=-1), dict(slices=65),
                   dict(table=ctypes.c_void_p(m.table.data_ptr() + 2)), dict(table=ctypes.c_void_p(m.table.data_ptr() + 8))):
            assert call(keyed, **kw) == -2, kw
        assert call(keyed, ws_bytes=need - 1) == -3
    assert call(True, ex_rowptr=None) == -1 and call(True, ex_col=None) == -1 and call(True, bad_count=None) == -1
    assert call(True, n_keys=-1) == -1 and call(False, n_keys=1) == -1 and call(False, ex_col=p(m.ex[1])) == -1
    torch.cuda.synchronize()
    assert (out_i == 12345).all() and (out_s == 7.0).all() and int(bad) == 0      # nothing was launched
    assert call(False) == 0 and call(True) == 0
    torch.cuda.synchronize()
    assert same((out_i, out_s), reference(m, 256, True))


# ---- 9. diversified lists: the fp32 entry on the widened table, bit for bit
DP, DR = 600, 37
SHAPES = ((1, 1), (5, 5), (16, 10), (17, 17), (64, 16), (65, 10), (200, 200), (256, 32), (256, 256))
TYPE_SIZES = (400, 150, 50)                # pools of 256: full, short, shorter


@pytest.fixture(scope="module", params=[128, 256], ids=lambda d: f"D{d}")
def gauss(request):
    from p_companion_amd import ops
    dim = request.param
    rng = np.random.default_rng(1900 + dim)
    t16 = ops.catalogue_bf16(cuda(rng.standard_normal((DP, dim)).astype(np.float32)))
    type_idx = rng.permutation(np.repeat(np.arange(3), TYPE_SIZES)).astype(np.int32)
    order = np.argsort(type_idx, kind="stable").astype(np.int32)
    rowptr = np.concatenate([[0], np.cumsum(TYPE_SIZES)]).astype(np.int32)
    types = rng.permutation(np.repeat(np.arange(3), (25, 8, 4))).astype(np.int32)
    proj = rng.standard_normal((DR, dim)).astype(np.float32)
    lists = {}

    def pool(m):                                          # retrieve_list_grouped(m) over the bf16 table, once per m
        if m not in lists:
            lists[m] = ops.retrieve_list_grouped(cuda(proj), cuda(types), cuda(rowptr), cuda(order), t16, m)
        return lists[m]

    wide = t16.float()
    return SimpleNamespace(dim=dim, t16=t16, wide=wide, scale16=ops.inv_norm_bf16(t16), scale32=ops.inv_norm(wide), pool=pool)


@pytest.mark.parametrize("m,n", SHAPES)
def test_diversified_lists_equal_the_fp32_entry_on_the_widened_table(gauss, m, n):
    from p_companion_amd import ops
    g = gauss
    idx, sc = g.pool(m)
    assert int((idx >= 0).sum()) >= 25 * min(m, 256) // 2
    for s16, s32 in ((None, None), (g.scale16, g.scale32)):
        for lam in (0.0, 0.3, 0.7, 1.0):
            got = ops.diversify_lists_bf16(idx, sc, g.t16, n, lam, scale=s16)
            want = ops.diversify_lists(idx, sc, g.wide, n, lam, scale=s32)
            assert got[0].shape == (DR, n) and got[0].dtype == torch.int32 and got[1].dtype == torch.float32
            assert same(got, want), (lam, s16 is not None)


@pytest.mark.parametrize("m,n", [(65, 10), (256, 32)])
def test_a_pool_with_holes_bad_scores_and_bad_ids(gauss, m, n):
    from p_companion_amd import ops
    g = gauss
    idx, sc = (t.clone() for t in g.pool(m))
    rng = np.random.default_rng(m)
    idx[cuda(rng.random((DR, m)) < 0.2)] = -1             # -1 slots anywhere in the pool
    idx[3] = -1                                           # a row without a candidate
    sc[5, 0], sc[5, m // 2], sc[6, m - 1] = float("nan"), float("inf"), float("-inf")
    out_of_range = [DP, DP + 1000, -2, 2 ** 31 - 1, -2 ** 31]
    for k, x in enumerate(out_of_range):
        idx[7 + k, (3 * k) % m] = x
    bad16, bad32 = (torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(2))
    for lam in (0.3, 0.7):
        got = ops.diversify_lists_bf16(idx, sc, g.t16, n, lam, scale=g.scale16, bad=bad16)
        want = ops.diversify_lists(idx, sc, g.wide, n, lam, scale=g.scale32, bad=bad32)
        assert same(got, want), lam
    assert int(bad16) == int(bad32) == 2 * len(out_of_range)
    assert (got[0][3] == -1).all() and torch.isneginf(got[1][3]).all()
    e_i, e_s = ops.diversify_lists_bf16(idx[:0], sc[:0], g.t16, n, 0.5)
    assert e_i.shape == (0, n) and e_s.shape == (0, n)


# ---- 10. the cosine's factors
@pytest.mark.parametrize("dim", [128, 256])
def test_inv_norm_bf16_is_inv_norm_of_the_widened_table(dim):
    from p_companion_amd import ops
    rng = np.random.default_rng(60 + dim)
    table = rng.standard_normal((1000, dim)).astype(np.float32)
    table[5] = 0
    table[6] = 0
    table[6, 3] = 4.0
    table[9] = 0
    table[9, dim - 1] = 2.0 ** -7
    t16 = ops.catalogue_bf16(cuda(table))
    got = ops.inv_norm_bf16(t16)
    assert got.dtype == torch.float32 and got.shape == (1000,)
    assert torch.equal(bits(got), bits(ops.inv_norm(t16.float())))
    g = got.cpu().numpy()
    assert g[5] == 0.0 and g[6] == 0.25 and g[9] == 128.0
    for rows in (1, 15, 17, 999):                         # every grid: the same bits
        assert torch.equal(bits(ops.inv_norm_bf16(t16[:rows])), bits(got[:rows])), rows


# ---- 11. the diversify entries' refusals
def test_diversify_bf16_return_codes():
    from p_companion_amd import _lib
    L = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    m, n, dim = 20, 5, 128
    idx = torch.zeros(DR, m, dtype=torch.int32, device="cuda")
    sc = torch.zeros(DR, m, device="cuda")
    table = torch.zeros(DP + 1, dim, dtype=torch.bfloat16, device="cuda")
    out_i = torch.full((DR, m), 12345, dtype=torch.int32, device="cuda")
    out_s = torch.full((DR, m), 7.0, device="cuda")

    def call(**kw):
        a = dict(idx=p(idx), score=p(sc), rows=DR, m=m, table=p(table), scale=None, num_products=DP, dim=dim, n=n, lam=0.5,
                 out_idx=p(out_i), out_score=p(out_s), bad=None, stream=st)
        a.update(kw)
        return L.pc_diversify_lists_bf16(*a.values())

    for kw in (dict(m=0), dict(m=257), dict(n=0), dict(n=m + 1), dict(dim=64), dict(dim=192), dict(lam=-0.01), dict(lam=1.01),
               dict(lam=float("nan")), dict(rows=-1), dict(num_products=0), dict(idx=None), dict(score=None), dict(table=None),
               dict(out_idx=None), dict(out_score=None), dict(table=ctypes.c_void_p(table.data_ptr() + 2)),
               dict(table=ctypes.c_void_p(table.data_ptr() + 8))):
        assert call(**kw) == -2, kw
    assert call(rows=0) == 0 and call(rows=0, idx=None, score=None, out_idx=None, out_score=None) == 0
    torch.cuda.synchronize()
    assert (out_i == 12345).all() and (out_s == 7.0).all()          # nothing was launched
    assert call() == 0 and call(lam=0.0) == 0 and call(lam=1.0) == 0
    norm = torch.empty(DP, device="cuda")
    assert L.pc_inv_norm_bf16(p(table), DP, dim, p(norm), st) == 0
    assert L.pc_inv_norm_bf16(None, DP, dim, p(norm), st) == -1 and L.pc_inv_norm_bf16(p(table), DP, dim, None, st) == -1
    assert L.pc_inv_norm_bf16(p(table), 0, dim, p(norm), st) == -1 and L.pc_inv_norm_bf16(p(table), DP, 64, p(norm), st) == -2
    assert L.pc_inv_norm_bf16(ctypes.c_void_p(table.data_ptr() + 2), DP, dim, p(norm), st) == -2
    torch.cuda.synchronize()


# ---- 12. through PCompanionInference
def test_a_compact_catalogue_serves_long_and_diversified_lists_without_the_fp32_features():
    from test_gpu_catalogue_eval import cfg
    from p_companion_amd import ops
    from p_companion_amd.data import DeviceBPG, generate_device_bpg
    from p_companion_amd.inference import PCompanionInference
    from p_companion_amd.p_companion import PCompanion
    dim, products = 128, 20_000
    bpg = generate_device_bpg(products, 100, seed=3, dim=dim)
    features = bpg.arrays["features"]
    c = cfg(100, dim)
    torch.manual_seed(0)
    model = PCompanion(c, torch.randn(products, dim, generator=torch.Generator().manual_seed(11)))
    no_feat = DeviceBPG({k: v for k, v in bpg.arrays.items() if k != "features"}, bpg.n_types, bpg.dim)
    cc = ops.CompactCatalogue(features)
    assert cc.table.dtype == torch.bfloat16 and torch.equal(cc.table, ops.catalogue_bf16(features))
    assert ops.CompactCatalogue(cc.table).table is cc.table                       # a bf16 input is taken as it is
    assert torch.equal(bits(cc.inv_norm), bits(ops.inv_norm(cc.table.float()))) and cc.inv_norm is cc.inv_norm
    compact = PCompanionInference(model, c, no_feat, catalogue=cc)
    bare = PCompanionInference(model, c, no_feat, catalogue=cc.table)
    assert compact.catalogue is cc.table and compact.features is None and compact.compact is cc and bare.compact is None
    q = torch.arange(0, products, 39, dtype=torch.int32)[:512]
    assert len(q) == 512
    b, k = len(q), c.NUM_COMP_TYPES
    out = compact.model({"query_idx": q.cuda(), "query_types": compact.type_idx[q.cuda().long()]})
    proj = out["projected_embeddings"].contiguous().reshape(b * k, -1)
    row_types = out["complementary_types"].to(torch.int32).reshape(-1).contiguous()
    row_key = q.cuda().repeat_interleave(k).contiguous()
    mask = torch.rand(products, generator=torch.Generator().manual_seed(5)).cuda() < 0.7
    wide = cc.table.float()
    cosine = ops.inv_norm(wide)
    flat = lambda t, n: t.reshape(b * k, n)
    for situation in ("plain", "both"):
        for inf in (compact, bare):
            if situation == "both":
                inf.set_exclusions()
                inf.set_eligible(mask)
            else:
                inf.set_exclusions(False)
                inf.set_eligible(None)
        exclude = (row_key,) + compact.exclusions if compact.exclusions is not None else None
        # up to 16: the bare tensor's bits
        got, want = compact.recommend_batch(q, 10), bare.recommend_batch(q, 10)
        assert torch.equal(got[0], want[0]) and same(got[1:], want[1:]), situation
        # 100: the direct call on the bf16 table
        types, idx, sc = compact.recommend_batch(q, 100)
        assert idx.shape == (b, k, 100) and torch.equal(types, out["complementary_types"])
        want = ops.retrieve_list_grouped(proj, row_types, compact.type_rowptr, compact.type_col, cc.table, 100, exclude=exclude)
        assert same((flat(idx, 100), flat(sc, 100)), want), situation
        assert (idx[:, :, 16:] >= 0).sum() > 0.5 * idx[:, :, 16:].numel()
        if situation == "both":
            assert mask[idx[idx >= 0].long()].all() and not (idx == q.cuda()[:, None, None]).any()
        # diversified: ops.diversify_lists over the widened table on that pool
        _, p_idx, p_sc = compact.recommend_batch(q, 64)
        for sim, scale in (("cosine", cosine), ("dot", None)):
            got = compact.recommend_diverse_batch(q, 10, pool=64, diversity=0.3, similarity=sim)
            ref = ops.diversify_lists(flat(p_idx, 64), flat(p_sc, 64), wide, 10, 1.0 - 0.3, scale=scale)
            assert torch.equal(got[0], types) and same((flat(got[1], 10), flat(got[2], 10)), ref), (situation, sim)
        assert not torch.equal(got[1], compact.recommend_batch(q, 10)[1])          # the re-rank does something
        for pool in (16, 64, 256):
            got, want = compact.recommend_diverse_batch(q, 10, pool=pool, diversity=0.0), compact.recommend_batch(q, 10)
            assert torch.equal(got[0], want[0]) and same(got[1:], want[1:]), (situation, pool)
        # the bare tensor beside it refuses what it refused
        with pytest.raises(ValueError, match="bf16 catalogue serves at most 16"):
            bare.recommend_batch(q, 17)
        with pytest.raises(ValueError, match="without them"):
            bare.recommend_diverse_batch(q, 10, pool=16)
    # ranks still need the fp32 catalogue
    with pytest.raises(ValueError, match="fp32 catalogue"):
        compact.rank_targets(q, q)
    with pytest.raises(ValueError, match="fp32 catalogue"):
        compact.evaluate_catalogue(None)                                          # (refused before the dataset is looked at)
    with pytest.raises(ValueError, match="256"):
        compact.recommend_batch(q, 257)
