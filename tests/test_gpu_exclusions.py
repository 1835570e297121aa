"""Per-row exclusion lists in the grouped retrieval and rank (pc_retrieve_topk_grouped_excluding / pc_rank_grouped_excluding,
ops.exclusion_csr, PCompanionInference.set_exclusions / set_eligible).

The oracle is the EXISTING unfiltered entry on a reduced catalogue: for every key a type_col without that key's ids is built
with torch and the rows of the key go through ops.retrieve_topk_grouped / ops.rank_grouped as they are.  A (row, product) score
has the same bits wherever it is computed (tests/test_gpu_retrieval_grouped.py, tests/test_gpu_rank_grouped.py), so every
comparison is bit for bit; the one tolerance is the float64 band of tests/test_gpu_rank_grouped.py, 2 (1e-5 + 1e-5 |g|), taken
from that file.  Needs an MI355X."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

P = 12_250
SIZES = (9000, 3000, 200, 40, 10, 0)                           # three automatic slices, ..., shorter than n = 16, empty
T = len(SIZES)
ROW_TYPES = [0] * 70 + [1] * 17 + [2] + [3] * 3 + [4] * 2 + [5] + [-1] * 2
R = len(ROW_TYPES)                                             # 96: tiles of 64 + 6 (D = 128), 32 + 32 + 6 (D = 256)
N_KEYS = 8                                                     # keys 0..6 carry the lists below, key 7 is not used by a row
LENGTHS = {0: 0, 1: 1, 2: 15, 3: 16, 4: 17, 5: 33}             # (key 6: the whole 40-product type and more)


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def csr_of(type_idx, keep=None):
    """type_rowptr / type_col (device) over the products with keep[p] (all if None), ascending inside a type."""
    ids = np.arange(P) if keep is None else np.nonzero(keep)[0]
    order = ids[np.argsort(type_idx[ids], kind="stable")].astype(np.int32)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(type_idx[ids], minlength=T))]).astype(np.int32)
    return cuda(rowptr), cuda(order)


def ex_csr(lists):
    rowptr = np.concatenate([[0], np.cumsum([len(lists[k]) for k in range(N_KEYS)])]).astype(np.int32)
    col = np.concatenate([np.asarray(lists[k], np.int64) for k in range(N_KEYS)] + [np.zeros(0, np.int64)]).astype(np.int32)
    return cuda(rowptr), cuda(col)


@pytest.fixture(scope="module", params=[128, 256], ids=lambda d: f"D{d}")
def cat(request):
    from p_companion_amd import ops
    dim = request.param
    rng = np.random.default_rng(dim)
    type_idx = rng.permutation(np.repeat(np.arange(T), SIZES)).astype(np.int32)
    # products 1 (the key that lists itself) and the four tied ones are of type 0
    by = lambda t: np.nonzero(type_idx == t)[0]
    if type_idx[1] != 0:
        j = by(0)[5]
        type_idx[[1, j]] = type_idx[[j, 1]]
    features = rng.standard_normal((P, dim)).astype(np.float32)
    t0 = by(0)
    t0 = t0[t0 > 10]
    a1, b1, a2, b2 = t0[100], t0[2000], t0[300], t0[3000]      # a < b: b is a copy of a
    features[b1], features[b2] = features[a1], features[a2]
    proj = rng.standard_normal((R, dim)).astype(np.float32)
    types = np.array(ROW_TYPES, np.int32)
    # rows 1..3 look at both tied pairs: the four products head their lists (scores about D against N(0, D))
    proj[1:4] = features[a1] + features[a2]
    key = ((np.arange(R) % 8) - 1).astype(np.int32)            # -1, 0..6 spread over the rows
    key[0] = 5                                                 # row 0: its list is its own unfiltered top 16 (+ other types)
    key[1:4] = 2                                               # the tied rows
    key[4] = 1                                                 # the key that lists itself
    t3rows = np.nonzero(types == 3)[0]
    t4rows = np.nonzero(types == 4)[0]
    key[t3rows] = [6, 0, 6]                                    # key 6 covers the whole 40-product type
    key[t4rows] = [4, -1]                                      # key 4 covers the whole 10-product type
    rowptr, col = csr_of(type_idx)
    table, dproj, dtypes = cuda(features), cuda(proj), cuda(types)
    top, _ = ops.retrieve_topk_grouped(dproj, dtypes, rowptr, col, table, 16)
    top = top.cpu().numpy()

    def fill(first, length, pool):
        """`first` and then ids of `pool` (in the pool's order) up to `length` distinct ids, ascending"""
        out = list(dict.fromkeys(int(x) for x in first))[:length]
        for x in pool:
            if len(out) >= length:
                break
            if int(x) not in out:
                out.append(int(x))
        assert len(out) == length
        return sorted(out)

    heads = lambda k: [x for r in np.nonzero(key == k)[0] for x in top[r, :3] if x >= 0]      # what the key's rows serve first
    others = rng.permutation(np.concatenate([by(1), by(2)]))
    lists = {0: [], 7: []}
    lists[1] = [1]
    free = lambda pool: [x for x in pool if x not in (b1, a2)]
    lists[2] = fill([a1, b2], 15, free(heads(2) + list(rng.permutation(P))))  # excluded a1 < kept b1, kept a2 < excluded b2
    assert b1 not in lists[2] and a2 not in lists[2]
    lists[3] = fill(heads(3), 16, rng.permutation(P))
    lists[4] = fill(by(4), 17, heads(4) + list(rng.permutation(P)))
    lists[5] = fill(top[0], 33, others)                        # row 0's unfiltered top 16 and 17 products of types 1 and 2
    lists[6] = fill(by(3), 45, list(by(2)[:3]) + heads(6))
    for k, n in LENGTHS.items():
        assert len(lists[k]) == n
    ex_rowptr, ex_col = ex_csr(lists)
    # targets: heads of the unfiltered lists (some of them excluded), products deep in the type, the special ones
    targets = np.zeros(R, np.int32)
    for r in range(R):
        t = types[r]
        mine = by(t) if t >= 0 else by(0)
        if len(mine) == 0:
            targets[r] = by(0)[0]                              # the empty type: any product, no candidate of it
        elif r % 3 == 1 or top[r, r % 5] < 0:
            targets[r] = rng.choice(mine)
        else:
            targets[r] = top[r, r % 16] if top[r, r % 16] >= 0 else top[r, 0]
    targets[0] = top[0, 3]                                     # excluded: in its own key's list
    targets[1], targets[2], targets[3] = b1, a2, a1            # kept copy above, kept original below, excluded original
    targets[4] = 1                                             # the key itself
    targets[t3rows] = by(3)[[0, 7, 39]]
    return SimpleNamespace(dim=dim, type_idx=type_idx, features=features, proj=proj, types=types, key=key, lists=lists,
                           targets=targets, top=top, tied=(a1, b1, a2, b2), rowptr=rowptr, col=col, table=table, dproj=dproj,
                           dtypes=dtypes, dkey=cuda(key), dtargets=cuda(targets), ex=(ex_rowptr, ex_col),
                           cand_type=cuda(type_idx), by=by)


def rows_of(m, k):
    return np.nonzero(m.key == k)[0]


def reduced(m, k, lists=None):
    """the catalogue's CSR without key k's ids"""
    keep = np.ones(P, bool)
    ids = np.asarray((lists or m.lists)[k] if k >= 0 else [], np.int64)
    keep[ids[ids < P]] = False
    return csr_of(m.type_idx, keep)


def filtered(m, n, slices=0, key=None, ex=None, col=None, bad=None):
    from p_companion_amd import ops
    return ops.retrieve_topk_grouped(m.dproj, m.dtypes, m.rowptr, m.col if col is None else col, m.table, n, slices=slices,
                                     exclude=(m.dkey if key is None else key,) + (m.ex if ex is None else ex), bad=bad)


def ranked(m, key=None, ex=None, col=None, slices=0, bad=None, targets=None):
    from p_companion_amd import ops
    return ops.rank_grouped(m.dproj, m.dtypes, m.dtargets if targets is None else targets, m.rowptr,
                            m.col if col is None else col, m.table, slices=slices, bad=bad,
                            exclude=(m.dkey if key is None else key,) + (m.ex if ex is None else ex), cand_type=m.cand_type)


# ---- 1. retrieval against reduced catalogues
def test_filtered_lists_equal_the_unfiltered_entry_on_reduced_catalogues(cat):
    from p_companion_amd import ops
    m = cat
    for n in (1, 10, 16):
        want_i = torch.empty(R, n, dtype=torch.int32, device="cuda")
        want_s = torch.empty(R, n, dtype=torch.float32, device="cuda")
        for k in range(-1, 7):
            rows = torch.from_numpy(rows_of(m, k)).cuda()
            rp, cl = reduced(m, k)
            want_i[rows], want_s[rows] = ops.retrieve_topk_grouped(m.dproj[rows], m.dtypes[rows], rp, cl, m.table, n)
        for slices in (1, 7, 64, 0):
            idx, sc = filtered(m, n, slices)
            assert torch.equal(idx, want_i), (n, slices, torch.nonzero((idx != want_i).any(1)).reshape(-1)[:10].tolist())
            assert torch.equal(sc, want_s), (n, slices)
        got = idx.cpu().numpy()
        for r in range(R):
            assert not set(got[r].tolist()) & set(m.lists[m.key[r]] if m.key[r] >= 0 else []), r
    # the filter bit: most rows with a list serve something else than without it
    assert (got != m.top).any(1).sum() >= 10
    # row 0, whose list is its unfiltered top 16: unfiltered positions 17..32, from two reduced runs
    one = slice(0, 1)
    keep = np.ones(P, bool)
    first, _ = ops.retrieve_topk_grouped(m.dproj[one], m.dtypes[one], *csr_of(m.type_idx, keep), m.table, 16)
    keep[first.cpu().numpy()[0]] = False
    second, sc2 = ops.retrieve_topk_grouped(m.dproj[one], m.dtypes[one], *csr_of(m.type_idx, keep), m.table, 16)
    assert sorted(first.cpu().tolist()[0]) == [x for x in m.lists[5] if m.type_idx[x] == 0]
    assert torch.equal(idx[one], second) and torch.equal(sc[one], sc2) and not set(first.cpu().tolist()[0]) & set(got[0].tolist())
    # the short and the fully excluded types
    t3, t4 = np.nonzero(m.types == 3)[0], np.nonzero(m.types == 4)[0]
    assert (got[t3[0]] == -1).all() and (got[t3[2]] == -1).all() and (got[t3[1]] >= 0).all()
    assert (got[t4[0]] == -1).all() and (got[t4[1], :10] >= 0).all() and (got[t4[1], 10:] == -1).all()
    assert torch.isinf(sc[int(t3[0])]).all()


# ---- 2. no lists
def test_no_key_and_empty_lists_equal_the_existing_entries(cat):
    from p_companion_amd import ops
    m = cat
    idx0, sc0 = ops.retrieve_topk_grouped(m.dproj, m.dtypes, m.rowptr, m.col, m.table, 16)
    rank0, _ = ops.rank_grouped(m.dproj, m.dtypes, m.dtargets, m.rowptr, m.col, m.table)
    none = torch.full_like(m.dkey, -1)
    empty = (torch.zeros(N_KEYS + 1, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"))
    for key, ex in ((none, m.ex), (m.dkey, empty), (none, empty)):
        idx, sc = filtered(m, 16, key=key, ex=ex)
        assert torch.equal(idx, idx0) and torch.equal(sc, sc0)
        rank, bad = ranked(m, key=key, ex=ex)
        # (the one difference the contract names: a target that is no candidate of the row's type -- the empty type's row)
        want = torch.where(m.cand_type[m.dtargets.long()] == m.dtypes, rank0, torch.full_like(rank0, -1))
        assert torch.equal(rank, want) and int(bad) == 0
        assert int((want != rank0).sum()) == 1


# ---- 3. rank consistency
def test_rank_below_16_exactly_where_the_filtered_list_holds_the_target(cat):
    m = cat
    idx, _ = filtered(m, 16)
    rank, bad = ranked(m)
    idx, rank = idx.cpu().numpy(), rank.cpu().numpy()
    assert int(bad) == 0
    inside = (rank >= 0) & (rank < 16)
    r = np.nonzero(inside)[0]
    assert (idx[r, rank[r]] == m.targets[r]).all(), r[idx[r, rank[r]] != m.targets[r]][:10]
    assert not (idx[~inside] == m.targets[~inside][:, None]).any()
    assert 20 < inside.sum() < R and (rank >= 16).sum() > 10   # (every branch saw rows)


# ---- 4. rank against reduced catalogues and float64
def expected_ranks(m, lists=None):
    from p_companion_amd import ops
    lists = lists or m.lists
    want = torch.empty(R, dtype=torch.int32, device="cuda")
    for k in range(-1, 7):
        rows = torch.from_numpy(rows_of(m, k)).cuda()
        rp, cl = reduced(m, k, lists)
        want[rows], _ = ops.rank_grouped(m.dproj[rows], m.dtypes[rows], m.dtargets[rows], rp, cl, m.table)
    want = want.cpu().numpy()
    for r in range(R):
        out = m.key[r] >= 0 and m.targets[r] in lists[m.key[r]]
        if m.types[r] >= 0 and (out or m.type_idx[m.targets[r]] != m.types[r]):
            want[r] = -1
    return want


def test_ranks_equal_the_unfiltered_entry_on_reduced_catalogues(cat):
    from test_gpu_rank_grouped import band64
    m = cat
    want = expected_ranks(m)
    rank, bad = ranked(m)
    rank = rank.cpu().numpy()
    assert int(bad) == 0 and (rank == want).all(), np.nonzero(rank != want)[0][:10]
    a1, b1, a2, b2 = m.tied
    t3 = np.nonzero(m.types == 3)[0]
    # excluded target, the kept copy above an excluded original, the kept original below an excluded copy, excluded original,
    # the key itself, the fully excluded type (and a row of that type under another key), the empty type, no type
    assert rank[0] == -1 and rank[3] == -1 and rank[4] == -1 and rank[t3[0]] == -1 and rank[t3[2]] == -1 and rank[t3[1]] >= 0
    assert rank[m.types == 5][0] == -1 and (rank[m.types == -1] == -1).all()
    unf = ranked(m, key=torch.full_like(m.dkey, -1))[0].cpu().numpy()
    # a1 (excluded, the same score, the lower index) stood in front of b1; b2 stands behind a2 and was never counted
    assert rank[1] in (unf[1] - 1, unf[1] - 2) and rank[2] in (unf[2], unf[2] - 1) and unf[1] <= 3 and unf[2] <= 3
    assert (rank >= 1000).sum() >= 5 and ((rank >= 0) & (rank < 16)).sum() >= 20        # deep and head targets
    assert (rank != unf).sum() > 5
    # list ids of other types change nothing: key 5 without its 17 products of types 1 and 2, over the rows of type 0
    lists = dict(m.lists)
    lists[5] = [x for x in m.lists[5] if m.type_idx[x] == 0]
    assert len(lists[5]) == 16
    rows0 = (m.key == 5) & (m.types == 0)
    assert rows0.sum() >= 5
    assert (ranked(m, ex=ex_csr(lists))[0].cpu().numpy()[rows0] == rank[rows0]).all()
    assert torch.equal(filtered(m, 16, ex=ex_csr(lists))[0][cuda(rows0)], filtered(m, 16)[0][cuda(rows0)])
    # float64: the band of tests/test_gpu_rank_grouped.py over each key's reduced catalogue
    for k in range(-1, 7):
        rows = rows_of(m, k)
        rows = rows[rank[rows] >= 0]
        ti = m.type_idx.copy()
        if k >= 0:
            ti[np.asarray(m.lists[k], np.int64)] = -2
        lo, hi = band64(m.proj[rows], m.types[rows], m.targets[rows], ti, m.features)
        off = rows[(rank[rows] < lo) | (rank[rows] > hi)]
        assert off.size == 0, (k, off[:10])


# ---- 5. range
def test_keys_and_ids_out_of_range_and_error_codes(cat):
    from p_companion_amd import _lib
    m = cat
    idx0, sc0 = filtered(m, 16)
    rank0, _ = ranked(m)
    key = m.key.copy()
    free = np.nonzero(m.key == -1)[0]
    key[free[:4]] = [N_KEYS, N_KEYS + 1000, -2, 2 ** 31 - 1]
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    idx, sc = filtered(m, 16, key=cuda(key), bad=bad)
    assert torch.equal(idx, idx0) and torch.equal(sc, sc0) and int(bad) == 4
    rank, bad = ranked(m, key=cuda(key), bad=bad)
    assert torch.equal(rank, rank0) and int(bad) == 8          # (a counter is added to)
    # list ids past the table (the lists stay ascending)
    lists = {k: list(v) + ([P, P + 7, 2 ** 31 - 1] if k in (2, 3, 5) else []) for k, v in m.lists.items()}
    idx, sc = filtered(m, 16, ex=ex_csr(lists))
    assert torch.equal(idx, idx0) and torch.equal(sc, sc0)
    rank, bad = ranked(m, ex=ex_csr(lists))
    assert torch.equal(rank, rank0) and int(bad) == 0
    # error codes, before anything is launched
    L = _lib.lib()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out_i = torch.full((R, 17), 12345, dtype=torch.int32, device="cuda")
    out_s = torch.zeros(R, 17, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    need = L.pc_retrieve_topk_grouped_excluding_workspace_bytes(R, T, 16, 0)
    assert need == L.pc_retrieve_topk_grouped_workspace_bytes(R, T, 16, 0) and need > 0
    assert L.pc_retrieve_topk_grouped_excluding_workspace_bytes(R, T, 17, 0) == 0
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")

    def call(n=16, nbytes=need, null=None, n_keys=N_KEYS):
        args = [p(m.dproj), p(m.dtypes), p(m.dkey), R, p(m.rowptr), p(m.col), p(m.table), T, p(m.ex[0]), p(m.ex[1]), n_keys, n,
                m.dim, 0, p(out_i), p(out_s), p(bad), p(ws), nbytes, st]
        if null is not None:
            args[null] = None
        return L.pc_retrieve_topk_grouped_excluding(*args)

    assert call(n=17) == -2 and call(n=0) == -2                # PC_ESHAPE
    assert call(nbytes=need - 1) == -3                         # PC_EWORKSPACE
    for pos in (2, 8, 9, 16):
        assert call(null=pos) == -1, pos                       # PC_EINVAL
    assert call(n_keys=-1) == -1
    rank = torch.full((R,), 12345, dtype=torch.int32, device="cuda")
    rneed = L.pc_rank_grouped_workspace_bytes(R, T, 0)
    rws = torch.empty(rneed, dtype=torch.uint8, device="cuda")

    def rcall(nbytes=rneed, null=None, dim=m.dim):
        args = [p(m.dproj), p(m.dtypes), p(m.dtargets), p(m.dkey), R, p(m.rowptr), p(m.col), p(m.table), T, P, p(m.ex[0]),
                p(m.ex[1]), N_KEYS, p(m.cand_type), dim, 0, p(rank), p(bad), p(rws), nbytes, st]
        if null is not None:
            args[null] = None
        return L.pc_rank_grouped_excluding(*args)

    assert rcall(nbytes=rneed - 1) == -3 and rcall(dim=192) == -2
    for pos in (3, 10, 11, 13, 16, 17):
        assert rcall(null=pos) == -1, pos
    torch.cuda.synchronize()
    assert (out_i == 12345).all() and (rank == 12345).all() and int(bad) == 0      # nothing was launched
    assert rcall() == 0
    assert torch.equal(rank, rank0)


# ---- 6. permuted type_col, repeat runs
def test_same_bits_for_every_candidate_order_and_call(cat):
    m = cat
    idx0, sc0 = filtered(m, 16)
    rank0, _ = ranked(m)
    rowptr = m.rowptr.cpu().numpy()
    col = m.col.cpu().numpy().copy()
    rng = np.random.default_rng(9)
    for t in range(T):
        rng.shuffle(col[rowptr[t]:rowptr[t + 1]])
    for c, s in ((None, 0), (cuda(col), 0), (cuda(col), 7)):
        idx, sc = filtered(m, 16, slices=s, col=c)
        assert torch.equal(idx, idx0) and torch.equal(sc, sc0), s
        assert torch.equal(ranked(m, col=c, slices=s)[0], rank0), s


# ---- 7. exclusion_csr
@pytest.mark.parametrize("include_self", [True, False])
def test_exclusion_csr_against_python_sets(include_self):
    from p_companion_amd import ops
    rows = [[3, 1, 3, 0], [], [2, 2, 2], [9, -1, 4, 3, 6], [5, 0], [4]]       # duplicates, a self-loop, unsorted, empty, out of range
    n_products = 6
    rowptr = cuda(np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32))
    col = cuda(np.array([x for r in rows for x in r], np.int32))
    ex_rowptr, ex_col = ops.exclusion_csr(rowptr, col, include_self=include_self, num_products=n_products)
    assert ex_rowptr.dtype == ex_col.dtype == torch.int32 and ex_rowptr.is_cuda
    rp, cl = ex_rowptr.cpu().tolist(), ex_col.cpu().tolist()
    assert len(rp) == len(rows) + 1 and rp[0] == 0 and rp[-1] == len(cl)
    for k, r in enumerate(rows):
        want = {x for x in r if 0 <= x < n_products} | ({k} if include_self else set())
        assert cl[rp[k]:rp[k + 1]] == sorted(want), k
    # num_products defaults to the number of keys
    d_rowptr, d_col = ops.exclusion_csr(rowptr, col, include_self=include_self)
    assert torch.equal(d_rowptr, ex_rowptr) and torch.equal(d_col, ex_col)
    # no entries at all
    z_rowptr, z_col = ops.exclusion_csr(torch.zeros(4, dtype=torch.int32, device="cuda"),
                                        torch.zeros(0, dtype=torch.int32, device="cuda"), include_self=include_self)
    assert z_rowptr.cpu().tolist() == ([0, 1, 2, 3] if include_self else [0, 0, 0, 0])
    assert z_col.cpu().tolist() == ([0, 1, 2] if include_self else [])


# ---- 8. through PCompanionInference
def _graphs(kind, dim):
    from p_companion_amd.data import DeviceBPG, generate_scaled_bpg
    host = generate_scaled_bpg(20_000, 100, seed=3, dim=dim)
    if kind == "int":
        return host
    g = dict(host.cuda())
    g["comp_pairs"] = cuda(host.complementary_pairs.astype(np.int32))
    g["max_degree"] = int(np.diff(host.cv_rowptr).max())
    return DeviceBPG(g, 100, dim)


@pytest.mark.parametrize("kind,dim", [("int", 128), ("device", 256)])
def test_through_the_inference_object(kind, dim):
    from test_gpu_catalogue_eval import cfg
    from p_companion_amd import ops
    from p_companion_amd.data import ComplementaryIndexDataset
    from p_companion_amd.inference import PCompanionInference
    from p_companion_amd.p_companion import PCompanion
    bpg = _graphs(kind, dim)
    c = cfg(100, dim)
    torch.manual_seed(0)
    table = torch.randn(bpg.num_products, dim, generator=torch.Generator().manual_seed(11))
    inf = PCompanionInference(PCompanion(c, table), c, bpg)
    assert inf.grouped == (kind == "device")
    g = bpg.cuda()
    cv_rowptr, cv_col = g["cv_rowptr"].cpu().numpy(), g["cv_col"].cpu().numpy()
    ds = ComplementaryIndexDataset(bpg, "test", seed=2)
    before = inf.evaluate_catalogue(ds)
    q = torch.arange(0, 20_000, 41, dtype=torch.int32)
    types0, idx0, sc0 = inf.recommend_batch(q, 16)
    all_products = (inf.type_rowptr, inf.type_col)

    # the unfiltered lists of a larger request, from the grouped search (an installed set with no entry): an uploaded IntBPG is
    # otherwise served by the per-row kernel, whose dot product sums in another order
    inf.set_exclusions(torch.zeros(20_001, dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"),
                       include_self=False)
    _, idx0g, sc0g = inf.recommend_batch(q, 16)
    assert torch.equal(idx0g, idx0) and (kind == "int" or torch.equal(sc0g, sc0))
    assert inf.set_exclusions() is inf
    types, idx, sc = inf.recommend_batch(q, 10)
    assert torch.equal(types, types0)
    idx_h, sc_h, idx0_h, sc0_h = idx.cpu().numpy(), sc.cpu().numpy(), idx0g.cpu().numpy(), sc0g.cpu().numpy()
    shown = 0
    for b, query in enumerate(q.tolist()):
        out = set(cv_col[cv_rowptr[query]:cv_rowptr[query + 1]].tolist()) | {query}
        for k in range(idx_h.shape[1]):
            assert not set(idx_h[b, k].tolist()) & out, (query, k)
            kept = [j for j in range(16) if idx0_h[b, k, j] not in out and idx0_h[b, k, j] >= 0]
            if len(kept) >= 10:                                # 16 unfiltered entries suffice to show the 10 filtered ones
                assert (idx_h[b, k] == idx0_h[b, k, kept[:10]]).all() and (sc_h[b, k] == sc0_h[b, k, kept[:10]]).all()
                shown += 1
    assert shown > 0.9 * idx_h.shape[0] * idx_h.shape[1]
    # filtered_targets: the +1 test pairs whose target is co-viewed with its query, counted with torch
    pairs = ds.pairs if torch.is_tensor(ds.pairs) else cuda(ds.pairs)
    pairs = pairs[pairs[:, 2] == 1].long()
    src = torch.repeat_interleave(torch.arange(20_000, device="cuda"), (g["cv_rowptr"][1:] - g["cv_rowptr"][:-1]).long())
    edges = torch.cat([src * 20_000 + g["cv_col"].long(), torch.arange(20_000, device="cuda") * 20_001])
    co = torch.isin(pairs[:, 0] * 20_000 + pairs[:, 1], edges)
    got = inf.evaluate_catalogue(ds)
    assert list(got) == list(before) + ["filtered_targets"] and got["filtered_targets"] == int(co.sum())
    assert got["pairs"] == before["pairs"] and got["type_hit"] == before["type_hit"]
    slot, rank = inf.rank_targets(pairs[:2000, 0].int(), pairs[:2000, 1].int())
    assert (rank[co[:2000]] == -1).all() and torch.equal(rank[~co[:2000]] >= 0, slot[~co[:2000]] >= 0)
    inf.set_exclusions(False)
    assert inf.evaluate_catalogue(ds) == before
    assert all(torch.equal(a, b) for a, b in zip(inf.recommend_batch(q, 16), (types0, idx0, sc0)))

    # set_eligible: a random 70 % of the catalogue
    mask = torch.rand(20_000, generator=torch.Generator().manual_seed(5)).cuda() < 0.7
    for with_lists in (False, True):
        if with_lists:
            inf.set_exclusions(include_self=False)
        assert inf.set_eligible(mask) is inf
        _, idx, _ = inf.recommend_batch(q, 16)
        assert mask[idx[idx >= 0].long()].all()
        slot, rank = inf.rank_targets(pairs[:2000, 0].int(), pairs[:2000, 1].int())
        out = ~mask[pairs[:2000, 1]]
        if with_lists:
            out |= co[:2000]
        assert (rank[out] == -1).all() and int(out.sum()) > 100
        got = inf.evaluate_catalogue(ds)
        full = ~mask[pairs[:, 1]] | (co if with_lists else torch.zeros_like(co))
        assert got["filtered_targets"] == int(full.sum())
        if not with_lists:
            # the ranks are rank_grouped's over the masked CSR
            ids = torch.nonzero(mask).reshape(-1).to(torch.int32)
            rp, local = ops.type_csr(inf.type_idx[ids.long()].contiguous(), 100)
            assert torch.equal(inf.type_rowptr, rp) and torch.equal(inf.type_col, ids[local.long()])
            out_m = inf.model({"query_idx": pairs[:2000, 0].int(), "query_types": inf.type_idx[pairs[:2000, 0]]})
            sel = (slot >= 0) & ~out
            proj = out_m["projected_embeddings"][torch.arange(2000, device="cuda"), slot.long().clamp(min=0)].contiguous()
            want, _ = ops.rank_grouped(proj[sel].contiguous(), inf.type_idx[pairs[:2000, 1]][sel].contiguous(),
                                       pairs[:2000, 1][sel].int().contiguous(), inf.type_rowptr, inf.type_col, inf.features)
            assert torch.equal(rank[sel], want) and int(sel.sum()) > 20
        inf.set_eligible(None)
        assert inf.type_rowptr is all_products[0] and inf.type_col is all_products[1] and inf.cand_type is inf.type_idx
    inf.set_exclusions(False)
    assert inf.evaluate_catalogue(ds) == before
