"""Type-filtered lists from a bf16 copy of the catalogue (pc_retrieve_topk_grouped_bf16, ops.catalogue_bf16,
ops.retrieve_topk_grouped on a bf16 table, PCompanionInference(catalogue=)).

The stored table is scored against the unrounded query, split into three bf16 pieces whose products with a bf16 row are exact,
so the oracle is the float64 computation of tests/test_gpu_retrieval_grouped.py over the ROUNDED table at that file's own
tolerance (TOL = 1e-5), and on data whose partial sums are exact in fp32 the scores are the reference's bits.  Needs an MI355X."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import joint_oracle
from test_gpu_retrieval_grouped import (TOL, cfg, check_rows, grouped_reference, host_csr, mixed_catalogue, mixed_rows)

assert TOL == 1e-5


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def upload_bf16(type_idx, features, T):
    """(rowptr, col, bf16 table) on the device and the rounded table as float32 on the host: ops.catalogue_bf16 is
    round-to-nearest-even, which is what torch does on the host too."""
    from p_companion_amd import ops
    rowptr, col = host_csr(type_idx, T)
    table = ops.catalogue_bf16(cuda(features))
    assert table.dtype == torch.bfloat16 and table.shape == features.shape and table.is_contiguous()
    rounded = table.float().cpu().numpy()
    assert np.array_equal(rounded, torch.from_numpy(features).to(torch.bfloat16).float().numpy())
    return cuda(rowptr), cuda(col), table, rounded


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.fixture(scope="module", params=[128, 256], ids=lambda d: f"D{d}")
def mixed(request):
    dim = request.param
    P, R = 40_000, 203                                        # 203 rows: not a multiple of a 32- or 64-row tile
    type_idx, features, T = mixed_catalogue(P, dim, seed=dim)
    assert (type_idx == 0).sum() > P // 2 > 4 * 4096          # the heavy type: several slices
    assert [(type_idx == t).sum() for t in (1, 2, 3, 4, 5)] == [0, 0, 3, 3, 30]
    types = mixed_rows(R, T, seed=dim)
    proj = np.random.default_rng(7).standard_normal((R, dim)).astype(np.float32)
    rowptr, col, table, rounded = upload_bf16(type_idx, features, T)
    ref16 = grouped_reference(proj, types, type_idx, rounded, 16)
    return SimpleNamespace(dim=dim, type_idx=type_idx, rounded=rounded, T=T, types=types, proj=proj, ref16=ref16,
                           rowptr=rowptr, col=col, table=table, dproj=cuda(proj), dtypes=cuda(types))


# ---- 1. oracle parity: float64 over the rounded table
@pytest.mark.parametrize("n", [1, 10, 16])
def test_oracle_parity_mixed_catalogue(mixed, n):
    from p_companion_amd import ops
    m = mixed
    idx, sc = ops.retrieve_topk_grouped(m.dproj, m.dtypes, m.rowptr, m.col, m.table, n)
    assert idx.dtype == torch.int32 and sc.dtype == torch.float32
    ref = [(i[:n], s[:n]) for i, s in m.ref16]
    check_rows(idx.cpu().numpy(), sc.cpu().numpy(), ref, m.proj, m.rounded, m.type_idx, m.types, n)
    got = idx.cpu().numpy()
    assert (got[:4] == -1).all()                              # types -1 / n_types / the two empty types
    assert (got[4:6, :min(n, 3)] >= 0).all() and (got[4:6, 3:] == -1).all()


@pytest.mark.parametrize("dim", [128, 256])
@pytest.mark.parametrize("n", [1, 10, 16])
def test_oracle_parity_uniform_types(dim, n):
    from p_companion_amd import ops
    P, T, R = 20_000, 50, 333
    rng = np.random.default_rng(dim + n)
    type_idx = rng.integers(0, T, P).astype(np.int32)
    features = rng.standard_normal((P, dim)).astype(np.float32)
    types = rng.integers(0, T, R).astype(np.int32)
    proj = rng.standard_normal((R, dim)).astype(np.float32)
    rowptr, col, table, rounded = upload_bf16(type_idx, features, T)
    idx, sc = ops.retrieve_topk_grouped(cuda(proj), cuda(types), rowptr, col, table, n)
    ref = joint_oracle.recommend(proj, types, type_idx, rounded, n)
    check_rows(idx.cpu().numpy(), sc.cpu().numpy(), ref, proj, rounded, type_idx, types, n)


def test_one_row_per_type_and_a_single_product_catalogue():
    from p_companion_amd import ops
    P, T, R, n = 30_000, 3_000, 1_000, 10
    rng = np.random.default_rng(11)
    type_idx = rng.integers(0, T, P).astype(np.int32)
    features = rng.standard_normal((P, 128)).astype(np.float32)
    types = rng.permutation(T)[:R].astype(np.int32)
    proj = rng.standard_normal((R, 128)).astype(np.float32)
    rowptr, col, table, rounded = upload_bf16(type_idx, features, T)
    idx, sc = ops.retrieve_topk_grouped(cuda(proj), cuda(types), rowptr, col, table, n)
    ref = joint_oracle.recommend(proj, types, type_idx, rounded, n)
    check_rows(idx.cpu().numpy(), sc.cpu().numpy(), ref, proj, rounded, type_idx, types, n)
    one = torch.zeros(1, 128, device="cuda")
    one[0, 0] = 2.0
    idx, sc = ops.retrieve_topk_grouped(one, torch.zeros(1, dtype=torch.int32, device="cuda"),
                                        torch.tensor([0, 1], dtype=torch.int32, device="cuda"),
                                        torch.zeros(1, dtype=torch.int32, device="cuda"), ops.catalogue_bf16(one), 3)
    assert idx.cpu().tolist() == [[0, -1, -1]] and sc[0, 0].item() == 4.0 and torch.isneginf(sc[0, 1:]).all()


# ---- 2. exactness, and that all three pieces are used
def exact_case(seed):
    """D = 128, n = 4, 300 products over 5 types of which type 3 has none; 70 rows of which 65 are of type 0 (two 64-row tiles),
    one of type -1 and one of type 5 (out of range)."""
    D, n, P, T, R = 128, 4, 300, 5, 70
    rng = np.random.default_rng(seed)
    type_idx = rng.choice(np.array([0, 1, 2, 4], np.int32), P)
    types = np.zeros(R, np.int32)
    types[5], types[40], types[67:] = -1, 5, [1, 3, 4]
    assert (types == 0).sum() == 65 and (type_idx == 3).sum() == 0
    return SimpleNamespace(D=D, n=n, P=P, T=T, R=R, rng=rng, type_idx=type_idx, types=types)


def assert_equals_reference(c, idx, sc, proj, features):
    """Every row EQUALS grouped_reference: indices equal, scores the same bits (the float64 scores are fp32 numbers)."""
    idx, sc = idx.cpu().numpy(), sc.cpu().numpy()
    for r in (5, 40):
        assert (idx[r] == -1).all() and np.isneginf(sc[r]).all(), r
    for r, (rid, rsc) in enumerate(grouped_reference(proj, c.types, c.type_idx, features, c.n)):
        want_idx, want_sc = np.full(c.n, -1, np.int64), np.full(c.n, -np.inf, np.float32)
        want_idx[:len(rid)], want_sc[:len(rid)] = rid, rsc.astype(np.float32)
        assert (rsc.astype(np.float32).astype(np.float64) == rsc).all()           # the reference survives the round trip
        assert (idx[r] == want_idx).all() and (sc[r].view(np.int32) == want_sc.view(np.int32)).all(), r


@pytest.fixture(scope="module")
def integers():
    """Small-integer features and queries in [-3, 3]: every score exact in bf16 x bf16, fp32 and fp64 alike."""
    c = exact_case(21)
    c.features = c.rng.integers(-3, 4, (c.P, c.D)).astype(np.float32)
    c.proj = c.rng.integers(-3, 4, (c.R, c.D)).astype(np.float32)
    c.rowptr, c.col, c.table, rounded = upload_bf16(c.type_idx, c.features, c.T)
    assert np.array_equal(rounded, c.features)
    c.dproj, c.dtypes = cuda(c.proj), cuda(c.types)
    return c


def test_small_integers_equal_the_reference_and_the_fp32_entry_bit_for_bit(integers):
    from p_companion_amd import ops
    c = integers
    idx, sc = ops.retrieve_topk_grouped(c.dproj, c.dtypes, c.rowptr, c.col, c.table, c.n)
    assert_equals_reference(c, idx, sc, c.proj, c.features)
    idx32, sc32 = ops.retrieve_topk_grouped(c.dproj, c.dtypes, c.rowptr, c.col, c.table.float(), c.n)
    assert torch.equal(idx, idx32) and same_bits(sc, sc32)


def test_all_three_pieces_of_the_query_are_used():
    """Table values in {-1, 0, 1} with exactly 32 non-zeros per row, queries a + b 2^-9 + c 2^-18 with a, b, c in {-1, 0, 1}:
    a query element needs all three truncation pieces (1 - 2^-9 + 2^-18 has set bits 2^-1 .. 2^-9 and 2^-18), every partial
    sum is a multiple of 2^-18 below 2^6 -- exact in fp32 in any order -- so the scores are the float64 reference's bits.  A
    kernel that drops the second or the third piece fails."""
    from p_companion_amd import ops
    c = exact_case(22)
    features = np.zeros((c.P, c.D), np.float32)
    for p in range(c.P):
        features[p, c.rng.choice(c.D, 32, replace=False)] = c.rng.choice(np.array([-1.0, 1.0], np.float32), 32)
    assert ((features != 0).sum(1) == 32).all()
    a, b, cc = (c.rng.integers(-1, 2, (c.R, c.D)).astype(np.float64) for _ in range(3))
    q64 = a + b * 2.0 ** -9 + cc * 2.0 ** -18
    proj = q64.astype(np.float32)
    assert (proj.astype(np.float64) == q64).all()
    # the pieces: two of them do not hold the queries
    top = lambda x: (x.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
    p0 = top(proj)
    p1 = top(proj - p0)
    assert (proj - p0 - p1 != 0).mean() > 0.2 and (p0 + p1 + top(proj - p0 - p1) == proj).all()
    rowptr, col, table, rounded = upload_bf16(c.type_idx, features, c.T)
    assert np.array_equal(rounded, features)
    idx, sc = ops.retrieve_topk_grouped(cuda(proj), cuda(c.types), rowptr, col, table, c.n)
    assert_equals_reference(c, idx, sc, proj, features)
    # (what a two-piece kernel would return differs from the reference on this data)
    two = grouped_reference((p0 + p1).astype(np.float32), c.types, c.type_idx, features, c.n)
    full = grouped_reference(proj, c.types, c.type_idx, features, c.n)
    assert sum((x[1] != y[1]).any() for x, y in zip(two, full) if len(x[1])) > 30


# ---- 3. determinism
def test_bitwise_run_to_run_across_slices_and_candidate_order(mixed):
    from p_companion_amd import ops
    m = mixed
    run = lambda col, s: ops.retrieve_topk_grouped(m.dproj, m.dtypes, m.rowptr, col, m.table, 16, slices=s)
    i0, s0 = run(m.col, 0)
    i1, s1 = run(m.col, 0)
    assert torch.equal(i0, i1) and same_bits(s0, s1)
    for s in (1, 7, 64):
        i, sc = run(m.col, s)
        assert torch.equal(i, i0) and same_bits(sc, s0), s
    rowptr = m.rowptr.cpu().numpy()
    col = m.col.cpu().numpy().copy()
    rng = np.random.default_rng(5)
    for t in range(m.T):                                      # type_col permuted inside every type's segment
        seg = col[rowptr[t]:rowptr[t + 1]]
        rng.shuffle(seg)
    assert (col != m.col.cpu().numpy()).sum() > 1000
    i, sc = run(cuda(col), 0)
    assert torch.equal(i, i0) and same_bits(sc, s0)


# ---- 4. exclusions
def test_exclusions_equal_the_fp32_entry_on_the_widened_table_bit_for_bit(integers):
    """The integer catalogue: both entries form exact scores, so with the same lists they must agree in every bit.  Row key =
    the row's query product; the lists are a small co-view CSR through ops.exclusion_csr with the query itself."""
    from p_companion_amd import ops
    c = integers
    rng = np.random.default_rng(31)
    key = rng.integers(0, c.P, c.R).astype(np.int32)
    key[3], key[9] = -1, -1                                   # rows without a list
    deg = rng.integers(0, 40, c.P)
    cv_rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int32)
    cv_col = rng.integers(0, c.P, int(deg.sum())).astype(np.int32)
    ex = ops.exclusion_csr(cuda(cv_rowptr), cuda(cv_col), include_self=True, num_products=c.P)
    exclude = (cuda(key),) + ex
    for n in (c.n, 16):
        bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        idx, sc = ops.retrieve_topk_grouped(c.dproj, c.dtypes, c.rowptr, c.col, c.table, n, exclude=exclude, bad=bad)
        want_i, want_s = ops.retrieve_topk_grouped(c.dproj, c.dtypes, c.rowptr, c.col, c.table.float(), n, exclude=exclude)
        assert torch.equal(idx, want_i) and same_bits(sc, want_s) and int(bad) == 0
    plain, _ = ops.retrieve_topk_grouped(c.dproj, c.dtypes, c.rowptr, c.col, c.table, 16)
    assert (idx != plain).any(1).sum() >= 10                  # the filter bit
    ex_rowptr, ex_col = ex[0].cpu().numpy(), ex[1].cpu().numpy()
    got = idx.cpu().numpy()
    for r in range(c.R):
        if key[r] >= 0:
            assert not set(got[r].tolist()) & set(ex_col[ex_rowptr[key[r]]:ex_rowptr[key[r] + 1]].tolist()), r


@pytest.fixture(scope="module", params=[128, 256], ids=lambda d: f"D{d}")
def listed(request):
    """Random data with lists that hold the heads of the rows' unfiltered lists; the float64 reference with the excluded
    products removed from the catalogue of each key's rows."""
    dim = request.param
    P, T, R, K = 12_000, 20, 150, 16
    rng = np.random.default_rng(40 + dim)
    type_idx = rng.integers(0, T, P).astype(np.int32)
    type_idx[:9000][rng.random(9000) < 0.8] = 0               # one type of about 7 000: two slices
    features = rng.standard_normal((P, dim)).astype(np.float32)
    types = rng.integers(0, T, R).astype(np.int32)
    types[:70] = 0
    proj = rng.standard_normal((R, dim)).astype(np.float32)
    key = (np.arange(R) % (K + 1) - 1).astype(np.int32)       # -1, 0 .. K - 1
    rowptr, col, table, rounded = upload_bf16(type_idx, features, T)
    free = grouped_reference(proj, types, type_idx, rounded, 16)
    lists = []
    for k in range(K):
        heads = [int(x) for r in np.nonzero(key == k)[0] for x in free[r][0][:1 + k % 5]]
        lists.append(sorted(set(heads) | set(rng.choice(P, 3 * k, replace=False).tolist())))
    ref = [None] * R
    for k in range(-1, K):
        rows = np.nonzero(key == k)[0]
        reduced = type_idx.copy()
        if k >= 0:
            reduced[lists[k]] = T                             # (a type no row asks for)
        for r, x in zip(rows, grouped_reference(proj[rows], types[rows], reduced, rounded, 16)):
            ref[r] = x
    ex_rowptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
    ex_col = np.concatenate([np.asarray(x, np.int32) for x in lists]).astype(np.int32)
    return SimpleNamespace(dim=dim, P=P, T=T, R=R, K=K, type_idx=type_idx, rounded=rounded, types=types, proj=proj, key=key,
                           lists=lists, ref=ref, free=free, rowptr=rowptr, col=col, table=table, dproj=cuda(proj),
                           dtypes=cuda(types), ex=(cuda(ex_rowptr), cuda(ex_col)))


@pytest.mark.parametrize("n", [1, 10, 16])
def test_exclusions_against_the_float64_reference(listed, n):
    from p_companion_amd import ops
    m = listed
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    idx, sc = ops.retrieve_topk_grouped(m.dproj, m.dtypes, m.rowptr, m.col, m.table, n, exclude=(cuda(m.key),) + m.ex, bad=bad)
    ref = [(i[:n], s[:n]) for i, s in m.ref]
    check_rows(idx.cpu().numpy(), sc.cpu().numpy(), ref, m.proj, m.rounded, m.type_idx, m.types, n)
    got = idx.cpu().numpy()
    changed = 0
    for r in range(m.R):
        if m.key[r] >= 0:
            assert not set(got[r].tolist()) & set(m.lists[m.key[r]]), r
            changed += int(m.free[r][0][0] != got[r][0])
    assert changed >= 100 and int(bad) == 0                   # every listed row lost its head


def test_a_key_out_of_range_is_served_without_a_list_and_counted(listed):
    from p_companion_amd import ops
    m = listed
    key = m.key.copy()
    wild = np.arange(0, m.R, 7)
    key[wild] = np.where(np.arange(len(wild)) % 2 == 0, m.K, -2)
    key[wild[-1]] = 2 ** 31 - 1
    want_key = key.copy()
    want_key[wild] = -1
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    idx, sc = ops.retrieve_topk_grouped(m.dproj, m.dtypes, m.rowptr, m.col, m.table, 16, exclude=(cuda(key),) + m.ex, bad=bad)
    want_i, want_s = ops.retrieve_topk_grouped(m.dproj, m.dtypes, m.rowptr, m.col, m.table, 16, exclude=(cuda(want_key),) + m.ex)
    assert torch.equal(idx, want_i) and same_bits(sc, want_s)
    assert int(bad) == len(wild)
    ops.retrieve_topk_grouped(m.dproj, m.dtypes, m.rowptr, m.col, m.table, 16, exclude=(cuda(key),) + m.ex, bad=bad)
    assert int(bad) == 2 * len(wild)                          # added to
    # no list at all: the unfiltered call
    none = torch.full((m.R,), -1, dtype=torch.int32, device="cuda")
    a = ops.retrieve_topk_grouped(m.dproj, m.dtypes, m.rowptr, m.col, m.table, 16, exclude=(none,) + m.ex)
    b = ops.retrieve_topk_grouped(m.dproj, m.dtypes, m.rowptr, m.col, m.table, 16)
    assert torch.equal(a[0], b[0]) and same_bits(a[1], b[1])


# ---- 5. errors through ctypes
def test_error_codes():
    from p_companion_amd import _lib
    L = _lib.lib()
    R, T = 4, 2
    dev = "cuda"
    proj = torch.zeros(R, 256, device=dev)
    types = torch.zeros(R, dtype=torch.int32, device=dev)
    rowptr = torch.tensor([0, 2, 4], dtype=torch.int32, device=dev)
    col = torch.arange(4, dtype=torch.int32, device=dev)
    table = torch.zeros(5, 256, dtype=torch.bfloat16, device=dev)
    key = torch.zeros(R, dtype=torch.int32, device=dev)
    ex_rowptr = torch.tensor([0, 1], dtype=torch.int32, device=dev)
    ex_col = torch.zeros(1, dtype=torch.int32, device=dev)
    bad_count = torch.zeros(1, dtype=torch.int32, device=dev)
    oi = torch.empty(R, 16, dtype=torch.int32, device=dev)
    os_ = torch.empty(R, 16, device=dev)
    need = L.pc_retrieve_topk_grouped_bf16_workspace_bytes(R, T, 16, 64)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert table.data_ptr() % 16 == 0

    def call(n=10, dim=128, slices=0, nbytes=need, null=None, rows=R, lists=True, tab=None, n_keys=1):
        args = [p(proj), p(types), p(key) if lists else None, rows, p(rowptr), p(col), p(table) if tab is None else tab, T,
                p(ex_rowptr) if lists else None, p(ex_col) if lists else None, n_keys if lists else 0, n, dim, slices, p(oi),
                p(os_), p(bad_count) if lists else None, p(ws), nbytes, st]
        if null is not None:
            args[null] = None
        return L.pc_retrieve_topk_grouped_bf16(*args)

    for lists in (True, False):
        assert call(lists=lists) == 0 and call(dim=256, n=16, slices=64, lists=lists) == 0
        torch.cuda.synchronize()
        for bad in ({"n": 0}, {"n": 17}, {"dim": 192}, {"slices": -1}, {"slices": 65}):
            assert call(lists=lists, **bad) == -2, bad                                         # PC_ESHAPE
        for off in (2, 8):                                                                     # a misaligned table pointer
            assert call(lists=lists, tab=ctypes.c_void_p(table.data_ptr() + off)) == -2, off
        for pos in (0, 1, 4, 5, 6, 14, 15, 17):
            assert call(null=pos, lists=lists) == -1, pos                                      # PC_EINVAL
        assert call(rows=0, lists=lists) == -1
        assert call(nbytes=L.pc_retrieve_topk_grouped_bf16_workspace_bytes(R, T, 10, 0) - 1, lists=lists) == -3
    for pos in (2, 8, 9, 16):                                                                  # the lists: all or none
        assert call(null=pos) == -1, pos
    assert call(n_keys=-1) == -1
    assert L.pc_retrieve_topk_grouped_bf16_workspace_bytes(R, T, 17, 0) == 0
    torch.cuda.synchronize()


# ---- 6. PCompanionInference
def test_inference_serves_from_a_bf16_catalogue():
    from p_companion_amd import ops
    from p_companion_amd.data import DeviceBPG, generate_device_bpg
    from p_companion_amd.inference import PCompanionInference
    from p_companion_amd.p_companion import PCompanion
    dbpg = generate_device_bpg(200_000, 100, seed=6, world=1)
    c = cfg(NUM_TYPES=dbpg.n_types)
    torch.manual_seed(4)
    g = dbpg.cuda()
    model = PCompanion(c, g["features"])
    fp32 = PCompanionInference(model, c, dbpg)
    bf16 = PCompanionInference(model, c, dbpg, catalogue=torch.bfloat16)
    assert fp32.catalogue is None and bf16.features is None and bf16.catalogue.dtype == torch.bfloat16
    assert torch.equal(bf16.catalogue, ops.catalogue_bf16(g["features"]))
    q = torch.from_numpy(np.random.default_rng(8).choice(dbpg.num_products, 512, replace=False).astype(np.int32))
    n = 10
    t_f, i_f, s_f = fp32.recommend_batch(q, n)
    t_b, i_b, s_b = bf16.recommend_batch(q, n)
    assert torch.equal(t_b, t_f) and i_b.shape == i_f.shape == (512, 3, n)
    # the float64 reference over the rounded table
    out = fp32.model({"query_idx": q.cuda(), "query_types": fp32.type_idx[q.long().cuda()]})
    dproj = out["projected_embeddings"].contiguous().reshape(-1, 128)
    row_types = t_f.reshape(-1).to(torch.int32).contiguous()
    proj, types = dproj.cpu().numpy(), row_types.cpu().numpy()
    rounded, type_idx = bf16.catalogue.float().cpu().numpy(), g["type_idx"].cpu().numpy()
    ref = grouped_reference(proj, types, type_idx, rounded, n)
    check_rows(i_b.reshape(-1, n).cpu().numpy(), s_b.reshape(-1, n).cpu().numpy(), ref, proj, rounded, type_idx, types, n)
    # catalogue=None: the direct call with the fp32 table, bit for bit
    want_i, want_s = ops.retrieve_topk_grouped(dproj, row_types, fp32.type_rowptr, fp32.type_col, g["features"], n)
    assert torch.equal(i_f.reshape(-1, n), want_i) and same_bits(s_f.reshape(-1, n), want_s)

    # a given bf16 tensor over a graph without features: identical bits
    no_feat = DeviceBPG({k: v for k, v in dbpg.arrays.items() if k != "features"}, dbpg.n_types, dbpg.dim)
    with pytest.raises(ValueError, match="without features"):
        PCompanionInference(model, c, no_feat, catalogue=torch.bfloat16)
    given = PCompanionInference(model, c, no_feat, catalogue=bf16.catalogue.clone())
    t_g, i_g, s_g = given.recommend_batch(q, n)
    assert torch.equal(t_g, t_b) and torch.equal(i_g, i_b) and same_bits(s_g, s_b)
    rec_b, rec_g = bf16.recommend("P000007", 5), given.recommend(7, 5)
    assert rec_b["complementary_types"] == rec_g["complementary_types"] and len(rec_b["recommendations"]) >= 1
    assert rec_b["recommendations"] == rec_g["recommendations"]
    assert all(len(x) == 5 for x in rec_b["recommendations"])

    # exclusions: no served product is in its query's list; eligibility: only eligible products are served
    given.set_exclusions()
    _, i_x, _ = given.recommend_batch(q, n)
    ex_rowptr, ex_col = (x.cpu().numpy() for x in given.exclusions)
    got, qs = i_x.cpu().numpy(), q.numpy()
    for b in range(len(qs)):
        mine = set(ex_col[ex_rowptr[qs[b]]:ex_rowptr[qs[b] + 1]].tolist())
        assert qs[b] in mine and not mine & set(got[b].reshape(-1).tolist()), b
    # a set that names what was served first: every slot's head of every query (include_self=False: nothing else)
    heads = i_b[:, :, 0].cpu().numpy()
    order = np.argsort(qs)
    counts = np.zeros(dbpg.num_products, np.int64)
    counts[qs] = heads.shape[1]
    given.set_exclusions(cuda(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)),
                         cuda(heads[order].reshape(-1).astype(np.int32)), include_self=False)
    _, i_h, _ = given.recommend_batch(q, n)
    i_h = i_h.cpu().numpy()
    for b in range(len(qs)):
        assert not set(heads[b].tolist()) & set(i_h[b].reshape(-1).tolist()), b
    assert (i_h[:, :, 0] == i_b[:, :, 1].cpu().numpy()).all()                  # the second of each list moved up
    given.set_exclusions(False)
    mask = torch.rand(dbpg.num_products, device="cuda") < 0.5
    _, i_e, _ = given.set_eligible(mask).recommend_batch(q, n)
    assert (i_e >= 0).all() and mask[i_e.reshape(-1).long()].all()
    given.set_eligible(None)
    assert torch.equal(given.recommend_batch(q, n)[1], i_b)

    # what a bf16 catalogue does not serve names the fp32 catalogue
    for inf in (bf16, given):
        with pytest.raises(ValueError, match="fp32 catalogue"):
            inf.recommend_batch(q, 17)
        with pytest.raises(ValueError, match="fp32 catalogue"):
            inf.rank_targets(q, q)
        with pytest.raises(ValueError, match="fp32 catalogue"):
            inf.evaluate_catalogue(None)
    assert bf16.recommend_batch(q, 16)[1].shape == (512, 3, 16)
