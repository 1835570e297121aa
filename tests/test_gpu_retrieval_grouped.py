"""Type-filtered retrieval grouped by type (pc_retrieve_topk_grouped, ops.type_csr) and PCompanionInference over a
DeviceBPG.  The checker is oracle/joint_oracle.recommend (float64 numpy); for the larger catalogues the same computation
grouped by type (one float64 matmul per type, a stable sort) stands in for it on every row and the oracle itself is run on
a subset of rows.  Needs an MI355X."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import joint_oracle

TOL = 1e-5


def cfg(**over):
    c = SimpleNamespace(PRODUCT_EMB_DIM=128, TYPE_EMB_DIM=64, HIDDEN_SIZE=256, NUM_ATTENTION_HEADS=4, DROPOUT=0.0,
                        MARGIN=1.0, ALPHA=0.8, NUM_COMP_TYPES=3, NUM_TYPES=100, DEVICE=torch.device("cuda"))
    c.__dict__.update(over)
    return c


def host_csr(type_idx, n_types):
    """inference.py's host construction (the IntBPG path)."""
    order = np.argsort(type_idx, kind="stable").astype(np.int32)
    counts = np.bincount(type_idx, minlength=n_types)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), order


def grouped_reference(proj, types, type_idx, features, n):
    """joint_oracle.recommend computed one type at a time: [(ids, float64 scores)] per row."""
    out = [None] * len(types)
    f = torch.from_numpy(features)
    p = torch.from_numpy(proj).double()
    for t in np.unique(types):
        rows = np.nonzero(types == t)[0]
        cand = np.nonzero(type_idx == t)[0]
        if cand.size == 0:
            for r in rows:
                out[r] = (np.zeros(0, np.int64), np.zeros(0))
            continue
        sims = (f[torch.from_numpy(cand)].double() @ p[torch.from_numpy(rows)].T).numpy()      # [cand, rows]
        k = min(n, cand.size)
        for j, r in enumerate(rows):
            top = np.argsort(-sims[:, j], kind="stable")[:k]
            out[r] = (cand[top], sims[top, j])
    return out


def check_rows(idx, sc, ref, proj, features, type_idx, types, n):
    """Scores within 1e-5 (rtol and atol) of the reference; indices equal, or differing only where the returned product's
    own float64 score equals the reference score of that rank within the tolerance; products distinct and of the row's
    type; exactly equal scores in ascending product order; missing slots -1 / -inf."""
    for r, (rid, rsc) in enumerate(ref):
        k = len(rid)
        assert (idx[r, k:] == -1).all() and np.isneginf(sc[r, k:]).all(), r
        np.testing.assert_allclose(sc[r, :k], rsc, rtol=TOL, atol=TOL, err_msg=f"row {r}")
        got = idx[r, :k]
        assert (got >= 0).all() and len(set(got.tolist())) == k, r
        assert (type_idx[got] == types[r]).all(), r
        diff = got != rid
        if diff.any():
            own = features[got[diff]].astype(np.float64) @ proj[r].astype(np.float64)
            np.testing.assert_allclose(own, rsc[diff], rtol=TOL, atol=TOL, err_msg=f"row {r}: index mismatch")
        if k > 1:
            tie = sc[r, 1:k] == sc[r, :k - 1]
            assert (got[1:][tie] > got[:-1][tie]).all(), f"row {r}: equal scores not in ascending product order"


def mixed_catalogue(P, dim, seed):
    """40 types: type 0 holds over half of the products (a type that splits into many slices), types 1 and 2 are empty,
    types 3 and 4 hold 3 products each (fewer than n), type 5 holds 30 products whose features are copies of 3 rows
    (exactly tied scores), the rest share the remainder uniformly."""
    T = 40
    rng = np.random.default_rng(seed)
    type_idx = rng.integers(6, T, P).astype(np.int32)
    type_idx[rng.random(P) < 0.55] = 0
    type_idx[np.isin(type_idx, (1, 2))] = 0
    free = np.nonzero(type_idx != 0)[0]
    pick = rng.choice(free, 36, replace=False)
    type_idx[pick[:3]], type_idx[pick[3:6]], type_idx[pick[6:36]] = 3, 4, 5
    features = rng.standard_normal((P, dim)).astype(np.float32)
    dup = np.sort(pick[6:36])
    features[dup] = features[dup[:3]][np.arange(30) % 3]
    return type_idx, features, T


def mixed_rows(R, T, seed, heavy_share=0.35):
    rng = np.random.default_rng(seed + 1)
    types = rng.integers(0, T, R).astype(np.int32)
    types[rng.random(R) < heavy_share] = 0
    types[:8] = [-1, T, 1, 2, 3, 4, 5, 5]
    return types


def upload(type_idx, features, T):
    rowptr, col = host_csr(type_idx, T)
    return (torch.from_numpy(rowptr).cuda(), torch.from_numpy(col).cuda(), torch.from_numpy(features).cuda())


@pytest.fixture(scope="module", params=[128, 256])
def mixed(request):
    dim = request.param
    P, R = 300_000, 203                                       # 203 rows: not a multiple of a 32- or 64-row tile
    type_idx, features, T = mixed_catalogue(P, dim, seed=dim)
    assert (type_idx == 0).sum() > P // 2
    types = mixed_rows(R, T, seed=dim)
    proj = np.random.default_rng(7).standard_normal((R, dim)).astype(np.float32)
    ref16 = grouped_reference(proj, types, type_idx, features, 16)
    # the stand-in against the oracle itself on a subset: the special rows and a few heavy-type rows
    sub = np.concatenate([np.arange(8), np.nonzero(types == 0)[0][:4], np.nonzero(types > 5)[0][:4]])
    # (float64 BLAS does not give bit-equal scores to duplicated rows, so the two may order an exact tie differently)
    for r, (oid, osc) in zip(sub, joint_oracle.recommend(proj[sub], types[sub], type_idx, features, 16)):
        rid, rsc = ref16[r]
        assert len(rid) == len(oid) and np.allclose(rsc, osc, rtol=1e-6, atol=1e-6)
        diff = rid != oid
        own = features[rid[diff]].astype(np.float64) @ proj[r].astype(np.float64)
        assert np.allclose(own, osc[diff], rtol=1e-6, atol=1e-6)
    rowptr, col, table = upload(type_idx, features, T)
    return SimpleNamespace(dim=dim, type_idx=type_idx, features=features, T=T, types=types, proj=proj, ref16=ref16,
                           rowptr=rowptr, col=col, table=table, dproj=torch.from_numpy(proj).cuda(),
                           dtypes=torch.from_numpy(types).cuda())


# ---- 1. oracle parity on hand-made catalogues
@pytest.mark.parametrize("n", [1, 10, 16])
def test_oracle_parity_mixed_catalogue(mixed, n):
    from p_companion_amd import ops
    m = mixed
    idx, sc = ops.retrieve_topk_grouped(m.dproj, m.dtypes, m.rowptr, m.col, m.table, n)
    ref = [(i[:n], s[:n]) for i, s in m.ref16]
    check_rows(idx.cpu().numpy(), sc.cpu().numpy(), ref, m.proj, m.features, m.type_idx, m.types, n)
    # the special rows: types -1 / n_types / empty give nothing, short types give what they have
    got = idx.cpu().numpy()
    assert (got[:4] == -1).all()
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
    rowptr, col, table = upload(type_idx, features, T)
    idx, sc = ops.retrieve_topk_grouped(torch.from_numpy(proj).cuda(), torch.from_numpy(types).cuda(), rowptr, col, table, n)
    ref = joint_oracle.recommend(proj, types, type_idx, features, n)
    check_rows(idx.cpu().numpy(), sc.cpu().numpy(), ref, proj, features, type_idx, types, n)


def test_one_row_per_type_and_a_single_product_catalogue():
    """Many types with about one row each (the 10 M / 34 800-type regime in miniature), and the smallest catalogue."""
    from p_companion_amd import ops
    P, T, R, n = 30_000, 3_000, 1_000, 10
    rng = np.random.default_rng(11)
    type_idx = rng.integers(0, T, P).astype(np.int32)
    features = rng.standard_normal((P, 128)).astype(np.float32)
    types = rng.permutation(T)[:R].astype(np.int32)
    proj = rng.standard_normal((R, 128)).astype(np.float32)
    rowptr, col, table = upload(type_idx, features, T)
    idx, sc = ops.retrieve_topk_grouped(torch.from_numpy(proj).cuda(), torch.from_numpy(types).cuda(), rowptr, col, table, n)
    ref = joint_oracle.recommend(proj, types, type_idx, features, n)
    check_rows(idx.cpu().numpy(), sc.cpu().numpy(), ref, proj, features, type_idx, types, n)
    one = torch.zeros(1, 128, device="cuda")
    one[0, 0] = 2.0
    idx, sc = ops.retrieve_topk_grouped(one, torch.zeros(1, dtype=torch.int32, device="cuda"),
                                        torch.tensor([0, 1], dtype=torch.int32, device="cuda"),
                                        torch.zeros(1, dtype=torch.int32, device="cuda"), one.clone(), 3)
    assert idx.cpu().tolist() == [[0, -1, -1]] and sc[0, 0].item() == 4.0 and torch.isneginf(sc[0, 1:]).all()


def test_rows_without_a_valid_type_beside_a_two_tile_type_exact():
    """The planning pass on the retrieval side: D = 128, n = 4, 300 products over 5 types of which type 3 has none, 70 rows of
    which 65 are of type 0 (two 64-row tiles), one of type -1 and one of type 5 (out of range).  Small-integer features and
    queries make every score exact in fp32 and fp64 alike, so the two invalid rows give -1 / -inf in every slot and every
    other row EQUALS grouped_reference: indices equal, scores the same bits."""
    from p_companion_amd import ops
    D, n, P, T, R = 128, 4, 300, 5, 70
    rng = np.random.default_rng(21)
    type_idx = rng.choice(np.array([0, 1, 2, 4], np.int32), P)
    features = rng.integers(-3, 4, (P, D)).astype(np.float32)
    proj = rng.integers(-3, 4, (R, D)).astype(np.float32)
    types = np.zeros(R, np.int32)
    types[5], types[40], types[67:] = -1, 5, [1, 3, 4]
    assert (types == 0).sum() == 65 and (type_idx == 3).sum() == 0
    rowptr, col, table = upload(type_idx, features, T)
    idx, sc = ops.retrieve_topk_grouped(torch.from_numpy(proj).cuda(), torch.from_numpy(types).cuda(), rowptr, col, table, n)
    idx, sc = idx.cpu().numpy(), sc.cpu().numpy()
    for r in (5, 40):
        assert (idx[r] == -1).all() and np.isneginf(sc[r]).all(), r
    for r, (rid, rsc) in enumerate(grouped_reference(proj, types, type_idx, features, n)):
        want_idx, want_sc = np.full(n, -1, np.int64), np.full(n, -np.inf, np.float32)
        want_idx[:len(rid)], want_sc[:len(rid)] = rid, rsc.astype(np.float32)
        assert (rsc.astype(np.float32).astype(np.float64) == rsc).all()
        assert (idx[r] == want_idx).all() and (sc[r].view(np.int32) == want_sc.view(np.int32)).all(), r


# ---- 2. agreement with pc_retrieve_topk
def _agree_with_old(proj, types, type_idx, features, rowptr, col, table, n):
    from p_companion_amd import ops
    dp, dt = torch.from_numpy(proj).cuda(), torch.from_numpy(types).cuda()
    a_idx, a_sc = ops.retrieve_topk(dp, dt, rowptr, col, table, n)
    b_idx, b_sc = ops.retrieve_topk_grouped(dp, dt, rowptr, col, table, n)
    a_idx, a_sc = a_idx.cpu().numpy(), a_sc.cpu().numpy()
    ref = [(a_idx[r][a_idx[r] >= 0], a_sc[r][a_idx[r] >= 0].astype(np.float64)) for r in range(len(types))]
    check_rows(b_idx.cpu().numpy(), b_sc.cpu().numpy(), ref, proj, features, type_idx, types, n)


def test_agrees_with_pc_retrieve_topk_on_the_reference_graph(golden):
    from p_companion_amd.data import IntBPG
    bpg = IntBPG.from_arrays(golden("g2_bpg1000.npz"))
    rng = np.random.default_rng(2)
    R = 600
    types = rng.integers(0, bpg.n_types, R).astype(np.int32)
    proj = rng.standard_normal((R, 128)).astype(np.float32)
    rowptr, col, table = upload(bpg.type_idx.astype(np.int32), np.ascontiguousarray(bpg.features, np.float32), bpg.n_types)
    _agree_with_old(proj, types, bpg.type_idx, np.asarray(bpg.features, np.float32), rowptr, col, table, 10)


def test_agrees_with_pc_retrieve_topk_on_a_scaled_catalogue():
    from p_companion_amd.data import generate_scaled_bpg
    bpg = generate_scaled_bpg(100_000, 100, seed=4)
    rng = np.random.default_rng(3)
    R = 4096 * 3 // 4
    types = rng.integers(0, bpg.n_types, R).astype(np.int32)
    proj = rng.standard_normal((R, 128)).astype(np.float32)
    g = bpg.cuda()
    rowptr, col = host_csr(bpg.type_idx, bpg.n_types)
    _agree_with_old(proj, types, bpg.type_idx, bpg.features, torch.from_numpy(rowptr).cuda(), torch.from_numpy(col).cuda(),
                    g["features"], 10)


# ---- 3. bit-exactness
def test_bitwise_run_to_run_across_slices_and_candidate_order(mixed):
    from p_companion_amd import ops
    m = mixed
    run = lambda col, s: ops.retrieve_topk_grouped(m.dproj, m.dtypes, m.rowptr, col, m.table, 16, slices=s)
    i0, s0 = run(m.col, 0)
    i1, s1 = run(m.col, 0)
    assert torch.equal(i0, i1) and torch.equal(s0.view(torch.int32), s1.view(torch.int32))
    for s in (1, 7, 64):
        i, sc = run(m.col, s)
        assert torch.equal(i, i0) and torch.equal(sc.view(torch.int32), s0.view(torch.int32)), s
    # type_col permuted inside every type's segment
    rowptr = m.rowptr.cpu().numpy()
    col = m.col.cpu().numpy().copy()
    rng = np.random.default_rng(5)
    for t in range(m.T):
        seg = col[rowptr[t]:rowptr[t + 1]]
        rng.shuffle(seg)
    i, sc = run(torch.from_numpy(col).cuda(), 0)
    assert torch.equal(i, i0) and torch.equal(sc.view(torch.int32), s0.view(torch.int32))


# ---- 4. the device-built type CSR
def test_type_csr_equals_the_host_construction():
    from p_companion_amd import ops
    from p_companion_amd.data import generate_device_bpg, generate_scaled_bpg
    for bpg in (generate_scaled_bpg(100_000, 100, seed=1), generate_device_bpg(200_000, 300, seed=2).to_host()):
        rowptr, col = ops.type_csr(torch.from_numpy(bpg.type_idx.astype(np.int32)).cuda(), bpg.n_types)
        want_rowptr, want_col = host_csr(bpg.type_idx, bpg.n_types)
        assert rowptr.dtype == torch.int32 and col.dtype == torch.int32
        assert torch.equal(rowptr.cpu(), torch.from_numpy(want_rowptr))
        assert torch.equal(col.cpu(), torch.from_numpy(want_col))
    with pytest.raises(ValueError):
        ops.type_csr(torch.tensor([0, 3], dtype=torch.int32, device="cuda"), 3)


# ---- 5. PCompanionInference over a DeviceBPG
def test_inference_over_a_device_bpg_matches_the_intbpg_path():
    """Fails before the grouped path existed: the constructor read the host type_idx (AttributeError)."""
    from p_companion_amd.data import DeviceBPG, generate_device_bpg
    from p_companion_amd.inference import PCompanionInference
    from p_companion_amd.p_companion import PCompanion
    dbpg = generate_device_bpg(200_000, 100, seed=6, world=1)
    hbpg = dbpg.to_host()
    c = cfg(NUM_TYPES=dbpg.n_types)
    torch.manual_seed(4)
    model = PCompanion(c, dbpg.cuda()["features"])
    dev_inf = PCompanionInference(model, c, dbpg)
    host_inf = PCompanionInference(model, c, hbpg)
    q = torch.from_numpy(np.random.default_rng(8).choice(dbpg.num_products, 512, replace=False).astype(np.int32))
    t_d, i_d, s_d = dev_inf.recommend_batch(q, 10)
    t_h, i_h, s_h = host_inf.recommend_batch(q, 10)
    assert torch.equal(t_d, t_h)
    types = t_h.reshape(-1).to(torch.int32).cpu().numpy()
    i_h, s_h = i_h.reshape(-1, 10).cpu().numpy(), s_h.reshape(-1, 10).cpu().numpy()
    ref = [(i_h[r][i_h[r] >= 0], s_h[r][i_h[r] >= 0].astype(np.float64)) for r in range(len(types))]
    out = dev_inf.model({"query_idx": q.cuda(), "query_types": dev_inf.type_idx[q.long().cuda()]})
    proj = out["projected_embeddings"].reshape(-1, 128).cpu().numpy()
    check_rows(i_d.reshape(-1, 10).cpu().numpy(), s_d.reshape(-1, 10).cpu().numpy(), ref, proj, hbpg.features,
               hbpg.type_idx, types, 10)

    rec_d, rec_h = dev_inf.recommend("P000007", 5), host_inf.recommend("P000007", 5)
    assert rec_d["complementary_types"] == rec_h["complementary_types"]
    assert len(rec_d["recommendations"]) == len(rec_h["recommendations"]) >= 1
    for a, b, sa, sb in zip(rec_d["recommendations"], rec_h["recommendations"], rec_d["scores"], rec_h["scores"]):
        np.testing.assert_allclose(sa, sb, rtol=TOL, atol=TOL)
        assert len(a) == len(b)
    with pytest.raises(ValueError):
        dev_inf.recommend("P999999")
    with pytest.raises(ValueError):
        dev_inf.recommend(dbpg.num_products)

    shard = generate_device_bpg(20_000, 100, seed=6, rank=0, world=2, with_complementary=False)
    with pytest.raises(ValueError, match="shard"):
        PCompanionInference(model, c, shard)
    no_feat = DeviceBPG({k: v for k, v in dbpg.arrays.items() if k != "features"}, dbpg.n_types, dbpg.dim)
    with pytest.raises(ValueError, match="without features"):
        PCompanionInference(model, c, no_feat)


# ---- 6. a 10 M spot check
def test_10M_catalogue_spot_check():
    """generate_device_bpg(10 M, 100 types): 64 rows against a float64 torch computation of their types' candidates.
    Time limit: about 60 s on one MI355X (generation, the device CSR, one call, 64 float64 reference rows)."""
    import time
    from p_companion_amd import ops
    from p_companion_amd.data import generate_device_bpg
    t0 = time.time()
    bpg = generate_device_bpg(10_000_000, 100, seed=0, world=1, with_complementary=False)
    g = bpg.cuda()
    rowptr, col = ops.type_csr(g["type_idx"], bpg.n_types)
    rng = np.random.default_rng(9)
    R, n = 64, 10
    types = torch.from_numpy(rng.integers(0, 100, R).astype(np.int32)).cuda()
    proj = torch.from_numpy(rng.standard_normal((R, 128)).astype(np.float32)).cuda()
    idx, sc = ops.retrieve_topk_grouped(proj, types, rowptr, col, g["features"], n)
    idx, sc = idx.cpu().numpy(), sc.cpu().numpy()
    for r in range(R):
        cand = torch.nonzero(g["type_idx"] == types[r]).reshape(-1)
        sims = g["features"][cand].double() @ proj[r].double()
        top = torch.topk(sims, n)
        want_sc = top.values.cpu().numpy()
        np.testing.assert_allclose(sc[r], want_sc, rtol=TOL, atol=TOL, err_msg=f"row {r}")
        got = torch.from_numpy(idx[r]).cuda().long()
        assert (g["type_idx"][got] == types[r]).all()
        own = (g["features"][got].double() @ proj[r].double()).cpu().numpy()
        np.testing.assert_allclose(own, want_sc, rtol=TOL, atol=TOL)
    assert time.time() - t0 < 60


# ---- 7. errors
def test_error_codes():
    from p_companion_amd import _lib
    L = _lib.lib()
    R, T = 4, 2
    dev = "cuda"
    proj = torch.zeros(R, 256, device=dev)
    types = torch.zeros(R, dtype=torch.int32, device=dev)
    rowptr = torch.tensor([0, 2, 4], dtype=torch.int32, device=dev)
    col = torch.arange(4, dtype=torch.int32, device=dev)
    table = torch.zeros(4, 256, device=dev)
    oi = torch.empty(R, 16, dtype=torch.int32, device=dev)
    os_ = torch.empty(R, 16, device=dev)
    need = L.pc_retrieve_topk_grouped_workspace_bytes(R, T, 16, 64)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(n=10, dim=128, slices=0, nbytes=need, null=None, rows=R):
        args = [p(proj), p(types), rows, p(rowptr), p(col), p(table), T, n, dim, slices, p(oi), p(os_), p(ws), nbytes, st]
        if null is not None:
            args[null] = None
        return L.pc_retrieve_topk_grouped(*args)

    assert call() == 0 and call(dim=256, n=16, slices=64) == 0
    torch.cuda.synchronize()
    for bad in ({"n": 0}, {"n": 17}, {"dim": 192}, {"slices": -1}, {"slices": 65}):
        assert call(**bad) == -2, bad                                          # PC_ESHAPE
    for pos in (0, 1, 3, 4, 5, 10, 11, 12):
        assert call(null=pos) == -1, pos                                       # PC_EINVAL
    assert call(rows=0) == -1
    assert call(nbytes=L.pc_retrieve_topk_grouped_workspace_bytes(R, T, 10, 0) - 1) == -3        # PC_EWORKSPACE
    assert L.pc_retrieve_topk_grouped_workspace_bytes(R, T, 17, 0) == 0


# ---- 8. PCompanion over an EmbeddingMapping
def test_pcompanion_takes_an_embedding_mapping_as_is():
    from p_companion_amd.data import EmbeddingMapping
    from p_companion_amd.p_companion import PCompanion, _IdentityIds
    table = torch.randn(5000, 128, device="cuda")
    mapping = EmbeddingMapping(table)
    model = PCompanion(cfg(NUM_TYPES=10), mapping)
    w = model.product_embeddings.weight
    assert w.device == table.device and torch.equal(w, table) and not w.requires_grad
    assert isinstance(model.product_to_idx, _IdentityIds) and model.product_to_idx["P000123"] == 123
    with pytest.raises(KeyError):
        model.product_to_idx["P005000"]
