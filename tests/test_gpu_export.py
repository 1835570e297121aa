"""The device-CSR embedding export (Product2Vec.generate_all_embeddings, product2vec.py:83-111, eval mode) through
pc_p2v_export_embeddings: the co-view CSR stays in HBM, products go in bounded chunks, a ragged attention core reads each
node's neighbour rows through cv_col.  Checked against the reference's own fixture (g10), the host-CSR path, the oracle
on hand-made ragged graphs, and at configs[3] size.  Needs an MI355X."""
from collections.abc import Mapping
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import p2v_oracle


def cfg(d=128, **over):
    c = SimpleNamespace(PRODUCT_EMB_DIM=d, TYPE_EMB_DIM=64, HIDDEN_SIZE=256, NUM_ATTENTION_HEADS=4, DROPOUT=0.0,
                        MARGIN=1.0, ALPHA=0.8, NUM_COMP_TYPES=3, NUM_TYPES=100, DEVICE=torch.device("cuda"),
                        LEARNING_RATE=1e-3)
    c.__dict__.update(over)
    return c


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def state(d, seed=11):
    """Oracle state with non-trivial BatchNorm affine / running statistics and attention biases (eval mode reads them)."""
    st = p2v_oracle.init_state(seed, d=d)
    st["ffn.1.weight"] = 1.0 + 0.1 * rnd(256, seed=seed + 1)
    st["ffn.1.bias"] = 0.1 * rnd(256, seed=seed + 2)
    st["ffn.1.running_mean"] = 0.1 * rnd(256, seed=seed + 3)
    st["ffn.1.running_var"] = 0.5 + rnd(256, seed=seed + 4).abs()
    st["attention.in_proj_bias"] = 0.05 * rnd(3 * d, seed=seed + 5)
    st["attention.out_proj.bias"] = 0.05 * rnd(d, seed=seed + 6)
    return st


def model_from(st, d):
    from p_companion_amd.product2vec import Product2Vec
    m = Product2Vec(cfg(d)).to("cuda")
    m.load_state_dict({k: v.clone() for k, v in st.items()})
    return m.eval()


def i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


def max_err(a, b):
    return float((torch.as_tensor(a).cpu().float() - torch.as_tensor(b).cpu().float()).abs().max())


# ---- 1. the reference's own export
def test_golden_g10_export_from_device_csr(golden):
    from p_companion_amd.data import IntBPG
    g = golden("g10_p2v_epochs.npz")
    bpg = IntBPG.from_arrays(golden("g2_bpg1000.npz"))
    st = {k[6:]: torch.from_numpy(g[k]) for k in g.files if k.startswith("final.")}
    model = model_from(st, 128)
    dev = bpg.cuda("cuda")
    table = model.generate_embedding_table(dev["features"], dev["cv_rowptr"], dev["cv_col"])
    assert model.last_embedding_table is table and not model.training
    np.testing.assert_allclose(table.cpu().numpy(), g["embeddings"], rtol=0, atol=2e-5)
    assert int((np.diff(bpg.cv_rowptr) == 0).sum()) == 32


# ---- 2. agreement with the host-CSR path
@pytest.mark.parametrize("P,d", [(100_000, 128), (6_000, 256)])
def test_device_csr_agrees_with_host_csr_path(P, d):
    from p_companion_amd.data import generate_scaled_bpg
    bpg = generate_scaled_bpg(P, dim=d, seed=3)
    model = model_from(state(d), d)
    dev = bpg.cuda("cuda")
    host = model.generate_embedding_table(dev["features"], bpg.cv_rowptr, bpg.cv_col).clone()
    devt = model.generate_embedding_table(dev["features"], dev["cv_rowptr"], dev["cv_col"])
    assert devt.shape == (P, d)
    assert max_err(devt, host) <= 1e-5


# ---- 3. ragged edge cases against the oracle
def ragged_csr(P=57, hub=3000, seed=5):
    """degree 0 and 1, duplicate ids, a self-loop, one node of degree `hub` (far past any LDS-resident score array)."""
    rng = np.random.default_rng(seed)
    lists = [[] for _ in range(P)]
    lists[1] = [4]                                   # degree 1
    lists[2] = [9, 9, 9, 3]                          # duplicates
    lists[3] = [3]                                   # self-loop alone
    lists[4] = [4, 0, 4]                             # self-loop among duplicates
    lists[5] = list(rng.integers(0, P, hub))         # the hub (repeats as well)
    lists[6] = list(range(P))                        # every product
    for i in range(7, P):
        if i % 5:                                    # every fifth product: degree 0
            lists[i] = list(rng.integers(0, P, int(rng.integers(1, 70))))
    rowptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int32)
    col = np.array([t for x in lists for t in x], np.int32)
    return rowptr, col


@pytest.mark.parametrize("d", [128, 256])
@pytest.mark.parametrize("chunk_rows", [7, 1024, None])
def test_ragged_edge_cases_against_the_oracle(d, chunk_rows):
    from p_companion_amd import ops
    P = 57
    rowptr, col = ragged_csr(P)
    st = state(d)
    feats = rnd(P, d, seed=21)
    ref = p2v_oracle.generate_all_embeddings(feats, rowptr, col, st)
    dst = {k: v.cuda() for k, v in st.items()}
    out = ops.export_embeddings(dst, feats.cuda(), i32(rowptr), i32(col), chunk_rows=chunk_rows)
    assert max_err(out, ref) <= 2e-5
    e1 = p2v_oracle.ffn(feats, st, False)
    assert max_err(out[0], e1[0]) <= 2e-5 and max_err(out[10], e1[10]) <= 2e-5  # degree 0 keeps ffn(x)


# ---- 4. chunk invariance, determinism
def test_chunk_invariance_and_determinism():
    from p_companion_amd import ops
    from p_companion_amd.data import generate_scaled_bpg
    bpg = generate_scaled_bpg(150_000, seed=4)
    dst = {k: v.cuda() for k, v in state(128).items()}
    dev = bpg.cuda("cuda")
    run = lambda c: ops.export_embeddings(dst, dev["features"], dev["cv_rowptr"], dev["cv_col"], chunk_rows=c)
    a, b, c = run(1024), run(65536), run(None)
    assert max_err(a, b) <= 1e-6 and max_err(a, c) <= 1e-6
    assert torch.equal(run(1024), a) and torch.equal(run(65536), b)


# ---- 5. DeviceBPG: the Mapping, and train_model end to end
def test_generate_all_embeddings_on_a_device_bpg_returns_a_mapping():
    from p_companion_amd.data import EmbeddingMapping, generate_device_bpg
    bpg = generate_device_bpg(20_000, 100, seed=2, world=1, with_complementary=False)
    model = model_from(state(128), 128)
    emb = model.generate_all_embeddings(bpg)
    assert isinstance(emb, Mapping) and isinstance(emb, EmbeddingMapping) and not isinstance(emb, dict)
    host = bpg.to_host()
    hd = host.cuda("cuda")
    ref = model.generate_embedding_table(hd["features"], hd["cv_rowptr"], hd["cv_col"])
    assert len(emb) == 20_000 and list(emb)[:3] == ["P000000", "P000001", "P000002"] and list(emb)[-1] == "P019999"
    assert torch.equal(emb.table, ref)
    for i in (0, 1, 4321, 19_999):
        v = emb[f"P{i:06d}"]
        assert v.device.type == "cpu" and torch.equal(v, ref[i].cpu())
    assert "P020000" not in emb and "P1" not in emb
    with pytest.raises(KeyError):
        emb["P020000"]


def test_train_model_over_a_device_bpg_loader_returns_the_mapping():
    from p_companion_amd.data import SimilarityIndexLoader, generate_device_bpg
    from p_companion_amd.product2vec import FusedAdam, Product2Vec
    bpg = generate_device_bpg(20_000, 100, seed=6, world=1, with_complementary=False)
    torch.manual_seed(0)
    model = Product2Vec(cfg()).to("cuda")
    loader = SimilarityIndexLoader(bpg, 512, sampler="philox", device="cuda")
    emb = model.train_model(loader, FusedAdam(model), num_epochs=1)
    assert isinstance(emb, Mapping) and len(emb) == 20_000
    g = bpg.cuda()
    ref = model.generate_embedding_table(g["features"], g["cv_rowptr"], g["cv_col"])
    assert torch.equal(emb.table, ref) and torch.equal(emb["P000123"], ref[123].cpu())
    assert torch.isfinite(ref).all()


# ---- 6. configs[3] size
def test_config3_10M_products_export_spot_checked_against_the_oracle():
    from p_companion_amd import ops
    from p_companion_amd.data import generate_device_bpg
    P = 10_000_000
    bpg = generate_device_bpg(P, 100, seed=0, degree_cap=32, world=1, with_complementary=False)
    g = bpg.cuda()
    st = state(128)
    model = model_from(st, 128)
    assert ops.EXPORT_CHUNK_ROWS < P and _lib_ws(ops.EXPORT_CHUNK_ROWS) < 2 ** 30          # bounded by the chunk, not by P
    table = model.generate_embedding_table(g["features"], g["cv_rowptr"], g["cv_col"])
    torch.cuda.synchronize()
    assert table.shape == (P, 128)
    rng = np.random.default_rng(0)
    nodes = np.sort(rng.choice(P, 256, replace=False)).astype(np.int64)
    idx = torch.from_numpy(nodes).cuda()
    lo_hi = torch.stack([g["cv_rowptr"][idx], g["cv_rowptr"][idx + 1]], 1).cpu().numpy()
    assert (lo_hi[:, 1] == lo_hi[:, 0]).any() and (lo_hi[:, 1] > lo_hi[:, 0]).any()
    for i, (lo, hi) in zip(nodes, lo_hi):
        lo, hi = int(lo), int(hi)
        x = g["features"][i:i + 1].cpu()
        e1 = p2v_oracle.ffn(x, st, False)
        if hi == lo:
            ref = e1[0]
        else:
            nb = g["cv_col"][lo:hi].long()
            keys = p2v_oracle.ffn(g["features"][nb].cpu(), st, False)
            ref = p2v_oracle.attention(p2v_oracle.ffn(e1, st, False), keys.unsqueeze(0), st)[0]
        assert max_err(table[int(i)], ref) <= 2e-5, int(i)


def _lib_ws(chunk, d=128):
    from p_companion_amd import _lib
    return _lib.lib().pc_p2v_export_workspace_bytes(chunk, d)


# ---- 7. refusals
def test_refusals_before_launch():
    from p_companion_amd import ops
    from p_companion_amd.data import generate_device_bpg
    model = model_from(state(128), 128)
    bpg = generate_device_bpg(4_000, 100, seed=1, rank=0, world=2, with_complementary=False)
    with pytest.raises(ValueError, match="world"):
        model.generate_all_embeddings(bpg)
    P = 40
    rowptr, col = ragged_csr(P, hub=10)
    feats = rnd(P, 128, seed=3).cuda()
    with pytest.raises(TypeError):
        model.generate_embedding_table(feats, torch.from_numpy(rowptr), i32(col))           # host tensor
    with pytest.raises(TypeError):
        model.generate_embedding_table(feats, i32(rowptr), col)                             # mixed
    with pytest.raises(TypeError):
        model.generate_embedding_table(feats.cpu(), i32(rowptr), i32(col))
    dst = model._tensor_dict()
    with pytest.raises(ValueError, match="offsets"):
        ops.export_embeddings(dst, feats, i32(rowptr[:-1]), i32(col))                       # wrong length
    with pytest.raises(ValueError, match="len\\(cv_col\\)"):
        ops.export_embeddings(dst, feats, i32(rowptr), i32(col[:-1]))                       # rowptr[-1] != len(cv_col)
    with pytest.raises(TypeError):
        ops.export_embeddings(dst, feats, i32(rowptr).long(), i32(col))
    with pytest.raises(ValueError, match="chunk_rows"):
        ops.export_embeddings(dst, feats, i32(rowptr), i32(col), chunk_rows=0)
