"""Joint P-Companion training over a device-resident catalogue (a DeviceBPG): the labelled-pair split on the device
(pc_comp_split_pairs) against its definition, the dim-generic batch builder (pc_build_complementary_batch_dim), the device
dataset as a drop-in for the host one in train.train, train.main end to end into PCompanionInference, the per-op path at
dim 256 against the oracle, a 10 M spot check and the refusals.  Needs an MI355X."""
import ctypes
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import joint_oracle, philox_oracle


def cfg(tmp, **over):
    c = SimpleNamespace(PRODUCT_EMB_DIM=128, TYPE_EMB_DIM=64, HIDDEN_SIZE=256, NUM_ATTENTION_HEADS=4, DROPOUT=0.0,
                        MARGIN=1.0, ALPHA=0.8, NUM_COMP_TYPES=3, NUM_TYPES=100, DEVICE=torch.device("cuda"),
                        LEARNING_RATE=1e-3, BATCH_SIZE=256, PRODUCT2VEC_EPOCHS=1, NUM_EPOCHS=1, MODEL_DIR=str(tmp))
    c.__dict__.update(over)
    return c


def labelled(comp, sim):
    """data_loader.py:113-116: complementary pairs (+1), then similarity pairs (-1)."""
    return np.concatenate([np.concatenate([comp, np.ones((len(comp), 1), np.int32)], 1),
                           np.concatenate([sim, -np.ones((len(sim), 1), np.int32)], 1)])


# ------------------------------------------------------------------ 1. the split equals its definition
@pytest.mark.parametrize("n_comp,n_sim", [(6, 4), (1, 0), (0, 3), (1000, 537), (600_001, 400_123)])
def test_split_equals_its_definition(n_comp, n_sim):
    from p_companion_amd import ops
    rng = np.random.default_rng(n_comp + n_sim)
    comp = rng.integers(0, 1 << 30, (n_comp, 2)).astype(np.int32)
    sim = rng.integers(0, 1 << 30, (n_sim, 2)).astype(np.int32)
    L = labelled(comp, sim)
    n = len(L)
    dc, ds = torch.from_numpy(comp).cuda(), torch.from_numpy(sim).cuda()
    for seed in (0, 2 ** 63 + 12345):
        for mode, m in (("train", 0), ("val", 1), ("test", 2)):
            got = ops.comp_split_pairs(dc, ds, seed, mode)
            lo, hi = {"train": (0, int(0.8 * n)), "val": (int(0.8 * n), int(0.9 * n)), "test": (int(0.9 * n), n)}[mode]
            want = L[philox_oracle.epoch_permutation(n, seed, m)[lo:hi]]
            assert got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == (hi - lo, 3), (seed, mode)
            assert np.array_equal(got.cpu().numpy(), want), (seed, mode)


def test_split_error_codes_through_ctypes():
    from p_companion_amd import _lib
    L = _lib.lib()
    comp = torch.zeros(4, 2, dtype=torch.int32, device="cuda")
    out = torch.full((8, 3), 7, dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    call = lambda *a: L.pc_comp_split_pairs(*a, s)
    assert call(p(comp), 4, p(comp), 4, 0, 0, 0, 0, p(out)) == 0
    for bad in ((p(comp), 4, p(comp), 4, 0, 9, 0, 0, p(out)), (p(comp), 4, p(comp), 4, 0, 8, 0, 3, p(out)),
                (None, 4, p(comp), 4, 0, 8, 0, 0, p(out)), (p(comp), 4, p(comp), 4, 0, 8, 0, 0, None),
                (p(comp), 1 << 31, p(comp), 4, 0, 8, 0, 0, p(out)), (None, 0, None, 0, 0, 0, 0, 0, p(out))):
        assert call(*bad) == -1, bad
    torch.cuda.synchronize()
    assert bool((out == 7).all())                                     # nothing was written


# ------------------------------------------------------------------ 2. the dim-generic builder
def _build_dim(pairs, feats, type_idx, n_types, seed, step, dim, targets=True):
    from p_companion_amd import _lib, ops
    b = pairs.shape[0]
    i32 = lambda: torch.empty(b, dtype=torch.int32, device="cuda")
    f32 = lambda: torch.empty(b, dim, dtype=torch.float32, device="cuda")
    o = {"query_idx": i32(), "query_types": i32(), "positive_types": i32(), "negative_types": i32(),
         "positive_items": f32(), "negative_items": f32(), "target_features": f32() if targets else None}
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    rc = _lib.lib().pc_build_complementary_batch_dim(
        p(pairs), b, p(feats), p(type_idx), n_types, dim, seed, step, p(o["query_idx"]), p(o["query_types"]),
        p(o["positive_types"]), p(o["negative_types"]), p(o["positive_items"]), p(o["negative_items"]), p(o["target_features"]),
        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "pc_build_complementary_batch_dim")
    return o


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_builder_dim128_is_bit_identical_to_the_existing_entry():
    from p_companion_amd import ops
    g = torch.Generator().manual_seed(0)
    P, T, B = 3000, 37, 1000
    feats = torch.randn(P, 128, generator=g).cuda()
    type_idx = torch.randint(0, T, (P,), generator=g, dtype=torch.int32).cuda()
    pairs = torch.stack([torch.randint(0, P, (B,), generator=g), torch.randint(0, P, (B,), generator=g),
                         torch.randint(0, 2, (B,), generator=g) * 2 - 1], 1).to(torch.int32).cuda()
    for targets in (True, False):
        old = ops.build_complementary_batch(pairs, feats, type_idx, T, 2 ** 40 + 9, 77, want_targets=targets)
        new = _build_dim(pairs, feats, type_idx, T, 2 ** 40 + 9, 77, 128, targets)
        for k in ("query_idx", "query_types", "positive_types", "negative_types"):
            assert torch.equal(old[k].reshape(-1), new[k]), k
        for k in ("positive_items", "negative_items") + (("target_features",) if targets else ()):
            assert torch.equal(_bits(old[k]), _bits(new[k])), k


def test_builder_dim256_rows_types_and_filler():
    from p_companion_amd import ops
    g = torch.Generator().manual_seed(1)
    P, T, B = 2000, 23, 700
    feats = torch.randn(P, 256, generator=g)
    type_idx = torch.randint(0, T, (P,), generator=g, dtype=torch.int32)
    q, t = torch.randint(0, P, (B,), generator=g), torch.randint(0, P, (B,), generator=g)
    lab = torch.randint(0, 2, (B,), generator=g) * 2 - 1
    pairs = torch.stack([q, t, lab], 1).to(torch.int32).cuda()
    b = ops.build_complementary_batch(pairs, feats.cuda(), type_idx.cuda(), T, 5, 3)
    assert b["positive_items"].shape == (B, 256) and b["target_features"].shape == (B, 256)
    tt = type_idx[t].long()
    pos = lab == 1
    assert torch.equal(b["query_idx"].cpu().long(), q) and torch.equal(b["query_types"].cpu().long(), type_idx[q].long())
    assert torch.equal(b["positive_types"].cpu().view(-1).long(), torch.where(pos, tt, torch.zeros_like(tt)))
    assert torch.equal(b["negative_types"].cpu().view(-1).long(), torch.where(pos, (tt + 1) % T, tt))
    pi, ni, tf = b["positive_items"].cpu(), b["negative_items"].cpu(), b["target_features"].cpu()
    assert torch.equal(tf, feats[t]) and torch.equal(pi[pos], feats[t][pos]) and torch.equal(ni[~pos], feats[t][~pos])
    fill = torch.cat([ni[pos], pi[~pos]]).numpy().ravel()
    assert abs(fill.mean()) < 0.02 and abs(fill.std() - 1.0) < 0.02 and abs((fill ** 3).mean()) < 0.05
    # deterministic in (seed, step), new bits for a new step
    again = ops.build_complementary_batch(pairs, feats.cuda(), type_idx.cuda(), T, 5, 3)
    assert torch.equal(_bits(again["negative_items"]), _bits(b["negative_items"]))
    other = ops.build_complementary_batch(pairs, feats.cuda(), type_idx.cuda(), T, 5, 4)
    assert not torch.equal(other["negative_items"][pairs[:, 2] == 1], b["negative_items"][pairs[:, 2] == 1])
    # filler chunk t = b * (dim / 4) + c: a dim-256 batch of B rows carries the fillers of a dim-128 batch of 2 B rows
    allpos = pairs.clone()
    allpos[:, 2] = 1
    f256 = ops.build_complementary_batch(allpos, feats.cuda(), type_idx.cuda(), T, 5, 3)["negative_items"]
    pairs2 = torch.cat([allpos, allpos]).contiguous()
    f128 = ops.build_complementary_batch(pairs2, feats[:, :128].contiguous().cuda(), type_idx.cuda(), T, 5, 3)["negative_items"]
    assert torch.equal(_bits(f256).reshape(-1), _bits(f128).reshape(-1))
    with pytest.raises(ValueError, match="features"):
        ops.build_complementary_batch(pairs, feats[:, :64].contiguous().cuda(), type_idx.cuda(), T, 5, 3)


# ------------------------------------------------------------------ 3. drop-in parity with the host dataset
def test_device_dataset_is_a_drop_in_for_the_host_dataset(tmp_path):
    from p_companion_amd import train as drv
    from p_companion_amd.data import ComplementaryIndexDataset, ComplementaryIndexLoader, generate_device_bpg
    bpg = generate_device_bpg(5_000, 100, seed=4)
    host = bpg.to_host()
    runs = []
    table = torch.randn(bpg.num_products, 128, generator=torch.Generator().manual_seed(3))
    for src in ("device", "host"):
        loaders = []
        for mode, shuffle in (("train", True), ("val", False)):
            dds = ComplementaryIndexDataset(bpg, mode, seed=5)
            assert dds.pairs.is_cuda and len(dds) == dds.pairs.shape[0]
            if src == "host":
                ds = ComplementaryIndexDataset(host, mode, seed=5)
                assert len(ds) == len(dds)                            # the same 80/10/10 sizes
                ds.pairs = dds.pairs.cpu().numpy()
            else:
                ds = dds
            loaders.append(ComplementaryIndexLoader(ds, 256, shuffle=shuffle, seed=1))
        c = cfg(tmp_path / src, NUM_EPOCHS=2)
        torch.manual_seed(0)
        runs.append(drv.train(c, loaders[0], loaders[1], table))
    a, b = runs
    assert a.step_losses.numel() == 2 * len(loaders[0]) and torch.isfinite(a.step_losses).all()
    assert torch.equal(a.step_losses, b.step_losses)
    assert a.epoch_metrics == b.epoch_metrics
    for (k, va), (_, vb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.equal(va, vb), k


# ------------------------------------------------------------------ 4. end to end
def test_main_over_a_device_catalogue_into_serving(tmp_path):
    from p_companion_amd import train as drv
    from p_companion_amd.data import generate_device_bpg
    from p_companion_amd.inference import PCompanionInference
    bpg = generate_device_bpg(20_000, 100, seed=7)
    c = cfg(tmp_path, BATCH_SIZE=1024)
    torch.manual_seed(0)
    model = drv.main(c, bpg)
    assert torch.isfinite(model.step_losses).all() and model.step_losses.numel() > 0
    assert model.index_errors() == 0
    p2v = torch.load(os.path.join(c.MODEL_DIR, "product2vec.pth"), weights_only=True)
    assert set(p2v) == {"model_state_dict", "embeddings", "type_to_idx"} and p2v["type_to_idx"] is None
    assert isinstance(p2v["embeddings"], torch.Tensor) and p2v["embeddings"].shape == (20_000, 128)
    best = os.path.join(c.MODEL_DIR, "best_model.pth")
    assert os.path.exists(best)
    inf = PCompanionInference(best, c, bpg)
    q = torch.arange(0, 20_000, 97, dtype=torch.int32)
    types, idx, sc = inf.recommend_batch(q, 10)
    assert types.shape == (q.numel(), 3) and idx.shape == (q.numel(), 3, 10)
    idx, types = idx.cpu().long(), types.cpu().long()
    assert bool(((idx >= -1) & (idx < 20_000)).all()) and bool((idx[:, :, 0] >= 0).all())
    ti = bpg.arrays["type_idx"].cpu().long()
    live = idx >= 0
    assert torch.equal(ti[idx.clamp(min=0)][live], types[:, :, None].expand_as(idx)[live])     # of the predicted types


# ------------------------------------------------------------------ 5. dim 256 through train()
def test_dim256_device_catalogue_through_train_matches_the_oracle(tmp_path):
    from p_companion_amd import train as drv
    from p_companion_amd.data import ComplementaryIndexDataset, ComplementaryIndexLoader, generate_device_bpg
    from p_companion_amd.p_companion import PCompanion
    bpg = generate_device_bpg(3_000, 50, seed=3, dim=256)
    c = cfg(tmp_path, PRODUCT_EMB_DIM=256, NUM_TYPES=50, BATCH_SIZE=128)
    table = torch.randn(bpg.num_products, 256, generator=torch.Generator().manual_seed(2))
    tr_ds, va_ds = ComplementaryIndexDataset(bpg, "train", seed=1), ComplementaryIndexDataset(bpg, "val", seed=1)
    tr = ComplementaryIndexLoader(tr_ds, 128, shuffle=True, seed=6)
    va = ComplementaryIndexLoader(va_ds, 128, shuffle=False, seed=6)
    first = next(iter(ComplementaryIndexLoader(tr_ds, 128, shuffle=True, seed=6)))       # the batch train() steps first
    assert first["positive_items"].shape == (128, 256)
    torch.manual_seed(9)
    st0 = {k: v.detach().cpu().clone() for k, v in PCompanion(c, table).state_dict().items()}
    torch.manual_seed(9)
    model = drv.train(c, tr, va, table)
    assert model.step_losses.numel() == len(tr) and torch.isfinite(model.step_losses).all()
    hb = {k: first[k].cpu() for k in ("query_idx", "positive_items", "negative_items")}
    for k in ("query_types", "positive_types", "negative_types"):
        hb[k] = first[k].cpu().long()
    ref = joint_oracle.train_step({k: v.clone() for k, v in st0.items()}, hb, joint_oracle.new_moments(st0), 1)
    assert abs(float(model.step_losses[0]) - float(ref["loss"])) < 1e-4, (float(model.step_losses[0]), float(ref["loss"]))
    assert len(model.epoch_metrics) == 1 and os.path.exists(os.path.join(c.MODEL_DIR, "best_model.pth"))


# ------------------------------------------------------------------ 6. 10 M spot check
def test_10M_catalogue_split_and_graphed_steps():
    from p_companion_amd.data import ComplementaryIndexDataset, ComplementaryIndexLoader, generate_device_bpg
    from p_companion_amd.p_companion import GraphedJointStep, PCompanion
    from p_companion_amd.product2vec import FusedAdam, Product2Vec
    P = 10_000_000
    bpg = generate_device_bpg(P, 100, seed=0)
    n = int(bpg.arrays["comp_pairs"].shape[0]) + bpg.n_similarity_pairs
    ds = ComplementaryIndexDataset(bpg, "train", seed=0)
    assert ds.pairs.is_cuda and len(ds) == int(0.8 * n)
    lab = ds.pairs[:, 2]
    assert bool(((lab == 1) | (lab == -1)).all()) and int(ds.pairs[:, :2].min()) >= 0 and int(ds.pairs[:, :2].max()) < P
    c = cfg("unused")
    torch.manual_seed(0)
    emb = Product2Vec(c).to("cuda").eval().generate_all_embeddings(bpg)           # the exported [P,128] table, on the device
    m = PCompanion(c, emb).to("cuda").train()
    step = GraphedJointStep(m, FusedAdam(m), 4096, warmup=0, mode="direct")
    ld = ComplementaryIndexLoader(ds, 4096, shuffle=True, out=step.static)
    losses = step.run_epoch(ld, max_steps=50)
    assert losses.shape == (50, 3) and bool(torch.isfinite(losses).all())
    assert m.index_errors() == 0


# ------------------------------------------------------------------ 7. refusals
def test_refusals_on_the_device():
    from p_companion_amd import ops
    from p_companion_amd.data import ComplementaryIndexDataset, ComplementaryIndexLoader, DeviceBPG, generate_device_bpg
    with pytest.raises(ValueError, match="complementary pairs"):
        ComplementaryIndexDataset(generate_device_bpg(2_000, 20, seed=1, with_complementary=False), "train")
    with pytest.raises(ValueError, match="world = 1"):
        ComplementaryIndexDataset(generate_device_bpg(2_000, 20, seed=1, rank=0, world=2), "train")
    bpg = generate_device_bpg(2_000, 20, seed=1)
    with pytest.raises(ValueError, match="philox"):
        ComplementaryIndexDataset(bpg, "train", sampler="cpython")
    nofeat = ops.generate_catalogue(2_000, 20, 1, 16.0, 32, 128, "cuda", with_features=False)
    with pytest.raises(ValueError, match="features"):
        ComplementaryIndexDataset(DeviceBPG(nofeat, 20, 128), "train")
    ds = ComplementaryIndexDataset(bpg, "test")
    narrow = DeviceBPG(bpg.arrays, 10, 128)                           # type ids reach 19: the device range check
    ds.bpg = narrow
    with pytest.raises(IndexError, match="n_types"):
        ComplementaryIndexLoader(ds, 64)
