"""Metrics.evaluate_model over a device-resident split as one call (pc_joint_eval_epoch) against the existing per-batch loop
(fused=False) on loaders built alike: the five metrics, the plan's complementary types, the per-batch hit counts, the state
the loader is left in, and train.train end to end.

Hit counts of the two paths may differ only in rows whose score sits on a threshold: `fragile_k` is the number of eligible
rows of the existing loop's own score matrix whose hit status at k changes when g_r moves by +- 2 (1e-5 + 1e-5 |g_r|) (the
project's score-agreement tolerance, once per path); per batch |new - old| <= fragile_k, and the data must keep fragile_k small
(<= max(2, 1 % of the old hits) per evaluation) so that the bound means something.  Needs an MI355X."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KEYS = ("hit@1", "hit@3", "hit@10", "type_diversity", "mean_relevance")


def cfg(T, dim=128, **over):
    c = SimpleNamespace(PRODUCT_EMB_DIM=dim, TYPE_EMB_DIM=64, HIDDEN_SIZE=256, NUM_ATTENTION_HEADS=4, DROPOUT=0.0, MARGIN=1.0,
                        ALPHA=0.8, NUM_COMP_TYPES=3, NUM_TYPES=T, DEVICE=torch.device("cuda"), LEARNING_RATE=1e-3,
                        BATCH_SIZE=256, NUM_EPOCHS=1)
    c.__dict__.update(over)
    return c


def trained_model(bpg, T, dim, steps=40):
    """A PCompanion over a seeded random product table, a few dozen training steps away from its initialiser."""
    from p_companion_amd.data import ComplementaryIndexDataset, ComplementaryIndexLoader
    from p_companion_amd.p_companion import GraphedJointStep, PCompanion
    from p_companion_amd.product2vec import FusedAdam
    c = cfg(T, dim)
    table = torch.randn(bpg.num_products, dim, generator=torch.Generator().manual_seed(11))
    torch.manual_seed(0)
    m = PCompanion(c, table).to("cuda").train()
    ds = ComplementaryIndexDataset(bpg, "train", seed=2)
    opt = FusedAdam(m, lr=1e-3)
    if dim == 128:
        step = GraphedJointStep(m, opt, 256, warmup=0, mode="direct")
        step.run_epoch(ComplementaryIndexLoader(ds, 256, shuffle=True, seed=4, out=step.static), max_steps=steps)
    else:
        for i, batch in enumerate(ComplementaryIndexLoader(ds, 256, shuffle=True, seed=4)):
            if i == steps:
                break
            m.train_step(batch, optimizer=opt)
    assert m.index_errors() == 0
    return m


def val_loader(bpg, B, shuffle, n_pairs=None, seed=3):
    from p_companion_amd.data import ComplementaryIndexDataset, ComplementaryIndexLoader
    ds = ComplementaryIndexDataset(bpg, "val", seed=2)
    if n_pairs is not None:
        assert len(ds) >= n_pairs, (len(ds), n_pairs)
        ds.pairs = ds.pairs[:n_pairs].contiguous() if torch.is_tensor(ds.pairs) else np.ascontiguousarray(ds.pairs[:n_pairs])
    return ComplementaryIndexLoader(ds, B, shuffle=shuffle, seed=seed)


def sims64(m):
    """float64 restatement of the plan's similarity rows, [T, T] (type_transition.py:17-19, p_companion.py:60-63)."""
    sd = {k: v.detach().double() for k, v in m.state_dict().items()}
    h = torch.relu(sd["query_type_embeddings.weight"] @ sd["type_transition.encoder.weight"].T + sd["type_transition.encoder.bias"])
    c = h @ sd["type_transition.decoder.weight"].T + sd["type_transition.decoder.bias"]
    return c @ sd["complementary_type_embeddings.weight"].T


def old_loop_counts(m, loader):
    """The existing loop's body (metrics.py:84-100), batch by batch: hit counts from ops.hit_rank on its own score matrix, the
    fragile rows, the forward's complementary types and the batch's query types."""
    from p_companion_amd import ops
    m.eval()
    out = []
    with torch.no_grad():
        for batch in loader:
            o = m(batch)
            proj = o["projected_embeddings"]
            sims = ops.linear_forward(proj.reshape(-1, proj.size(-1)).contiguous(), batch["target_features"].float().contiguous())
            rank = ops.hit_rank(sims)
            B = sims.shape[1]
            S = sims[:B].double()
            g = S.diagonal().clone()
            d = 2 * (1e-5 + 1e-5 * g.abs())
            off = ~torch.eye(B, dtype=torch.bool, device=S.device)
            few = ((S > (g + d)[:, None]) & off).sum(1)               # beat count if g_r were d higher
            many = ((S >= (g - d)[:, None]) & off).sum(1)             # ... if it were d lower
            hits, fragile = [], []
            for k in (1, 3, min(10, B)):
                kk = min(k, B)
                hits.append(int((rank < kk).sum()))
                fragile.append(int(((few < kk) != (many < kk)).sum()))
            out.append({"hits": hits, "fragile": fragile, "rows": B, "types": o["complementary_types"].to(torch.int32),
                        "query_types": batch["query_types"].long().clone()})
    return out


def compare(m, new, old_counts, old_metrics, log):
    stats = new["stats"].cpu().numpy()
    assert len(old_counts) == stats.shape[0]
    table = new["topk_table"].clone()
    s64 = None
    swapped = 0
    tot_old, tot_fragile = np.zeros(3, np.int64), np.zeros(3, np.int64)
    for i, oc in enumerate(old_counts):
        assert stats[i, 4] == oc["rows"] and stats[i, 3] == 3
        mine = table[oc["query_types"]]
        bad = (mine != oc["types"]).nonzero()
        if bad.numel():                                               # accepted only between types of equal similarity
            s64 = sims64(m) if s64 is None else s64
            for b, k in bad.tolist():
                t = int(oc["query_types"][b])
                a, z = float(s64[t, int(mine[b, k])]), float(s64[t, int(oc["types"][b, k])])
                assert abs(a - z) <= 1e-5 + 1e-5 * abs(z), (i, b, k, a, z)
            swapped += bad.shape[0]
        for j in range(3):
            assert abs(int(stats[i, j]) - oc["hits"][j]) <= oc["fragile"][j], (i, j, stats[i].tolist(), oc["hits"], oc["fragile"])
        tot_old += np.array(oc["hits"]); tot_fragile += np.array(oc["fragile"])
    for j in range(3):                                                # the data keep the band nearly empty
        assert tot_fragile[j] <= max(2, tot_old[j] // 100), (tot_fragile, tot_old)
    assert tot_old[2] >= 20, tot_old
    nm = dict(zip(KEYS, new["metrics"].cpu().tolist()))
    assert nm["type_diversity"] == old_metrics["type_diversity"]
    assert abs(nm["mean_relevance"] - old_metrics["mean_relevance"]) <= 1e-4
    new_hits = stats[:, :3].sum(0)
    for j, key in enumerate(KEYS[:3]):
        if all(int(stats[i, j]) == oc["hits"][j] for i, oc in enumerate(old_counts)):
            # equal counts: what is left is how each path rounds a batch's rate to fp32 (hits / rows here; torch's mean()
            # may multiply by a rounded reciprocal instead): at most two roundings of a number <= 1 per path, 2^-24 each
            assert abs(nm[key] - old_metrics[key]) <= 2.0 ** -22, (key, nm[key], old_metrics[key])
    print(f"{log}: batches {len(old_counts)} old hits {tot_old.tolist()} new hits {new_hits.tolist()} fragile "
          f"{tot_fragile.tolist()} swapped types {swapped} |d mean_relevance| "
          f"{abs(nm['mean_relevance'] - old_metrics['mean_relevance']):.3g}")
    return nm


def plan_equals_forward_for_every_type(m, table, T):
    """Every row of the plan's [T, K] table -- every chunk of it, whether or not the val split holds a query of that type --
    against PCompanion.forward in eval mode over query_types = arange(T); the same rule for a swap as in compare()."""
    m.eval()
    with torch.no_grad():
        o = m({"query_idx": torch.zeros(T, dtype=torch.int32, device="cuda"), "query_types": torch.arange(T, device="cuda")})
    want = o["complementary_types"].to(torch.int32)
    assert tuple(table.shape) == tuple(want.shape)
    bad = (table != want).nonzero()
    if bad.numel():
        s64 = sims64(m)
        for t, k in bad.tolist():
            a, z = float(s64[t, int(table[t, k])]), float(s64[t, int(want[t, k])])
            assert abs(a - z) <= 1e-5 + 1e-5 * abs(z), (t, k, a, z)
    print(f"plan T={T}: {bad.shape[0]} of {want.numel()} entries swapped between types of equal similarity")


CASES = [
    # kind, products, T, B, dim, shuffle, val pairs (None: the whole split; else trimmed for a ragged rest >= 10)
    ("host", 20_000, 100, 256, 128, False, 256 * 6 + 37),
    ("host", 20_000, 1000, 256, 128, True, 256 * 5 + 10),
    # the plan runs over row chunks of 1024 types: T = 2500 is three chunks, the last of 452 rows (config.py:27's 34 800 is 34,
    # the last of 1008), so the chunks' offsets into E_q and both tables and the short last chunk are exercised
    ("host", 20_000, 2500, 256, 128, False, 256 * 5 + 41),
    ("device", 40_000, 2500, 4096, 128, True, 4096 * 5 + 77),
    ("device", 40_000, 100, 4096, 128, False, None),
    ("device", 40_000, 1000, 4096, 128, True, 4096 * 5 + 1234),
    ("device", 4_000, 50, 256, 256, True, 256 * 4 + 99),
    ("device", 4_000, 50, 256, 256, False, 256 * 4),
]


@pytest.mark.parametrize("kind,P,T,B,dim,shuffle,n_val", CASES)
def test_one_call_evaluation_matches_the_loop(kind, P, T, B, dim, shuffle, n_val):
    from p_companion_amd.data import generate_device_bpg, generate_scaled_bpg
    from p_companion_amd.metrics import Metrics
    bpg = generate_device_bpg(P, T, seed=6, dim=dim) if kind == "device" else generate_scaled_bpg(P, T, seed=6, dim=dim)
    m = trained_model(bpg, T, dim)
    la, lb, lc = (val_loader(bpg, B, shuffle, n_val) for _ in range(3))
    n = len(la.dataset)
    assert n % B == 0 or n % B >= 10
    if B == 4096:
        assert len(la) >= 5
    for rnd in range(2):                                              # the second evaluation: the filler steps continue
        new = Metrics.evaluate_on_device(m, la)
        new = {k: v.clone() for k, v in new.items()}
        counts = old_loop_counts(m, lb)
        old = Metrics.evaluate_model(m, lc, "cuda", fused=False)
        nm = compare(m, new, counts, old, f"{kind} P={P} T={T} B={B} dim={dim} shuffle={shuffle} round {rnd}")
        assert la.step == lb.step == lc.step == (rnd + 1) * len(la) and la.epoch == lb.epoch == lc.epoch == rnd + 1
        assert all(isinstance(v, float) and np.isfinite(v) for v in nm.values())
    assert m.index_errors() == 0
    plan_equals_forward_for_every_type(m, new["topk_table"], T)
    # the default takes the one-call form here and returns Python floats; twice on loaders built alike: identical doubles
    ld, le = val_loader(bpg, B, shuffle, n_val), val_loader(bpg, B, shuffle, n_val)
    a, b = Metrics.evaluate_model(m, ld, "cuda"), Metrics.evaluate_model(m, le, "cuda", fused=True)
    assert list(a) == list(KEYS) and a == b and all(type(v) is float for v in a.values())
    assert ld.step == len(ld) and ld.epoch == 1


def test_out_of_range_ids_are_counted_and_never_dereferenced():
    """The one-call form ONLY, on purpose.  The existing loop builds its batch with pc_build_complementary_batch[_dim], which reads
    features[target] and type_idx[query] unclamped (sampler.hip, build_complementary_batch_kernel): an id outside the table
    pushed through fused=False would be an out-of-bounds device read, i.e. a fault provoked on purpose.  Do not "complete" this
    test with the loop: its ids come from the graph, whose sizes train._check_ranges checks once against the tables."""
    from p_companion_amd.data import generate_device_bpg
    from p_companion_amd.metrics import Metrics
    P, T, B = 4_000, 50, 128
    bpg = generate_device_bpg(P, T, seed=1)
    m = trained_model(bpg, T, 128, steps=5)
    ld = val_loader(bpg, B, False, 3 * B + 20)
    clean = Metrics.evaluate_model(m, val_loader(bpg, B, False, 3 * B + 20), "cuda", fused=True)
    ld.dataset.pairs[5, 1] = P + 7                                    # a target past the table
    ld.dataset.pairs[B + 9, 0] = -3                                   # a query before it
    ld.dataset.pairs[2 * B + 1, 1] = 2 ** 31 - 1
    got = Metrics.evaluate_model(m, ld, "cuda")
    assert all(np.isfinite(v) for v in got.values()) and got["type_diversity"] == clean["type_diversity"]
    assert m.index_errors() == 3 and m.index_errors() == 0
    with pytest.raises(IndexError):
        ld2 = val_loader(bpg, B, False, 3 * B + 20)
        ld2.dataset.pairs[0, 1] = P
        Metrics.evaluate_model(m, ld2, "cuda")
        m.raise_index_errors()


def test_a_ragged_rest_under_ten_rows_takes_the_existing_loop():
    """metrics.py:103: the last batch's key is 'hit@5', which the reference's dict does not hold -- both entries behave as the
    existing loop does, and fused=True says why it does not apply."""
    from p_companion_amd.data import generate_device_bpg
    from p_companion_amd.metrics import Metrics
    bpg = generate_device_bpg(4_000, 50, seed=1)
    m = trained_model(bpg, 50, 128, steps=5)
    la, lb, lc = (val_loader(bpg, 128, False, 2 * 128 + 5) for _ in range(3))
    with pytest.raises(KeyError):
        Metrics.evaluate_model(m, la, "cuda")
    with pytest.raises(KeyError):
        Metrics.evaluate_model(m, lb, "cuda", fused=False)
    assert la.step == lb.step and la.epoch == lb.epoch
    with pytest.raises(ValueError, match="fewer than 10"):
        Metrics.evaluate_model(m, lc, "cuda", fused=True)
    assert lc.step == 0 and lc.epoch == 0
    # a model on the GPU over a loader of host batches: the loop, as before
    with pytest.raises(ValueError, match="ComplementaryIndexLoader"):
        Metrics.evaluate_model(m, list(val_loader(bpg, 128, False, 256)), "cuda", fused=True)


def test_train_runs_the_one_call_evaluation(tmp_path, monkeypatch):
    import os
    from p_companion_amd import train as drv
    from p_companion_amd.data import ComplementaryIndexDataset, ComplementaryIndexLoader, generate_device_bpg
    from p_companion_amd.metrics import Metrics
    bpg = generate_device_bpg(8_000, 100, seed=4)
    table = torch.randn(bpg.num_products, 128, generator=torch.Generator().manual_seed(3))
    B = 256
    calls = []
    real = Metrics.evaluate_model
    on_device = Metrics.evaluate_on_device

    def spy(model, loader):
        calls.append("one call")
        return on_device(model, loader)

    monkeypatch.setattr(Metrics, "evaluate_on_device", staticmethod(spy))
    runs = []
    for forced in (False, True):
        if forced:
            monkeypatch.setattr(Metrics, "evaluate_model", staticmethod(lambda mo, ld, dev: real(mo, ld, dev, fused=False)))
        tr = ComplementaryIndexLoader(ComplementaryIndexDataset(bpg, "train", seed=5), B, shuffle=True, seed=1)
        va_ds = ComplementaryIndexDataset(bpg, "val", seed=5)
        if 0 < len(va_ds) % B < 10:
            va_ds.pairs = va_ds.pairs[:len(va_ds) - len(va_ds) % B].contiguous()
        va = ComplementaryIndexLoader(va_ds, B, shuffle=False, seed=1)
        c = cfg(100, NUM_EPOCHS=2, MODEL_DIR=str(tmp_path / ("loop" if forced else "one_call")))
        torch.manual_seed(0)
        n_before = len(calls)
        runs.append(drv.train(c, tr, va, table))
        assert len(calls) - n_before == (0 if forced else 2)
        assert os.path.exists(os.path.join(c.MODEL_DIR, "best_model.pth"))
        ck = torch.load(os.path.join(c.MODEL_DIR, "best_model.pth"), weights_only=False)
        assert list(ck["metrics"]) == list(KEYS) and all(type(v) is float for v in ck["metrics"].values())
        nb, rows_last = len(va), (len(va_ds) % B or B)
    new, old = runs
    assert torch.equal(new.step_losses, old.step_losses)
    assert len(new.epoch_metrics) == len(old.epoch_metrics) == 2
    for a, b in zip(new.epoch_metrics, old.epoch_metrics):
        assert list(a) == list(KEYS) and all(type(v) is float for v in a.values())
        assert a["type_diversity"] == b["type_diversity"] and abs(a["mean_relevance"] - b["mean_relevance"]) <= 1e-4
        for key in KEYS[:3]:
            # counts differ by at most max(2, 1 % of the old hits) per evaluation (above); a count is worth at most
            # 1 / (rows of the smallest batch * K) of a batch's rate, and the metric is the mean over nb batches
            old_hits = b[key] * B * 3 * nb
            assert abs(a[key] - b[key]) <= max(2.0, 0.01 * old_hits) / (rows_last * 3 * nb), (key, a[key], b[key])
