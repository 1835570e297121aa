"""Ingestion of behaviour edge lists on the device (csrc/ingest.hip, ops.build_catalogue, data.device_bpg_from_edges) against
the host twin IntBPG.from_edges, bit for bit: the reference's own graph, the hand-made graph of tests/test_ingest_host.py,
every row-length class at its limits, the generator's graphs fed back as edge lists, ids outside the catalogue, and the
existing consumers over a built graph.  Needs an MI355X."""
import numpy as np
import pytest
import torch

from test_ingest_host import (HAND_CAP, HAND_CP, HAND_CV, HAND_EXPECT, HAND_EXPECT_NO_PV, HAND_PV, HAND_TYPES, _keys,
                              check_against)

pytestmark = pytest.mark.gpu

ARRAYS = ("cv_rowptr", "cv_col", "similarity_pairs", "sim_rowptr", "sim_col", "complementary_pairs")


def assert_equal_to_host(dev_bpg, host_bpg):
    """cv_rowptr, cv_col, sim_pairs, sim_rowptr, sim_col, complementary_pairs, pair_deg and max_degree, array for array."""
    h = dev_bpg.to_host()
    for k in ARRAYS:
        a, b = getattr(h, k), getattr(host_bpg, k)
        assert a.dtype == b.dtype == np.int32 and a.shape == b.shape and np.array_equal(a, b), k
    assert np.array_equal(dev_bpg.arrays["pair_deg"].cpu().numpy(), host_bpg.degree(host_bpg.similarity_pairs[:, 0]))
    assert dev_bpg.max_degree == host_bpg.max_degree == h.max_degree
    assert dev_bpg.n_similarity_pairs == len(host_bpg.similarity_pairs)


def assert_same_bits(a, b):
    assert a.arrays.keys() == b.arrays.keys()
    for k, v in a.arrays.items():
        assert torch.equal(v, b.arrays[k]) if torch.is_tensor(v) else v == b.arrays[k], k


@pytest.fixture(scope="module")
def golden_lists(golden):
    z = golden("g2_bpg1000.npz")
    return {k: z[k] for k in ("features", "type_idx", "co_view", "purchase_after_view", "co_purchase")}


@pytest.fixture(scope="module")
def golden_graph(golden_lists):
    from p_companion_amd.data import device_bpg_from_edges
    g = golden_lists
    return device_bpg_from_edges(g["features"], g["type_idx"], 20, g["co_view"], g["purchase_after_view"], g["co_purchase"],
                                 degree_cap=64)


def test_golden_graph_equals_the_host_builder(golden_lists, golden_graph):
    from p_companion_amd.data import IntBPG
    g = golden_lists
    host = IntBPG.from_edges(g["features"], g["type_idx"], g["co_view"], g["purchase_after_view"], g["co_purchase"],
                             degree_cap=64)
    assert_equal_to_host(golden_graph, host)
    assert golden_graph.max_degree == 48 and golden_graph.n_similarity_pairs == 2949
    assert golden_graph.arrays["comp_pairs"].shape == (4523, 2) and golden_graph.dim == 128 and golden_graph.world == 1
    h = golden_graph.to_host()
    assert np.array_equal(h.features, g["features"]) and np.array_equal(h.type_idx, g["type_idx"])


def test_hand_made_graph_gives_the_literal_arrays():
    from p_companion_amd.data import device_bpg_from_edges
    d = device_bpg_from_edges(None, HAND_TYPES, 3, HAND_CV, HAND_PV, HAND_CP, degree_cap=HAND_CAP)
    check_against(HAND_EXPECT, d.to_host(), d.arrays["pair_deg"].cpu().numpy())
    assert d.max_degree == 3 and "features" not in d.arrays and d.to_host().features.shape == (12, 0)
    e = device_bpg_from_edges(None, HAND_TYPES, 3, HAND_CV, np.zeros((0, 2), np.int32), HAND_CP, degree_cap=HAND_CAP)
    check_against(HAND_EXPECT_NO_PV, e.to_host(), e.arrays["pair_deg"].cpu().numpy())
    assert e.n_similarity_pairs == 0


def _class_lists(P, seed):
    """Sources 0..4 have raw co_view rows at the wave path's limit, one past it, at the LDS path's limit and one past it, and
    of length 1 -- drawn with replacement from the 299 other products, so weights differ; the other two lists have rows of the
    same raw lengths on other sources (they meet the same paths without weights)."""
    from p_companion_amd import ops
    rng = np.random.default_rng(seed)
    lengths = [ops.INGEST_WAVE_ROW_MAX, ops.INGEST_WAVE_ROW_MAX + 1, ops.INGEST_LDS_ROW_MAX, ops.INGEST_LDS_ROW_MAX + 1, 1]

    def rows(sources):
        out = []
        for s, n in zip(sources, lengths):
            others = np.delete(np.arange(P), s)
            # a skewed draw: low ids are frequent (weights up to a few hundred in the long rows), high ids come once or never
            t = others[np.minimum((rng.random(n) ** 2 * 299).astype(np.int64), 298)]
            out.append(np.stack([np.full(n, s), t], 1))
        return out

    cv = rows([0, 1, 2, 3, 4]) + [np.stack([np.full(40, 7), rng.integers(8, 300, 40)], 1)]
    both = np.concatenate(cv)
    # the other lists' own limit rows sit on sources without co-view edges; besides, co-view edges with an even target are
    # purchased after view and those with target = 1 mod 3 co-purchased (at every cap some kept edges are similarity pairs and
    # some are not; a co-purchase of a co-viewed pair -- kept or dropped -- is no complement), and a fifth of the
    # purchase-after-view rows is co-purchased too (no complement either)
    pv = rows([10, 11, 12, 13, 5])
    cp = rows([20, 21, 22, 23, 6]) + [e[e[:, 1] % 5 == 0] for e in pv[:4]] + [both[both[:, 1] % 3 == 1]]
    pv = pv + [both[both[:, 1] % 2 == 0]]
    mix = lambda parts: np.concatenate(parts).astype(np.int32)[rng.permutation(sum(len(p) for p in parts))]
    return mix(cv), mix(pv), mix(cp)


@pytest.fixture(scope="module")
def class_lists():
    return _class_lists(300, 5)


@pytest.mark.parametrize("cap", [1, 32, 64])
def test_row_length_classes_equal_the_host_builder(class_lists, cap):
    from p_companion_amd.data import IntBPG, device_bpg_from_edges
    P = 300
    cv, pv, cp = class_lists
    types = (np.arange(P) % 7).astype(np.int32)
    host = IntBPG.from_edges(None, types, cv, pv, cp, degree_cap=cap)
    assert host.max_degree == cap and len(host.similarity_pairs) > 0 and len(host.complementary_pairs) > 0
    for edges, sources in ((cv, [0, 1, 2, 3, 4]), (pv, [10, 11, 12, 13, 5]), (cp, [20, 21, 22, 23, 6])):
        assert np.bincount(edges[:, 0], minlength=P)[sources].tolist() == [128, 129, 4096, 4097, 1]
    dev = [torch.from_numpy(a).cuda() for a in (cv, pv, cp)]
    d = device_bpg_from_edges(None, types, 7, *dev, degree_cap=cap)
    assert_equal_to_host(d, host)
    # the same call again, and the same lists in another order: identical bits
    assert_same_bits(d, device_bpg_from_edges(None, types, 7, *dev, degree_cap=cap))
    gen = torch.Generator(device="cuda").manual_seed(11)
    shuffled = [a[torch.randperm(a.shape[0], device="cuda", generator=gen)].contiguous() for a in dev]
    assert not torch.equal(shuffled[0], dev[0])
    assert_same_bits(d, device_bpg_from_edges(None, types, 7, *shuffled, degree_cap=cap))


def test_ids_above_16_bits_take_the_longer_radix_sort():
    """Above 65 536 products the workgroup paths sort in four digit passes instead of two: an LDS-path row and a row sorted
    between the global buffers whose targets span the whole id range, among short rows."""
    from p_companion_amd.data import IntBPG, device_bpg_from_edges
    P = 200_000
    rng = np.random.default_rng(9)
    hub = lambda s, n: np.stack([np.full(n, s), rng.integers(0, P, n)], 1)
    short = np.stack([rng.integers(0, P, 30_000), rng.integers(0, P, 30_000)], 1)
    cv = np.concatenate([hub(17, 6000), hub(199_999, 1500), hub(17, 500), short, short[:3000]]).astype(np.int32)
    pv = np.concatenate([cv[::3], hub(199_999, 5000)]).astype(np.int32)
    cp = np.concatenate([cv[::5], hub(17, 4500), hub(70_000, 200)]).astype(np.int32)
    types = (np.arange(P) % 11).astype(np.int32)
    host = IntBPG.from_edges(None, types, cv, pv, cp, degree_cap=32)
    assert host.max_degree == 32 and host.cv_col.max() > 65_536
    assert_equal_to_host(device_bpg_from_edges(None, types, 11, cv, pv, cp, degree_cap=32), host)


def test_round_trip_through_the_generator():
    """The generator's similarity pairs are flagged co-view edges and its complements are never co-viewed, so its graph fed
    back as (co_view, purchase_after_view = sim_pairs, co_purchase = comp_pairs) is rebuilt: rows as sets (the generator's
    rows are unsorted), the similarity set and the complementary set."""
    from p_companion_amd.data import device_bpg_from_edges, generate_device_bpg
    P = 2000
    g = generate_device_bpg(P, 20, seed=3)
    a = g.arrays
    src = torch.repeat_interleave(torch.arange(P, dtype=torch.int32, device="cuda"), (a["cv_rowptr"][1:] - a["cv_rowptr"][:-1]).long())
    cv = torch.stack([src, a["cv_col"]], 1).contiguous()
    d = device_bpg_from_edges(a["features"], a["type_idx"], 20, cv, a["sim_pairs"].contiguous(), a["comp_pairs"].contiguous(),
                              degree_cap=32)
    assert torch.equal(d.arrays["cv_rowptr"], a["cv_rowptr"])
    rp, mine, theirs = a["cv_rowptr"].cpu().numpy(), d.arrays["cv_col"].cpu().numpy(), a["cv_col"].cpu().numpy()
    for i in range(P):
        row = mine[rp[i]:rp[i + 1]]
        assert np.all(np.diff(row) > 0) and np.array_equal(row, np.sort(theirs[rp[i]:rp[i + 1]])), i
    assert d.n_similarity_pairs == g.n_similarity_pairs
    assert _keys(d.arrays["sim_pairs"].cpu().numpy(), P) == _keys(a["sim_pairs"].cpu().numpy(), P)
    assert d.arrays["comp_pairs"].shape == a["comp_pairs"].shape
    assert _keys(d.arrays["comp_pairs"].cpu().numpy(), P) == _keys(a["comp_pairs"].cpu().numpy(), P)
    assert torch.equal(d.arrays["sim_rowptr"], a["sim_rowptr"]) and d.max_degree <= 32
    assert torch.equal(d.arrays["pair_deg"], a["pair_deg"])               # (both in source order)


def test_ids_outside_the_catalogue_raise_and_the_device_stays_usable():
    from p_companion_amd.data import device_bpg_from_edges
    lists = dict(co_view=HAND_CV, purchase_after_view=HAND_PV, co_purchase=HAND_CP)
    for name in lists:
        for bad in ((3, 12), (12, 3), (-1, 3), (3, -1), (2 ** 31 - 1, 0)):
            kw = dict(lists)
            kw[name] = np.concatenate([lists[name][:5], np.array([bad], np.int32), lists[name][5:]])
            with pytest.raises(ValueError, match=name) as err:
                device_bpg_from_edges(None, HAND_TYPES, 3, degree_cap=HAND_CAP, **kw)
            assert all(other not in str(err.value) for other in lists if other != name)
    both = dict(lists, co_view=np.concatenate([HAND_CV, np.array([(0, 12)], np.int32)]),
                co_purchase=np.concatenate([np.array([(-5, 1)], np.int32), HAND_CP]))
    with pytest.raises(ValueError, match="co_view, co_purchase"):
        device_bpg_from_edges(None, HAND_TYPES, 3, degree_cap=HAND_CAP, **both)
    with pytest.raises(ValueError, match="type ids"):
        device_bpg_from_edges(None, HAND_TYPES, 2, degree_cap=HAND_CAP, **lists)
    # a valid call afterwards, on the same device
    d = device_bpg_from_edges(None, HAND_TYPES, 3, degree_cap=HAND_CAP, **lists)
    check_against(HAND_EXPECT, d.to_host(), d.arrays["pair_deg"].cpu().numpy())


def test_existing_consumers_take_a_built_graph(golden_graph):
    from test_gpu_catalogue_eval import cfg
    from p_companion_amd.data import ComplementaryIndexDataset, SimilarityIndexLoader
    from p_companion_amd.inference import PCompanionInference
    from p_companion_amd.p_companion import PCompanion
    from p_companion_amd.product2vec import Product2Vec
    bpg = golden_graph
    # ---- one epoch of the throughput loader, one fused Product2Vec step
    assert SimilarityIndexLoader(bpg, 256).drop_last is False             # the default keeps the short batch: 12 batches
    ld = SimilarityIndexLoader(bpg, 256, seed=3, drop_last=True)
    assert len(ld) == 2949 // 256 == 11
    batches = list(ld)
    assert len(batches) == 11 and all(b["anchor_idx"].shape[0] == 256 for b in batches)
    c = cfg(20, 128)
    torch.manual_seed(0)
    loss = Product2Vec(c).cuda().train().train_step_indexed(bpg.cuda()["features"], batches[0])
    assert torch.isfinite(loss).all()
    # ---- the labelled pairs' 80 / 10 / 10 split
    n = 2949 + 4523
    assert n == 7472
    want = {"train": int(0.8 * n), "val": int(0.9 * n) - int(0.8 * n), "test": n - int(0.9 * n)}
    for mode, size in want.items():
        assert len(ComplementaryIndexDataset(bpg, mode, seed=1)) == size, mode
    # ---- serving with the graph's own exclusions: no co-viewed product, never the query itself
    table = torch.randn(1000, 128, generator=torch.Generator().manual_seed(11))
    inf = PCompanionInference(PCompanion(c, table), c, bpg).set_exclusions()
    q = torch.arange(0, 1000, 7, dtype=torch.int32)
    types, idx, scores = inf.recommend_batch(q, 10)
    idx = idx.cpu().numpy()
    assert idx.shape == (len(q), 3, 10) and (idx >= 0).any()
    rp, col = bpg.arrays["cv_rowptr"].cpu().numpy(), bpg.arrays["cv_col"].cpu().numpy()
    for b, query in enumerate(q.tolist()):
        out = set(col[rp[query]:rp[query + 1]].tolist()) | {query}
        assert not set(idx[b].reshape(-1).tolist()) & out, query
