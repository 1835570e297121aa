"""Substitutes and evaluation from the bf16 copy of the catalogue alone: ops.half_sq_norm_bias_bf16,
ops.retrieve_list_grouped_bf16_biased, inference.CompactSimilarProducts and inference.CompactInference.  Needs an MI355X.

The fixtures, the float64 reference over the ROUNDED table and the allowance a(r, p) = (3 D + 4) 2^-24 (sum_d |q_d e_pd| + |b_p|)
are tests/test_gpu_rank_bf16.py's.  Where a bit-for-bit comparison with the fp32 classes is made the table holds small integers:
bf16 represents it exactly AND every partial sum of both score chains is exact, so the two chains -- whose summation orders
differ -- give the same bits, and with them the same order."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_nearest import as_csr, dev, ordered
from test_gpu_rank_bf16 import LIST_LENGTHS, N, SLICES, exact, exclusion_lists, mixed, serve, view     # noqa: F401 (fixtures)


def bits(t):
    return t.view(torch.int32)


def same(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(bits(a[1]), bits(b[1]))


# ---- the bias kernel
@pytest.mark.parametrize("dim", [128, 256])
def test_half_sq_norm_bias_bf16_is_the_fp32_kernel_on_the_widened_table(dim):
    from p_companion_amd import ops
    table = torch.from_numpy(np.random.default_rng(dim).standard_normal((1000, dim)).astype(np.float32)).cuda().to(torch.bfloat16)
    for P in (1, 15, 16, 17, 1000):
        t = table[:P].contiguous()
        got = ops.half_sq_norm_bias_bf16(t)
        assert got.dtype == torch.float32 and tuple(got.shape) == (P,)
        assert torch.equal(bits(got), bits(ops.half_sq_norm_bias(t.float()))), P
    z = torch.zeros(3, dim, device="cuda", dtype=torch.bfloat16)
    z[1, dim - 1] = 3.0
    assert ops.half_sq_norm_bias_bf16(z).cpu().tolist() == [0.0, -4.5, 0.0]
    with pytest.raises(ValueError, match="half_sq_norm_bias"):
        ops.half_sq_norm_bias_bf16(table.float())


# ---- the biased bf16 list
def keyed(m, seed):
    lists = exclusion_lists(m, seed)
    return lists, (torch.arange(len(m.types), dtype=torch.int32, device="cuda"),) + as_csr(lists)


@pytest.mark.parametrize("n", [1, 16, 17, 64, 65, 255, 256])
def test_the_biased_bf16_list(mixed, n):
    from p_companion_amd import ops
    m = mixed
    zero = torch.zeros(m.P, device="cuda")
    rowptr, col = m.rowptr.cpu().numpy(), m.col.cpu().numpy().copy()
    rng = np.random.default_rng(5)
    for t in range(m.T):
        rng.shuffle(col[rowptr[t]:rowptr[t + 1]])
    shuffled = dev(col)
    lists, triple = keyed(m, 17)
    for exclude in (None, triple):
        run = lambda bias, s=0, c=m.col: ops.retrieve_list_grouped_bf16_biased(m.dproj, m.dtypes, m.rowptr, c, m.table, bias, n,
                                                                                slices=s, exclude=exclude)
        plain = ops.retrieve_list_grouped(m.dproj, m.dtypes, m.rowptr, m.col, m.table, n, exclude=exclude)
        # a zero bias: the bf16 list, bit for bit
        assert same(run(zero), plain)
        # the same bits for every slices and candidate order
        for kind in ("random", "half_norm"):
            first = run(m.bias[kind])
            assert first[0].dtype == torch.int32 and first[1].dtype == torch.float32 and tuple(first[0].shape) == (len(m.types), n)
            for s in SLICES:
                assert same(run(m.bias[kind], s), first), (kind, s)
            assert same(run(m.bias[kind], 0, shuffled), first), kind
        # s = fl(d + b) in fp32, on every row of the full catalogue -- type 0 in its many chunks and slices included
        for kind in ("random", "half_norm"):
            one_addition_on_the_full_catalogue(m, kind, n, lists if exclude is not None else None, exclude)


def one_addition_on_the_full_catalogue(m, kind, n, lists, exclude):
    """s(r, p) = fl(d(r, p) + bias[p]) bit for bit for EVERY product the biased list serves over the full catalogue, whatever
    the size of its type.  d(r, p) comes from the unbiased bf16 list over a CSR of one type per row that holds exactly the
    products the biased list served that row (at most 256, so the unbiased list returns them all): the bits of a (row,
    product) chain do not depend on the row's tile, the product's chunk or the slices (the unbiased entry's own tests), so this
    is the d the biased kernel formed in type 0's many chunks.  An accumulator that started at the bias, or a second rounding,
    fails here on the large types too.  Every row must serve min(n, what the row's lists leave of its type) products."""
    from p_companion_amd import ops
    bias, hb = m.bias[kind], m.hbias[kind]
    s_i, s_s = (x.cpu().numpy() for x in ops.retrieve_list_grouped_bf16_biased(m.dproj, m.dtypes, m.rowptr, m.col, m.table, bias, n,
                                                                                exclude=exclude))
    rows = sorted(m.where)
    want_k = []
    for r in rows:
        cand = m.per_type[m.where[r][0]][0]
        left = len(cand) if lists is None else int((~np.isin(cand, lists[r])).sum())
        want_k.append(min(n, left))
        assert (s_i[r, :want_k[-1]] >= 0).all() and (s_i[r, want_k[-1]:] == -1).all(), r
    live = [(r, k) for r, k in zip(rows, want_k) if k]
    own = [np.sort(s_i[r, :k]) for r, k in live]
    rowptr = dev(np.concatenate([[0], np.cumsum([len(x) for x in own])]).astype(np.int32))
    col = dev(np.concatenate(own).astype(np.int32))
    proj = m.dproj[torch.tensor([r for r, _ in live], device="cuda")].contiguous()
    d_i, d_s = (x.cpu().numpy() for x in ops.retrieve_list_grouped(proj, torch.arange(len(live), dtype=torch.int32, device="cuda"),
                                                                    rowptr, col, m.table, N))
    seen = heavy = 0
    for j, (r, k) in enumerate(live):
        assert sorted(d_i[j, :k].tolist()) == own[j].tolist() and (d_i[j, k:] == -1).all(), r
        d = dict(zip(d_i[j, :k].tolist(), d_s[j, :k]))
        want = np.array([np.float32(d[p]) + hb[p] for p in s_i[r, :k]], np.float32)
        assert (s_s[r, :k].view(np.int32) == want.view(np.int32)).all(), (kind, n, r)
        seen += k
        heavy += k if m.types[r] == 0 else 0
    # every row of the many-chunk type serves a full list, and they are most of what is checked
    assert heavy == n * int((m.types == 0).sum()) and seen == sum(want_k) and int((m.types == 0).sum()) >= 50


@pytest.mark.parametrize("kind", ["random", "half_norm"])
def test_the_score_is_one_fp32_addition_after_the_list_chain(mixed, kind):
    """tests/test_gpu_nearest_list.py's form of the check: s = fl(d + b) bit for bit with d read from the unbiased bf16 list of
    the SAME call shape, plain and excluding, where both lists hold every candidate -- every type of at most 256 products, and
    type 0 cut to 256 products in the CSR (four chunks; its rows fill several 16-row tiles)."""
    from p_companion_amd import ops
    m = mixed
    rowptr, col = m.rowptr.cpu().numpy().copy(), m.col.cpu().numpy().copy()
    cut = rowptr[1] - N
    assert cut > 0
    col = np.concatenate([col[:N], col[rowptr[1]:]])
    rowptr[1:] -= cut
    kept0 = np.sort(col[:N])
    rowptr, col = dev(rowptr.astype(np.int32)), dev(col.astype(np.int32))
    hb = m.hbias[kind]
    lists, exclude = keyed(m, 23)
    n0 = int((m.types == 0).sum())
    for ls, ex in ((None, None), (lists, exclude)):
        d_i, d_s = (x.cpu().numpy() for x in ops.retrieve_list_grouped(m.dproj, m.dtypes, rowptr, col, m.table, N, exclude=ex))
        s_i, s_s = (x.cpu().numpy() for x in ops.retrieve_list_grouped_bf16_biased(m.dproj, m.dtypes, rowptr, col, m.table,
                                                                                    m.bias[kind], N, exclude=ex))
        seen = 0
        for r, (t, _) in m.where.items():
            cand = kept0 if t == 0 else m.per_type[t][0]
            if len(cand) > N:
                continue
            if ls is not None:
                cand = cand[~np.isin(cand, ls[r])]
            k = len(cand)
            assert sorted(d_i[r, :k].tolist()) == sorted(s_i[r, :k].tolist()) == cand.tolist(), r
            assert (s_i[r, k:] == -1).all() and np.isneginf(s_s[r, k:]).all(), r
            d = dict(zip(d_i[r, :k].tolist(), d_s[r, :k]))
            want = np.array([np.float32(d[p]) + hb[p] for p in s_i[r, :k]], np.float32)
            assert (s_s[r, :k].view(np.int32) == want.view(np.int32)).all(), r
            seen += k
        # the rows of the cut type alone: at least three 16-row tiles of full (or, excluding, nearly full) lists
        assert n0 >= 3 * 16 + 1 and seen >= (N - max(LIST_LENGTHS) - 1) * n0


def test_integer_data_equals_the_fp32_biased_list_bit_for_bit(exact):
    from p_companion_amd import ops
    m = exact
    ib = np.random.default_rng(4).integers(-50, 51, m.P).astype(np.float32)
    ib[[3, 5, 9]] = 7.0                                       # the copied rows stay tied
    wide = m.table.float()
    for bias in (dev(ib), ops.half_sq_norm_bias_bf16(m.table)):
        for exclude in (None, keyed(m, 18)[1]):
            for n in (1, 16, 17, 64, 65, 255, 256):
                got = ops.retrieve_list_grouped_bf16_biased(m.dproj, m.dtypes, m.rowptr, m.col, m.table, bias, n, exclude=exclude)
                want = ops.retrieve_list_grouped_biased(m.dproj, m.dtypes, m.rowptr, m.col, wide, bias, n, exclude=exclude)
                assert same(got, want), n


def check_band(m, idx, sc, hbias, n, lists=None):
    """tests/test_gpu_nearest.py's check_biased under the allowance a: every score within a of float64; an index that differs
    from the reference's at its rank only where the two float64 scores lie within the sum of the two allowances; equal
    scores in ascending product order; -1 / -inf past the end."""
    for r in range(len(m.types)):
        cand, s64, a = view(m, r, hbias)
        if lists is not None and len(lists[r]):
            keep = ~np.isin(cand, lists[r])
            cand, s64, a = cand[keep], s64[keep], a[keep]
        o = ordered(cand, s64)[:n]
        k = len(o)
        assert (idx[r, k:] == -1).all() and np.isneginf(sc[r, k:]).all(), r
        got = idx[r, :k]
        assert len(set(got.tolist())) == k and np.isin(got, cand).all(), r
        pos = np.searchsorted(cand, got)
        err = np.abs(sc[r, :k].astype(np.float64) - s64[pos])
        assert (err <= a[pos]).all(), f"row {r}: score error {err.max():.3e} above the allowance"
        diff = got != cand[o]
        if diff.any():
            gap = np.abs(s64[pos][diff] - s64[o][diff])
            assert (gap <= a[pos][diff] + a[o][diff]).all(), f"row {r}: index mismatch, float64 gap {gap.max():.3e}"
        if k > 1:
            tie = sc[r, 1:k] == sc[r, :k - 1]
            assert (got[1:][tie] > got[:-1][tie]).all(), f"row {r}: equal scores not in ascending product order"


@pytest.mark.parametrize("kind", ["random", "half_norm"])
def test_the_list_of_200_against_float64(mixed, kind):
    m = mixed
    lists, exclude = keyed(m, 19)
    for ls, ex in ((None, None), (lists, exclude)):
        idx, sc = serve(m, m.bias[kind], 200, exclude=ex)
        check_band(m, idx, sc, m.hbias[kind], 200, ls)


# ---- CompactSimilarProducts
@pytest.fixture(scope="module")
def graph():
    from p_companion_amd.data import generate_device_bpg
    bpg = generate_device_bpg(4_000, 20, seed=3, world=1, with_complementary=False)
    g = bpg.cuda()
    rng = np.random.default_rng(1)
    q = rng.choice(bpg.num_products, 256, replace=False).astype(np.int32)
    integers = torch.from_numpy(rng.integers(-4, 5, (4_000, 128)).astype(np.float32)).cuda()
    group = torch.from_numpy(rng.integers(-1, 300, 4_000).astype(np.int32)).cuda()
    return SimpleNamespace(bpg=bpg, features=g["features"], type_idx=g["type_idx"].cpu().numpy(), q=torch.from_numpy(q),
                           integers=integers, group=group)


def both(a, b):
    return torch.equal(a[0], b[0]) and torch.equal(bits(a[1]), bits(b[1]))


@pytest.mark.parametrize("scope", ["type", "catalogue"])
def test_compact_similar_products_equals_the_fp32_class_on_an_exact_table(graph, scope):
    from p_companion_amd import ops
    from p_companion_amd.inference import CompactSimilarProducts, SimilarProducts
    c = graph
    P = c.bpg.num_products
    ref = SimilarProducts(c.integers, c.bpg, scope=scope)
    cc = ops.CompactCatalogue(c.integers)
    sp = CompactSimilarProducts(cc, c.bpg, scope=scope)
    assert sp.table is cc.table and sp.table.dtype == torch.bfloat16 and sp.bias is cc.half_sq_norm
    assert torch.equal(bits(sp.bias), bits(ref.bias))
    assert CompactSimilarProducts(cc.table, c.bpg, scope=scope).table is cc.table          # a bf16 tensor is taken as it is
    rng = np.random.default_rng(5)
    pairs = np.stack([rng.integers(0, P, 3000), rng.integers(0, P, 3000)], 1).astype(np.int32)
    near, _ = ref.similar_list_batch(c.q, 40)
    pairs[:2560, 0], pairs[:2560, 1] = np.repeat(c.q.numpy()[:64], 40), near[:64].cpu().numpy().reshape(-1)
    mask = torch.from_numpy(rng.random(P) < 0.7).cuda()
    for eligible in (None, mask):
        ref.set_eligible(eligible)
        sp.set_eligible(eligible)
        for n in (1, 10, 16):
            assert both(sp.similar_batch(c.q, n), ref.similar_batch(c.q, n)), n
            assert both(sp.similar_capped_batch(c.q, n, c.group, cap=2), ref.similar_capped_batch(c.q, n, c.group, cap=2)), n
        for n in (16, 17, 100, 256):
            assert both(sp.similar_list_batch(c.q, n), ref.similar_list_batch(c.q, n)), n
        assert both(sp.similar_capped_list_batch(c.q, 20, c.group, cap=1, pool=200),
                    ref.similar_capped_list_batch(c.q, 20, c.group, cap=1, pool=200))
        a, b = (torch.from_numpy(np.ascontiguousarray(pairs[:, j])) for j in (0, 1))
        got, want = sp.rank_pairs(a, b), ref.rank_pairs(a, b)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        assert (got[1] >= 0).sum() > 500
        assert sp.evaluate_pairs(pairs, chunk=1000) == ref.evaluate_pairs(pairs, chunk=1000)
    sp.set_exclusions(False)
    ref.set_exclusions(False)
    assert both(sp.similar_list_batch(c.q, 30), ref.similar_list_batch(c.q, 30))
    got, want = sp.rank_pairs(a, b), ref.rank_pairs(a, b)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    with pytest.raises(ValueError, match="16"):
        sp.similar_batch(c.q, 17)
    with pytest.raises(ValueError, match="256"):
        sp.similar_list_batch(c.q, 257)


@pytest.mark.parametrize("scope", ["type", "catalogue"])
def test_compact_similar_products_on_a_rounded_table(graph, scope):
    """The float64 L2 order over the ROUNDED rows, up to pairs inside the allowance; rank < n exactly where the list holds the
    target; the capped methods are ops.cap_lists on the object's own pool."""
    from p_companion_amd import ops
    from p_companion_amd.inference import CompactSimilarProducts
    c = graph
    sp = CompactSimilarProducts(ops.CompactCatalogue(c.features), c.bpg, scope=scope)
    assert not hasattr(sp, "features")
    n, P = 50, c.bpg.num_products
    f64 = sp.table.float().cpu().numpy().astype(np.float64)
    D = f64.shape[1]
    assert not np.array_equal(f64, c.features.cpu().numpy().astype(np.float64))    # (the table is not representable)
    idx, dist = sp.similar_list_batch(c.q, n)
    assert idx.dtype == torch.int32 and dist.dtype == torch.float32 and tuple(idx.shape) == tuple(dist.shape) == (len(c.q), n)
    h_idx, h_dist = idx.cpu().numpy(), dist.cpu().numpy()
    b64 = sp.bias.cpu().numpy().astype(np.float64)
    q = c.q.numpy()
    assert (h_idx != q[:, None]).all() and (h_idx >= 0).all()
    for j, qi in enumerate(q):
        cand = np.nonzero(c.type_idx == c.type_idx[qi])[0] if scope == "type" else np.arange(P)
        cand = cand[cand != qi]
        s64 = f64[cand] @ f64[qi] + b64[cand]
        a = (3 * D + 4) * 2.0 ** -24 * (np.abs(f64[cand]) @ np.abs(f64[qi]) + np.abs(b64[cand]))
        o = ordered(cand, s64)[:n]
        got = h_idx[j]
        assert np.isin(got, cand).all() and len(set(got.tolist())) == n
        pos = np.searchsorted(cand, got)
        diff = got != cand[o]
        assert (np.abs(s64[pos][diff] - s64[o][diff]) <= a[pos][diff] + a[o][diff]).all(), j
        d64 = np.sqrt(((f64[qi][None, :] - f64[got] + 1e-6) ** 2).sum(1))
        np.testing.assert_allclose(h_dist[j], d64, rtol=1e-4, atol=0)
    # similar_batch is the list's head, bit for bit (one entry serves every n)
    assert both(sp.similar_batch(c.q, 16), (idx[:, :16].contiguous(), dist[:, :16].contiguous()))
    # rank_pairs against similar_list_batch: the served products stand at their positions; others are past the list
    anchors = torch.from_numpy(np.repeat(q[:64], n))
    slot, rank = sp.rank_pairs(anchors, torch.from_numpy(h_idx[:64].reshape(-1).copy()))
    assert (slot.cpu().numpy() == 0).all() and (rank.cpu().numpy().reshape(64, n) == np.arange(n)[None, :]).all()
    rng = np.random.default_rng(9)
    tg = np.array([rng.choice(np.nonzero(c.type_idx == c.type_idx[qi])[0]) for qi in q], np.int32)
    slot, rank = (x.cpu().numpy() for x in sp.rank_pairs(c.q, torch.from_numpy(tg)))
    for j in range(len(q)):
        if tg[j] == q[j]:
            assert rank[j] == -1
        elif rank[j] < n:
            assert h_idx[j, rank[j]] == tg[j], j
        else:
            assert tg[j] not in h_idx[j], j
    assert (rank >= n).sum() > 20
    slot, rank = sp.rank_pairs(c.q, c.q)                      # the query itself: excluded by default
    assert (slot.cpu().numpy() == 0).all() and (rank.cpu().numpy() == -1).all()
    # the capped methods: ops.cap_lists on the object's own pool
    ban = c.group[c.q.cuda().long()].contiguous()
    p_idx, p_dist = sp.similar_list_batch(c.q, 120)
    w_idx, w_near = ops.cap_lists(p_idx, -p_dist, 20, c.group, 2, row_ban=ban)
    assert both(sp.similar_capped_list_batch(c.q, 20, c.group, cap=2, pool=120), (w_idx, -w_near))
    p_idx, p_dist = sp.similar_batch(c.q, 16)
    w_idx, w_near = ops.cap_lists(p_idx, -p_dist, 8, c.group, 1, row_ban=None)
    assert both(sp.similar_capped_batch(c.q, 8, c.group, cap=1, own_group=True), (w_idx, -w_near))


# ---- CompactInference
def test_compact_inference_ranks_what_it_serves():
    from test_gpu_catalogue_eval import SEED, cfg
    from p_companion_amd import ops
    from p_companion_amd.data import ComplementaryIndexDataset, DeviceBPG, generate_device_bpg
    from p_companion_amd.inference import CompactInference, PCompanionInference
    from p_companion_amd.p_companion import PCompanion
    dim, products, T = 128, 8_000, 20
    bpg = generate_device_bpg(products, T, seed=3, dim=dim)
    c = cfg(T, dim)
    torch.manual_seed(0)
    model = PCompanion(c, torch.randn(products, dim, generator=torch.Generator().manual_seed(11)))
    no_feat = DeviceBPG({k: v for k, v in bpg.arrays.items() if k != "features"}, bpg.n_types, bpg.dim)
    cc = ops.CompactCatalogue(bpg.arrays["features"])
    # (the dataset of held-out pairs is built over a graph WITH features, and evaluate_catalogue wants its own graph: the
    # object over the full graph evaluates, its twin over the graph without features shows that none are read)
    inf = CompactInference(model, c, bpg, catalogue=cc)
    bare = CompactInference(model, c, no_feat, catalogue=cc)
    for x in (inf, bare):
        assert x.features is None and x.catalogue is cc.table and x.compact is cc
    with pytest.raises(ValueError, match="fp32 catalogue"):    # the parent's refusal stands
        PCompanionInference(model, c, no_feat, catalogue=cc).rank_targets(torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32))
    q = torch.arange(0, products, 11, dtype=torch.int32)[:512]
    b, k = len(q), c.NUM_COMP_TYPES
    mask = torch.rand(products, generator=torch.Generator().manual_seed(5)).cuda() < 0.7
    ds = ComplementaryIndexDataset(bpg, "test", seed=SEED)
    rng = np.random.default_rng(2)
    for situation in ("plain", "both"):
        if situation == "both":
            for x in (inf, bare):
                x.set_exclusions()
                x.set_eligible(mask)
        types, idx, _ = inf.recommend_batch(q, N)
        types, idx = types.cpu().numpy(), idx.cpu().numpy()
        # targets: a product of a served list (any position), any product of a predicted type, any product at all
        tg = np.zeros(b, np.int32)
        type_idx = inf.type_idx.cpu().numpy()
        for j in range(b):
            s = rng.integers(0, k)
            have = (idx[j, s] >= 0).sum()
            if j % 3 == 0 and have:
                tg[j] = idx[j, s, rng.integers(0, have)]
            elif j % 3 == 1:
                tg[j] = rng.choice(np.nonzero(type_idx == types[j, s])[0])
            else:
                tg[j] = rng.integers(0, products)
        slot, rank = inf.rank_targets(q, torch.from_numpy(tg))
        assert all(torch.equal(u, v) for u, v in zip(bare.rank_targets(q, torch.from_numpy(tg)), (slot, rank)))
        slot, rank = slot.cpu().numpy(), rank.cpu().numpy()
        below = past = 0
        for j in range(b):
            hit = np.nonzero(types[j] == type_idx[tg[j]])[0]
            assert slot[j] == (hit[0] if len(hit) else -1), j
            if slot[j] < 0:
                assert rank[j] == -1, j
            elif 0 <= rank[j] < N:
                assert idx[j, slot[j], rank[j]] == tg[j], j
                below += 1
            else:
                assert tg[j] not in idx[j, slot[j]], j                           # past the list, or kept out (-1)
                past += 1
        assert below > 100 and past > 20, (situation, below, past)
        # evaluate_catalogue: hit@k is the share counted from recommend_batch(q, k) directly
        res = inf.evaluate_catalogue(ds, ks=(10, 100), chunk=4096)
        pairs = ds.pairs[ds.pairs[:, 2] == 1]
        for kk in (10, 100):
            hits = 0
            for lo in range(0, pairs.shape[0], 4096):
                _, lists, _ = inf.recommend_batch(pairs[lo:lo + 4096, 0].contiguous(), kk)
                hits += int((lists == pairs[lo:lo + 4096, 1][:, None, None]).any(2).any(1).sum())
            assert res[f"hit@{kk}"] == hits / pairs.shape[0], (situation, kk)
        assert res["pairs"] == pairs.shape[0] and res["hit@100"] > 0
