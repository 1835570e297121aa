"""Group caps and the merged page: pc_cap_lists / ops.cap_lists (at most `cap` products of one product group among the first n
of a pool, on the device), PCompanionInference.recommend_capped_batch / recommend_page_batch and
SimilarProducts.similar_capped_batch.

One reference: the rule restated in numpy (oracle below) -- filter the candidates, np.lexsort((id, -score)), count per group.
The kernel compares integers and floats and copies bits, so every comparison here is bit for bit; nothing is tolerated.
Needs an MI355X."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

P, R = 1000, 37
POOLS = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256)        # both sort widths (2 and 4 slots per lane) and their edges
INT32_MIN = -2 ** 31


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(sc):
    return sc.contiguous().view(torch.int32)


def same(got, want):
    return torch.equal(got[0], want[0]) and torch.equal(bits(got[1]), bits(want[1]))


def oracle(idx, score, n, group=None, cap=1, row_ban=None, num_products=None):
    """The contract: (ids [R, n] int32, scores [R, n] fp32 with the input bits)."""
    p = 2 ** 31 - 1 if group is None else len(group) if num_products is None else num_products
    out_i = np.full((idx.shape[0], n), -1, np.int32)
    out_s = np.full((idx.shape[0], n), -np.inf, np.float32)
    for r in range(idx.shape[0]):
        ok = (idx[r] >= 0) & (idx[r] < p) & np.isfinite(score[r])
        ids, sc = idx[r][ok].astype(np.int64), score[r][ok]
        g = group[ids] if group is not None else np.full(len(ids), -1)
        if row_ban is not None and row_ban[r] >= 0:
            ids, sc, g = ids[g != row_ban[r]], sc[g != row_ban[r]], g[g != row_ban[r]]
        room, k = {}, 0
        for j in np.lexsort((ids, -sc)):                  # score descending, product index ascending
            if g[j] >= 0:
                if room.get(g[j], 0) >= cap:
                    continue
                room[g[j]] = room.get(g[j], 0) + 1
            if k < n:
                out_i[r, k], out_s[r, k] = ids[j], sc[j]
                k += 1
    return out_i, out_s


def check(idx, score, n, group=None, cap=1, row_ban=None, want=None, **kw):
    """ops.cap_lists against the oracle (or `want`, an oracle run with n = m whose first n columns are this call's)."""
    from p_companion_amd import ops
    got = ops.cap_lists(cuda(idx), cuda(score), n, None if group is None else cuda(group), cap,
                        None if row_ban is None else cuda(row_ban), **kw)
    assert got[0].shape == (idx.shape[0], n) and got[0].dtype == torch.int32 and got[1].dtype == torch.float32
    if want is None:
        want = oracle(idx, score, n, group, cap, row_ban)
    assert same(got, (cuda(want[0][:, :n]), cuda(want[1][:, :n]))), (idx.shape, n, cap)
    return got


def make_pool(rng, rows, m, holes=True):
    """Distinct ids per row, scores from {k / 4: |k| <= 8} with both zeros; a fifth of the slots is no candidate."""
    idx = np.stack([rng.permutation(P)[:m] for _ in range(rows)]).astype(np.int32)
    k = rng.integers(-8, 9, (rows, m))
    score = (k / 4).astype(np.float32)
    score[(k == 0) & (rng.random((rows, m)) < 0.5)] = -0.0
    if holes:
        kind = rng.integers(0, 4, (rows, m))
        hole = rng.random((rows, m)) < 0.2
        idx[hole & (kind == 0)] = -1
        score[hole & (kind == 1)] = -np.inf
        score[hole & (kind == 2)] = np.inf
        score[hole & (kind == 3)] = np.nan
    return idx, score


def group_cases(rng):
    mixed = (np.arange(P) % 7).astype(np.int32)
    mixed[rng.random(P) < 0.2] = -1
    mixed[rng.random(P) < 0.02] = -5                      # (any negative entry is "ungrouped")
    return {"one": np.zeros(P, np.int32),
            "distinct": (np.arange(P) + (2 ** 31 - 1 - P)).astype(np.int32),      # ids are only compared: up to INT32_MAX
            "none": np.full(P, -1, np.int32),
            "mod7": mixed}


# ---- 1. every boundary of the variants
@pytest.mark.parametrize("m", POOLS)
def test_every_pool_length_list_length_cap_and_grouping_matches_the_oracle(m):
    rng = np.random.default_rng(100 + m)
    idx, score = make_pool(rng, R, m)
    if m >= 63:
        assert np.signbit(score[score == 0]).any() and not np.signbit(score[score == 0]).all()       # both zeros
    for name, group in group_cases(rng).items():
        for cap in sorted({1, 2, m}):
            full = oracle(idx, score, m, group, cap)      # once per (group, cap): a shorter list is its prefix
            for n in sorted({1, min(10, m), m}):
                check(idx, score, n, group, cap, want=full)
    # without a group array: the sort alone (and the same with every product ungrouped)
    full = oracle(idx, score, m)
    for n in sorted({1, min(10, m), m}):
        got = check(idx, score, n, want=full)
        assert same(got, check(idx, score, n, np.full(P, -1, np.int32), 1, want=full))


# ---- 2. ids out of range
@pytest.mark.parametrize("m", (20, 200))
def test_bad_ids_are_counted_never_served_and_never_used(m):
    from p_companion_amd import ops
    rng = np.random.default_rng(7 + m)
    idx, score = make_pool(rng, R, m)
    group = group_cases(rng)["mod7"]
    planted = [P, P + 5, -2, INT32_MIN]
    for k, x in enumerate(planted):
        idx[3 + 2 * k, (5 * k) % m] = x
        score[3 + 2 * k, (5 * k) % m] = 2.0               # (the best score of its row, were it a candidate)
    idx[20, :4] = planted
    score[20, :4] = 2.0
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = check(idx, score, min(10, m), group, 2, bad=bad)
    assert int(bad) == 2 * len(planted)
    served = got[0].cpu().numpy()
    assert not np.isin(served, planted).any()
    # the counter is added to; without a counter the ids are passed over all the same
    assert same(check(idx, score, min(10, m), group, 2, bad=bad), got) and int(bad) == 4 * len(planted)
    assert same(check(idx, score, min(10, m), group, 2), got)
    # without groups every non-negative id is a candidate: only the negative ones are bad
    bad.zero_()
    want = oracle(idx, score, m)
    got = check(idx, score, m, bad=bad, want=want)
    assert int(bad) == 4 and np.isin(got[0].cpu().numpy(), [P, P + 5]).any()
    # a row's output does not depend on the other rows of the call
    whole = ops.cap_lists(cuda(idx), cuda(score), 5, cuda(group), 1)
    for lo, hi in ((0, 1), (3, 10), (R - 1, R)):
        part = ops.cap_lists(cuda(idx[lo:hi]), cuda(score[lo:hi]), 5, cuda(group), 1)
        assert same(part, (whole[0][lo:hi], whole[1][lo:hi]))


# ---- 3. bans
@pytest.mark.parametrize("m", (16, 100, 256))
def test_a_banned_group_is_never_served(m):
    rng = np.random.default_rng(31 + m)
    idx, score = make_pool(rng, R, m)
    group = group_cases(rng)["mod7"]
    ban = rng.integers(0, 7, R).astype(np.int32)
    ban[rng.random(R) < 0.4] = -1
    ban[1], ban[2] = -7, 2 ** 31 - 1                      # a negative entry bans nothing; a group nobody has
    assert (ban >= 0).any() and (ban < 0).any()
    for cap in (1, 3, m):
        got = check(idx, score, min(10, m), group, cap, ban)
        served = got[0].cpu().numpy()
        for r in range(R):
            ids = served[r][served[r] >= 0]
            assert ban[r] < 0 or not (group[ids] == ban[r]).any(), r
            grouped = group[ids][group[ids] >= 0]
            assert len(grouped) == 0 or np.bincount(grouped).max() <= cap
    # an all -1 ban is no ban
    assert same(check(idx, score, m, group, 2, np.full(R, -1, np.int32)), check(idx, score, m, group, 2))


# ---- 4. invariances
@pytest.mark.parametrize("m", (64, 128, 256))
def test_a_permutation_of_the_slots_and_a_second_call_change_no_bit(m):
    from p_companion_amd import ops
    rng = np.random.default_rng(50 + m)
    idx, score = make_pool(rng, R, m)
    group, ban = cuda(group_cases(rng)["mod7"]), cuda(rng.integers(-1, 7, R).astype(np.int32))
    d_idx, d_sc = cuda(idx), cuda(score)
    for n, cap in ((min(10, m), 1), (m, 2)):
        got = ops.cap_lists(d_idx, d_sc, n, group, cap, ban)
        assert same(ops.cap_lists(d_idx, d_sc, n, group, cap, ban), got)
        for _ in range(2):
            perm = torch.stack([torch.randperm(m, device="cuda") for _ in range(R)])
            assert same(ops.cap_lists(d_idx.gather(1, perm).contiguous(), d_sc.gather(1, perm).contiguous(), n, group, cap, ban),
                        got)


def test_the_two_sort_widths_agree_at_the_boundary():
    """A 128-slot pool goes through two slots per lane; the same pool with one -1 slot behind it through four."""
    from p_companion_amd import ops
    rng = np.random.default_rng(128)
    idx, score = make_pool(rng, R, 128)
    group = cuda(group_cases(rng)["mod7"])
    wide_i = np.concatenate([idx, np.full((R, 1), -1, np.int32)], 1)
    wide_s = np.concatenate([score, np.full((R, 1), 1.5, np.float32)], 1)
    for n, cap in ((1, 1), (10, 2), (128, 1), (128, 128)):
        narrow = ops.cap_lists(cuda(idx), cuda(score), n, group, cap)
        assert same(ops.cap_lists(cuda(wide_i), cuda(wide_s), n, group, cap), narrow), (n, cap)
        assert same(ops.cap_lists(cuda(idx), cuda(score), n), ops.cap_lists(cuda(wide_i), cuda(wide_s), n))


# ---- 5. identity: the first n of a grouped entry's own list
def test_a_retrieved_list_comes_back_as_its_own_first_n():
    from p_companion_amd import ops
    rng = np.random.default_rng(900)
    dim, sizes = 128, (400, 150, 50)                      # pools of 64: full, full, short
    table = rng.standard_normal((600, dim)).astype(np.float32)
    type_idx = rng.permutation(np.repeat(np.arange(3), sizes)).astype(np.int32)
    order = np.argsort(type_idx, kind="stable").astype(np.int32)
    rowptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    types = rng.permutation(np.repeat(np.arange(3), (25, 8, 4))).astype(np.int32)
    proj = rng.standard_normal((R, dim)).astype(np.float32)
    args = (cuda(proj), cuda(types), cuda(rowptr), cuda(order), cuda(table))
    pool = ops.retrieve_list_grouped(*args, 64)
    want = ops.retrieve_list_grouped(*args, 10)
    assert (pool[0] < 0).any()                            # (the short type leaves -1 slots in the pool)
    group = cuda((np.arange(600) % 5).astype(np.int32))
    assert same(ops.cap_lists(*pool, 10), want)
    assert same(ops.cap_lists(*pool, 10, group, 64), want)
    assert same(ops.cap_lists(*pool, 64), pool) and same(ops.cap_lists(*pool, 64, group, 64), pool)


# ---- 6. more rows than the grid holds at once, and none
def test_grid_stride_and_no_rows():
    from p_companion_amd import ops
    rows, m = 4 * 4096 + 5, 8
    rng = np.random.default_rng(4096)
    idx = rng.integers(0, P, (rows, m)).astype(np.int32)
    idx += (np.arange(m) * P).astype(np.int32)            # distinct within a row: slot j draws from [j P, (j + 1) P)
    k = rng.integers(-8, 9, (rows, m))
    score = (k / 4).astype(np.float32)
    idx[rng.random((rows, m)) < 0.2] = -1
    group = (np.arange(m * P) % 3).astype(np.int32)
    check(idx, score, 4, group, 1)
    check(idx, score, m, group, 2)
    e_i, e_s = ops.cap_lists(cuda(idx[:0]), cuda(score[:0]), 3, cuda(group), 1)
    assert e_i.shape == (0, 3) and e_i.dtype == torch.int32 and e_s.shape == (0, 3) and e_s.dtype == torch.float32


# ---- 7. through PCompanionInference
@pytest.fixture(scope="module")
def served():
    from types import SimpleNamespace
    from test_gpu_catalogue_eval import cfg
    from p_companion_amd.data import DeviceBPG, generate_scaled_bpg
    from p_companion_amd.inference import PCompanionInference
    from p_companion_amd.p_companion import PCompanion
    dim, products, n_types = 128, 2000, 8
    host = generate_scaled_bpg(products, n_types, seed=3, dim=dim)
    g = dict(host.cuda())
    g["comp_pairs"] = cuda(host.complementary_pairs.astype(np.int32))
    g["max_degree"] = int(np.diff(host.cv_rowptr).max())
    bpg = DeviceBPG(g, n_types, dim)
    c = cfg(n_types, dim)
    torch.manual_seed(0)
    model = PCompanion(c, torch.randn(products, dim, generator=torch.Generator().manual_seed(11)))
    inf = PCompanionInference(model, c, bpg)
    return SimpleNamespace(inf=inf, model=model, cfg=c, bpg=bpg, host=host, features=g["features"],
                           q=torch.arange(0, products, 41, dtype=torch.int32),
                           group=(torch.arange(products, dtype=torch.int32) % 8).cuda(),
                           mask=torch.rand(products, generator=torch.Generator().manual_seed(5)).cuda() < 0.7)


def most_of_a_group(idx, group):
    """the largest number of products of one group in any list of idx [..., n]"""
    idx = idx.reshape(-1, idx.shape[-1])
    g = torch.where(idx >= 0, group[idx.clamp(min=0).long()], -1)
    return int(((g[:, :, None] == g[:, None, :]) & (g[:, :, None] >= 0)).sum(2).max())


def test_recommend_capped_batch(served):
    from p_companion_amd import ops
    from p_companion_amd.inference import PCompanionInference
    s, q, group = served, served.q, served.group
    compact = PCompanionInference(s.model, s.cfg, s.bpg, catalogue=ops.CompactCatalogue(s.features))
    for inf, situation in ((s.inf, "plain"), (s.inf, "filtered"), (compact, "compact")):
        if situation == "filtered":
            inf.set_exclusions()
            inf.set_eligible(s.mask)
        types, p_idx, p_sc = inf.recommend_batch(q, 64)
        b, k, _ = p_idx.shape
        flat = (p_idx.reshape(b * k, 64), p_sc.reshape(b * k, 64))
        assert (p_idx >= 0).all()                         # full pools: 64 candidates over 8 groups, so the cap must bite
        got = inf.recommend_capped_batch(q, 10, group=group, cap=2)
        assert torch.equal(got[0], types) and got[1].shape == (b, k, 10)
        assert same((got[1].reshape(b * k, 10), got[2].reshape(b * k, 10)), ops.cap_lists(*flat, 10, group, 2)), situation
        assert most_of_a_group(got[1], group) == 2 and most_of_a_group(p_idx[:, :, :10], group) > 2
        plain = inf.recommend_batch(q, 10)
        assert not torch.equal(got[1], plain[1])
        assert (got[1] >= 0).all()                        # at most 16 survive, at least 10: the lists are full
        # a diversity: recommend_diverse_batch's re-rank over every kept product of the pool
        kept = ops.cap_lists(*flat, 64, group, 2)
        assert int((kept[0] >= 0).sum(1).max()) <= 16
        for sim in ("cosine", "dot"):
            if situation == "compact":
                ref = ops.diversify_lists_bf16(*kept, inf.catalogue, 10, 1.0 - 0.3,
                                               scale=inf.compact.inv_norm if sim == "cosine" else None)
            else:
                ref = ops.diversify_lists(*kept, inf.features, 10, 1.0 - 0.3,
                                          scale=ops.inv_norm(inf.features) if sim == "cosine" else None)
            div = inf.recommend_capped_batch(q, 10, group=group, cap=2, diversity=0.3, similarity=sim)
            assert torch.equal(div[0], types)
            assert same((div[1].reshape(b * k, 10), div[2].reshape(b * k, 10)), ref), (situation, sim)
            assert most_of_a_group(div[1], group) <= 2
        # no group: recommend_batch itself; and with a diversity recommend_diverse_batch itself
        none = inf.recommend_capped_batch(q, 10)
        assert torch.equal(none[0], plain[0]) and same(none[1:], plain[1:]), situation
        both = inf.recommend_capped_batch(q, 10, diversity=0.3)
        want = inf.recommend_diverse_batch(q, 10, pool=64, diversity=0.3)
        assert same(both[1:], want[1:]), situation
        if situation == "filtered":
            assert s.mask[got[1].long()].all()
            idx_h = got[1].cpu().numpy()
            for i, query in enumerate(q.tolist()):
                gone = set(s.host.cv_col[s.host.cv_rowptr[query]:s.host.cv_rowptr[query + 1]].tolist()) | {query}
                assert not set(idx_h[i].reshape(-1).tolist()) & gone, query
            inf.set_exclusions(False)
            inf.set_eligible(None)
    with pytest.raises(ValueError, match="one entry per product"):
        s.inf.recommend_capped_batch(q, 10, group=group[:-1].contiguous())


@pytest.mark.parametrize("per_type,n,cap", [(4, 10, 1), (8, 24, 2), (85, 40, 3)])
def test_recommend_page_batch(served, per_type, n, cap):
    s, q, group = served, served.q, served.group
    types, p_idx, p_sc = s.inf.recommend_batch(q, per_type)
    b, k, _ = p_idx.shape
    idx, sc, ptypes = s.inf.recommend_page_batch(q, n, per_type=per_type, group=group, cap=cap)
    assert idx.shape == (b, n) and idx.dtype == torch.int32 and sc.dtype == torch.float32 and ptypes.dtype == torch.int64
    want = oracle(p_idx.reshape(b, -1).cpu().numpy(), p_sc.reshape(b, -1).cpu().numpy(), n, group.cpu().numpy(), cap)
    assert same((idx, sc), (cuda(want[0]), cuda(want[1])))
    type_idx = s.inf.type_idx.long()
    assert torch.equal(ptypes, torch.where(idx >= 0, type_idx[idx.clamp(min=0).long()], -1))
    assert most_of_a_group(idx, group) <= cap
    assert most_of_a_group(idx, s.inf.type_idx) <= per_type
    for i in range(b):                                    # only the predicted types are on a query's page
        assert set(ptypes[i][ptypes[i] >= 0].tolist()) <= set(types[i].tolist())
    # without groups: the merge of the K lists alone
    idx0, sc0, _ = s.inf.recommend_page_batch(q, n, per_type=per_type)
    want = oracle(p_idx.reshape(b, -1).cpu().numpy(), p_sc.reshape(b, -1).cpu().numpy(), n)
    assert same((idx0, sc0), (cuda(want[0]), cuda(want[1])))


# ---- 8. substitutes
def test_similar_capped_batch():
    from p_companion_amd.data import generate_device_bpg
    from p_companion_amd.inference import IndexedSimilarProducts, SimilarProducts
    products, dim = 2000, 128
    bpg = generate_device_bpg(products, 8, seed=3, world=1, with_complementary=False)
    gen = torch.Generator().manual_seed(9)
    centres = torch.randn(products // 4, dim, generator=gen)
    table = (centres.repeat_interleave(4, dim=0) + 1e-3 * torch.randn(products, dim, generator=gen)).cuda().contiguous()
    group = (torch.arange(products, dtype=torch.int32) // 4).cuda()
    q = torch.arange(0, products, 37, dtype=torch.int32).cuda()
    own = group[q.long()]
    exact = SimilarProducts(table, bpg, scope="catalogue")
    indexed = IndexedSimilarProducts(table, bpg, n_cells=8, nprobe=8, iters=3, seed=1)
    for sp in (exact, indexed):
        p_idx, p_dist = sp.similar_batch(q, 16)
        assert (group[p_idx[:, :3].long()] == own[:, None]).all()       # the three copies come first
        idx, dist = sp.similar_capped_batch(q, 10, group=group)
        assert idx.shape == (len(q), 10) and idx.dtype == torch.int32 and dist.dtype == torch.float32
        g = torch.where(idx >= 0, group[idx.clamp(min=0).long()], -1)
        assert not (g == own[:, None]).any()              # none of the query's own variants
        assert most_of_a_group(idx, group) == 1           # one product per other group
        assert ((idx >= 0).sum(1) >= 4).all()             # 13 foreign neighbours of groups of four: at least four groups
        # the distances are those similar_batch reported for the same ids; +inf past the end
        at = (idx[:, :, None] == p_idx[:, None, :]) & (idx[:, :, None] >= 0)
        assert (at.sum(2) == (idx >= 0)).all()
        reported = torch.where(at, p_dist[:, None, :], 0).sum(2)
        assert torch.equal(bits(torch.where(idx >= 0, dist, 0)), bits(torch.where(idx >= 0, reported, 0)))
        assert torch.isposinf(dist[idx < 0]).all()
        # the rule, restated
        want = oracle(p_idx.cpu().numpy(), -p_dist.cpu().numpy(), 10, group.cpu().numpy(), 1, own.cpu().numpy())
        assert same((idx, -dist), (cuda(want[0]), cuda(want[1])))
        # own_group: the query's variants compete like any other group -- the two nearest of them lead the list
        idx_o, dist_o = sp.similar_capped_batch(q, 10, group=group, cap=2, own_group=True)
        want = oracle(p_idx.cpu().numpy(), -p_dist.cpu().numpy(), 10, group.cpu().numpy(), 2)
        assert same((idx_o, -dist_o), (cuda(want[0]), cuda(want[1])))
        assert (group[idx_o[:, :2].long()] == own[:, None]).all() and most_of_a_group(idx_o, group) == 2
        # no group: similar_batch's own first n
        idx_n, dist_n = sp.similar_capped_batch(q, 10)
        want = oracle(p_idx.cpu().numpy(), -p_dist.cpu().numpy(), 10)
        assert same((idx_n, -dist_n), (cuda(want[0]), cuda(want[1])))
    e_i, e_d = exact.similar_capped_batch(q[:0], 5, group=group)
    assert e_i.shape == (0, 5) and e_d.shape == (0, 5)
