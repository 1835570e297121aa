"""Basket recommendations: pc_fuse_lists / ops.fuse_lists (the lists of a basket's items fused into one list, on the device)
and PCompanionInference.recommend_basket_batch.

One reference: the contract restated in numpy (oracle below) -- filter the candidates, drop the ban set, per product id sort
the slot scores descending and add them as np.float32 one at a time, np.lexsort((id, -fused)).  The kernel copies score bits
or adds them in that pinned order, so every comparison here is bit for bit; nothing is tolerated.  Needs an MI355X."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

P, B = 1000, 37
EDGES = (1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024)      # 2 / 4 / 8 / 16 slots per lane
MIXED = {1: (1, 1), 2: (2, 1), 63: (3, 21), 64: (4, 16), 65: (5, 13), 127: (127, 1), 128: (8, 16), 129: (3, 43), 255: (5, 51),
         256: (16, 16), 257: (257, 1), 511: (7, 73), 512: (32, 16), 513: (27, 19), 1023: (11, 93), 1024: (16, 64)}
INT32_MIN = -2 ** 31


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(sc):
    return sc.contiguous().view(torch.int32)


def same(got, want):
    """(idx, score[, support]) tuples: equal ids, equal score BITS, equal supports"""
    return (len(got) == len(want) and torch.equal(got[0], want[0]) and torch.equal(bits(got[1]), bits(want[1]))
            and all(torch.equal(g, w) for g, w in zip(got[2:], want[2:])))


def oracle(idx, score, n, combine="sum", source=None, exclude=None, num_products=None):
    """The contract: (ids [B, n] int32, fused scores [B, n] fp32, supports [B, n] int32, the bad count)."""
    b, s, w = idx.shape
    p = num_products if num_products is not None else len(exclude[0]) - 1 if exclude is not None else 2 ** 31 - 1
    out_i = np.full((b, n), -1, np.int32)
    out_s = np.full((b, n), -np.inf, np.float32)
    out_c = np.zeros((b, n), np.int32)
    bad = int(((idx < -1) | (idx >= p)).sum())
    for r in range(b):
        src = np.zeros(s, np.int64) if source is None else source[r].astype(np.int64)
        bad += int(((src < -1) | (src >= p)).sum())
        live = (src >= 0) & (src < p)
        ban = set()
        if source is not None:
            ban = set(src[live].tolist())
            if exclude is not None:
                for q in src[live]:
                    ban |= set(exclude[1][exclude[0][q]:exclude[0][q + 1]].tolist())
        ok = (idx[r] >= 0) & (idx[r] < p) & np.isfinite(score[r]) & live[:, None]
        ids, sc = idx[r][ok].astype(np.int64), score[r][ok]
        fused = {}
        for i in np.unique(ids):
            if int(i) in ban:
                continue
            mine = sc[ids == i]
            mine = mine[np.lexsort((np.signbit(mine), -mine))]           # descending, +0.0 before -0.0
            f = np.float32(mine[0])
            if combine == "sum":
                for x in mine[1:]:
                    f = np.float32(f + np.float32(x))
            fused[int(i)] = (f, len(mine))
        keys = np.array(sorted(fused), np.int64)
        val = np.array([fused[i][0] for i in keys], np.float32)
        for k, j in enumerate(np.lexsort((keys, -val))[:n]):             # fused score descending, product index ascending
            out_i[r, k], out_s[r, k], out_c[r, k] = keys[j], val[j], fused[int(keys[j])][1]
    return out_i, out_s, out_c, bad


def fuse(idx, score, n, combine="sum", source=None, exclude=None, **kw):
    from p_companion_amd import ops
    got = ops.fuse_lists(cuda(idx), cuda(score), n, combine, None if source is None else cuda(source),
                         None if exclude is None else (cuda(exclude[0]), cuda(exclude[1])), **kw)
    assert [tuple(t.shape) for t in got] == [(idx.shape[0], n)] * 3
    assert [t.dtype for t in got] == [torch.int32, torch.float32, torch.int32]
    return got


def check(idx, score, n, combine="sum", source=None, exclude=None, want=None, **kw):
    """ops.fuse_lists against the oracle (or `want`, an oracle run with a longer n whose first n columns are this call's)."""
    got = fuse(idx, score, n, combine, source, exclude, **kw)
    if want is None:
        want = oracle(idx, score, n, combine, source, exclude, kw.get("num_products"))
    assert same(got, tuple(cuda(a[:, :n]) for a in want[:3])), (idx.shape, n, combine)
    return got


def make_pool(rng, b, s, w, ids=60, holes=True):
    """Ids drawn with replacement from a small range (most products repeat across a basket's rows), scores from
    {k / 4: |k| <= 8} with both zeros (sums are exact, ties are frequent: the id order decides); a fifth of the slots is no
    candidate."""
    idx = rng.integers(0, ids, (b, s, w)).astype(np.int32)
    k = rng.integers(-8, 9, (b, s, w))
    score = (k / 4).astype(np.float32)
    score[(k == 0) & (rng.random((b, s, w)) < 0.5)] = -0.0
    if holes:
        kind = rng.integers(0, 4, (b, s, w))
        hole = rng.random((b, s, w)) < 0.2
        idx[hole & (kind == 0)] = -1
        score[hole & (kind == 1)] = -np.inf
        score[hole & (kind == 2)] = np.inf
        score[hole & (kind == 3)] = np.nan
    return idx, score


def make_sources(rng, b, s, lo=500):
    """Basket members from [lo, P) (outside make_pool's ids; an item may be listed twice), a quarter of the rows padding."""
    source = rng.integers(lo, P, (b, s)).astype(np.int32)
    source[rng.random((b, s)) < 0.25] = -1
    return source


def make_exclusions(rng, per_key=6, ids=60):
    """A strictly ascending CSR over P keys whose rows name make_pool's ids."""
    rows = [np.sort(rng.choice(ids, rng.integers(0, min(per_key, ids) + 1), replace=False)) for _ in range(P)]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    return rowptr, np.concatenate(rows).astype(np.int32)


# ---- 1. every boundary of the variants, reached as one row, as one slot per row and as a mixed shape
@pytest.mark.parametrize("pool", EDGES)
def test_every_pool_edge_shape_list_length_and_combine_matches_the_oracle(pool):
    rng = np.random.default_rng(100 + pool)
    ids = max(4, min(60, pool // 3))
    ex = make_exclusions(rng, ids=ids // 2)               # (the sets name the lower half of the ids: the rest survives)
    for s, w in sorted({(1, pool), (pool, 1), MIXED[pool]}):
        assert s * w == pool
        idx, score = make_pool(rng, B, s, w, ids=ids)
        if pool >= 63:
            assert np.signbit(score[score == 0]).any() and not np.signbit(score[score == 0]).all()   # both zeros
        source = make_sources(rng, B, s)
        top = min(pool, 256)
        for combine in ("sum", "max"):
            plain = oracle(idx, score, top, combine)
            banned = oracle(idx, score, top, combine, source, ex)
            if pool >= 63:
                assert (plain[2] > 1).any() and (banned[0] >= 0).any() and not np.array_equal(plain[0], banned[0])
            for n in sorted({1, min(10, pool), top}):
                check(idx, score, n, combine, want=plain)
                check(idx, score, n, combine, source, ex, want=banned)


# ---- 2. the pinned order of the sum
def test_the_sum_adds_the_largest_first_under_every_permutation():
    big = np.float32(2 ** 24)
    assert np.float32(np.float32(big + np.float32(1)) + np.float32(1)) == big                        # descending: 2^24
    assert np.float32(np.float32(np.float32(1) + np.float32(1)) + big) == np.float32(2 ** 24 + 2)    # any other order ties
    rng = np.random.default_rng(24)
    for s, w in ((3, 2), (1, 6), (6, 1), (3, 50), (9, 100)):
        idx = np.full((B, s, w), -1, np.int32)
        score = np.zeros((B, s, w), np.float32)
        for r in range(B):
            at = rng.permutation(s * w)[:4]
            idx[r].reshape(-1)[at] = (7, 7, 7, 3)
            score[r].reshape(-1)[at] = (big, 1, 1, 2 ** 24 + 2)
        got = check(idx, score, 2)
        want = (cuda(np.tile(np.array([3, 7], np.int32), (B, 1))),
                cuda(np.tile(np.array([2 ** 24 + 2, 2 ** 24], np.float32), (B, 1))),
                cuda(np.tile(np.array([1, 3], np.int32), (B, 1))))
        assert same(got, want)
        got = check(idx, score, 2, "max")
        assert torch.equal(got[0], want[0]) and torch.equal(got[2], want[2]) and got[1][:, 1].eq(2 ** 24).all()


# ---- 3. invariances
@pytest.mark.parametrize("s,w", [(4, 24), (3, 85), (6, 80), (16, 48)])
def test_a_permutation_of_rows_or_slots_and_a_second_call_change_no_bit(s, w):
    from p_companion_amd import ops
    rng = np.random.default_rng(50 + s * w)
    idx, score = make_pool(rng, B, s, w)
    d_idx, d_sc, d_src = cuda(idx), cuda(score), cuda(make_sources(rng, B, s))
    ex = tuple(cuda(a) for a in make_exclusions(rng))
    for n, combine in ((10, "sum"), (min(s * w, 256), "sum"), (10, "max")):
        got = ops.fuse_lists(d_idx, d_sc, n, combine, d_src, ex)
        assert same(ops.fuse_lists(d_idx, d_sc, n, combine, d_src, ex), got)
        for _ in range(2):
            rows = torch.stack([torch.randperm(s, device="cuda") for _ in range(B)])
            slots = torch.stack([torch.randperm(w, device="cuda") for _ in range(B * s)]).reshape(B, s, w)
            moved = [t.gather(1, rows[:, :, None].expand(B, s, w)).gather(2, slots).contiguous() for t in (d_idx, d_sc)]
            assert same(ops.fuse_lists(*moved, n, combine, d_src.gather(1, rows).contiguous(), ex), got), (n, combine)
        # without sources the pool is one bag of slots: any permutation of all of them
        free = ops.fuse_lists(d_idx, d_sc, n, combine)
        perm = torch.stack([torch.randperm(s * w, device="cuda") for _ in range(B)])
        moved = [t.reshape(B, -1).gather(1, perm).reshape(B, s, w).contiguous() for t in (d_idx, d_sc)]
        assert same(ops.fuse_lists(*moved, n, combine), free)
        assert same(ops.fuse_lists(d_idx.reshape(B, 1, -1), d_sc.reshape(B, 1, -1), n, combine), free)


def test_the_sort_widths_agree_at_their_boundaries():
    """A pool at the edge of a variant, and the same pool with one -1 slot behind it in the next."""
    rng = np.random.default_rng(128)
    for pool in (128, 256, 512):
        idx, score = make_pool(rng, B, 1, pool)
        wide_i = np.concatenate([idx, np.full((B, 1, 1), -1, np.int32)], 2)
        wide_s = np.concatenate([score, np.full((B, 1, 1), 1.5, np.float32)], 2)
        for n, combine in ((1, "sum"), (10, "max"), (min(pool, 256), "sum")):
            assert same(fuse(wide_i, wide_s, n, combine), fuse(idx, score, n, combine)), (pool, n, combine)


# ---- 4. one row of distinct ids: the sort alone
@pytest.mark.parametrize("m", (1, 64, 200, 256))
def test_one_row_of_distinct_ids_is_cap_lists(m):
    from p_companion_amd import ops
    rng = np.random.default_rng(7 + m)
    idx, score = make_pool(rng, B, 1, m)
    idx[:, 0, :] = np.where(idx[:, 0, :] >= 0, np.stack([rng.permutation(P)[:m] for _ in range(B)]), -1)
    for n in sorted({1, min(10, m), m}):
        want = ops.cap_lists(cuda(idx[:, 0]), cuda(score[:, 0]), n)
        for combine in ("sum", "max"):
            got = fuse(idx, score, n, combine)
            assert same(got[:2], want), (n, combine)
            assert torch.equal(got[2], (got[0] >= 0).int())


def test_max_is_a_dedupe_with_the_best_slots_bits():
    rng = np.random.default_rng(77)
    idx, score = make_pool(rng, B, 5, 40, ids=30)
    got = check(idx, score, 30, "max")
    g_i, g_s, g_c = (t.cpu().numpy() for t in got)
    for r in range(B):
        ok = (idx[r] >= 0) & np.isfinite(score[r])
        served = g_i[r][g_i[r] >= 0]
        assert len(served) == len(set(served.tolist())) == len(np.unique(idx[r][ok]))
        for i, f, c in zip(g_i[r], g_s[r], g_c[r]):
            if i >= 0:
                mine = score[r][ok & (idx[r] == i)]
                assert f == mine.max() and c == len(mine)
                assert f.view(np.int32) in set(mine[mine == mine.max()].view(np.int32).tolist())
    assert (g_c > 1).any()


# ---- 5. the ban set
def test_the_ban_set():
    rng = np.random.default_rng(31)
    s, w = 4, 30
    idx, score = make_pool(rng, B, s, w, holes=False)
    source = make_sources(rng, B, s, lo=0)                # members from the whole catalogue: some are offered by other rows
    source[0], source[1] = (5, 6, 7, 8), (-1, -1, -1, -1)
    idx[0, 1, :4], score[0, 1, :4] = (5, 6, 9, 10), 2.0   # row 1 offers the members 5 and 6 with the best score
    ex_rows = [np.array([], np.int64)] * P
    ex_rows[7], ex_rows[8] = np.array([7, 9]), np.array([8, 11, 999])             # item 7 excludes 9: row 1 offers it
    for q in range(20, 60):
        ex_rows[q] = np.sort(rng.choice(60, 5, replace=False))
    ex = (np.concatenate([[0], np.cumsum([len(r) for r in ex_rows])]).astype(np.int32), np.concatenate(ex_rows).astype(np.int32))
    for combine in ("sum", "max"):
        top = min(s * w, 256)
        with_ex = check(idx, score, top, combine, source, ex)
        without = check(idx, score, top, combine, source, num_products=P)
        none = check(idx, score, top, combine)
        i_ex, i_wo, i_no = (t[0].cpu().numpy() for t in (with_ex, without, none))
        assert {5, 6, 9, 10} <= set(i_no[0].tolist())                             # offered
        assert not {5, 6} & set(i_wo[0].tolist()) and {9, 10} <= set(i_wo[0].tolist())     # a member is never served
        assert not {5, 6, 9} & set(i_ex[0].tolist()) and 10 in i_ex[0]            # ... nor the substitute of ANOTHER row's item
        for r in range(B):
            members = set(source[r][source[r] >= 0].tolist())
            assert not members & set(i_wo[r].tolist()) and not members & set(i_ex[r].tolist())
            gone = set().union(*[set(ex_rows[q].tolist()) for q in members]) if members else set()
            assert not gone & set(i_ex[r].tolist())
        # a basket of padding alone serves nothing, although its rows hold valid ids
        assert (idx[1] >= 0).all() and (i_wo[1] == -1).all() and (i_ex[1] == -1).all() and (i_no[1] >= 0).any()
        assert torch.isneginf(with_ex[1][1]).all() and (with_ex[2][1] == 0).all()
        # a row whose source is -1 contributes nothing: the same basket without that row's slots
        hollow_i = np.where((source == -1)[:, :, None], -1, idx)
        assert same(fuse(hollow_i, score, top, combine, source, ex), with_ex)
        # an empty exclusion set is no set
        empty = (np.zeros(P + 1, np.int32), np.zeros(0, np.int32))
        assert same(check(idx, score, top, combine, source, empty), without)


def test_the_ban_set_past_64_sources_and_past_one_chunk_of_exclusion_ids():
    """S = 65, w = 1, four ids per source: the 64 sources of the first round bring 256 ids -- behind the 64 sources the first
    256-entry chunk holds the ids 0 .. 191, a second one 192 .. 255 --, and the 65th source makes a second round (256 .. 259)."""
    rng = np.random.default_rng(65)
    b, s = 5, 65
    source = np.tile(np.arange(700, 700 + s, dtype=np.int32), (b, 1))             # source j excludes 4 j .. 4 j + 3
    ex = (np.zeros(P + 1, np.int32), np.arange(4 * s, dtype=np.int32))
    ex[0][701:] = np.minimum(4 * np.arange(1, P - 699), 4 * s)
    assert ex[0][700] == 0 and ex[0][764] == 256 and ex[0][765] == ex[0][P] == 260
    idx = rng.integers(0, 330, (b, s, 1)).astype(np.int32)                        # banned by a row (< 260) or not
    score = (rng.permutation(b * s).reshape(b, s, 1) / 4).astype(np.float32)
    planted = (191, 192, 200, 255, 256, 259, 764, 700)    # the chunks' and rounds' edges, a source of either round
    idx[:, :len(planted), 0], idx[:, len(planted), 0] = planted, 300
    for combine in ("sum", "max"):
        with_ex = check(idx, score, s, combine, source, ex)[0].cpu().numpy()
        without = check(idx, score, s, combine, source, num_products=P)[0].cpu().numpy()
        for r in range(b):
            assert set(planted[:6]) | {300} <= set(without[r].tolist()) and not {764, 700} & set(without[r].tolist())
            assert 300 in with_ex[r] and (with_ex[r][with_ex[r] >= 0] >= 260).all() and not {764, 700} & set(with_ex[r].tolist())


def test_short_baskets_end_in_minus_one_minus_inf_and_zero():
    s, w = 3, 10
    idx = np.full((4, s, w), -1, np.int32)
    score = np.ones((4, s, w), np.float32)
    source = np.array([[100, 101, 102], [-1, -1, -1], [100, 101, 102], [100, -1, 102]], np.int32)
    idx[0, :, :2] = [[1, 2], [2, 3], [3, 4]]              # four products survive
    idx[1, :, :] = np.arange(w)                           # a basket of padding alone
    idx[2, :, :3] = [[101, 102, 50], [100, 50, 102], [51, 100, 101]]              # every candidate is banned: 50, 51 by the set
    idx[3, :, :2] = [[7, 8], [9, 10], [8, 11]]            # the middle row is padding
    ex = (np.zeros(P + 1, np.int32), np.array([50, 51], np.int32))
    ex[0][101:] = 1
    ex[0][103:] = 2                                       # 100 excludes 50, 102 excludes 51
    for combine in ("sum", "max"):
        got = check(idx, score, 10, combine, source, ex)
        g_i, g_s, g_c = (t.cpu().numpy() for t in got)
        two = 2.0 if combine == "sum" else 1.0
        assert g_i[0].tolist() == ([2, 3, 1, 4] if combine == "sum" else [1, 2, 3, 4]) + [-1] * 6
        assert g_s[0][:4].tolist() == ([two, two, 1.0, 1.0]) and g_c[0][:4].tolist() == ([2, 2, 1, 1] if combine == "sum" else [1, 2, 2, 1])
        for r, kept in ((0, 4), (1, 0), (2, 0), (3, 3)):
            assert (g_i[r][kept:] == -1).all() and np.isneginf(g_s[r][kept:]).all() and (g_c[r][kept:] == 0).all()
            assert (g_i[r][:kept] >= 0).all()
        assert sorted(g_i[3][:3].tolist()) == [7, 8, 11]


# ---- 6. ids and sources out of range
@pytest.mark.parametrize("s,w", [(4, 20), (5, 120)])
def test_bad_ids_and_sources_are_counted_never_served_and_never_used(s, w):
    rng = np.random.default_rng(7 + s * w)
    idx, score = make_pool(rng, B, s, w)
    source = make_sources(rng, B, s)
    ex = make_exclusions(rng)
    planted = [P, P + 5, -2, INT32_MIN, 2 ** 31 - 1]
    for k, x in enumerate(planted):
        idx[3 + 2 * k, k % s, (5 * k) % w] = x
        score[3 + 2 * k, k % s, (5 * k) % w] = 64.0       # (the best score of its basket, were it a candidate)
    idx[20, 0, :5] = planted
    score[20, 0, :5] = 64.0
    source[22, 0], source[23, 1], source[24, 2], source[25, 3] = P, -2, INT32_MIN, 2 ** 31 - 1
    for r in (22, 23, 24, 25):
        idx[r, r - 22, 0], score[r, r - 22, 0] = 59, 64.0  # the dropped row's offer, the best of its basket
        idx[r][idx[r] == 59] = np.where(np.arange((idx[r] == 59).sum()) == 0, 59, 58)
    want = oracle(idx, score, 10, "sum", source, ex)
    assert want[3] == 2 * len(planted) + 4
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = check(idx, score, 10, "sum", source, ex, want=want, bad=bad)
    assert int(bad) == want[3]
    served = got[0].cpu().numpy()
    assert not np.isin(served, planted).any() and not (served[22:26] == 59).any()
    # the counter is added to; without a counter the ids are passed over all the same
    assert same(check(idx, score, 10, "sum", source, ex, want=want, bad=bad), got) and int(bad) == 2 * want[3]
    assert same(check(idx, score, 10, "sum", source, ex, want=want), got)
    # without sources and without a catalogue size every id in [0, 2^31 - 1) is a candidate: the negative ones and 2^31 - 1 are bad
    bad.zero_()
    free = check(idx, score, 10, "max", bad=bad)
    assert int(bad) == 6 and np.isin(free[0].cpu().numpy(), [P, P + 5]).any()
    # a basket's output does not depend on the other baskets of the call
    for lo, hi in ((0, 1), (3, 10), (B - 1, B)):
        part = fuse(idx[lo:hi], score[lo:hi], 10, "sum", source[lo:hi], ex)
        assert same(part, tuple(t[lo:hi] for t in got))


# ---- 7. more baskets than the grid holds at once, and none
def test_grid_stride_and_no_baskets():
    from p_companion_amd import ops
    b, s, w = 4 * 4096 + 5, 2, 4
    rng = np.random.default_rng(4096)
    idx, score = make_pool(rng, b, s, w, ids=6)
    source = rng.integers(-1, 6, (b, s)).astype(np.int32)
    check(idx, score, 4, "sum", source, num_products=P)
    check(idx, score, 8, "max")
    out = ops.fuse_lists(cuda(idx[:0]), cuda(score[:0]), 3, "sum", cuda(source[:0]))
    assert [tuple(t.shape) for t in out] == [(0, 3)] * 3 and [t.dtype for t in out] == [torch.int32, torch.float32, torch.int32]


# ---- 8. through PCompanionInference
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
    return SimpleNamespace(inf=inf, model=model, cfg=c, bpg=bpg, host=host, features=g["features"], products=products,
                           q=torch.arange(0, products, 41, dtype=torch.int32))


def basket_oracle(inf, basket, n, per_item, combine):
    """the numpy contract over the items' separately served recommend_batch outputs"""
    b, items = basket.shape
    flat = basket.reshape(-1).clamp(min=0)
    _, idx, sc = inf.recommend_batch(flat, per_item)
    ex = None if inf.exclusions is None else tuple(t.cpu().numpy() for t in inf.exclusions)
    pool_i, pool_s = idx.reshape(b, items, -1).cpu().numpy(), sc.reshape(b, items, -1).cpu().numpy()
    assert np.isfinite(pool_s[pool_i >= 0]).all()         # (what is served has a finite score)
    return pool_i, oracle(pool_i, pool_s, n, combine, basket.cpu().numpy(), ex, int(inf.type_idx.shape[0]))


def test_one_item_baskets_are_the_merged_page(served):
    from p_companion_amd import ops
    s, q = served, served.q
    for n, per_item in ((10, 8), (24, 16), (40, 30)):
        _, p_idx, p_sc = s.inf.recommend_batch(q, per_item)
        b = p_idx.shape[0]
        want = ops.cap_lists(p_idx.reshape(b, -1), p_sc.reshape(b, -1), n)
        page = s.inf.recommend_page_batch(q, n, per_type=per_item)
        for combine in ("sum", "max"):
            idx, sc, types, support = s.inf.recommend_basket_batch(q.reshape(-1, 1), n, per_item=per_item, combine=combine)
            assert idx.shape == (b, n) and types.dtype == torch.int64 and support.dtype == torch.int32
            # (the query is no candidate of its own lists only once exclusions are installed: here it may be offered, and the
            # fusion then bans it -- a basket member --, which the page does not)
            own = (want[0] == q.cuda()[:, None]).any(1)
            assert same((idx[~own], sc[~own]), (want[0][~own], want[1][~own])) and (~own).any()
            assert same((idx[~own], sc[~own]), (page[0][~own], page[1][~own])) and torch.equal(types[~own], page[2][~own])
            assert torch.equal(support, (idx >= 0).int())
    s.inf.set_exclusions()
    try:
        _, p_idx, p_sc = s.inf.recommend_batch(q, 8)
        want = ops.cap_lists(p_idx.reshape(len(q), -1), p_sc.reshape(len(q), -1), 10)
        page = s.inf.recommend_page_batch(q, 10, per_type=8)
        got = s.inf.recommend_basket_batch(q.reshape(-1, 1), 10, per_item=8)
        assert same(got[:2], want) and same(got[:2], page[:2]) and torch.equal(got[2], page[2])
        assert torch.equal(got[3], (got[0] >= 0).int())
    finally:
        s.inf.set_exclusions(False)


def _baskets(s, items, rng):
    """A first draw of baskets and, by hand, baskets in which a co-viewed product of one item is offered by another item's
    list, and baskets whose first two items' lists share a product -- both read off the lists every product is served under
    the installed exclusions."""
    drawn = rng.integers(0, s.products, (12, items)).astype(np.int32)
    s.inf.set_exclusions()
    try:
        every = torch.arange(s.products, dtype=torch.int32)
        offered = torch.cat([s.inf.recommend_batch(every[lo:lo + 500], 8)[1].reshape(-1, s.cfg.NUM_COMP_TYPES * 8).cpu()
                             for lo in range(0, s.products, 500)]).numpy()
    finally:
        s.inf.set_exclusions(False)
    offers = {}                                           # product -> the queries whose lists hold it
    for q in range(s.products):
        for c in offered[q][offered[q] >= 0].tolist():
            offers.setdefault(c, []).append(q)
    rest = lambda q: [(q + 7 * (j + 1)) % s.products for j in range(items - 2)]
    crossing, sharing = [], []
    for q in range(s.products):
        for c in s.host.cv_col[s.host.cv_rowptr[q]:s.host.cv_rowptr[q + 1]].tolist():
            other = [x for x in offers.get(c, []) if x != q]
            if other and len(crossing) < 20:
                crossing.append([q, other[0]] + rest(q))
    for c, qs in sorted(offers.items()):
        if len(qs) >= 2 and len(sharing) < 20:
            sharing.append(qs[:2] + rest(qs[0]))
    assert crossing and sharing
    return torch.from_numpy(np.concatenate([drawn, np.array(crossing, np.int32), np.array(sharing, np.int32)]))


@pytest.mark.parametrize("items", (2, 3))
def test_baskets_against_the_oracle_with_and_without_exclusions(served, items):
    s, k = served, served.cfg.NUM_COMP_TYPES
    basket = _baskets(s, items, np.random.default_rng(items))
    b = basket.shape[0]
    whole = items * k * 8                                 # the whole pool of the per_item = 8 lists: every product is served
    for installed in (False, True):
        if installed:
            s.inf.set_exclusions()
        try:
            for n, per_item, combine in ((10, 8, "sum"), (10, 8, "max"), (whole, 8, "sum"), (48, 16, "sum"),
                                         (min(256, items * k * 40), 40, "sum")):
                pool_i, want = basket_oracle(s.inf, basket, n, per_item, combine)
                got = s.inf.recommend_basket_batch(basket, n, per_item=per_item, combine=combine)
                assert same(got[:2] + got[3:], tuple(cuda(a) for a in want[:3])), (installed, n, per_item, combine)
                type_idx = s.inf.type_idx.long()
                assert torch.equal(got[2], torch.where(got[0] >= 0, type_idx[got[0].clamp(min=0).long()], -1))
                # a padded basket serves the same bits, wherever the padding stands
                if (items + 2) * k * per_item <= 1024:
                    wide = torch.full((b, items + 2), -1, dtype=torch.int32)
                    wide[:, [0, 2, 4][:items]] = basket
                    assert same(s.inf.recommend_basket_batch(wide, n, per_item=per_item, combine=combine), got)
                if (n, per_item) != (whole, 8):
                    continue
                served_ids, members, cross = got[0].cpu().numpy(), basket.numpy(), 0
                for r in range(b):
                    assert not set(members[r].tolist()) & set(served_ids[r].tolist())               # nothing already in the basket
                    for a in range(items):                # the co-viewed products of item a that ANOTHER item's list offers
                        subs = set(s.host.cv_col[s.host.cv_rowptr[members[r, a]]:s.host.cv_rowptr[members[r, a] + 1]].tolist())
                        offered_by_others = subs & set(np.delete(pool_i[r], a, 0).reshape(-1).tolist())
                        if installed:
                            cross += len(offered_by_others)
                            assert not subs & set(served_ids[r].tolist())
                        else:                             # without a set they are served (unless they are basket members)
                            assert offered_by_others - set(members[r].tolist()) <= set(served_ids[r].tolist()), (
                                r, a, members[r], sorted(offered_by_others), pool_i[r], served_ids[r])
                if installed:
                    assert cross > 0, "no basket offers a substitute of one item through another item's list"
                    assert (got[3] > 1).any()             # a product two lists of a basket offered is one product
        finally:
            s.inf.set_exclusions(False)


def test_the_bf16_catalogues(served):
    from p_companion_amd import ops
    from p_companion_amd.inference import PCompanionInference
    s = served
    basket = _baskets(s, 3, np.random.default_rng(16))
    compact = PCompanionInference(s.model, s.cfg, s.bpg, catalogue=ops.CompactCatalogue(s.features))
    bare = PCompanionInference(s.model, s.cfg, s.bpg, catalogue=torch.bfloat16)
    for inf, per_item in ((compact, 8), (compact, 40), (bare, 8), (bare, 16)):
        inf.set_exclusions()
        _, want = basket_oracle(inf, basket, 20, per_item, "sum")
        got = inf.recommend_basket_batch(basket, 20, per_item=per_item)
        assert same(got[:2] + got[3:], tuple(cuda(a) for a in want[:3])), per_item
        assert (got[0][:, 0] >= 0).all()
    with pytest.raises(ValueError, match="bf16 catalogue serves at most 16"):
        bare.recommend_basket_batch(basket, 20, per_item=17)
