"""Session recommendations: pc_fuse_sessions / ops.fuse_sessions (ragged sessions with a weight per item fused on the device,
on a walk that is linear in the pool) and PCompanionInference.recommend_session_batch.

Two references, neither of them the code under test: ops.fuse_lists, whose bits a rectangular pool must reproduce, and the
contract restated in numpy (oracle below) -- live rows, offering rows, t = np.float32(w) * np.float32(s), the ban set of ALL
rows, per product id the terms sorted descending (+0.0 before -0.0) and added as np.float32 one at a time,
np.lexsort((id, -fused)), with the clamping of seg_rowptr and both counters.  The kernel forms one rounded product per slot and
adds in that pinned order, so every comparison here is bit for bit; nothing is tolerated.  Needs an MI355X."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

P, B = 1000, 23
EDGES = (1, 2, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024)                  # 2 / 4 / 8 / 16 slots per lane
MIXED = {1: (1, 1), 2: (2, 1), 127: (127, 1), 128: (8, 16), 129: (3, 43), 255: (5, 51), 256: (16, 16), 257: (257, 1),
         511: (7, 73), 512: (32, 16), 513: (27, 19), 1023: (11, 93), 1024: (16, 64)}
EXACT = np.array([0.25, 0.5, 0.75, 1, 1.5, 2, 4], np.float32)     # weights whose products with k / 4 are exact
INT32_MIN = -2 ** 31


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(sc):
    return sc.contiguous().view(torch.int32)


def same(got, want):
    """(idx, score[, support]) tuples: equal ids, equal score BITS, equal supports"""
    return (len(got) == len(want) and torch.equal(got[0], want[0]) and torch.equal(bits(got[1]), bits(want[1]))
            and all(torch.equal(g, w) for g, w in zip(got[2:], want[2:])))


def clamp_ends(ptr, rows):
    """The contract's reading of seg_rowptr: per session (lo, hi) inside [0, rows] with lo <= hi, and the bad entries -- every
    entry outside [0, rows] or below its predecessor, each once."""
    ends, bad = [], 0
    for b in range(len(ptr) - 1):
        lo_raw, hi_raw = int(ptr[b]), int(ptr[b + 1])
        bad += int(hi_raw < 0 or hi_raw > rows or hi_raw < lo_raw) + int(b == 0 and (lo_raw < 0 or lo_raw > rows))
        lo = min(max(lo_raw, 0), rows)
        ends.append((lo, min(max(hi_raw, lo), rows)))
    return ends, bad


def oracle(idx, score, ptr, n, combine="sum", source=None, weight=None, exclude=None, num_products=None, max_items=None):
    """The contract: (ids [B, n] int32, fused scores [B, n] fp32, supports [B, n] int32, the bad count, the truncated count)."""
    rows, w = idx.shape
    p = num_products if num_products is not None else len(exclude[0]) - 1 if exclude is not None else 2 ** 31 - 1
    ends, bad = clamp_ends(ptr, rows)
    b = len(ends)
    out_i = np.full((b, n), -1, np.int32)
    out_s = np.full((b, n), -np.inf, np.float32)
    out_c = np.zeros((b, n), np.int32)
    cap = 1024 // w if not max_items else min(1024 // w, max_items)
    truncated = 0
    for r, (lo, hi) in enumerate(ends):
        live = min(hi - lo, cap)
        truncated += int(hi - lo > cap)
        ban = set()
        if source is not None:                            # every row of the session bans
            src = source[lo:hi].astype(np.int64)
            bad += int(((src < -1) | (src >= p)).sum())
            ban = set(src[(src >= 0) & (src < p)].tolist())
            if exclude is not None:
                for q in sorted(ban):
                    ban |= set(exclude[1][exclude[0][q]:exclude[0][q + 1]].tolist())
        at = slice(hi - live, hi)                         # the last rows offer
        l_idx, l_sc = idx[at].astype(np.int64), score[at]
        bad += int(((l_idx < -1) | (l_idx >= p)).sum())
        src = np.zeros(live, np.int64) if source is None else source[at].astype(np.int64)
        wt = np.ones(live, np.float32) if weight is None else weight[at]
        offers = (src >= 0) & (src < p) & np.isfinite(wt) & (wt > 0)
        with np.errstate(all="ignore"):
            term = (wt[:, None].astype(np.float32) * l_sc.astype(np.float32)).astype(np.float32)       # one fp32 product
        ok = (l_idx >= 0) & (l_idx < p) & np.isfinite(term) & offers[:, None]
        ids, terms = l_idx[ok], term[ok]
        fused = {}
        for i in np.unique(ids):
            if int(i) in ban:
                continue
            mine = terms[ids == i]
            mine = mine[np.lexsort((np.signbit(mine), -mine))]           # descending, +0.0 before -0.0
            f = np.float32(mine[0])
            if combine == "sum":
                with np.errstate(over="ignore"):
                    for x in mine[1:]:
                        f = np.float32(f + np.float32(x))
            fused[int(i)] = (f, len(mine))
        keys = np.array(sorted(fused), np.int64)
        val = np.array([fused[i][0] for i in keys], np.float32)
        for k, j in enumerate(np.lexsort((keys, -val))[:n]):             # fused score descending, product index ascending
            out_i[r, k], out_s[r, k], out_c[r, k] = keys[j], val[j], fused[int(keys[j])][1]
    return out_i, out_s, out_c, bad, truncated


def fuse(idx, score, ptr, n, combine="sum", source=None, weight=None, exclude=None, **kw):
    from p_companion_amd import ops
    got = ops.fuse_sessions(cuda(idx), cuda(score), cuda(np.asarray(ptr, np.int32)), n, combine,
                            None if source is None else cuda(source), None if weight is None else cuda(weight),
                            None if exclude is None else (cuda(exclude[0]), cuda(exclude[1])), **kw)
    assert [tuple(t.shape) for t in got] == [(len(ptr) - 1, n)] * 3
    assert [t.dtype for t in got] == [torch.int32, torch.float32, torch.int32]
    return got


def check(idx, score, ptr, n, combine="sum", source=None, weight=None, exclude=None, want=None, **kw):
    """ops.fuse_sessions against the oracle (or `want`, an oracle run with a longer n whose first n columns are this call's)."""
    got = fuse(idx, score, ptr, n, combine, source, weight, exclude, **kw)
    if want is None:
        want = oracle(idx, score, ptr, n, combine, source, weight, exclude, kw.get("num_products"), kw.get("max_items"))
    assert same(got, tuple(cuda(a[:, :n]) for a in want[:3])), (idx.shape, n, combine)
    return got


def make_rows(rng, rows, w, ids=60, holes=True):
    """The test-data convention: ids drawn with replacement from a small range (most products repeat across a session's rows),
    scores from {k / 4: |k| <= 8} with both zeros (sums are exact, ties are frequent: the id order decides); a fifth of the
    slots is no candidate."""
    idx = rng.integers(0, ids, (rows, w)).astype(np.int32)
    k = rng.integers(-8, 9, (rows, w))
    score = (k / 4).astype(np.float32)
    score[(k == 0) & (rng.random((rows, w)) < 0.5)] = -0.0
    if holes:
        kind = rng.integers(0, 4, (rows, w))
        hole = rng.random((rows, w)) < 0.2
        idx[hole & (kind == 0)] = -1
        score[hole & (kind == 1)] = -np.inf
        score[hole & (kind == 2)] = np.inf
        score[hole & (kind == 3)] = np.nan
    return idx, score


def make_sources(rng, rows, lo=500):
    """Session members from [lo, P) (outside make_rows' ids; an item may be listed twice), a quarter of the rows no item."""
    source = rng.integers(lo, P, rows).astype(np.int32)
    source[rng.random(rows) < 0.25] = -1
    return source


def make_exclusions(rng, per_key=6, ids=30):
    """A strictly ascending CSR over P keys whose rows name the lower half of make_rows' ids: the rest survives any session."""
    sets = [np.sort(rng.choice(ids, rng.integers(0, min(per_key, ids) + 1), replace=False)) for _ in range(P)]
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in sets])]).astype(np.int32)
    return rowptr, np.concatenate(sets).astype(np.int32)


def ragged(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)


# ---- 1. rectangular pools are the existing entry's bits, at every edge of the variants
@pytest.mark.parametrize("pool", EDGES)
def test_rectangular_sessions_are_fuse_lists_bit_for_bit(pool):
    from p_companion_amd import ops
    rng = np.random.default_rng(100 + pool)
    ids = max(4, min(60, pool // 3))
    ex = tuple(cuda(a) for a in make_exclusions(rng, ids=max(1, ids // 2)))
    for s, w in sorted({(1, pool), (pool, 1), MIXED[pool]}):
        assert s * w == pool
        idx, score = make_rows(rng, B * s, w, ids=ids)
        d_idx, d_sc, d_src = cuda(idx), cuda(score), cuda(make_sources(rng, B * s))
        ptr = cuda(ragged([s] * B))
        ones = torch.ones(B * s, device="cuda")
        top = min(pool, 256)
        for combine in ("sum", "max"):
            for source, exclude in ((None, None), (d_src, None), (d_src, ex)):
                for n in sorted({1, min(10, pool), top}):
                    want = ops.fuse_lists(d_idx.reshape(B, s, w), d_sc.reshape(B, s, w), n, combine,
                                          None if source is None else source.reshape(B, s), exclude, num_products=P)
                    for weight in (None, ones):
                        got = ops.fuse_sessions(d_idx, d_sc, ptr, n, combine, source, weight, exclude, num_products=P)
                        assert same(got, want), (s, w, combine, source is not None, exclude is not None, n, weight is not None)
                if pool >= 127 and exclude is not None:
                    assert (want[0] >= 0).any() and (want[2] > 1).any()


# ---- 2. weights: the existing entry over scores scaled in torch (one IEEE multiplication per slot)
@pytest.mark.parametrize("s,w", [(3, 20), (8, 16), (9, 24), (11, 48), (16, 64)])
def test_weighted_sessions_are_fuse_lists_over_prescaled_scores(s, w):
    from p_companion_amd import ops
    rng = np.random.default_rng(7 * s + w)
    idx, score = make_rows(rng, B * s, w)
    d_idx, d_sc, d_src = cuda(idx), cuda(score), cuda(make_sources(rng, B * s))
    ex = tuple(cuda(a) for a in make_exclusions(rng))
    ptr = cuda(ragged([s] * B))
    exact = cuda(rng.choice(EXACT, B * s))
    inexact = cuda(rng.uniform(0.1, 3.0, B * s).astype(np.float32))      # the products round: the same rounding on both sides
    for weight in (exact, inexact):
        scaled = weight[:, None] * d_sc
        assert scaled.dtype == torch.float32
        for n, combine in ((10, "sum"), (min(s * w, 256), "sum"), (10, "max")):
            want = ops.fuse_lists(d_idx.reshape(B, s, w), scaled.reshape(B, s, w), n, combine, d_src.reshape(B, s), ex)
            got = ops.fuse_sessions(d_idx, d_sc, ptr, n, combine, d_src, weight, ex)
            assert same(got, want), (n, combine)
            assert not same(got, ops.fuse_sessions(d_idx, d_sc, ptr, n, combine, d_src, None, ex))      # the weights matter


# ---- 3. one call with sessions of every class: each variant both serves and skips
def class_lengths(w):
    """session lengths whose pools are 0, w, 128, 129., 256, 257., 512, 513., 1024 (. : the next multiple of w) and more"""
    up = lambda x: -(-x // w)
    return [0, 1, 128 // w, up(129), 256 // w, up(257), 512 // w, up(513), 1024 // w, 1024 // w + 2]


@pytest.mark.parametrize("w", (1, 24, 48))
def test_sessions_of_every_class_in_one_call_match_the_oracle(w):
    rng = np.random.default_rng(300 + w)
    lengths = np.array(class_lengths(w) * 3)
    rng.shuffle(lengths)
    pools = np.minimum(lengths, 1024 // w) * w
    for lo, hi in ((0, 0), (1, 128), (129, 256), (257, 512), (513, 1024)):
        assert ((pools >= lo) & (pools <= hi)).any()       # every variant serves, and skips the others' sessions
    ptr = ragged(lengths)
    rows = int(ptr[-1])
    idx, score = make_rows(rng, rows, w)
    assert np.signbit(score[score == 0]).any() and not np.signbit(score[score == 0]).all()             # both zeros
    source = make_sources(rng, rows)
    weight = rng.choice(EXACT, rows)
    ex = make_exclusions(rng)
    for combine in ("sum", "max"):
        plain = oracle(idx, score, ptr, 256, combine, weight=weight)
        banned = oracle(idx, score, ptr, 256, combine, source, weight, ex)
        assert plain[4] == banned[4] == 3 and plain[3] == banned[3] == 0
        assert (plain[2] > 1).any() and (banned[0] >= 0).any() and not np.array_equal(plain[0], banned[0])
        for n in (1, 10, 256):
            counters = [torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(2)]
            check(idx, score, ptr, n, combine, weight=weight, want=plain)
            check(idx, score, ptr, n, combine, source, weight, ex, want=banned, bad=counters[0], truncated=counters[1])
            assert [int(c) for c in counters] == [0, 3]


# ---- 4. the variant that serves a session does not show in its bits
def klass(pool):
    return 2 if pool <= 128 else 4 if pool <= 256 else 8 if pool <= 512 else 16


def test_a_session_padded_into_the_next_variant_is_the_same_bits():
    rng = np.random.default_rng(128)
    w = 16
    ex = make_exclusions(rng)
    for rows, pad in ((1, 8), (8, 1), (8, 9), (16, 1), (16, 17), (32, 1), (32, 32), (3, 61)):
        idx, score = make_rows(rng, B * rows, w)
        source, weight = make_sources(rng, B * rows), rng.choice(EXACT, B * rows)
        # the padding rows stand in front of, behind and between the session's rows; they hold ids and scores like any row
        p_idx, p_sc = make_rows(rng, B * pad, w)
        wide = [np.concatenate([a.reshape(B, rows, -1), b.reshape(B, pad, -1)], 1)
                for a, b in ((idx, p_idx), (score, p_sc), (source[:, None], np.full((B * pad, 1), -1, np.int32)),
                             (weight[:, None], np.zeros((B * pad, 1), np.float32)))]
        order = np.stack([rng.permutation(rows + pad) for _ in range(B)])
        wide = [np.take_along_axis(a, order[:, :, None], 1).reshape(B * (rows + pad), -1) for a in wide]
        assert klass(rows * w) < klass((rows + pad) * w) and rows + pad <= 1024 // w                     # another variant, nothing cut
        for n, combine in ((1, "sum"), (10, "max"), (min(rows * w, 256), "sum")):
            alone = check(idx, score, ragged([rows] * B), n, combine, source, weight, ex)
            padded = fuse(wide[0], wide[1], ragged([rows + pad] * B), n, combine, wide[2][:, 0], wide[3][:, 0], ex)
            assert same(padded, alone), (rows, pad, n, combine)


# ---- 5. truncation: the last rows offer, every row bans
def test_a_long_session_offers_its_last_rows_and_bans_with_all_of_them():
    rng = np.random.default_rng(5)
    for w in (48, 64, 1024):
        cap = 1024 // w
        lengths = [cap + 3, cap, cap + 1, 1, 0, cap + 3]
        ptr = ragged(lengths)
        rows = int(ptr[-1])
        idx, score = make_rows(rng, rows, w)
        source, weight = make_sources(rng, rows), rng.choice(EXACT, rows)
        idx[idx >= 50] -= 10                                # ids 50 .. 59 are placed by hand below
        ex_sets = [np.array([], np.int64)] * P
        # session 0: an early row's source (51) and its exclusion row (52) ban what the late rows offer; 53 is offered by the
        # early rows alone, 54 by a late row
        source[0], source[1], source[2] = 51, 700, -1
        ex_sets[700] = np.array([52])
        source[3:cap + 3] = np.arange(800, 800 + cap)
        weight[:cap + 3] = 1.0
        idx[0, 0], idx[1, 0], idx[2, 0], score[:3, 0] = 53, 53, 53, 2.0
        idx[cap + 2, :4], score[cap + 2, :4] = (51, 52, 54, 55), 2.0
        ex = (np.concatenate([[0], np.cumsum([len(r) for r in ex_sets])]).astype(np.int32), np.concatenate(ex_sets).astype(np.int32))
        for combine in ("sum", "max"):
            counters = [torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(2)]
            got = check(idx, score, ptr, 64, combine, source, weight, ex, bad=counters[0], truncated=counters[1])
            assert [int(c) for c in counters] == [0, 3]    # the exact count: the sessions of cap + 3, cap + 1 and cap + 3 rows
            first = got[0][0].cpu().numpy().tolist()
            assert 54 in first and 55 in first and not {51, 52, 53} & set(first)
            # without the CSR the early row's source still bans 51, and 52 is served
            first = check(idx, score, ptr, 64, combine, source, weight, num_products=P)[0][0].cpu().numpy().tolist()
            assert 52 in first and 51 not in first and 53 not in first
            # the rows that do not offer are not read as slots: garbage in them changes nothing
            junk_i, junk_s = idx.copy(), score.copy()
            junk_i[:3], junk_s[:3] = rng.integers(0, 60, (3, w)), 8.0
            assert same(fuse(junk_i, junk_s, ptr, 64, combine, source, weight, ex), got)
            check(idx, score, ptr, 64, combine, source, weight, ex, truncated=counters[1])
            assert int(counters[1]) == 6                   # added to
        if w == 1024:
            continue
        for max_items in (1, 2, 1000, 0, None):
            t = torch.zeros(1, dtype=torch.int32, device="cuda")
            want = oracle(idx, score, ptr, 20, "sum", source, weight, ex, max_items=max_items)
            assert want[4] == sum(n > min(cap, max_items or cap) for n in lengths) >= 3
            check(idx, score, ptr, 20, "sum", source, weight, ex, want=want, max_items=max_items, truncated=t)
            assert int(t) == want[4]


def test_the_ban_set_past_64_rows_and_past_one_chunk_of_exclusion_ids():
    """w = 1.  A session of 65 rows, four ids per source: the 64 sources of the first round bring 256 ids -- behind the 64
    sources the first 256-entry chunk holds the ids 0 .. 191, a second one 192 .. 255 --, and the 65th row makes a second round
    (256 .. 259).  A session of 3 rows whose sources exclude 100 ids each: what it offers is among the last 40 of the 300, all
    of them in the second chunk."""
    rng = np.random.default_rng(65)
    long, short = 65, 3
    ptr = ragged([long, short])
    source = np.concatenate([np.arange(700, 700 + long), [900, 901, 902]]).astype(np.int32)
    sets = [np.array([], np.int64)] * P
    for j in range(long):
        sets[700 + j] = np.arange(4 * j, 4 * j + 4)
    for t in range(short):
        sets[900 + t] = np.arange(300 + 100 * t, 400 + 100 * t)
    ex = (np.concatenate([[0], np.cumsum([len(r) for r in sets])]).astype(np.int32), np.concatenate(sets).astype(np.int32))
    idx = rng.integers(0, 300, (long + short, 1)).astype(np.int32)                # the long session: banned by a row (< 260) or not
    score = (rng.permutation(long + short).reshape(-1, 1) / 4).astype(np.float32)
    planted = (191, 192, 200, 255, 256, 259, 764, 700)    # the chunks' and rounds' edges, a source of either round
    idx[:len(planted), 0], idx[len(planted), 0] = planted, 299
    idx[long:, 0] = (560, 580, 599)
    for combine in ("sum", "max"):
        with_ex = check(idx, score, ptr, 64, combine, source, None, ex)[0].cpu().numpy()
        without = check(idx, score, ptr, 64, combine, source, num_products=P)[0].cpu().numpy()
        assert set(planted[:6]) | {299} <= set(without[0].tolist()) and not {764, 700} & set(without[0].tolist())
        assert 299 in with_ex[0] and (with_ex[0][with_ex[0] >= 0] >= 260).all() and not {764, 700} & set(with_ex[0].tolist())
        assert sorted(without[1][:3].tolist()) == [560, 580, 599] and (with_ex[1] == -1).all()


def test_max_items_counts_exactly():
    lengths = [0, 1, 2, 3, 1, 2, 5, 1]
    rng = np.random.default_rng(9)
    ptr = ragged(lengths)
    idx, score = make_rows(rng, int(ptr[-1]), 24)
    for max_items, cut in ((1, 4), (2, 2), (3, 1), (5, 0), (100, 0)):
        t = torch.zeros(1, dtype=torch.int32, device="cuda")
        check(idx, score, ptr, 10, "sum", max_items=max_items, truncated=t)
        assert int(t) == cut


# ---- 6. the classes of a weight
def test_rows_whose_weight_is_not_finite_and_positive_offer_nothing_but_still_ban():
    rng = np.random.default_rng(6)
    w, rows = 24, 6
    idx, score = make_rows(rng, B * rows, w, holes=False)
    idx[idx >= 50] -= 10
    source = rng.integers(500, P, B * rows).astype(np.int32)
    weight = rng.choice(EXACT, B * rows)
    ptr = ragged([rows] * B)
    dead = (0.0, -0.0, -1.0, np.nan, np.inf, -np.inf)
    for b, x in enumerate(dead):
        r = b * rows + 2
        weight[r] = x
        idx[r, 0], score[r, 0] = 55, 2.0                   # offered by the dead row alone: never served
        source[r] = 56
        idx[r + 1, 0], score[r + 1, 0] = 56, 2.0           # the dead row's own product, offered by a live row: banned
        idx[r + 1, 1], score[r + 1, 1] = 57, 2.0           # ... beside one that is served
    # an overflowed term is no candidate: 2^100 * 2^100; the same row's score 1 is served as 2^100
    big = np.float32(2.0 ** 100)
    r = 10 * rows
    weight[r], idx[r, :2], score[r, :2], idx[r, 2:] = big, (58, 59), (big, 1.0), -1
    idx[r + 1, 0], score[r + 1, 0], weight[r + 1] = 58, 0.25, 1.0
    for combine in ("sum", "max"):
        got = check(idx, score, ptr, 64, combine, source, weight, num_products=P)
        g_i, g_s, g_c = (t.cpu().numpy() for t in got)
        for b in range(len(dead)):
            assert 57 in g_i[b] and 55 not in g_i[b] and 56 not in g_i[b], (b, dead[b])
        assert g_i[10, 0] == 59 and g_s[10, 0] == big and g_c[10, 0] == 1
        at = g_i[10].tolist().index(58)
        assert g_s[10, at] == 0.25 and g_c[10, at] == 1    # the overflowed slot was not fused into it
    # a session whose rows are all dead is all padding
    weight[:rows] = 0.0
    got = check(idx, score, ptr, 10, "sum", source, weight, num_products=P)
    assert (got[0][0] == -1).all() and torch.isneginf(got[1][0]).all() and (got[2][0] == 0).all()


# ---- 7. the pinned order, on the longest run there is
@pytest.mark.parametrize("rows,w", [(16, 64), (1024, 1), (1, 1024)])
def test_one_product_in_all_1024_slots_adds_the_largest_first(rows, w):
    big = np.float32(2 ** 24)
    assert np.float32(np.float32(big + np.float32(1)) + np.float32(1)) == big                        # descending: 2^24
    assert np.float32(np.float32(np.float32(1) + np.float32(1)) + big) == np.float32(2 ** 24 + 2)    # any other order gives more
    rng = np.random.default_rng(24)
    sessions = 9
    idx = np.full((sessions * rows, w), 7, np.int32)
    score = np.ones((sessions, 1024), np.float32)
    score[np.arange(sessions), rng.integers(0, 1024, sessions)] = big                                 # shuffled per session
    score[0, 0], score[1, 1023] = big, big
    score[0, 1:] = 1.0
    score[1, :1023] = 1.0
    score = score.reshape(sessions * rows, w)
    assert ((score == big).reshape(sessions, -1).sum(1) == 1).all()
    ptr = ragged([rows] * sessions)
    for weight, scale in ((None, 1.0), (np.full(sessions * rows, 2.0, np.float32), 0.5)):
        got = check(idx, (score * np.float32(scale)).astype(np.float32), ptr, 3, "sum", weight=weight)
        g_i, g_s, g_c = (t.cpu().numpy() for t in got)
        assert (g_i[:, 0] == 7).all() and (g_s[:, 0] == big).all() and (g_c[:, 0] == 1024).all()
        assert (g_i[:, 1:] == -1).all() and (g_c[:, 1:] == 0).all()
        got = check(idx, (score * np.float32(scale)).astype(np.float32), ptr, 1, "max", weight=weight)
        assert (got[1][:, 0] == float(big)).all() and (got[2][:, 0] == 1024).all()


# ---- 8. invariances
@pytest.mark.parametrize("w,top", [(24, 50), (48, 30), (85, 4)])
def test_a_permutation_of_rows_or_slots_and_a_second_call_change_no_bit(w, top):
    from p_companion_amd import ops
    rng = np.random.default_rng(50 + w)
    cap = 1024 // w
    lengths = rng.integers(0, top + 1, B)
    lengths[:2] = (top, cap + 1)                          # (sessions that are cut are among them)
    ptr = ragged(lengths)
    rows = int(ptr[-1])
    idx, score = make_rows(rng, rows, w)
    source, weight = make_sources(rng, rows), rng.choice(EXACT, rows)
    ex = make_exclusions(rng)
    d_ex = tuple(cuda(a) for a in ex)
    for n, combine in ((10, "sum"), (256, "sum"), (10, "max")):
        got = check(idx, score, ptr, n, combine, source, weight, ex)
        d = [cuda(a) for a in (idx, score, ptr, source, weight)]
        assert same(ops.fuse_sessions(d[0], d[1], d[2], n, combine, d[3], d[4], d_ex), got)             # a second call
        for _ in range(2):
            # rows move among the rows of one truncation status: the ones that offer among themselves, the others likewise
            order = np.arange(rows)
            for b in range(B):
                lo, hi = int(ptr[b]), int(ptr[b + 1])
                cut = hi - min(hi - lo, cap)
                order[lo:cut] = lo + rng.permutation(cut - lo)
                order[cut:hi] = cut + rng.permutation(hi - cut)
            slots = np.stack([rng.permutation(w) for _ in range(rows)]) if rows else np.zeros((0, w), np.int64)
            moved = [np.take_along_axis(a[order], slots, 1) for a in (idx, score)]
            assert same(fuse(moved[0], moved[1], ptr, n, combine, source[order], weight[order], ex), got), (n, combine)


# ---- 9. a session's output does not depend on the other sessions of the call
def test_sessions_served_together_equal_the_sessions_served_apart():
    rng = np.random.default_rng(90)
    w = 24
    lengths = np.array(class_lengths(w) + [3, 7])
    rng.shuffle(lengths)
    ptr = ragged(lengths)
    idx, score = make_rows(rng, int(ptr[-1]), w)
    source, weight = make_sources(rng, int(ptr[-1])), rng.choice(EXACT, int(ptr[-1]))
    ex = make_exclusions(rng)
    got = check(idx, score, ptr, 20, "sum", source, weight, ex)
    for lo, hi in ((0, 1), (1, 5), (5, len(lengths)), (3, 4)):
        a, z = int(ptr[lo]), int(ptr[hi])
        part = fuse(idx[a:z], score[a:z], ptr[lo:hi + 1] - a, 20, "sum", source[a:z], weight[a:z], ex)
        assert same(part, tuple(t[lo:hi] for t in got)), (lo, hi)


# ---- 10. ids, sources and row pointers out of range
def test_bad_ids_sources_and_row_pointers_are_counted_never_served_and_never_used():
    rng = np.random.default_rng(7)
    w = 20
    lengths = rng.integers(1, 9, 30)
    ptr = ragged(lengths)
    rows = int(ptr[-1])
    idx, score = make_rows(rng, rows, w)
    source, weight = make_sources(rng, rows), rng.choice(EXACT, rows)
    ex = make_exclusions(rng)
    clean = check(idx, score, ptr, 10, "sum", source, weight, ex)
    planted = [P, P + 5, -2, INT32_MIN, 2 ** 31 - 1]
    bad_i, bad_s, bad_src = idx.copy(), score.copy(), source.copy()
    touched = set()
    for k, x in enumerate(planted):
        b = 3 + 2 * k
        bad_i[ptr[b], (5 * k) % w], bad_s[ptr[b], (5 * k) % w] = x, 64.0       # (the best score of its session, were it a candidate)
        touched.add(b)
    bad_i[ptr[20], :5], bad_s[ptr[20], :5] = planted, 64.0
    touched.add(20)
    for b, x in ((22, P), (23, -2), (24, INT32_MIN), (25, 2 ** 31 - 1)):
        r = int(ptr[b])
        bad_src[r] = x
        bad_i[r, 0], bad_s[r, 0] = 59, 64.0                # the row's offer, the best of its session: the row offers nothing
        bad_i[ptr[b]:ptr[b + 1]][bad_i[ptr[b]:ptr[b + 1]] == 59] = 58
        bad_i[r, 0] = 59
        touched.add(b)
    want = oracle(bad_i, bad_s, ptr, 10, "sum", bad_src, weight, ex)
    assert want[3] == 2 * len(planted) + 4
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    got = check(bad_i, bad_s, ptr, 10, "sum", bad_src, weight, ex, want=want, bad=bad)
    assert int(bad) == want[3]
    served = got[0].cpu().numpy()
    assert not np.isin(served, planted).any() and not (served[22:26] == 59).any()
    rest = np.array([b not in touched for b in range(30)])
    assert same(tuple(t[cuda(rest)] for t in got), tuple(t[cuda(rest)] for t in clean))
    # the counter is added to; without a counter the ids are passed over all the same
    assert same(check(bad_i, bad_s, ptr, 10, "sum", bad_src, weight, ex, want=want, bad=bad), got) and int(bad) == 2 * want[3]
    assert same(check(bad_i, bad_s, ptr, 10, "sum", bad_src, weight, ex, want=want), got)
    # row pointers: a descending pair, an entry above R in the middle and at the end, a negative first entry
    for change, count, affected in (({5: int(ptr[4]) - 2}, 1, {4, 5}), ({30: rows + 7}, 1, set()), ({9: rows + 100}, 2, {8, 9}),
                                    ({0: -3}, 1, set()), ({0: -3, 5: int(ptr[4]) - 2, 9: rows + 100, 30: rows + 7}, 5, {4, 5, 8, 9}),
                                    ({12: INT32_MIN, 13: 2 ** 31 - 1}, 3, {11, 12, 13})):
        bent = ptr.copy()
        for at, x in change.items():
            bent[at] = x
        want = oracle(idx, score, bent, 10, "sum", source, weight, ex)
        assert want[3] == count, (change, want[3])
        bad.zero_()
        got = check(idx, score, bent, 10, "sum", source, weight, ex, want=want, bad=bad)
        assert int(bad) == count, change
        rest = cuda(np.array([b not in affected for b in range(30)]))
        assert same(tuple(t[rest] for t in got), tuple(t[rest] for t in clean)), change


# ---- 11. more sessions than the grid holds at once, none, and sessions without rows
def test_grid_stride_no_sessions_and_no_rows():
    from p_companion_amd import ops
    b, w = 4 * 4096 + 5, 8
    rng = np.random.default_rng(4096)
    idx, score = make_rows(rng, b, w, ids=6)
    source = rng.integers(-1, 6, b).astype(np.int32)
    weight = rng.choice(EXACT, b)
    ptr = ragged([1] * b)
    check(idx, score, ptr, 4, "sum", source, weight, num_products=P)
    check(idx, score, ptr, 8, "max")
    out = ops.fuse_sessions(cuda(idx), cuda(score), cuda(ptr[:1]), 3, "sum", cuda(source))
    assert [tuple(t.shape) for t in out] == [(0, 3)] * 3 and [t.dtype for t in out] == [torch.int32, torch.float32, torch.int32]
    # no rows, but sessions: all padding
    counters = [torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(2)]
    got = ops.fuse_sessions(cuda(idx[:0]), cuda(score[:0]), torch.zeros(8, dtype=torch.int32, device="cuda"), 5, "sum",
                            cuda(source[:0]), cuda(weight[:0]), tuple(cuda(a) for a in make_exclusions(rng)),
                            bad=counters[0], truncated=counters[1])
    assert (got[0] == -1).all() and torch.isneginf(got[1]).all() and (got[2] == 0).all() and got[0].shape == (7, 5)
    assert [int(c) for c in counters] == [0, 0]


# ---- 12. through PCompanionInference
def cfg(n_types, dim):
    from types import SimpleNamespace
    return SimpleNamespace(PRODUCT_EMB_DIM=dim, TYPE_EMB_DIM=64, HIDDEN_SIZE=256, NUM_ATTENTION_HEADS=4, DROPOUT=0.0, MARGIN=1.0,
                           ALPHA=0.8, NUM_COMP_TYPES=3, NUM_TYPES=n_types, DEVICE=torch.device("cuda"), LEARNING_RATE=1e-3,
                           BATCH_SIZE=256, NUM_EPOCHS=1)


@pytest.fixture(scope="module")
def served():
    from types import SimpleNamespace
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
    rng = np.random.default_rng(12)
    lengths = np.array([0, 1, 2, 3, 4, 5, 1, 3, 0, 5, 2, 4])
    ptr = ragged(lengths)
    # items drawn near each other, so that co-viewed products and shared complements occur inside a session
    items = np.concatenate([(rng.integers(0, products) + rng.integers(0, 40, n)) % products for n in lengths]).astype(np.int32)
    for b in np.flatnonzero(lengths >= 4):                # an item listed twice: its lists are offered twice
        items[ptr[b] + 1] = items[ptr[b]]
    return SimpleNamespace(inf=inf, model=model, cfg=c, bpg=bpg, host=host, features=g["features"], products=products,
                           lengths=lengths, ptr=ptr, items=items)


def padded(s, width):
    """the ragged sessions as a [B, width] basket, -1 behind each session's items"""
    basket = np.full((len(s.lengths), width), -1, np.int32)
    for b, n in enumerate(s.lengths):
        basket[b, :n] = s.items[s.ptr[b]:s.ptr[b + 1]]
    return torch.from_numpy(basket)


def test_ragged_and_rectangular_sessions_are_the_padded_baskets(served):
    s = served
    items, ptr = torch.from_numpy(s.items), torch.from_numpy(s.ptr)
    rect = torch.from_numpy(np.random.default_rng(3).integers(0, s.products, (9, 3)).astype(np.int32))
    for installed in (False, True):
        if installed:
            s.inf.set_exclusions()
        try:
            for n, per_item, combine in ((10, 8, "sum"), (10, 8, "max"), (48, 16, "sum"), (120, 40, "sum")):
                want = s.inf.recommend_basket_batch(padded(s, 5), n, per_item=per_item, combine=combine)
                got = s.inf.recommend_session_batch(items, ptr, n, per_item=per_item, combine=combine)
                assert got[2].dtype == torch.int64 and got[3].dtype == torch.int32
                assert same(got[:2] + got[3:], want[:2] + want[3:]) and torch.equal(got[2], want[2]), (installed, n, per_item)
                assert (got[0][cuda(s.lengths == 0)] == -1).all() and (got[0][cuda(s.lengths > 0), 0] >= 0).all()
                if per_item == 8:
                    assert (got[3] > 1).any()
                want = s.inf.recommend_basket_batch(rect, n, per_item=per_item, combine=combine)
                got = s.inf.recommend_session_batch(rect.reshape(-1), torch.arange(0, 28, 3, dtype=torch.int32), n,
                                                    per_item=per_item, combine=combine)
                assert same(got[:2] + got[3:], want[:2] + want[3:]) and torch.equal(got[2], want[2]), (installed, n, per_item)
        finally:
            s.inf.set_exclusions(False)


def session_oracle(inf, s, n, per_item, combine, weight, max_items=None):
    """the numpy contract over the items' separately served recommend_batch output"""
    _, idx, sc = inf.recommend_batch(torch.from_numpy(s.items), per_item)
    ex = None if inf.exclusions is None else tuple(t.cpu().numpy() for t in inf.exclusions)
    pool_i, pool_s = idx.reshape(len(s.items), -1).cpu().numpy(), sc.reshape(len(s.items), -1).cpu().numpy()
    assert np.isfinite(pool_s[pool_i >= 0]).all()         # (what is served has a finite score)
    return oracle(pool_i, pool_s, s.ptr, n, combine, s.items, weight, ex, int(inf.type_idx.shape[0]), max_items)


def test_weighted_sessions_against_the_oracle(served):
    s = served
    items, ptr = torch.from_numpy(s.items), torch.from_numpy(s.ptr)
    rng = np.random.default_rng(8)
    length = (ptr[1:] - ptr[:-1]).long()
    age = ptr[1:].repeat_interleave(length, output_size=len(items)) - 1 - torch.arange(len(items))
    recency = torch.pow(0.5, age.float())                  # the docstring's one-liner: powers of two, exact products
    bought = recency.clone()
    bought[torch.from_numpy(s.ptr[:-1][s.lengths >= 3]).long()] = 0.0           # the oldest item of the longer sessions: only banned
    inexact = torch.from_numpy(rng.uniform(0.2, 2.0, len(items)).astype(np.float32))
    for installed in (False, True):
        if installed:
            s.inf.set_exclusions()
        try:
            for weight in (recency, bought, inexact):
                for n, per_item, combine, max_items in ((10, 8, "sum", None), (10, 8, "max", None), (30, 16, "sum", 2)):
                    want = session_oracle(s.inf, s, n, per_item, combine, weight.numpy(), max_items)
                    got = s.inf.recommend_session_batch(items, ptr, n, per_item=per_item, weight=weight, combine=combine,
                                                        max_items=max_items)
                    assert same(got[:2] + got[3:], tuple(cuda(a) for a in want[:3])), (installed, n, per_item, combine)
                    type_idx = s.inf.type_idx.long()
                    assert torch.equal(got[2], torch.where(got[0] >= 0, type_idx[got[0].clamp(min=0).long()], -1))
                    members = [set(s.items[s.ptr[b]:s.ptr[b + 1]].tolist()) for b in range(len(s.lengths))]
                    for b, row in enumerate(got[0].cpu().numpy()):
                        assert not members[b] & set(row.tolist())       # nothing already in the session, bought or not
        finally:
            s.inf.set_exclusions(False)


def test_the_bf16_catalogues(served):
    from p_companion_amd import ops
    from p_companion_amd.inference import CompactInference, PCompanionInference
    s = served
    items, ptr = torch.from_numpy(s.items), torch.from_numpy(s.ptr)
    weight = torch.from_numpy(np.random.default_rng(4).choice(EXACT, len(items)))
    compact = PCompanionInference(s.model, s.cfg, s.bpg, catalogue=ops.CompactCatalogue(s.features))
    bare = PCompanionInference(s.model, s.cfg, s.bpg, catalogue=torch.bfloat16)
    for inf, per_item in ((compact, 8), (compact, 40), (bare, 8), (bare, 16)):
        inf.set_exclusions()
        want = session_oracle(inf, s, 20, per_item, "sum", weight.numpy())
        got = inf.recommend_session_batch(items, ptr, 20, per_item=per_item, weight=weight)
        assert same(got[:2] + got[3:], tuple(cuda(a) for a in want[:3])), per_item
        assert (got[0][cuda(s.lengths > 0), 0] >= 0).all()
        basket = inf.recommend_basket_batch(padded(s, 5), 20, per_item=per_item)
        assert same(inf.recommend_session_batch(items, ptr, 20, per_item=per_item), basket)
    with pytest.raises(ValueError, match="bf16 catalogue serves at most 16"):
        bare.recommend_session_batch(items, ptr, 20, per_item=17)
    assert CompactInference.recommend_session_batch is PCompanionInference.recommend_session_batch
