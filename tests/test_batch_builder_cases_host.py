"""CPU checks behind tests/test_gpu_batch_builders.py (batch_builder_cases.py holds the graphs, the lists and the references).
The case lists reach the branches they name; every sample of every sampler case terminates -- the rejection loop of
pairs_negatives_body has no exit of its own and ops.* does not repeat the loader's guard, so termination is established here, on
the Philox oracle, before a case is ever launched --; and the three builder entries refuse what they must before a launch."""
import ctypes

import numpy as np
import pytest

import batch_builder_cases as bb
from oracle import philox_oracle

PC_EINVAL, PC_ESHAPE, PC_EWORKSPACE = -1, -2, -3


# ------------------------------------------------------------------ graphs and the traced oracle
def test_make_graph_lists_only_the_given_anchors():
    g = bb.make_graph(50, [(49, [3, 4], [7]), (0, [9], []), (20, [1, 2, 3], [5, 5, 6])])
    assert g["n_products"] == 50 and g["sim_pairs"].tolist() == [[0, 9], [20, 1], [20, 2], [20, 3], [49, 3], [49, 4]]
    assert g["pair_start"] == {0: 0, 20: 1, 49: 4}
    assert g["sim_col"].tolist() == [9, 1, 2, 3, 3, 4] and g["cv_col"].tolist() == [5, 5, 6, 7]
    for key in ("sim_rowptr", "cv_rowptr"):
        assert g[key].dtype == np.int32 and len(g[key]) == 51 and g[key][0] == 0
    assert np.flatnonzero(np.diff(g["sim_rowptr"])).tolist() == [0, 20, 49]
    assert np.flatnonzero(np.diff(g["cv_rowptr"])).tolist() == [20, 49]
    assert bb.dense_neighbors(g, np.array([5, 0, 1]), 2).tolist() == [[7, -1], [-1, -1], [5, 5]]
    assert bb.capped_degrees(g, np.array([5, 0, 1]), 2).tolist() == [1, 0, 2]


def test_traced_oracle_counts_every_reason_and_leaves_the_oracle_unchanged():
    g = bb.make_graph(12, [(3, [0, 1, 2, 4, 5, 6, 7, 8, 9, 10], [1])])       # one eligible product: 11
    ids = np.zeros(3, np.int32)
    (a, p, ng, nb), tr = bb.traced_oracle(g, ids, 1, 1, 5, 9)
    plain = philox_oracle.build_batch(ids, g["sim_pairs"], g["cv_rowptr"], g["cv_col"], g["sim_rowptr"], g["sim_col"], 12, 1, 1, 5, 9)
    for x, y in zip((a, p, ng, nb), plain):
        assert np.array_equal(x, y)
    assert ng.tolist() == [[11]] * 3                                          # the one product left
    for t in tr:
        assert t["draws"] == 1 + sum(t[r] for r in bb.REASONS) and t["words"] >= t["draws"] and t["repeat"] == 0
    assert sum(t["first8"] for t in tr) > 0 and sum(t["tail"] for t in tr) > 0


# ------------------------------------------------------------------ negatives and pairs
def test_sampler_cases_cover_every_listed_value():
    cs = bb.SAMPLER_CASES
    assert {c[1] for c in cs} == {1, 5, 8, 9, 12} and {c[2] for c in cs} == {1, 127, 128, 129, 300}
    assert {c[0] for c in cs} == {"min", 1023, 1024, 1000, (1 << 20) + 1} and {c[3] for c in cs} == {0, 1, 2}
    assert {(c[0], c[1]) for c in cs} >= {(p, k) for p in bb.SAMPLER_PS for k in bb.SAMPLER_KS}
    assert {(c[2], c[3]) for c in cs if c[1] > bb.NNEG} >= {(b, s) for b in bb.SAMPLER_BS for s in range(3)}
    assert bb.SAMPLER_SEEDS == ((0, 0), ((7 << 33) + 9, 12345), (2 ** 40 + 5, 2 ** 32 + 3))
    assert bb.SAMPLER_SEEDS[2][1] >> 32 and bb.SAMPLER_SEEDS[2][0] >> 32 and bb.SAMPLER_SEEDS[1][0] >> 32
    assert {bb.pair_blocks(b) for b in bb.SAMPLER_BS} == {1, 2, 3} and bb.pair_blocks(128) == 1 and bb.pair_blocks(129) == 2
    assert {c[2] for c in bb.SAMPLER_WIDE_CASES} == {1025, 4096} and {bb.pair_blocks(c[2]) for c in bb.SAMPLER_WIDE_CASES} == {9, 32}
    assert any(c[1] > bb.NNEG for c in bb.SAMPLER_WIDE_CASES) and any(c[1] <= bb.NNEG for c in bb.SAMPLER_WIDE_CASES)
    n_pads = set()
    for c in cs + bb.SAMPLER_WIDE_CASES:
        g, ids, k, seed, step, n_pad = bb.sampler_inputs(c)
        p = g["n_products"]
        pos = np.diff(g["sim_rowptr"])
        assert sorted(pos[pos > 0].tolist()) == [1, 8, 9, 20]
        assert bb.loader_guard(int(pos.max()), k, p)                           # no case the loader would refuse
        assert (c[0] == "min") == (not bb.loader_guard(int(pos.max()), k, p - 1))
        assert len(ids) == c[2] and ids.max() < len(g["sim_pairs"])
        a = g["sim_pairs"][ids, 0]
        if c[2] >= 4:                                                          # 1, 8, 9 and 20 positives in one batch
            assert sorted(pos[a[:4]].tolist()) == [1, 8, 9, 20]
        else:
            assert pos[a[0]] == 20                                             # the single sample: both positive loops
        for x in set(a.tolist()):                                              # positives: distinct, never the anchor
            row = g["sim_col"][g["sim_rowptr"][x]:g["sim_rowptr"][x + 1]].tolist()
            assert len(set(row)) == len(row) and x not in row
        assert {p - 1, 0} <= set(g["anchors"])
        if c in cs:
            n_pads.add(n_pad)
    cv = np.diff(bb.sampler_graph(1000)["cv_rowptr"])
    assert cv.max() == 12 and n_pads == {0, 11, 12, 14} and sorted(cv[cv > 0].tolist()) == [3, 7, 12]


def test_every_sampler_case_terminates_and_every_rejection_reason_occurs():
    seen = {r: 0 for r in bb.REASONS}
    seen_k9 = dict(seen)
    tail8 = tail8_k9 = 0
    worst = (0, None)
    for c in bb.SAMPLER_CASES + bb.SAMPLER_WIDE_CASES:
        (a, p, ng, nb), tr = bb.sampler_expected(c)
        k = c[1]
        assert ng.shape == (c[2], k)
        for i, t in enumerate(tr):
            assert t["draws"] == k + sum(t[r] for r in bb.REASONS)
            assert len(set(ng[i].tolist())) == k
        words = max(t["words"] for t in tr)
        worst = max(worst, (words, c))
        if c not in bb.SAMPLER_CASES:
            continue
        for r in bb.REASONS:
            n = sum(t[r] for t in tr)
            seen[r] += n
            seen_k9[r] += n if k > bb.NNEG else 0
        tail8 += sum(t["tail8"] for t in tr)
        tail8_k9 += sum(t["tail8"] for t in tr) if k > bb.NNEG else 0
    print("largest draw count of a sample:", worst, "rejections:", seen, "at K > 8:", seen_k9, "as the ninth positive:", tail8)
    assert worst[0] <= bb.MAX_DRAWS                                            # what makes the GPU run safe
    assert all(seen[r] > 0 for r in bb.REASONS), seen
    assert seen_k9["tail"] > 0 and seen_k9["repeat"] > 0 and seen_k9["first8"] > 0 and seen_k9["anchor"] > 0, seen_k9
    assert tail8 > 0 and tail8_k9 > 0                                          # the FIRST positive the tail loop reads
    # a repeat of a negative past the eighth: only negative_idx holds it
    late = 0
    for c in bb.SAMPLER_CASES:
        if c[1] > bb.NNEG and c[0] == "min":
            g, ids, k, seed, step, n_pad = bb.sampler_inputs(c)
            hits = []
            philox_oracle.build_batch(ids, g["sim_pairs"], g["cv_rowptr"], g["cv_col"], g["sim_rowptr"], g["sim_col"],
                                      g["n_products"], 0, k, seed, step, on_draw=lambda i, x, s: hits.append((i, x)))
            ng = bb.sampler_expected(c)[0][2]
            got = {}
            for i, x in hits:
                row = ng[i].tolist()
                if x in row:
                    if x in got.setdefault(i, []) and row.index(x) >= bb.NNEG:
                        late += 1
                    got[i].append(x)
    assert late > 0


# ------------------------------------------------------------------ neighbour layouts
def test_unique_cases_fall_on_both_sides_of_every_dispatch_edge():
    assert bb.UNIQUE_PS == (1024, 1025, 5000, 262_144, 263_169, 1 << 20, (1 << 20) + 1, 4_000_000)
    assert bb.uq_chunk(1 << 20) == 1024 and bb.uq_chunk((1 << 20) + 1) == 4096
    assert bb.uq_threads(1 << 20) == 256 and bb.uq_threads((1 << 20) + 1) == 1024 and bb.uq_threads(4_000_000) == 1024
    assert [bb.uq_nblk(p) for p in bb.UNIQUE_PS] == [1, 2, 5, 256, 258, 1024, 257, 977]
    small = [bb.uq_nblk(p) for p in bb.UNIQUE_PS if bb.uq_threads(p) == 256]
    assert any(n <= 256 for n in small) and any(n > 256 for n in small) and 256 in small and 258 in small
    assert all(bb.uq_nblk(p) <= bb.UQ_MAX_BLOCKS for p in bb.UNIQUE_PS) and max(bb.UNIQUE_PS) == 4_000_000
    assert bb.uq_nblk(4096 * 4096) == 4096 and bb.uq_nblk(4096 * 4096 + 1) == 4097


@pytest.mark.parametrize("p", bb.UNIQUE_PS)
def test_unique_batches_place_products_on_the_chunk_edges(p):
    g, batches = bb.unique_batches(p)
    c, n = bb.uq_chunk(p), bb.uq_nblk(p)
    assert [name for name, _ in batches] == ["first", "again", "disjoint", "hot", "padding"]
    dense = {name: bb.dense_neighbors(g, ids, bb.NB_NPAD) for name, ids in batches}
    first = set(dense["first"][dense["first"] >= 0].tolist())
    edge = set(g["edge"])
    assert edge <= first                                                       # none cut by the cap, none left undealt
    assert {0, c - 1, (n - 1) * c, p - 1} <= edge                              # first / last of a chunk, of the first / last chunk
    assert any(x % c == 0 for x in edge) and any(x % c == c - 1 for x in edge)
    assert any(x // c == 0 for x in edge) and any(x // c == n - 1 for x in edge)
    if n > 256:                                                                # what the second trip of the prefix loop adds
        assert {x for x in (256 * c, 257 * c - 1) if x < p} <= edge and any(x // c >= 256 for x in edge)
        assert n <= bb.uq_threads(p) or any(x // c > 256 for x in edge)        # a chunk BEHIND one the second trip reads
    if n > 2:
        assert {c, 2 * c - 1, (n - 1) * c - 1} <= edge
    third = set(dense["disjoint"][dense["disjoint"] >= 0].tolist())
    assert third and not (third & first) and np.array_equal(batches[0][1], batches[1][1])
    assert len(first) < int((dense["first"] >= 0).sum())                       # products repeat: weights above 1
    assert (dense["hot"] == p - 1).all() and dense["hot"].shape == (bb.HOT_B, bb.NB_NPAD)
    assert (dense["padding"] == -1).all()
    deg = np.diff(g["cv_rowptr"])
    assert deg.max() > bb.NB_NPAD and {bb.NB_NPAD - 1, bb.NB_NPAD, bb.NB_NPAD + 1} <= set(deg.tolist())
    assert set(bb.capped_degrees(g, batches[0][1], bb.NB_NPAD).tolist()) == {0, 1, 2, 3, 5, 6}
    assert max(bb.DENSE_NPADS) > deg.max() and deg.max() in bb.DENSE_NPADS and 0 in bb.DENSE_NPADS
    assert any(0 < x < deg.max() for x in bb.DENSE_NPADS)


def test_compact_cases_cover_every_chunking_of_the_degree_scan():
    assert bb.COMPACT_BS == (1, 1023, 1024, 1025, 4096, 8193, 9000)
    assert [bb.scan_per(b) for b in bb.COMPACT_BS] == [1, 1, 1, 2, 4, 9, 9]
    assert 1025 - 512 * bb.scan_per(1025) == 1                                 # thread 512 owns one anchor, 513 .. 1023 none
    for b in (8193, 9000):                                                     # a second, ragged trip of the eight-wide loop
        per = bb.scan_per(b)
        assert per > 8 and per % 8
    assert 8193 % bb.scan_per(8193) and 9000 % bb.scan_per(9000) == 0          # a ragged last owner (thread 910) and a full one
    assert 4096 % bb.scan_per(4096) == 0 and 4096 // bb.scan_per(4096) == 1024 # every thread owns four
    g = bb.neighbour_graph(5000)
    for b in bb.COMPACT_BS:
        ids = bb.compact_batch(g, b)
        deg = np.diff(g["cv_rowptr"])[g["sim_pairs"][ids, 0]]
        assert len(ids) == b and (b < 100 or {0, 9} <= set(deg.tolist()))      # bare anchors and capped ones in one batch
    assert not bb.capped_degrees(g, bb.compact_batch(g, 1025, bare_only=True), bb.NB_NPAD).any()
    # What an output comparison can and cannot see of `per`: the scan is right for EVERY per with 1024 * per >= B (B / 1024 + 1
    # only moves the ownership), and wrong as soon as the threads do not cover the batch.
    for b in bb.COMPACT_BS:
        deg = bb.capped_degrees(g, bb.compact_batch(g, b), bb.NB_NPAD)
        want = np.concatenate([[0], np.cumsum(deg)])
        for per in (bb.scan_per(b), b // 1024 + 1):
            assert np.array_equal(bb.degree_scan_restated(deg, per), want), (b, per)
        if b > 1024 and b % 1024:
            assert not np.array_equal(bb.degree_scan_restated(deg, b // 1024), want), b


# ------------------------------------------------------------------ concat_step_rows, epoch_plan
def test_concat_and_plan_cases_cover_the_listed_shapes():
    kinds = set()
    for b, k, cap, nu in bb.CONCAT_CASES:
        kinds.add("zero" if nu == 0 else "full" if nu + 1 == cap else "over" if nu + 1 > cap else "negative" if nu < 0 else "part")
    assert kinds == {"zero", "full", "over", "negative", "part"}
    a, p, ng, nb = np.arange(2), np.arange(2) + 10, np.arange(6).reshape(2, 3) + 20, np.arange(4) + 30
    assert bb.concat_expected(a, p, ng, nb, 1, 13).tolist() == [0, 1, 30, 31, 10, 11, 20, 21, 22, 23, 24, 25, -77]
    assert bb.concat_expected(a, p, ng, nb, 9, 14).tolist() == [0, 1, 30, 31, 32, 33, 10, 11, 20, 21, 22, 23, 24, 25]
    assert bb.concat_expected(a, p, ng, nb, -3, 11).tolist()[:4] == [0, 1, 30, 10]
    cs = bb.PLAN_CASES
    assert {c[1] for c in cs} == {1, 255, 257, 4096} and {c[2] for c in cs} == {False, True}
    for b in bb.PLAN_BS:
        ns = {c[0] for c in cs if c[1] == b}
        assert 3 * b in ns and (b == 1 or any(n % b == 1 and n > b for n in ns) and any(n < b for n in ns))
    big = [c for c in cs if c[3] == "big"]
    assert {c[2] for c in big} == {False, True}
    for c in big:
        deg, order, nb_ = bb.plan_inputs(c)
        want = bb.plan_expected(deg, order, c[0], c[1])
        assert want.tolist() == [[1 << 20, 1 << 32], [1 << 20, 1 << 32], [1 << 20, 1 << 20]] and nb_ == 3
    deg, order, nb_ = bb.plan_inputs((511, 255, True, "small"))
    want = bb.plan_expected(deg, order, 511, 255)
    assert nb_ == 3 and want[2].tolist() == [deg[order[510]]] * 2 and sorted(order.tolist()) == list(range(511))


# ------------------------------------------------------------------ what the entries refuse before a launch
def _args(entry, **kw):
    """arguments that pass every check of `entry` up to the scratch size; no check dereferences the pointers"""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))
    a = dict(pair_ids=p, batch=4, sim_pairs=p, cv_rowptr=p, cv_col=p, sim_rowptr=p, sim_col=p, n_products=100, n_pad=3, k_neg=5,
             seed=1, step=2)
    if entry == "unique":
        a.update(n_real=7, anchor=p, positive=p, negative=p, nb_rows=p, weight=p, slot_row=p, ref_off=p, ref_slot=p, n_unique=p,
                 scratch=p, scratch_bytes=0, stream=None)
    elif entry == "compact":
        a.update(anchor=p, positive=p, negative=p, nb_rows=p, slot_row=p, row_off=p, stream=None)
    else:
        a.update(anchor=p, positive=p, negative=p, neighbor=p, stream=None)
    a.update(kw)
    return buf, list(a.values())


def _call(entry, **kw):
    from p_companion_amd import _lib
    name = {"unique": "pc_build_similarity_batch_unique", "compact": "pc_build_similarity_batch_compact",
            "dense": "pc_build_similarity_batch"}[entry]
    buf, args = _args(entry, **kw)
    return getattr(_lib.lib(), name)(*args)


def test_unique_entry_refuses_more_than_4096_chunks_and_a_short_scratch():
    from p_companion_amd import _lib
    assert _call("unique", n_products=4096 * 4096 + 1) == PC_ESHAPE
    assert _call("unique", n_products=4096 * 4096) == PC_EWORKSPACE             # accepted as a shape: the scratch is 0 bytes
    for p in ((1 << 20), (1 << 20) + 1, 4_000_000, 100):
        assert _call("unique", n_products=p) == PC_EWORKSPACE, p
    ws = _lib.lib().pc_build_similarity_batch_unique_scratch_bytes
    for p, slots in ((100, 12), (1024, 1), (1025, 300), ((1 << 20) + 1, 4096 * 32), (4_000_000, 4096 * 64)):
        need = ws(p, slots)
        assert need == 4 * (2 * p + 2 * ((p + 1023) // 1024) + slots + 1)
        assert _call("unique", n_products=p, batch=1, n_pad=slots, n_real=0, scratch_bytes=need - 1) == PC_EWORKSPACE
    assert ws(0, 5) == 0 and ws(5, 0) == 0


def test_builder_entries_refuse_bad_sizes_with_einval():
    # n_real outside [0, batch * n_pad]: PC_EINVAL; the two ends of the range pass on to the scratch check
    assert _call("unique", n_real=-1) == PC_EINVAL and _call("unique", n_real=13) == PC_EINVAL
    assert _call("unique", n_real=0) == PC_EWORKSPACE and _call("unique", n_real=12) == PC_EWORKSPACE
    assert _call("unique", n_products=7) == PC_EWORKSPACE                       # k_neg + 2 products: enough
    for entry in ("unique", "compact", "dense"):
        assert _call(entry, n_products=6) == PC_EINVAL, entry                   # k_neg + 1 products
        assert _call(entry, n_products=0) == PC_EINVAL and _call(entry, n_products=-5) == PC_EINVAL, entry
        assert _call(entry, batch=0) == PC_EINVAL and _call(entry, k_neg=0) == PC_EINVAL, entry
        assert _call(entry, n_pad=-1) == PC_EINVAL, entry
        for name in ("pair_ids", "sim_pairs", "cv_rowptr", "cv_col", "sim_rowptr", "sim_col", "anchor", "positive", "negative"):
            assert _call(entry, **{name: None}) == PC_EINVAL, (entry, name)
    assert _call("unique", n_pad=0) == PC_EINVAL and _call("compact", n_pad=0) == PC_EINVAL
    assert _call("dense", n_pad=3, neighbor=None) == PC_EINVAL
    for name in ("nb_rows", "weight", "slot_row", "ref_off", "ref_slot", "n_unique", "scratch"):
        assert _call("unique", **{name: None}) == PC_EINVAL, name
    for name in ("nb_rows", "slot_row", "row_off"):
        assert _call("compact", **{name: None}) == PC_EINVAL, name
