"""The Product2Vec batch builders of csrc/sampler.hip and pc_p2v_concat_step_rows at every dispatch edge, each output array
compared EXACTLY (integers throughout; `weight` holds small counts) with the project's host references: the Philox oracle
(philox_oracle.build_batch), ops.unique_neighbors / ops.compact_neighbors of the dense matrix, and numpy.  The graphs, the case
lists and the restated dispatch arithmetic are batch_builder_cases.py's; test_batch_builder_cases_host.py proves on the CPU that
the lists reach the branches they name and that every sampler case terminates (the rejection loop has no exit of its own: no
case here is launched without that).  Every assertion names the array that differs.  Needs an MI355X."""
import functools

import numpy as np
import pytest
import torch

import batch_builder_cases as bb

pytestmark = pytest.mark.gpu

K_NB, SEED_NB, STEP_NB = 5, 2 ** 40 + 5, 2 ** 32 + 3            # the sampler's arguments in the neighbour-layout tests


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _to_device(g):
    d = {k: _dev(g[k]) for k in bb.GRAPH_ARRAYS}
    d["n_products"] = g["n_products"]
    return d


@functools.lru_cache(maxsize=None)
def _sampler_graph_dev(p):
    return _to_device(bb.sampler_graph(p))


@functools.lru_cache(maxsize=2)                                   # (the 4 M-product graph is 32 MB: not kept for the session)
def _neighbour_graph_dev(p):
    return _to_device(bb.neighbour_graph(p))


def _same(name, got, want):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = want.detach().cpu().numpy() if isinstance(want, torch.Tensor) else np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape, got.dtype, want.dtype)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        first = tuple(bad[0])
        raise AssertionError(f"{name}: {len(bad)} of {got.size} entries differ, the first at {first}: {got[first]} for {want[first]}")


def _compact_out(b, n_pad, k, n_real):
    i32 = lambda *s: torch.full(s, -9, dtype=torch.int32, device="cuda")
    return {"a": i32(b), "p": i32(b), "ng": i32(b, k), "nb_rows": i32(n_real + 1), "slot_row": i32(b, n_pad), "row_off": i32(b + 1)}


def _check_compact(ops, out, dense, deg):
    ref = ops.compact_neighbors(torch.from_numpy(dense))
    _same("compact nb_rows", out["nb_rows"], ref["nb_rows"])
    _same("compact slot_row", out["slot_row"], ref["slot_row"])
    _same("compact row_off", out["row_off"], np.concatenate([[0], np.cumsum(deg)]).astype(np.int32))


def _check_unique(ops, u, dense):
    ref = ops.unique_neighbors(torch.from_numpy(dense))
    n_u = int(u["n_unique"][0])
    assert n_u == ref["n_unique"], ("n_unique", n_u, ref["n_unique"])
    _same("unique nb_rows", u["nb_rows"][:n_u + 1], ref["nb_rows"])
    _same("unique weight", u["weight"][:n_u + 1], ref["weight"])
    _same("unique slot_row", u["slot_row"], ref["slot_row"])
    _same("unique ref_off", u["ref_off"][:n_u + 2], ref["ref_off"])
    ro, rs, rr = ref["ref_off"].numpy(), u["ref_slot"].cpu().numpy(), ref["ref_slot"].numpy()
    for r in range(n_u):                                          # the same slots per row (arrival order is free)
        assert sorted(rs[ro[r]:ro[r + 1]].tolist()) == rr[ro[r]:ro[r + 1]].tolist(), ("unique ref_slot of row", r)
    return n_u


def _all_entries(ops, g, gd, ids, k, seed, step, n_pad):
    """the dense entry at n_pad, the compact and unique entries at max(n_pad, 1): the three sampler arrays of the latter two
    equal the dense entry's bit for bit, their layouts equal the host constructions of the dense matrix.  Returns the dense
    entry's four arrays."""
    idd = _dev(ids)
    b = len(ids)
    a, p, ng, nb = ops.build_similarity_batch(idd, gd, n_pad, k, seed, step)
    assert (nb is None) == (n_pad == 0)
    n2 = max(n_pad, 1)
    deg = bb.capped_degrees(g, ids, n2)
    dense = bb.dense_neighbors(g, ids, n2)
    n_real = int(deg.sum())
    out = _compact_out(b, n2, k, n_real)
    ca, cp, cng, comp = ops.build_similarity_batch_compact(idd, gd, n2, k, seed, step, n_real, out=out)
    ua, up, ung, uq = ops.build_similarity_batch_unique(idd, gd, n2, k, seed, step, n_real)
    for name, x, y, z in (("anchor_idx", a, ca, ua), ("positive_idx", p, cp, up), ("negative_idx", ng, cng, ung)):
        _same("compact entry's " + name, y, x)
        _same("unique entry's " + name, z, x)
    _check_compact(ops, out, dense, deg)
    _check_unique(ops, uq, dense)
    return a, p, ng, nb


# ------------------------------------------------------------------ negatives and pairs
@pytest.mark.parametrize("case", bb.SAMPLER_CASES, ids=bb.case_id)
def test_sampler_equals_the_philox_oracle_through_every_entry(case):
    """K in {1, 5, 8, 9, 12} (8 negatives in registers / re-read from negative_idx), anchors with 1, 8, 9 and 20 positives (the
    tail loop past the eighth), B on both sides of the 128-thread workgroup, P from the loader guard's minimum (the anchor with
    20 positives has K eligible products) over 1023 / 1024 (`bits`) to 2^20 + 1, and (seed, step) with all four key / counter
    words in use."""
    from p_companion_amd import ops
    g, ids, k, seed, step, n_pad = bb.sampler_inputs(case)
    (ra, rp, rng_, rnb), trace = bb.sampler_expected(case)
    assert max(t["words"] for t in trace) <= bb.MAX_DRAWS          # terminates: established on the host, before the launch
    a, p, ng, nb = _all_entries(ops, g, _sampler_graph_dev(g["n_products"]), ids, k, seed, step, n_pad)
    _same("anchor_idx", a, ra)
    _same("positive_idx", p, rp)
    _same("negative_idx", ng, rng_)
    if n_pad:
        _same("neighbor_idx", nb, rnb)


@pytest.mark.parametrize("case", bb.SAMPLER_WIDE_CASES, ids=bb.case_id)
def test_sampler_workgroups_in_front_of_the_counting_workgroups(case):
    """B = 1025 and 4096: 9 and 32 sampler workgroups lead uq_pairs_count_kernel's grid, with the block arithmetic of that
    kernel; the three arrays equal the dense entry's (no oracle: pure Python is too slow at this size)."""
    from p_companion_amd import ops
    g, ids, k, seed, step, n_pad = bb.sampler_inputs(case)
    assert max(t["words"] for t in bb.sampler_expected(case)[1]) <= bb.MAX_DRAWS
    a, p, ng, nb = _all_entries(ops, g, _sampler_graph_dev(g["n_products"]), ids, k, seed, step, n_pad)
    _same("anchor_idx", a, g["sim_pairs"][ids, 0])
    _same("positive_idx", p, g["sim_pairs"][ids, 1])
    _same("neighbor_idx", nb, bb.dense_neighbors(g, ids, n_pad))
    _same("negative_idx", ng, bb.sampler_expected(case)[0][2])      # (the host run that proved termination has them anyway)


# ------------------------------------------------------------------ dense neighbours
@pytest.mark.parametrize("n_pad", bb.DENSE_NPADS)
def test_dense_neighbours_below_at_and_above_the_largest_degree(n_pad):
    from p_companion_amd import ops
    g = bb.neighbour_graph(5000)
    ids = bb.compact_batch(g, 300)
    a, p, ng, nb = ops.build_similarity_batch(_dev(ids), _neighbour_graph_dev(5000), n_pad, K_NB, SEED_NB, STEP_NB)
    _same("anchor_idx", a, g["sim_pairs"][ids, 0])
    if n_pad == 0:
        assert nb is None
        return
    want = bb.dense_neighbors(g, ids, n_pad)
    assert (want[:, 0] == -1).any() and (want >= 0).any()           # anchors of degree 0 among the others
    _same("neighbor_idx", nb, want)


# ------------------------------------------------------------------ compact layout
@pytest.mark.parametrize("b", bb.COMPACT_BS)
def test_compact_layout_at_every_chunking_of_the_degree_scan(b):
    """per = ceil(B / 1024) anchors per thread, read eight at a time: 1, 2 (B = 1025: threads past 512 own nothing), 4 and 9 (a
    second, ragged trip); degrees 0 .. 9 capped at n_pad = 6"""
    from p_companion_amd import ops
    g = bb.neighbour_graph(5000)
    ids = bb.compact_batch(g, b)
    deg = bb.capped_degrees(g, ids, bb.NB_NPAD)
    out = _compact_out(b, bb.NB_NPAD, K_NB, int(deg.sum()))
    a, p, ng, comp = ops.build_similarity_batch_compact(_dev(ids), _neighbour_graph_dev(5000), bb.NB_NPAD, K_NB, SEED_NB, STEP_NB,
                                                        int(deg.sum()), out=out)
    assert comp["nb_rows"] is out["nb_rows"] and comp["slot_row"] is out["slot_row"]
    _same("anchor_idx", a, g["sim_pairs"][ids, 0])
    _check_compact(ops, out, bb.dense_neighbors(g, ids, bb.NB_NPAD), deg)
    assert int(out["row_off"][b]) == int(deg.sum())


@pytest.mark.parametrize("b", (1, 1025))
def test_compact_layout_of_a_batch_without_any_neighbour(b):
    from p_companion_amd import ops
    g = bb.neighbour_graph(5000)
    ids = bb.compact_batch(g, b, bare_only=True)
    out = _compact_out(b, bb.NB_NPAD, K_NB, 0)
    ops.build_similarity_batch_compact(_dev(ids), _neighbour_graph_dev(5000), bb.NB_NPAD, K_NB, SEED_NB, STEP_NB, 0, out=out)
    _same("compact nb_rows", out["nb_rows"], np.asarray([-1], np.int32))
    _same("compact slot_row", out["slot_row"], np.zeros((b, bb.NB_NPAD), np.int32))
    _same("compact row_off", out["row_off"], np.zeros(b + 1, np.int32))


# ------------------------------------------------------------------ unique layout
@pytest.mark.parametrize("p", bb.UNIQUE_PS)
def test_unique_layout_on_chunk_edges_on_one_scratch(p):
    """One to 1024 chunks of 1024 products (256 threads; more than 256 chunks: the predecessor loop strides) and 257 / 977
    chunks of 4096 (1024 threads), neighbours on the first and last product of the first, last and 257th chunk.  Five batches on
    one scratch -- the batch, the batch again, one over disjoint products, one product in every slot, padding alone -- and
    after each the per-product counters (the first 4 * P bytes of the scratch) are all zero."""
    from p_companion_amd import ops
    g, batches = bb.unique_batches(p)
    gd = _neighbour_graph_dev(p)
    scratch = None
    for name, ids in batches:
        dense = bb.dense_neighbors(g, ids, bb.NB_NPAD)
        n_real = int((dense >= 0).sum())
        idd = _dev(ids)
        a, p_, ng, u = ops.build_similarity_batch_unique(idd, gd, bb.NB_NPAD, K_NB, SEED_NB, STEP_NB, n_real)
        try:
            n_u = _check_unique(ops, u, dense)
        except AssertionError as e:
            raise AssertionError(f"batch '{name}': {e}") from None
        a2, p2, ng2, _ = ops.build_similarity_batch(idd, gd, 0, K_NB, SEED_NB, STEP_NB)
        _same(name + ": anchor_idx", a, a2); _same(name + ": positive_idx", p_, p2); _same(name + ": negative_idx", ng, ng2)
        if name == "hot":
            assert n_u == 1 and u["nb_rows"][:2].tolist() == [p - 1, -1]
            assert u["weight"][:2].tolist() == [float(bb.HOT_B * bb.NB_NPAD), 0.0]
        if name == "padding":
            assert n_u == 0 and u["nb_rows"][:1].tolist() == [-1] and u["weight"][:1].tolist() == [float(len(ids) * bb.NB_NPAD)]
        mine = [v for key, v in ops._uq_scratch.items() if key[1] == p and key[2] == torch.cuda.current_stream().cuda_stream]
        assert len(mine) == 1 and (scratch is None or mine[0] is scratch), "the five calls must share one scratch"
        scratch = mine[0]
        cnt = scratch[:4 * p].view(torch.int32)
        assert cnt.numel() == p and not bool(cnt.any()), f"batch '{name}' left {int((cnt != 0).sum())} counters set"


# ------------------------------------------------------------------ concat_step_rows
@pytest.mark.parametrize("case", bb.CONCAT_CASES, ids=bb.case_id)
def test_concat_step_rows_clamps_the_device_count_and_writes_no_further(case):
    """[anchor | nb_rows[0 .. U] | positive | negatives] with U read on the device and clamped into [0, capacity - 1]; the
    entries behind the written length keep the sentinel"""
    from p_companion_amd import ops
    b, k, cap, n_unique = case
    rng = np.random.default_rng(b + k + cap)
    a, p = rng.integers(0, 1 << 30, b).astype(np.int32), rng.integers(0, 1 << 30, b).astype(np.int32)
    ng, nb_rows = rng.integers(0, 1 << 30, (b, k)).astype(np.int32), rng.integers(0, 1 << 30, cap).astype(np.int32)
    out_len = b * (2 + k) + cap + 3
    out = torch.full((out_len,), bb.CONCAT_SENTINEL, dtype=torch.int32, device="cuda")
    got = ops.concat_step_rows(_dev(a), _dev(p), _dev(ng), _dev(nb_rows), _dev(np.asarray([n_unique], np.int32)), out=out)
    assert got is out
    _same("step_rows", out, bb.concat_expected(a, p, ng, nb_rows, n_unique, out_len))


# ------------------------------------------------------------------ epoch_plan
@pytest.mark.parametrize("case", bb.PLAN_CASES, ids=bb.case_id)
def test_epoch_plan_of_every_batch(case):
    """(max, sum) of every batch against numpy: n < B, n = 3 B, a last batch of one element, B below and above the 256
    threads, with and without an order; degrees of 2^20 at B = 4096 sum to 2^32 (the long long accumulation)"""
    from p_companion_amd import ops
    n, b, shuffled, kind = case
    deg, order, n_batches = bb.plan_inputs(case)
    plan = ops.epoch_plan(_dev(order) if shuffled else None, _dev(deg), n, b, n_batches)
    _same("plan", plan, bb.plan_expected(deg, order, n, b))
