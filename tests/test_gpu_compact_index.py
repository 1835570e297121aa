"""The cell index over the bf16 catalogue: pc_cell_means_bf16 (csrc/cells_bf16.hip), ops.cell_means_bf16,
ops.build_cell_index_bf16 and inference.IndexedCompactSimilarProducts.  Needs an MI355X.

References are float64 numpy in this file, over the STORED (rounded) rows widened.  Bounds:
  means        bit for bit ops.cell_means on the widened table: the same lanes own the same columns, the same groups add the same
               members in the same order, the same tree, the same division -- and the widening is exact.  Against float64 the
               fp32 kernel's own bound, |got - fp64| <= (m + 1) 2^-24 (sum_i |x_id|) / m per coordinate (the order-independent
               forward bound of an fp32 sum of m terms and the one division); on integer data every sum is exact and the result is
               np.float32(sum) / np.float32(m) bit for bit.
  build        every field of the index bit for bit ops.build_cell_index on the widened table, for any chunk_rows.
  build memory the widened chunk is chunk_rows * D * 4 bytes; the allowance above the fp32 build's peak is two of them, and the
               whole peak stays under half of a [P, D] fp32 table.
  lists        exact: with every cell probed, ids and distance bits equal CompactSimilarProducts(scope="catalogue"); with fewer
               cells, on data whose sums are exact in fp32, ids equal the float64 L2 order over the probed cells' products.
  probe        the biased entry's allowance of tests/test_gpu_nearest.py, (D + 2) 2^-24 (sum_d |x_d c_d| + |b_c|) per score
               (check_biased of that file): the centroids' means are no integers."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_nearest import U, check_biased, ordered

# around G (8 at D = 128, 4 at D = 256), 4 G (the unrolled loop) and the tree's widths, for both D
SIZES = (0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1000)
FIELDS = ("centroids", "centroid_bias", "cell_of", "cell_rowptr", "cell_col")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy() if t.dtype == torch.float32 else t.detach().cpu().numpy()


def rounded(x):
    """(the bf16 device table of x, its widened rows as fp32 numpy)"""
    tb = dev(x.astype(np.float32)).to(torch.bfloat16).contiguous()
    return tb, tb.float().cpu().numpy()


def cells_csr(P, seed):
    """len(SIZES) cells of SIZES members, a shuffled cell_col over a part of range(P): some products are in no cell."""
    rng = np.random.default_rng(seed)
    col = rng.permutation(P)[:sum(SIZES)].astype(np.int32)
    rowptr = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
    return rowptr, col


@functools.lru_cache(maxsize=None)
def normal_case(dim):
    """One table, CSR, prior and fp32 reference run per D, shared by the means tests and left unchanged."""
    from p_companion_amd import ops
    P = 4000
    rng = np.random.default_rng(dim)
    tb, x = rounded(rng.standard_normal((P, dim)))
    prior = rng.standard_normal((len(SIZES), dim)).astype(np.float32)
    rowptr, col = cells_csr(P, dim + 1)
    want = ops.cell_means(tb.float(), dev(rowptr), dev(col), dev(prior))
    return SimpleNamespace(P=P, tb=tb, x=x, prior=prior, rowptr=rowptr, col=col, want=bits(want))


# ---- 1. the means, bit for bit
@pytest.mark.parametrize("dim", [128, 256])
def test_means_have_the_bits_of_the_fp32_kernel_on_the_widened_table(dim):
    from p_companion_amd import ops
    c = normal_case(dim)
    cen = dev(c.prior)
    out = ops.cell_means_bf16(c.tb, dev(c.rowptr), dev(c.col), cen)
    assert out is cen and cen.dtype == torch.float32
    got = bits(cen)
    for k, m in enumerate(SIZES):
        assert (got[k] == c.want[k]).all(), f"cell {k} ({m} members) differs from cell_means(table.float())"
    with pytest.raises(TypeError):                                                # (new names only)
        ops.cell_means(c.tb, dev(c.rowptr), dev(c.col), dev(c.prior))


# ---- 2. the means, other properties
@pytest.mark.parametrize("dim", [128, 256])
def test_means_against_float64_the_empty_cell_and_run_to_run(dim):
    from p_companion_amd import ops
    c = normal_case(dim)
    cen = dev(c.prior)
    ops.cell_means_bf16(c.tb, dev(c.rowptr), dev(c.col), cen)
    got = cen.cpu().numpy()
    worst = 0.0
    for k, m in enumerate(SIZES):
        ids = c.col[c.rowptr[k]:c.rowptr[k + 1]]
        if m == 0:
            assert (got[k].view(np.int32) == c.prior[k].view(np.int32)).all()      # the empty cell keeps its prior bits
            continue
        x64 = c.x[ids].astype(np.float64)
        err = np.abs(got[k].astype(np.float64) - x64.sum(0) / m)
        bound = (m + 1) * U * np.abs(x64).sum(0) / m
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), f"cell {k} ({m} members): error / bound = {(err / bound).max():.3f}"
    print(f"cell_means_bf16 D = {dim}: worst error / bound = {worst:.4f}")
    runs = []
    for k in range(3):
        c2 = dev(c.prior)
        if k == 2:                                                                # (after unrelated work on the device)
            (torch.randn(512, 512, device="cuda") @ torch.randn(512, 512, device="cuda")).sum().item()
            ops.half_sq_norm_bias_bf16(c.tb)
        ops.cell_means_bf16(c.tb, dev(c.rowptr), dev(c.col), c2)
        runs.append(bits(c2))
    assert (runs[0] == bits(cen)).all() and (runs[1] == runs[0]).all() and (runs[2] == runs[0]).all()


@pytest.mark.parametrize("dim", [128, 256])
def test_means_on_integer_data_are_exact(dim):
    from p_companion_amd import ops
    P = 4000
    rng = np.random.default_rng(dim + 7)
    tb, x = rounded(rng.integers(-4, 5, (P, dim)))
    prior = rng.standard_normal((len(SIZES), dim)).astype(np.float32)
    rowptr, col = cells_csr(P, dim + 2)
    cen = dev(prior)
    ops.cell_means_bf16(tb, dev(rowptr), dev(col), cen)
    got = cen.cpu().numpy()
    for k, m in enumerate(SIZES):
        ids = col[rowptr[k]:rowptr[k + 1]]
        want = prior[k] if m == 0 else x[ids].astype(np.float64).sum(0).astype(np.float32) / np.float32(m)
        assert (got[k].view(np.int32) == want.astype(np.float32).view(np.int32)).all(), (k, m)


def test_means_pass_over_ids_out_of_range():
    from p_companion_amd import ops
    P, dim = 300, 128
    rng = np.random.default_rng(5)
    tb, x = rounded(rng.integers(-4, 5, (P, dim)))
    good = [rng.permutation(P)[:m].astype(np.int32) for m in (40, 9, 0)]
    junk = np.array([-1, -5, P, P + 100, 2 ** 31 - 1, -2 ** 31], np.int32)
    cells = [rng.permutation(np.concatenate([good[0], junk])), rng.permutation(np.concatenate([good[1], junk[:2]])), junk]
    rowptr = np.concatenate([[0], np.cumsum([len(c) for c in cells])]).astype(np.int32)
    prior = rng.standard_normal((3, dim)).astype(np.float32)
    cen = dev(prior)
    ops.cell_means_bf16(tb, dev(rowptr), dev(np.concatenate(cells).astype(np.int32)), cen)
    torch.cuda.synchronize()
    got = cen.cpu().numpy()
    for k, ids in enumerate(good):
        want = prior[k] if len(ids) == 0 else x[ids].astype(np.float64).sum(0).astype(np.float32) / np.float32(len(ids))
        assert (got[k].view(np.int32) == want.view(np.int32)).all(), k     # a cell of nothing but such ids keeps its centroid


# ---- 3. the build
@pytest.mark.parametrize("dim", [128, 256])
def test_build_has_the_bits_of_the_fp32_build_on_the_widened_table(dim):
    from p_companion_amd import ops
    P, C = 5000, 12
    rng = np.random.default_rng(dim + 3)
    tb, x = rounded(rng.standard_normal((P, dim)))
    tf = tb.float()
    init = dev(x[rng.permutation(P)[:C]] + np.float32(0.25))

    def same(a, b, what):
        for f in FIELDS:
            assert getattr(a, f).dtype == getattr(b, f).dtype and (bits(getattr(a, f)) == bits(getattr(b, f))).all(), (what, f)

    for kw in (dict(seed=1), dict(init=init)):
        want = ops.build_cell_index(tf, C, iters=3, **kw)
        got = ops.build_cell_index_bf16(tb, C, iters=3, chunk_rows=1024, **kw)     # four full chunks and a ragged one
        assert (got.n_cells, got.dim, got.num_products) == (C, dim, P)
        assert got.centroids.dtype == torch.float32 and got.centroid_bias.dtype == torch.float32
        same(got, want, kw.keys())
        same(ops.build_cell_index_bf16(tb, C, iters=3, chunk_rows=P, **kw), want, "one chunk")
        same(ops.build_cell_index_bf16(ops.CompactCatalogue(tb), C, iters=3, **kw), want, "the default chunk, a catalogue")
        same(ops.build_cell_index_bf16(tb, C, iters=3, chunk_rows=1024, **kw), got, "a second build")
    # the starting centroids: the widened rows at the first C entries of a CPU generator's permutation
    gen = torch.Generator(device="cpu")
    gen.manual_seed(1)
    first = torch.randperm(P, generator=gen)[:C].numpy()
    zero = ops.build_cell_index_bf16(tb, C, iters=0, seed=1)
    assert (bits(zero.centroids) == x[first].view(np.int32)).all()


# ---- 4. the build's memory
def test_build_never_widens_the_whole_table():
    from p_companion_amd import ops
    P, dim, C, chunk = 65536, 128, 16, 4096
    tb, _ = rounded(np.random.default_rng(4).standard_normal((P, dim)))
    tf = tb.float()                                                               # (resident for the fp32 build: not its peak)
    builds = (lambda: ops.build_cell_index_bf16(tb, C, iters=1, chunk_rows=chunk),
              lambda: ops.build_cell_index(tf, C, iters=1, chunk_rows=chunk))
    for b in builds:                                                              # (the package's workspace cache is filled
        b()                                                                       # once and stays resident: not a build's peak)
    peaks = []
    for b in builds:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        entry = torch.cuda.memory_allocated()
        index = b()
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - entry)
        del index
    compact, full = peaks
    print(f"build peak above entry: bf16 {compact} B, fp32 {full} B; a widened chunk {chunk * dim * 4} B, "
          f"the widened table {P * dim * 4} B")
    assert compact <= full + 2 * chunk * dim * 4
    assert compact < P * dim * 4 // 2


# ---- 5. / 6. / 7. IndexedCompactSimilarProducts
@functools.lru_cache(maxsize=None)
def graph(P):
    from p_companion_amd.data import generate_device_bpg
    return generate_device_bpg(P, 20, seed=3, world=1, with_complementary=False)


@functools.lru_cache(maxsize=None)
def served(kind, dim, P, C):
    """One catalogue, exact object and indexed object (every cell probed by default) per case, and 64 queries."""
    from p_companion_amd import ops
    from p_companion_amd.inference import CompactSimilarProducts, IndexedCompactSimilarProducts
    rng = np.random.default_rng(dim + P + C)
    tb, x = rounded(rng.integers(-4, 5, (P, dim)) if kind == "integer" else rng.standard_normal((P, dim)))
    cat = ops.CompactCatalogue(tb)
    bpg = graph(P)
    exact = CompactSimilarProducts(cat, bpg, scope="catalogue")
    indexed = IndexedCompactSimilarProducts(cat, bpg, n_cells=C, nprobe=C, iters=3, seed=1)
    queries = rng.choice(P, 64, replace=False).astype(np.int32)
    return SimpleNamespace(P=P, dim=dim, C=C, tb=tb, x=x, cat=cat, bpg=bpg, exact=exact, indexed=indexed, queries=queries)


@pytest.mark.parametrize("kind,dim,P,C", [("integer", 128, 3000, 12), ("integer", 256, 3000, 12), ("normal", 128, 5000, 12),
                                          ("normal", 256, 5000, 12), ("integer", 128, 3000, 40)])
def test_probing_every_cell_is_the_exact_compact_list_bit_for_bit(kind, dim, P, C):
    """A mismatch on normal data would say that the bf16 list entry's score depends on where a candidate sits in its group
    (nearest_list_bf16.hip): the message names the row and the two bit patterns."""
    c = served(kind, dim, P, C)
    sp, isp = c.exact, c.indexed
    assert isp.scope == "catalogue" and isp.n_cells == C == isp.nprobe and isp.index.num_products == P
    assert isp.index.centroids.dtype == torch.float32 and tuple(isp.index.centroids.shape) == (C, dim)
    q = torch.from_numpy(c.queries)

    def same(what):
        for method, lengths in (("similar_batch", (1, 10, 16)), ("similar_list_batch", (17, 64, 256))):
            for n in lengths:
                want_i, want_d = getattr(sp, method)(q, n)
                got_i, got_d = getattr(isp, method)(q, n)
                assert got_i.dtype == torch.int32 and got_d.dtype == torch.float32
                assert tuple(got_i.shape) == tuple(got_d.shape) == (len(c.queries), n)
                wi, gi, wd, gd = want_i.cpu().numpy(), got_i.cpu().numpy(), bits(want_d), bits(got_d)
                bad = np.argwhere((wi != gi) | (wd != gd))
                assert len(bad) == 0, (f"{what}, {method}({n}): {len(bad)} entries differ; first at row {bad[0][0]} (query "
                                       f"{c.queries[bad[0][0]]}) column {bad[0][1]}: ids {wi[tuple(bad[0])]} / {gi[tuple(bad[0])]}, "
                                       f"distance bits {wd[tuple(bad[0])]:#010x} / {gd[tuple(bad[0])]:#010x}")
        return isp.similar_list_batch(q, 64)[0]

    try:
        same("self-exclusion")
        assert (isp.similar_batch(q, 10)[0].cpu().numpy() != c.queries[:, None]).all()
        for o in (sp, isp):
            o.set_exclusions(False)
        same("no exclusions")
        assert (isp.similar_batch(q, 1)[0].cpu().numpy()[:, 0] == c.queries).all()  # (the query is its own nearest product)
        g = c.bpg.cuda()
        for o in (sp, isp):
            o.set_exclusions(g["cv_rowptr"], g["cv_col"])
        lists = same("co-view exclusions").cpu().numpy()
        rowptr, col = g["cv_rowptr"].cpu().numpy(), g["cv_col"].cpu().numpy()
        for r, qi in enumerate(c.queries):
            assert not np.isin(lists[r], np.append(col[rowptr[qi]:rowptr[qi + 1]], qi)).any(), r
        # the mask empties cell 0 and halves cell 1
        cell_of = isp.index.cell_of.cpu().numpy()
        mask = np.ones(P, bool)
        mask[cell_of == 0] = False
        mask[np.nonzero(cell_of == 1)[0][::2]] = False
        dmask = torch.from_numpy(mask).cuda()
        for o in (sp, isp):
            o.set_eligible(dmask)
        lists = same("eligible")
        assert dmask[lists[lists >= 0].long()].all()
        counts = np.diff(isp.cell_rowptr.cpu().numpy())
        assert counts[0] == 0 and counts[1] == (cell_of == 1).sum() // 2
    finally:
        for o in (sp, isp):                                                       # (the objects are shared: as they were)
            o.set_eligible(None)
            o.set_exclusions()
    same("as it was")
    assert isp.cell_col is isp.index.cell_col


def l2_lists(x64, queries, cand_of, n):
    """[B, n] ids: the float64 L2 order (ties to the lower id) of every query over its own candidates, -1 past the end."""
    out = np.full((len(queries), n), -1, np.int64)
    for r, (qi, cand) in enumerate(zip(queries, cand_of)):
        d2 = ((x64[cand] - x64[qi]) ** 2).sum(1)
        o = np.lexsort((cand, d2))[:n]
        out[r, :len(o)] = cand[o]
    return out


@pytest.mark.parametrize("nprobe", [1, 3, 20])
def test_fewer_cells_probed_on_exact_data(nprobe):
    from p_companion_amd import ops
    from p_companion_amd.inference import IndexedCompactSimilarProducts, IndexedSimilarProducts
    c = served("integer", 128, 3000, 40)
    index, queries, B = c.indexed.index, c.queries, len(c.queries)
    isp = IndexedCompactSimilarProducts(c.cat, c.bpg, index=index, nprobe=nprobe)
    assert isp.index is index and isp.nprobe == nprobe
    q = torch.from_numpy(queries)
    tf = c.tb.float()
    x64 = c.x.astype(np.float64)
    cell_of = index.cell_of.cpu().numpy()
    cells = isp.probe_cells(q).cpu().numpy()
    assert cells.shape == (B, nprobe) and cells.dtype == np.int32
    # the probe: the float64 top nprobe of the centroids, within the biased entry's allowance (the means are no integers)
    cen64, cb = index.centroids.cpu().numpy().astype(np.float64), index.centroid_bias.cpu().numpy()
    mc = SimpleNamespace(dim=c.dim, types=np.zeros(B, np.int32),
                         per_type={0: (np.arange(c.C), np.arange(B), cen64 @ x64[queries].T, np.abs(cen64) @ np.abs(x64[queries]).T)},
                         where={r: (0, r) for r in range(B)})
    rows, zeros = tf[q.cuda().long()], torch.zeros(B, dtype=torch.int32, device="cuda")
    if nprobe <= 16:
        ci, cs = ops.retrieve_topk_grouped(rows, zeros, *isp._one_cell_type, index.centroids, nprobe, bias=index.centroid_bias)
        other = IndexedSimilarProducts(tf, c.bpg, index=index, nprobe=nprobe)     # the fp32 class, the same index and rows
        assert (other.probe_cells(q).cpu().numpy() == cells).all()
    else:
        ci, cs = ops.retrieve_list_grouped_biased(rows, zeros, *isp._one_cell_type, index.centroids, index.centroid_bias, nprobe)
        assert (isp.probe_cells(q, 16).cpu().numpy() == cells[:, :16]).all()      # the same total order on both sides of 16
    assert (ci.cpu().numpy() == cells).all()
    check_biased(mc, cells, cs.cpu().numpy(), cb, nprobe)
    assert all(len(set(row.tolist())) == nprobe for row in cells)

    cand_of = []
    for r, qi in enumerate(queries):
        cand = np.nonzero(np.isin(cell_of, cells[r]))[0]
        cand_of.append(cand[cand != qi])                                          # (the default exclusion: the query itself)
    for method, n in (("similar_batch", 10), ("similar_batch", 16), ("similar_list_batch", 64)):
        idx, dist = getattr(isp, method)(q, n)
        want = l2_lists(x64, queries, cand_of, n)
        got = idx.cpu().numpy()
        assert (got == want).all(), (method, n, np.argwhere(got != want)[:3])
        for r in range(B):
            assert np.isin(cell_of[got[r][got[r] >= 0]], cells[r]).all()          # every returned id lies in a probed cell
        # the distances: the compact parent's recomputation over the widened rows
        d = (rows[:, None, :] - tf[idx.clamp(min=0).long()] + 1e-6).norm(dim=2)
        d = torch.where(idx >= 0, d, torch.full_like(d, float("inf")))
        assert (bits(d) == bits(dist)).all(), (method, n)
    # recall: the share of the exact lists (over the rounded rows) that the indexed lists hold
    everyone = [np.delete(np.arange(c.P), qi) for qi in queries]
    exact = l2_lists(x64, queries, everyone, 10)
    got = l2_lists(x64, queries, cand_of, 10)
    held = sum(len(np.intersect1d(exact[r], got[r][got[r] >= 0])) for r in range(B))
    want = np.float32(held) / np.float32(exact.size)
    assert float(isp.recall(q, 10)) == float(want)
    print(f"exact data, nprobe = {nprobe} of {c.C}: recall@10 = {float(want):.3f}")
    assert float(isp.recall(q, 10, nprobe=c.C)) == 1.0


# ---- 7. small things
def test_small_things():
    from p_companion_amd import ops
    from p_companion_amd.inference import IndexedCompactSimilarProducts
    c = served("integer", 128, 3000, 12)
    isp = c.indexed
    none = torch.zeros(0, dtype=torch.int32)
    for method, n in (("similar_batch", 10), ("similar_list_batch", 64)):
        idx, dist = getattr(isp, method)(none, n)
        assert tuple(idx.shape) == tuple(dist.shape) == (0, n) and idx.dtype == torch.int32 and dist.dtype == torch.float32
    cells = isp.probe_cells(none, 5)
    assert tuple(cells.shape) == (0, 5) and cells.dtype == torch.int32
    slot, rank = isp.rank_pairs(none, none)
    assert tuple(slot.shape) == tuple(rank.shape) == (0,)
    with pytest.raises(NotImplementedError):
        isp.similar_where_batch(torch.from_numpy(c.queries), 10, need=torch.zeros(64, dtype=torch.int32))

    # an index built on the fp32 table before it was given back is accepted and serves the same lists
    early = ops.build_cell_index(c.tb.float(), c.C, iters=3, seed=1)
    other = IndexedCompactSimilarProducts(c.tb, c.bpg, index=early, nprobe=3)
    assert other.index is early and other.nprobe == 3
    mine = IndexedCompactSimilarProducts(c.cat, c.bpg, index=isp.index, nprobe=3)
    q = torch.from_numpy(c.queries)
    for method, n in (("similar_batch", 10), ("similar_list_batch", 64)):
        for a, b in zip(getattr(other, method)(q, n), getattr(mine, method)(q, n)):
            assert (bits(a) == bits(b)).all(), (method, n)
    with pytest.raises(ValueError, match="the index is over"):
        IndexedCompactSimilarProducts(c.tb[:100].contiguous(), c.bpg, index=early)

    # rank_pairs is the exact whole-catalogue rank: rank < n exactly where the list with every cell probed holds the target there
    n = 64
    lists = isp.similar_list_batch(q, n, nprobe=c.C)[0].cpu().numpy()
    rng = np.random.default_rng(8)
    targets = np.where(rng.random(64) < 0.6, lists[np.arange(64), rng.integers(0, n, 64)], rng.integers(0, c.P, 64)).astype(np.int32)
    targets[:3] = c.queries[:3]                                                   # (the anchor itself: excluded, rank -1)
    slot, rank = (t.cpu().numpy() for t in isp.rank_pairs(q, torch.from_numpy(targets)))
    for got, want in zip((slot, rank), c.exact.rank_pairs(q, torch.from_numpy(targets))):
        assert (got == want.cpu().numpy()).all()
    assert (rank[:3] == -1).all() and (slot == 0).all()
    for r in range(64):
        at = np.nonzero(lists[r] == targets[r])[0]
        if 0 <= rank[r] < n:
            assert len(at) == 1 and at[0] == rank[r], r
        else:
            assert len(at) == 0, r
    assert (rank >= 0).sum() >= 20 and (rank >= n).sum() >= 1
