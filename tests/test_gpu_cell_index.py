"""The k-means cell index: pc_cell_means and pc_merge_lists (csrc/cells.hip), ops.build_cell_index and
inference.IndexedSimilarProducts.  Needs an MI355X.

References are float64 numpy in this file.  Bounds:
  cell_means   |got - fp64| <= (m + 1) 2^-24 (sum_i |x_id|) / m per coordinate: the order-independent forward bound of an fp32
               sum of m terms (m - 1 additions, every partial sum bounded by the sum of the magnitudes) and the one division;
               on integer data every sum is exact and the result is np.float32(sum) / np.float32(m) bit for bit.
  scores       the biased entry's allowance of tests/test_gpu_nearest.py, (D + 2) 2^-24 (sum_d |x_d c_d| + |b_c|) per score; an
               index may differ from the float64 order only where the two float64 scores lie within the sum of their
               allowances -- no cap on such rows, each is held to it (check_biased of that file).
  merge        exact: indices equal, scores the same bits."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_nearest import U, check_biased, ordered

SIZES = (0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1000)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy() if t.dtype == torch.float32 else t.detach().cpu().numpy()


# ---- 1. cell_means
def cells_csr(P, seed):
    """14 cells of SIZES members, a shuffled cell_col over a part of range(P): some products are in no cell."""
    rng = np.random.default_rng(seed)
    col = rng.permutation(P)[:sum(SIZES)].astype(np.int32)
    rowptr = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
    return rowptr, col


@pytest.mark.parametrize("dim", [128, 256])
def test_cell_means_against_float64_on_normal_data(dim):
    from p_companion_amd import ops
    P = 4000
    rng = np.random.default_rng(dim)
    x = rng.standard_normal((P, dim)).astype(np.float32)
    prior = rng.standard_normal((len(SIZES), dim)).astype(np.float32)
    rowptr, col = cells_csr(P, dim + 1)
    table, cen = dev(x), dev(prior)
    out = ops.cell_means(table, dev(rowptr), dev(col), cen)
    assert out is cen
    got = cen.cpu().numpy()
    worst = 0.0
    for c, m in enumerate(SIZES):
        ids = col[rowptr[c]:rowptr[c + 1]]
        if m == 0:
            assert (got[c].view(np.int32) == prior[c].view(np.int32)).all()        # the empty cell keeps its prior bits
            continue
        x64 = x[ids].astype(np.float64)
        err = np.abs(got[c].astype(np.float64) - x64.sum(0) / m)
        bound = (m + 1) * U * np.abs(x64).sum(0) / m
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), f"cell {c} ({m} members): error / bound = {(err / bound).max():.3f}"
    print(f"cell_means D = {dim}: worst error / bound = {worst:.4f}")

    # the same bits on a second run, and on a run after unrelated work on the device
    runs = []
    for k in range(3):
        c2 = dev(prior)
        if k == 2:
            (torch.randn(512, 512, device="cuda") @ torch.randn(512, 512, device="cuda")).sum().item()
            ops.half_sq_norm_bias(table)
        ops.cell_means(table, dev(rowptr), dev(col), c2)
        runs.append(bits(c2))
    assert (runs[0] == bits(cen)).all() and (runs[1] == runs[0]).all() and (runs[2] == runs[0]).all()


@pytest.mark.parametrize("dim", [128, 256])
def test_cell_means_on_integer_data_is_exact(dim):
    from p_companion_amd import ops
    P = 4000
    rng = np.random.default_rng(dim + 7)
    x = rng.integers(-4, 5, (P, dim)).astype(np.float32)
    prior = rng.standard_normal((len(SIZES), dim)).astype(np.float32)
    rowptr, col = cells_csr(P, dim + 2)
    cen = dev(prior)
    ops.cell_means(dev(x), dev(rowptr), dev(col), cen)
    got = cen.cpu().numpy()
    for c, m in enumerate(SIZES):
        ids = col[rowptr[c]:rowptr[c + 1]]
        want = prior[c] if m == 0 else x[ids].astype(np.float64).sum(0).astype(np.float32) / np.float32(m)
        assert (got[c].view(np.int32) == want.astype(np.float32).view(np.int32)).all(), (c, m)


def test_cell_means_passes_over_ids_out_of_range():
    from p_companion_amd import ops
    P, dim = 300, 128
    rng = np.random.default_rng(5)
    x = rng.integers(-4, 5, (P, dim)).astype(np.float32)
    good = [rng.permutation(P)[:m].astype(np.int32) for m in (40, 9, 0)]
    junk = np.array([-1, -5, P, P + 100, 2 ** 31 - 1, -2 ** 31], np.int32)
    cells = [rng.permutation(np.concatenate([good[0], junk])), rng.permutation(np.concatenate([good[1], junk[:2]])), junk]
    rowptr = np.concatenate([[0], np.cumsum([len(c) for c in cells])]).astype(np.int32)
    prior = rng.standard_normal((3, dim)).astype(np.float32)
    cen = dev(prior)
    ops.cell_means(dev(x), dev(rowptr), dev(np.concatenate(cells).astype(np.int32)), cen)
    torch.cuda.synchronize()
    got = cen.cpu().numpy()
    for c, ids in enumerate(good):
        want = prior[c] if len(ids) == 0 else x[ids].astype(np.float64).sum(0).astype(np.float32) / np.float32(len(ids))
        assert (got[c].view(np.int32) == want.view(np.int32)).all(), c     # a cell of nothing but such ids keeps its centroid


# ---- 2. merge_lists
def merge_case(L, n, R=37, seed=0):
    """R rows of L lists: lengths cycle through 0 .. n; row 0 is empty, row 1 holds fewer than n in all; scores from 5 values."""
    rng = np.random.default_rng(1000 * L + n + seed)
    values = np.array([-3.5, -0.25, 0.0, 1.0, 7.75], np.float32)
    idx = np.full((R, L, n), -1, np.int32)
    sc = np.full((R, L, n), -np.inf, np.float32)
    want_i = np.full((R, n), -1, np.int32)
    want_s = np.full((R, n), -np.inf, np.float32)
    for r in range(R):
        lens = [(r * L + l) % (n + 1) for l in range(L)]
        if r == 0:
            lens = [0] * L
        elif r == 1:
            lens = [0] * L
            lens[0] = (n - 1) // 2 if L > 1 else n - 1
            if L > 1:
                lens[-1] = n - 1 - lens[0]
        ids = rng.permutation(100_000)[:sum(lens)].astype(np.int32)            # disjoint products
        s = values[rng.integers(0, 5, sum(lens))]
        at = 0
        for l, ln in enumerate(lens):
            li, ls = ids[at:at + ln], s[at:at + ln]
            o = np.lexsort((li, -ls))
            idx[r, l, :ln], sc[r, l, :ln] = li[o], ls[o]
            at += ln
        o = np.lexsort((ids, -s))[:n]
        want_i[r, :len(o)], want_s[r, :len(o)] = ids[o], s[o]
    return idx, sc, want_i, want_s


@pytest.mark.parametrize("n", [1, 10, 16, 17, 64, 256])
@pytest.mark.parametrize("L", [1, 2, 3, 16, 17, 64])
def test_merge_lists_against_a_numpy_sort(L, n):
    from p_companion_amd import ops
    idx, sc, want_i, want_s = merge_case(L, n)
    got_i, got_s = ops.merge_lists(dev(idx), dev(sc))
    assert got_i.dtype == torch.int32 and got_s.dtype == torch.float32 and tuple(got_i.shape) == tuple(got_s.shape) == (37, n)
    assert (got_i.cpu().numpy() == want_i).all()
    assert (bits(got_s) == want_s.view(np.int32)).all()


def test_merge_lists_error_codes_on_the_device():
    from p_companion_amd import _lib
    L = _lib.lib()
    idx, sc, want_i, _ = merge_case(3, 10)
    di, ds = dev(idx), dev(sc)
    oi, os_ = torch.empty(37, 10, dtype=torch.int32, device="cuda"), torch.empty(37, 10, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert L.pc_merge_lists(p(di), p(ds), 37, 3, 10, p(oi), p(os_), st) == 0
    torch.cuda.synchronize()
    assert (oi.cpu().numpy() == want_i).all()
    assert L.pc_merge_lists(p(di), p(ds), 0, 3, 10, p(oi), p(os_), st) == -1        # PC_EINVAL: no rows
    assert L.pc_merge_lists(None, p(ds), 37, 3, 10, p(oi), p(os_), st) == -1
    for l, n in ((0, 10), (65, 10), (3, 0), (3, 257)):
        assert L.pc_merge_lists(p(di), p(ds), 37, l, n, p(oi), p(os_), st) == -2   # PC_ESHAPE
    tab, cen = torch.zeros(8, 128, device="cuda"), torch.zeros(2, 128, device="cuda")
    rp, col = dev(np.array([0, 3, 8], np.int32)), dev(np.arange(8, dtype=np.int32))
    assert L.pc_cell_means(p(tab), p(rp), p(col), 2, 8, 128, p(cen), st) == 0
    assert L.pc_cell_means(p(tab), p(rp), p(col), 0, 8, 128, p(cen), st) == -1
    assert L.pc_cell_means(p(tab), p(rp), p(col), 2, 0, 128, p(cen), st) == -1
    assert L.pc_cell_means(p(tab), p(rp), p(col), 2, 8, 64, p(cen), st) == -2
    torch.cuda.synchronize()


# ---- 3. build_cell_index
@pytest.fixture(scope="module")
def clustered():
    """12 clusters, P = 6000, D = 128: the centres +-64 e_j, integer noise in [-2, 2]: every sum, dot product and half norm is
    exact in fp32.  One index (init = one member of each cluster, iters = 2) shared by the tests below."""
    from p_companion_amd import ops
    from p_companion_amd.data import generate_device_bpg
    P, dim, C = 6000, 128, 12
    rng = np.random.default_rng(11)
    labels = rng.permutation(np.arange(P) % C).astype(np.int32)
    centres = np.zeros((C, dim), np.float32)
    for c in range(C):
        centres[c, c // 2] = 64.0 if c % 2 == 0 else -64.0
    x = centres[labels] + rng.integers(-2, 3, (P, dim)).astype(np.float32)
    first = np.array([np.nonzero(labels == c)[0][0] for c in range(C)])
    table = dev(x)
    index = ops.build_cell_index(table, C, iters=2, init=dev(x[first]))
    bpg = generate_device_bpg(P, 20, seed=3, world=1, with_complementary=False)
    return SimpleNamespace(P=P, dim=dim, C=C, labels=labels, x=x, table=table, index=index, bpg=bpg)


def test_build_with_init_recovers_the_clusters_exactly(clustered):
    c = clustered
    ix = c.index
    assert (ix.n_cells, ix.dim, ix.num_products) == (c.C, c.dim, c.P)
    cell_of = ix.cell_of.cpu().numpy()
    assert ix.cell_of.dtype == torch.int32 and (cell_of == c.labels).all()
    cen = ix.centroids.cpu().numpy()
    for k in range(c.C):
        members = c.x[c.labels == k].astype(np.float64)
        want = members.sum(0).astype(np.float32) / np.float32(len(members))
        assert (cen[k].view(np.int32) == want.view(np.int32)).all(), k
    rowptr, col = ix.cell_rowptr.cpu().numpy(), ix.cell_col.cpu().numpy()
    assert (np.bincount(cell_of, minlength=c.C) == np.diff(rowptr)).all() and rowptr[0] == 0
    assert (np.sort(col) == np.arange(c.P)).all()
    assert (cell_of[col] == np.repeat(np.arange(c.C), np.diff(rowptr))).all()
    from p_companion_amd import ops
    assert (bits(ix.centroid_bias) == bits(ops.half_sq_norm_bias(ix.centroids))).all()


FIELDS = ("centroids", "centroid_bias", "cell_of", "cell_rowptr", "cell_col")


@pytest.mark.parametrize("dim", [128, 256])
def test_build_without_init_is_reproducible_and_assigns_to_the_nearest_centroid(dim):
    from p_companion_amd import ops
    P, C = 5000, 12
    x = np.random.default_rng(dim + 3).standard_normal((P, dim)).astype(np.float32)
    table = dev(x)
    a = ops.build_cell_index(table, C, iters=3, seed=5)
    b = ops.build_cell_index(table, C, iters=3, seed=5, chunk_rows=1777)         # (the chunks do not show either)
    for f in FIELDS:
        assert (bits(getattr(a, f)) == bits(getattr(b, f))).all(), f
    other = ops.build_cell_index(table, C, iters=3, seed=6)
    assert (other.cell_of != a.cell_of).any()
    # the starting centroids: the first C entries of a CPU generator's permutation
    gen = torch.Generator(device="cpu")
    gen.manual_seed(5)
    first = torch.randperm(P, generator=gen)[:C].numpy()
    zero = ops.build_cell_index(table, C, iters=0, seed=5)
    assert (bits(zero.centroids) == x[first].view(np.int32)).all()

    cell_of = a.cell_of.cpu().numpy()
    rowptr, col = a.cell_rowptr.cpu().numpy(), a.cell_col.cpu().numpy()
    assert (np.bincount(cell_of, minlength=C) == np.diff(rowptr)).all() and (np.sort(col) == np.arange(P)).all()
    cen, b64 = a.centroids.cpu().numpy().astype(np.float64), a.centroid_bias.cpu().numpy().astype(np.float64)
    x64 = x.astype(np.float64)
    s64 = x64 @ cen.T + b64[None, :]                                              # [P, C]
    allow = (dim + 2) * U * (np.abs(x64) @ np.abs(cen).T + np.abs(b64)[None, :])
    best = np.argmax(s64, axis=1)                                                 # (the lowest cell of equal scores)
    off = np.nonzero(cell_of != best)[0]
    gap = s64[off, best[off]] - s64[off, cell_of[off]]
    assert (gap <= allow[off, best[off]] + allow[off, cell_of[off]]).all(), f"{len(off)} rows off, largest gap {gap.max():.3e}"
    print(f"build D = {dim}: {len(off)} of {P} rows assigned to a cell within the allowance of the float64 best")


# ---- 4. IndexedSimilarProducts
@pytest.fixture(scope="module")
def queries():
    return np.random.default_rng(1).choice(6000, 203, replace=False).astype(np.int32)


def custom_exclusions(P, q, seed=2):
    """A CSR keyed by the query id: five random products for every second query."""
    rng = np.random.default_rng(seed)
    counts = np.zeros(P, np.int64)
    counts[q[::2]] = 5
    rowptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return dev(rowptr), dev(rng.integers(0, P, int(counts.sum())).astype(np.int32))


def test_probing_every_cell_is_the_exact_list_bit_for_bit(clustered, queries):
    """nprobe = n_cells = 12 over the generator's own features: ids and distances equal SimilarProducts(scope="catalogue")."""
    from p_companion_amd.inference import IndexedSimilarProducts, SimilarProducts
    c = clustered
    table = c.bpg.cuda()["features"]
    sp = SimilarProducts(table, c.bpg, scope="catalogue")
    isp = IndexedSimilarProducts(table, c.bpg, n_cells=12, nprobe=12, iters=3, seed=1)
    assert isp.scope == "catalogue" and isp.n_cells == 12 and isp.index.num_products == c.P
    q = torch.from_numpy(queries)

    def same(what):
        for n in (1, 10, 16):
            want_i, want_d = sp.similar_batch(q, n)
            got_i, got_d = isp.similar_batch(q, n)
            assert got_i.dtype == torch.int32 and tuple(got_i.shape) == (len(queries), n)
            assert (got_i == want_i).all(), (what, n)
            assert (bits(got_d) == bits(want_d)).all(), (what, n)
            assert float(isp.recall(q, n)) == 1.0

    same("self-exclusion")
    assert (isp.similar_batch(q, 10)[0].cpu().numpy() != queries[:, None]).all()
    for o in (sp, isp):
        o.set_exclusions(False)
    same("no exclusions")
    assert (isp.similar_batch(q, 1)[0].cpu().numpy()[:, 0] == queries).all()      # (the query is its own nearest product)
    rowptr, col = custom_exclusions(c.P, queries)
    for o in (sp, isp):
        o.set_exclusions(rowptr, col)
    same("custom exclusions")
    mask = torch.from_numpy(np.random.default_rng(6).random(c.P) < 0.6).cuda()
    for o in (sp, isp):
        o.set_eligible(mask)
    same("eligible")
    assert mask[isp.similar_batch(q, 16)[0].long()].all()
    for o in (sp, isp):
        o.set_eligible(None)
    same("eligible removed")
    assert isp.cell_col is isp.index.cell_col

    # rank_pairs is the parent's exact whole-catalogue code: the same bits, whatever the index
    rng = np.random.default_rng(9)
    anchors, targets = (torch.from_numpy(rng.integers(0, c.P, 500).astype(np.int32)) for _ in range(2))
    for got, want in zip(isp.rank_pairs(anchors, targets), sp.rank_pairs(anchors, targets)):
        assert (got == want).all()
    # an index handed over is used as it is; one over another table is refused
    again = IndexedSimilarProducts(table, c.bpg, index=isp.index, nprobe=3)
    assert again.index is isp.index and again.nprobe == 3
    with pytest.raises(ValueError, match="the index is over"):
        IndexedSimilarProducts(table[:100].contiguous(), c.bpg, index=isp.index)


def per_row_reference(x64, bias64, dim, q_ids, cand_of):
    """check_biased's fixture with every row a 'type' of its own: the row's candidates (ascending), float64 scores and
    magnitude sums."""
    per_type, where = {}, {}
    for r, (qi, cand) in enumerate(zip(q_ids, cand_of)):
        if len(cand) == 0:
            continue
        per_type[r] = (cand, [r], (x64[cand] @ x64[qi])[:, None], (np.abs(x64[cand]) @ np.abs(x64[qi]))[:, None])
        where[r] = (r, 0)
    return SimpleNamespace(dim=dim, types=np.arange(len(q_ids)), per_type=per_type, where=where)


def probed_candidates(cells, cell_of, eligible=None):
    out = []
    for row in cells:
        keep = np.isin(cell_of, row[row >= 0])
        if eligible is not None:
            keep &= eligible
        out.append(np.nonzero(keep)[0])
    return out


@pytest.mark.parametrize("nprobe", [1, 3])
def test_probed_lists_on_exact_data_are_the_float64_l2_order(clustered, queries, nprobe):
    from p_companion_amd import ops
    from p_companion_amd.inference import IndexedSimilarProducts
    c = clustered
    isp = IndexedSimilarProducts(c.table, c.bpg, index=c.index, nprobe=nprobe)
    q = torch.from_numpy(queries)
    x64 = c.x.astype(np.float64)
    cell_of = c.index.cell_of.cpu().numpy()
    cells = isp.probe_cells(q).cpu().numpy()
    assert cells.shape == (len(queries), nprobe) and cells.dtype == np.int32
    # the probe itself: the float64 top nprobe of the centroids, nearest first (exact data: no allowance needed for the products,
    # the centroids' means are not integers, so the probe goes through the allowance)
    cen64, cb = c.index.centroids.cpu().numpy().astype(np.float64), c.index.centroid_bias.cpu().numpy()
    mc = SimpleNamespace(dim=c.dim, types=np.zeros(len(queries), np.int32),
                         per_type={0: (np.arange(c.C), np.arange(len(queries)), cen64 @ x64[queries].T,
                                       np.abs(cen64) @ np.abs(x64[queries]).T)},
                         where={r: (0, r) for r in range(len(queries))})
    ci, cs = (t.cpu().numpy() for t in ops.retrieve_topk_grouped(
        c.table[q.cuda().long()], torch.zeros(len(queries), dtype=torch.int32, device="cuda"), *isp._one_cell_type,
        c.index.centroids, nprobe, bias=c.index.centroid_bias))
    assert (ci == cells).all()
    check_biased(mc, ci, cs, cb, nprobe)
    assert (cells[:, 0] == c.labels[queries]).all()                               # (a query's own cluster first)

    bias64 = isp.bias.cpu().numpy().astype(np.float64)
    for n in (1, 10, 16):
        idx, dist = isp.similar_batch(q, n)
        sidx, ssc = isp._search(q.cuda(), c.table[q.cuda().long()], n, nprobe)
        assert (sidx == idx).all()
        idx, dist, ssc = idx.cpu().numpy(), dist.cpu().numpy(), ssc.cpu().numpy()
        for r, qi in enumerate(queries):
            cand = probed_candidates(cells[r:r + 1], cell_of)[0]
            cand = cand[cand != qi]
            s64 = x64[cand] @ x64[qi] + bias64[cand]
            d2 = ((x64[cand] - x64[qi]) ** 2).sum(1)
            o = np.lexsort((cand, d2))[:n]                                        # the float64 L2 order, ties by id
            assert (o == ordered(cand, s64)[:n]).all()                            # (the score order IS the L2 order)
            assert (idx[r] == cand[o]).all(), (r, n)
            assert (ssc[r].view(np.int32) == s64[o].astype(np.float32).view(np.int32)).all(), (r, n)
            assert np.isin(cell_of[idx[r]], cells[r]).all()                       # every returned id lies in a probed cell
        want = (c.table[q.cuda().long()][:, None, :] - c.table[torch.from_numpy(idx).cuda().long()] + 1e-6).norm(dim=2)
        assert (bits(want) == dist.view(np.int32)).all()


def test_a_query_with_few_eligible_products_in_its_cells_gets_tails(clustered):
    from p_companion_amd.inference import IndexedSimilarProducts
    c = clustered
    isp = IndexedSimilarProducts(c.table, c.bpg, index=c.index, nprobe=1)
    in0 = np.nonzero(c.labels == 0)[0]
    eligible = c.labels != 0
    eligible[in0[:4]] = True                                                      # four eligible products in cell 0
    isp.set_eligible(torch.from_numpy(eligible).cuda())
    q = in0[[0, 1, 10, 11]].astype(np.int32)                                      # two of the four, two ineligible ones
    idx, dist = (t.cpu().numpy() for t in isp.similar_batch(torch.from_numpy(q), 10))
    x64 = c.x.astype(np.float64)
    for r, qi in enumerate(q):
        cand = in0[:4][in0[:4] != qi]
        o = np.lexsort((cand, ((x64[cand] - x64[qi]) ** 2).sum(1)))
        k = len(cand)
        assert k in (3, 4) and (idx[r, :k] == cand[o]).all()
        assert (idx[r, k:] == -1).all() and np.isposinf(dist[r, k:]).all() and np.isfinite(dist[r, :k]).all()
    rowptr, col = isp.cell_rowptr.cpu().numpy(), isp.cell_col.cpu().numpy()
    assert rowptr[1] - rowptr[0] == 4 and (np.sort(col) == np.nonzero(eligible)[0]).all()
    assert float(isp.recall(torch.from_numpy(q), 3, 12)) == 1.0                   # (every cell probed: the exact list)


@pytest.mark.parametrize("nprobe", [1, 3])
def test_probed_lists_on_normal_data_within_the_allowances(queries, clustered, nprobe):
    from p_companion_amd import ops
    from p_companion_amd.inference import IndexedSimilarProducts
    c = clustered
    dim, C = 128, 12
    x = np.random.default_rng(77).standard_normal((c.P, dim)).astype(np.float32)
    table = dev(x)
    index = ops.build_cell_index(table, C, iters=3, seed=2)
    isp = IndexedSimilarProducts(table, c.bpg, index=index, nprobe=nprobe)
    q = torch.from_numpy(queries).cuda()
    x64 = x.astype(np.float64)
    cell_of = index.cell_of.cpu().numpy()
    # the probe: the float64 top nprobe of the centroids, up to the allowance
    cen64, cb = index.centroids.cpu().numpy().astype(np.float64), index.centroid_bias.cpu().numpy()
    ci, cs = ops.retrieve_topk_grouped(table[q.long()], torch.zeros(len(queries), dtype=torch.int32, device="cuda"),
                                       *isp._one_cell_type, index.centroids, nprobe, bias=index.centroid_bias)
    cells = isp.probe_cells(q).cpu().numpy()
    assert (cells == ci.cpu().numpy()).all()
    mc = SimpleNamespace(dim=dim, types=np.zeros(len(queries), np.int32),
                         per_type={0: (np.arange(C), np.arange(len(queries)), cen64 @ x64[queries].T,
                                       np.abs(cen64) @ np.abs(x64[queries]).T)},
                         where={r: (0, r) for r in range(len(queries))})
    check_biased(mc, cells, cs.cpu().numpy(), cb, nprobe)
    # the lists: check_biased over each row's own candidates, the union of its probed cells' members, minus the query
    m = per_row_reference(x64, None, dim, queries, probed_candidates(cells, cell_of))
    excluded = {r: [int(qi)] for r, qi in enumerate(queries)}
    bias = isp.bias.cpu().numpy()
    for n in (1, 10, 16):
        idx, _ = isp.similar_batch(q, n)
        sidx, ssc = isp._search(q.to(torch.int32), table[q.long()], n, nprobe)
        assert (sidx == idx).all()
        idx = idx.cpu().numpy()
        check_biased(m, idx, ssc.cpu().numpy(), bias, n, excluded=excluded)
        for r in range(len(queries)):
            assert np.isin(cell_of[idx[r][idx[r] >= 0]], cells[r]).all()
    rec = float(isp.recall(q, 10))
    assert 0.0 < rec <= 1.0
    print(f"normal data, nprobe = {nprobe} of {C}: recall@10 = {rec:.3f}")
