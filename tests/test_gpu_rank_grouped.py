"""The rank of a known product among all products of its type (pc_rank_grouped / ops.rank_grouped).

Two checkers.  (1) The served lists themselves: rank < 16 exactly when ops.retrieve_topk_grouped(..., n=16) holds the target at
position rank -- no tolerance, because the rank kernel forms the target's score and every candidate's through the retrieval's
own MFMA chain and counts under its total order (score descending, product index ascending).  (2) float64: rank lies in
[lo, hi], lo = the candidates whose float64 score beats the target's by more than d = 2 (1e-5 + 1e-5 |g|) (the project's
score-agreement tolerance, once per score; tests/test_gpu_eval_epoch.py's band), hi = lo + the other candidates within d; the
inputs must keep hi > lo rare (at most 10 % of the rows, asserted from the float64 side alone).  Needs an MI355X."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def host_csr(type_idx, n_types):
    order = np.argsort(type_idx, kind="stable").astype(np.int32)
    counts = np.bincount(type_idx, minlength=n_types)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32), order


def upload(type_idx, features, T):
    rowptr, col = host_csr(type_idx, T)
    return torch.from_numpy(rowptr).cuda(), torch.from_numpy(col).cuda(), torch.from_numpy(np.ascontiguousarray(features)).cuda()


def draw_rows(rng, R, type_idx, T, dim):
    """R rows: a type that has products, a target inside it, a random projection."""
    have = np.nonzero(np.bincount(type_idx, minlength=T))[0]
    types = rng.choice(have, R).astype(np.int32)
    by_type = {t: np.nonzero(type_idx == t)[0] for t in np.unique(types)}
    targets = np.array([rng.choice(by_type[t]) for t in types], np.int32)
    proj = rng.standard_normal((R, dim)).astype(np.float32)
    return types, targets, proj


def band64(proj, types, targets, type_idx, features):
    """[lo, hi] per row from float64 scores (rows with types < 0: lo = hi = -1)."""
    R = len(types)
    lo, hi = np.full(R, -1, np.int64), np.full(R, -1, np.int64)
    f, p = torch.from_numpy(features).double(), torch.from_numpy(proj).double()
    for t in np.unique(types[types >= 0]):
        rows = np.nonzero(types == t)[0]
        cand = np.nonzero(type_idx == t)[0]
        y = targets[rows]
        S = f[torch.from_numpy(cand)] @ p[torch.from_numpy(rows)].T                                  # [cand, rows]
        g = (f[torch.from_numpy(y).long()] * p[torch.from_numpy(rows)]).sum(1)
        d = 2 * (1e-5 + 1e-5 * g.abs())
        other = torch.from_numpy(cand[:, None] != y[None, :])
        above = (S > (g + d)[None, :]).sum(0)
        near = (((S - g[None, :]).abs() <= d[None, :]) & other).sum(0)
        lo[rows], hi[rows] = above.numpy(), (above + near).numpy()
    return lo, hi


def check_against_served_lists(rank, idx, targets):
    """rank < 16: the list holds the target there; rank >= 16: it does not hold it."""
    rank, idx = rank.cpu().numpy(), idx.cpu().numpy()
    assert (rank >= 0).all()
    inside = rank < 16
    r = np.nonzero(inside)[0]
    assert (idx[r, rank[r]] == targets[r]).all(), np.nonzero(idx[r, rank[r]] != targets[r])[0][:10]
    assert not (idx[~inside] == targets[~inside][:, None]).any()
    return int(inside.sum())


@pytest.fixture(scope="module", params=[(100, 128), (100, 256), (1000, 128), (1000, 256)], ids=lambda p: f"T{p[0]}-D{p[1]}")
def scaled(request):
    """generate_scaled_bpg, 20 k products: about 200 per type at 100 types, about 20 (short types) at 1000."""
    from p_companion_amd.data import generate_scaled_bpg
    T, dim = request.param
    bpg = generate_scaled_bpg(20_000, T, seed=T + dim, dim=dim)
    rng = np.random.default_rng(T * dim)
    R = 1500 + 37                                              # not a multiple of a 32- or 64-row tile
    types, targets, proj = draw_rows(rng, R, bpg.type_idx, T, dim)
    rowptr, col, table = upload(bpg.type_idx.astype(np.int32), bpg.features, T)
    return SimpleNamespace(T=T, dim=dim, type_idx=bpg.type_idx, features=bpg.features, types=types, targets=targets, proj=proj,
                           rowptr=rowptr, col=col, table=table, dproj=torch.from_numpy(proj).cuda(),
                           dtypes=torch.from_numpy(types).cuda(), dtargets=torch.from_numpy(targets).cuda())


def heavy_catalogue(P, dim, seed):
    """40 types; type 0 holds over half of the products (several slices of >= 4096 candidates), type 1 is empty, type 2
    holds one product, type 3 holds 30 products whose features are copies of 3 rows (exactly tied scores)."""
    T = 40
    rng = np.random.default_rng(seed)
    type_idx = rng.integers(4, T, P).astype(np.int32)
    type_idx[rng.random(P) < 0.55] = 0
    free = np.nonzero(type_idx != 0)[0]
    pick = np.sort(rng.choice(free, 31, replace=False))
    type_idx[pick[0]] = 2
    type_idx[pick[1:]] = 3
    features = rng.standard_normal((P, dim)).astype(np.float32)
    features[pick[1:]] = features[pick[1:4]][np.arange(30) % 3]
    return type_idx, features, T, pick


@pytest.fixture(scope="module", params=[128, 256])
def heavy(request):
    dim = request.param
    P, R = 40_000, 203
    type_idx, features, T, pick = heavy_catalogue(P, dim, seed=dim)
    assert (type_idx == 0).sum() > 3 * 4096
    rng = np.random.default_rng(dim + 1)
    types, targets, proj = draw_rows(rng, R, type_idx, T, dim)
    heavy_rows = rng.random(R) < 0.5
    types[heavy_rows] = 0
    targets[heavy_rows] = rng.choice(np.nonzero(type_idx == 0)[0], int(heavy_rows.sum()))
    types[:4], targets[:4] = 3, pick[[1, 4, 2, 30]]            # tied rows: copies of one another
    types[4], targets[4] = 2, pick[0]                          # the one-product type
    rowptr, col, table = upload(type_idx, features, T)
    return SimpleNamespace(T=T, dim=dim, type_idx=type_idx, features=features, types=types, targets=targets, proj=proj,
                           pick=pick, rowptr=rowptr, col=col, table=table, dproj=torch.from_numpy(proj).cuda(),
                           dtypes=torch.from_numpy(types).cuda(), dtargets=torch.from_numpy(targets).cuda())


# ---- 1. exact against the served lists
def test_rank_is_the_position_in_the_served_list(scaled):
    from p_companion_amd import ops
    m = scaled
    rank, bad = ops.rank_grouped(m.dproj, m.dtypes, m.dtargets, m.rowptr, m.col, m.table)
    idx, _ = ops.retrieve_topk_grouped(m.dproj, m.dtypes, m.rowptr, m.col, m.table, 16)
    assert int(bad) == 0 and rank.dtype == torch.int32 and rank.shape == (len(m.types),)
    inside = check_against_served_lists(rank, idx, m.targets)
    print(f"T={m.T} D={m.dim}: {inside} of {len(m.types)} targets inside the served 16")
    assert 0 < inside                                          # (both branches of the check saw rows)
    if m.T == 100:
        assert inside < len(m.types)


def test_rank_is_the_position_in_the_served_list_heavy_type(heavy):
    from p_companion_amd import ops
    m = heavy
    rank, bad = ops.rank_grouped(m.dproj, m.dtypes, m.dtargets, m.rowptr, m.col, m.table)
    idx, _ = ops.retrieve_topk_grouped(m.dproj, m.dtypes, m.rowptr, m.col, m.table, 16)
    assert int(bad) == 0
    check_against_served_lists(rank, idx, m.targets)


# ---- 2. against float64
def _check_band(m, rank):
    lo, hi = band64(m.proj, m.types, m.targets, m.type_idx, m.features)
    wide = int((hi > lo).sum())
    print(f"T={m.T} D={m.dim}: {wide} of {len(lo)} rows with hi > lo")
    assert wide <= 0.10 * len(lo), "the fixture puts too many scores within the tolerance of a target's: choose another"
    rank = rank.cpu().numpy()
    off = np.nonzero((rank < lo) | (rank > hi))[0]
    assert off.size == 0, [(int(r), int(rank[r]), int(lo[r]), int(hi[r])) for r in off[:10]]


def test_rank_against_float64(scaled):
    from p_companion_amd import ops
    m = scaled
    rank, _ = ops.rank_grouped(m.dproj, m.dtypes, m.dtargets, m.rowptr, m.col, m.table)
    _check_band(m, rank)


def test_rank_against_float64_heavy_type(heavy):
    """A type of more than three slices' minimum: the counts of the slices add up."""
    from p_companion_amd import ops
    m = heavy
    rank, _ = ops.rank_grouped(m.dproj, m.dtypes, m.dtargets, m.rowptr, m.col, m.table)
    keep = np.arange(5, len(m.types))                          # (rows 0..4: exactly tied scores, checked on their own below)
    sub = SimpleNamespace(T=m.T, dim=m.dim, proj=m.proj[keep], types=m.types[keep], targets=m.targets[keep],
                          type_idx=m.type_idx, features=m.features)
    _check_band(sub, rank[torch.from_numpy(keep).cuda()])
    assert int(rank[4]) == 0                                   # a type with one candidate: nothing stands before it


# ---- 3. invariances
def test_same_ranks_for_every_slicing_candidate_order_and_call(heavy):
    from p_companion_amd import ops
    m = heavy
    run = lambda col, s: ops.rank_grouped(m.dproj, m.dtypes, m.dtargets, m.rowptr, col, m.table, slices=s)[0]
    r0 = run(m.col, 0)
    assert torch.equal(run(m.col, 0), r0)
    for s in (1, 7, 64):
        assert torch.equal(run(m.col, s), r0), s
    rowptr = m.rowptr.cpu().numpy()
    col = m.col.cpu().numpy().copy()
    rng = np.random.default_rng(5)
    for t in range(m.T):
        rng.shuffle(col[rowptr[t]:rowptr[t + 1]])
    assert torch.equal(run(torch.from_numpy(col).cuda(), 0), r0)
    assert torch.equal(run(torch.from_numpy(col).cuda(), 7), r0)


# ---- 4. edge cases
def test_equal_feature_rows_are_ordered_by_product_index(heavy):
    """Type 3: 30 products, copies of 3 rows.  Under any projection the ten copies of one row tie exactly, so their ranks
    are ten consecutive numbers in ascending product order."""
    from p_companion_amd import ops
    m = heavy
    dup = m.pick[1:]                                           # ascending product indices; dup[i] is a copy of dup[i % 3]
    proj = torch.from_numpy(np.repeat(m.proj[:1], 30, 0)).cuda()
    types = torch.full((30,), 3, dtype=torch.int32, device="cuda")
    rank, bad = ops.rank_grouped(proj, types, torch.from_numpy(dup.astype(np.int32)).cuda(), m.rowptr, m.col, m.table)
    rank = rank.cpu().numpy()
    assert int(bad) == 0 and sorted(rank.tolist()) == list(range(30))
    for j in range(3):
        mine = rank[j::3]                                      # the copies of row j, in ascending product order
        assert (np.diff(mine) == 1).all(), (j, mine)


def test_a_target_outside_its_rows_type_gets_the_defined_count(heavy):
    """The target need not be in the list: a product of ANOTHER type whose features copy those of an in-type product p
    ties with p exactly, so its count is p's rank plus one if p's index is lower, p's rank otherwise."""
    from p_companion_amd import ops
    m = heavy
    rng = np.random.default_rng(3)
    inside = np.nonzero(m.type_idx == 5)[0]
    p = inside[len(inside) // 2]
    outside = np.nonzero(m.type_idx == 6)[0]
    below, above = outside[outside < p][0], outside[outside > p][-1]
    feats = m.features.copy()
    feats[below] = feats[above] = feats[p]
    table = torch.from_numpy(feats).cuda()
    proj = torch.from_numpy(rng.standard_normal((3, m.dim)).astype(np.float32)[[0, 0, 0]]).cuda()
    types = torch.full((3,), 5, dtype=torch.int32, device="cuda")
    targets = torch.tensor([p, below, above], dtype=torch.int32, device="cuda")
    rank, bad = ops.rank_grouped(proj, types, targets, m.rowptr, m.col, table)
    rp, rb, ra = rank.cpu().tolist()
    assert int(bad) == 0 and rb == rp and ra == rp + 1, (rp, rb, ra)
    # and a foreign target with features of its own: the float64 band
    sub = SimpleNamespace(T=m.T, dim=m.dim, proj=m.proj[5:105], types=np.full(100, 5, np.int32),
                          targets=rng.choice(outside, 100).astype(np.int32), type_idx=m.type_idx, features=m.features)
    rank, bad = ops.rank_grouped(torch.from_numpy(sub.proj).cuda(), torch.from_numpy(sub.types).cuda(),
                                 torch.from_numpy(sub.targets).cuda(), m.rowptr, m.col, m.table)
    assert int(bad) == 0
    _check_band(sub, rank)


def test_rows_without_a_type_and_ids_out_of_range(heavy):
    from p_companion_amd import ops
    m = heavy
    P = m.table.shape[0]
    types = m.types.copy()
    targets = m.targets.copy()
    types[[7, 20, 90]] = -1                                    # no type matched: skipped
    targets[20] = P + 5                                        # (whatever the target of a skipped row is)
    types[11] = m.T                                            # a type past the CSR
    types[12] = m.T + 1000
    targets[13] = P                                            # a target past the table
    targets[14] = -1
    types[15] = 1                                              # an empty type: nothing stands before the target
    dt, dy = torch.from_numpy(types).cuda(), torch.from_numpy(targets).cuda()
    rank, bad = ops.rank_grouped(m.dproj, dt, dy, m.rowptr, m.col, m.table)
    ref, _ = ops.rank_grouped(m.dproj, m.dtypes, m.dtargets, m.rowptr, m.col, m.table)
    rank, ref = rank.cpu().numpy(), ref.cpu().numpy()
    assert int(bad) == 4
    special = [7, 20, 90, 11, 12, 13, 14, 15]
    assert (rank[[7, 20, 90, 11, 12, 13, 14]] == -1).all() and rank[15] == 0
    rest = np.setdiff1d(np.arange(len(types)), special)
    assert (rank[rest] == ref[rest]).all()                     # the other rows are not disturbed
    # the counter is added to, so one counter can serve many calls
    _, bad = ops.rank_grouped(m.dproj, dt, dy, m.rowptr, m.col, m.table, bad=bad)
    assert int(bad) == 8
    # every row skipped: no work item at all
    none = torch.full_like(dt, -1)
    rank, bad = ops.rank_grouped(m.dproj, none, dy, m.rowptr, m.col, m.table)
    assert int(bad) == 0 and (rank == -1).all()


@pytest.mark.parametrize("dim", [128, 256])
def test_a_single_row_and_a_single_product(dim):
    from p_companion_amd import ops
    rng = np.random.default_rng(dim)
    P, T = 3000, 7
    type_idx = rng.integers(0, T, P).astype(np.int32)
    features = rng.standard_normal((P, dim)).astype(np.float32)
    rowptr, col, table = upload(type_idx, features, T)
    types, targets, proj = draw_rows(rng, 1, type_idx, T, dim)
    rank, bad = ops.rank_grouped(torch.from_numpy(proj).cuda(), torch.from_numpy(types).cuda(), torch.from_numpy(targets).cuda(),
                                 rowptr, col, table)
    idx, _ = ops.retrieve_topk_grouped(torch.from_numpy(proj).cuda(), torch.from_numpy(types).cuda(), rowptr, col, table, 16)
    lo, hi = band64(proj, types, targets, type_idx, features)
    assert int(bad) == 0 and lo[0] <= int(rank[0]) <= hi[0]
    check_against_served_lists(rank, idx, targets)
    one = torch.zeros(1, dim, device="cuda")
    one[0, 0] = 2.0
    rank, bad = ops.rank_grouped(one, torch.zeros(1, dtype=torch.int32, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda"),
                                 torch.tensor([0, 1], dtype=torch.int32, device="cuda"),
                                 torch.zeros(1, dtype=torch.int32, device="cuda"), one.clone())
    assert rank.cpu().tolist() == [0] and int(bad) == 0


# ---- 5. errors
def test_error_codes_before_any_launch():
    from p_companion_amd import _lib
    L = _lib.lib()
    R, T, P = 4, 2, 4
    dev = "cuda"
    proj = torch.zeros(R, 256, device=dev)
    types = torch.zeros(R, dtype=torch.int32, device=dev)
    targets = torch.zeros(R, dtype=torch.int32, device=dev)
    rowptr = torch.tensor([0, 2, 4], dtype=torch.int32, device=dev)
    col = torch.arange(4, dtype=torch.int32, device=dev)
    table = torch.zeros(P, 256, device=dev)
    rank = torch.full((R,), 12345, dtype=torch.int32, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    need = L.pc_rank_grouped_workspace_bytes(R, T, 64)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(dim=128, slices=0, nbytes=need, null=None, rows=R, n_types=T, products=P):
        args = [p(proj), p(types), p(targets), rows, p(rowptr), p(col), p(table), n_types, products, dim, slices, p(rank), p(bad),
                p(ws), nbytes, st]
        if null is not None:
            args[null] = None
        return L.pc_rank_grouped(*args)

    for wrong in ({"dim": 192}, {"dim": 0}, {"slices": -1}, {"slices": 65}):
        assert call(**wrong) == -2, wrong                                      # PC_ESHAPE
    for pos in (0, 1, 2, 4, 5, 6, 11, 12, 13):
        assert call(null=pos) == -1, pos                                       # PC_EINVAL
    for wrong in ({"rows": 0}, {"rows": -3}, {"n_types": 0}, {"products": 0}):
        assert call(**wrong) == -1, wrong
    assert call(nbytes=need - 1) == -3                                         # PC_EWORKSPACE
    assert L.pc_rank_grouped_workspace_bytes(R, T, 65) == 0
    torch.cuda.synchronize()
    assert (rank == 12345).all() and int(bad) == 0                             # nothing was launched
    assert call() == 0 and call(dim=256, slices=64) == 0
    torch.cuda.synchronize()
    assert rank.cpu().tolist() == [0] * 4 and int(bad) == 0    # (all scores tie with the target's; product 0 is the lowest)
