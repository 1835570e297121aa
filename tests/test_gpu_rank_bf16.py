"""The rank over the bf16 copy of the catalogue (pc_rank_grouped_bf16, ops.rank_grouped_bf16).  Needs an MI355X.

The defining property is exact: a (row, product) score has the bits the bf16 list entries give it, so rank < 256 exactly when
ops.retrieve_list_grouped (unbiased) / ops.retrieve_list_grouped_bf16_biased holds the target at that position.  Beside it the
float64 reference of tests/test_gpu_nearest.py over the ROUNDED table, s64(r, p) = <q_r, e_p> + float64(bias_fp32[p]), with the
allowance of one entry

    a(r, p) = (3 D + 4) 2^-24 (sum_d |q_d e_pd| + |b_p|):

the chain accumulates 3 D exact products in fp32 (three bf16 pieces per dimension), split3 truncates the query once
(|q - (p0 + p1 + p2)| < 2^-24 |q|), and the bias is one more addition -- that file's derivation with the chain three times as
long.  Every row is held to  #{s64 > g64 + a_p + a_y} <= rank <= #{s64 >= g64 - a_p - a_y};  there is no cap on rows.
Worst |s - s64| / a observed on an MI355X over the 256-entry lists (gate: <= 1): 0.0110 / 0.0097 / 0.0063 at D = 128 and
0.0036 / 0.0036 / 0.0023 at D = 256 (no bias / random bias / half-norm bias)."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_nearest import as_csr, build_ref, dev, ordered
from test_gpu_retrieval_bf16 import exact_case, upload_bf16
from test_gpu_retrieval_grouped import host_csr, mixed_catalogue, mixed_rows, upload

U = 2.0 ** -24
N = 256
SLICES = (0, 1, 2, 64)
LIST_LENGTHS = (0, 1, 15, 16, 17, 40)          # the post-pass's block of 16 holds the target and 15 entries: both sides of the edge


def fixture_from(dim, type_idx, features, T, types, proj):
    """features: what bf16 holds exactly, or what is rounded here; the reference is over the rounded rows."""
    rowptr, col, table32 = upload(type_idx, features, T)
    table = table32.to(torch.bfloat16)
    rounded = table.float().cpu().numpy()
    per_type, where = build_ref(type_idx, rounded, types, proj, T)
    return SimpleNamespace(dim=dim, P=len(type_idx), type_idx=type_idx, rounded=rounded, T=T, types=types, proj=proj,
                           per_type=per_type, where=where, rowptr=rowptr, col=col, table=table,
                           dproj=dev(proj), dtypes=dev(types), dcand=dev(type_idx))


def view(m, r, bias):
    """(cand ascending, s64, allowance a) of row r under `bias` (fp32 numpy or None); empty for a row without candidates."""
    if r not in m.where:
        return np.zeros(0, np.int64), np.zeros(0), np.zeros(0)
    t, j = m.where[r]
    cand, _, dot, adot = m.per_type[t]
    b = np.zeros(len(cand)) if bias is None else bias.astype(np.float64)[cand]
    return cand, dot[:, j] + b, (3 * m.dim + 4) * U * (adot[:, j] + np.abs(b))


@pytest.fixture(scope="module", params=[128, 256], ids=lambda d: f"D{d}")
def mixed(request):
    """20 000 products, 203 rows: type 0 holds over 10 000 (many chunks, real slices), empty types, 3-product types, 30 tied
    copies, rows of type -1 and T, a last tile that is partial."""
    from p_companion_amd import ops
    dim = request.param
    type_idx, features, T = mixed_catalogue(20_000, dim, seed=dim)
    assert (type_idx == 0).sum() > 10_000
    types = mixed_rows(203, T, seed=dim)
    proj = np.random.default_rng(7).standard_normal((203, dim)).astype(np.float32)
    m = fixture_from(dim, type_idx, features, T, types, proj)
    m.bias = {"none": None, "random": dev((np.random.default_rng(3).standard_normal(m.P) * 10).astype(np.float32)),
              "half_norm": ops.half_sq_norm_bias_bf16(m.table)}
    m.hbias = {k: None if v is None else v.cpu().numpy() for k, v in m.bias.items()}
    return m


def serve(m, bias, n, exclude=None, rows=None, slices=0):
    """the bf16 list entry the rank describes: (idx, score) as numpy"""
    from p_companion_amd import ops
    proj, types = (m.dproj, m.dtypes) if rows is None else rows
    if bias is None:
        i, s = ops.retrieve_list_grouped(proj, types, m.rowptr, m.col, m.table, n, slices=slices, exclude=exclude)
    else:
        i, s = ops.retrieve_list_grouped_bf16_biased(proj, types, m.rowptr, m.col, m.table, bias, n, slices=slices, exclude=exclude)
    return i.cpu().numpy(), s.cpu().numpy()


def rank_case(m, hbias, seed):
    """tests/test_gpu_nearest.py's rank_case with its head range at 300: a member of the head of the order, any product of the
    row's type."""
    rng = np.random.default_rng(seed)
    R = len(m.types)
    targets = np.zeros(R, np.int32)
    for r in range(R):
        cand, s64, _ = view(m, r, hbias)
        if not len(cand):
            targets[r] = rng.integers(0, m.P)
        elif r % 3 == 0:
            targets[r] = cand[ordered(cand, s64)][rng.integers(0, min(len(cand), 300))]
        else:
            targets[r] = rng.choice(cand)
    return targets


def exclusion_lists(m, seed, lengths=LIST_LENGTHS):
    """One key per row: a list of lengths[r % len] products, of the row's own type and -- every fifth row -- one of another."""
    rng = np.random.default_rng(seed)
    lists = []
    for r in range(len(m.types)):
        cand = view(m, r, None)[0]
        own = rng.choice(cand, min(len(cand), lengths[r % len(lengths)]), replace=False) if len(cand) else cand
        if r % 5 == 2 and len(own):
            own = np.concatenate([own[1:], np.nonzero(m.type_idx != m.types[r])[0][r:r + 1]])
        lists.append(np.unique(own))
    return lists


# ---- 1. rank <-> list
@pytest.mark.parametrize("kind", ["none", "random", "half_norm"])
def test_rank_below_256_exactly_when_the_list_holds_the_target_there(mixed, kind):
    from p_companion_amd import ops
    m, bias = mixed, mixed.bias[kind]
    R = len(m.types)
    targets = rank_case(m, m.hbias[kind], seed=12)
    lists = exclusion_lists(m, seed=13)
    in_list = [r for r in range(R) if r % 7 == 0 and r in m.where]
    for r in in_list:
        lists[r] = np.unique(np.concatenate([lists[r], [targets[r]]]))
    other = [r for r in range(R) if r % 7 == 1 and r in m.where]
    t2 = targets.copy()
    for r in other:
        t2[r] = np.nonzero(m.type_idx != m.types[r])[0][r]
    assert {len(x) for x in lists} >= {0, 1, 15, 16, 17, 40}
    key = torch.arange(R, dtype=torch.int32, device="cuda")
    for exclude, tg in ((None, targets), ((key,) + as_csr(lists), t2)):
        served, _ = serve(m, bias, N, exclude)
        ct = None if exclude is None else m.dcand
        ranks = []
        for s in SLICES:
            rank, bad = ops.rank_grouped_bf16(m.dproj, m.dtypes, dev(tg), m.rowptr, m.col, m.table, slices=s, exclude=exclude,
                                              cand_type=ct, bias=bias)
            ranks.append(rank)
            assert rank.dtype == torch.int32 and torch.equal(rank, ranks[0]), s
            assert bad.item() == 1                            # the row of type T
        rank = ranks[0].cpu().numpy()
        for r in range(R):
            if r not in m.where:                              # types -1 and T: no rank; an empty type: nothing in front
                typed = 0 <= m.types[r] < m.T
                assert rank[r] == (0 if typed and exclude is None else -1), r
                continue
            if exclude is not None and (tg[r] in lists[r] or m.type_idx[tg[r]] != m.types[r]):
                assert rank[r] == -1, r                       # in the row's list, or no candidate of the row's type
                continue
            assert rank[r] >= 0, r
            if rank[r] < N:
                assert served[r, rank[r]] == tg[r], r
            else:
                assert tg[r] not in served[r], r
        got = rank[[r for r in range(R) if r in m.where]]
        assert ((got >= 0) & (got < N)).sum() >= 20 and (got >= N).sum() >= 20
        if exclude is not None:
            assert all(rank[r] == -1 for r in in_list + other)


@pytest.mark.parametrize("kind", ["none", "half_norm"])
def test_every_product_of_a_small_type_ranks_at_its_position(mixed, kind):
    """For every type of at most 256 products (the 3-product types and the tied type among them): one query, every product of
    the type as its target -- the ranks are the positions in the served list."""
    from p_companion_amd import ops
    m, bias = mixed, mixed.bias[kind]
    sizes = np.bincount(m.type_idx, minlength=m.T)
    small = [t for t in range(m.T) if 0 < sizes[t] <= N]
    assert {3, 4, 5} <= set(small) and len(small) >= 4
    rng = np.random.default_rng(21)
    q = rng.standard_normal((len(small), m.dim)).astype(np.float32)
    served, _ = serve(m, bias, N, rows=(dev(q), dev(np.array(small, np.int32))))
    rows_q, rows_t, rows_y, want = [], [], [], []
    for j, t in enumerate(small):
        k = sizes[t]
        assert (served[j, :k] >= 0).all() and (served[j, k:] == -1).all() and (m.type_idx[served[j, :k]] == t).all()
        rows_q.append(np.repeat(q[j:j + 1], k, 0)); rows_t.append(np.full(k, t, np.int32))
        rows_y.append(served[j, :k].astype(np.int32)); want.append(np.arange(k))
    order = rng.permutation(sum(len(x) for x in want))        # the rows of a type spread over the tiles
    cat = lambda xs: np.concatenate(xs)[order]
    for s in SLICES:
        rank, bad = ops.rank_grouped_bf16(dev(cat(rows_q)), dev(cat(rows_t)), dev(cat(rows_y)), m.rowptr, m.col, m.table,
                                          slices=s, bias=bias)
        assert bad.item() == 0 and (rank.cpu().numpy() == cat(want)).all(), s


# ---- every row-group count, a second tile, every chunk edge
@pytest.mark.parametrize("dim", [128, 256])
def test_type_sizes_and_rows_per_type_at_every_edge(dim):
    """Types of {1, 15, 16, 17, 63, 64, 65, 129} products and {1, 16, 17, 33, 49, 64, 65} rows per type: every row-group count of
    a tile (1..4 at D = 128, 1..2 at D = 256), a second tile, every chunk edge.  Every product of the type is a target."""
    from p_companion_amd import ops
    sizes, per = (1, 15, 16, 17, 63, 64, 65, 129), (1, 16, 17, 33, 49, 64, 65)
    rng = np.random.default_rng(dim + 1)
    type_idx = rng.permutation(np.repeat(np.arange(len(sizes)), sizes)).astype(np.int32)
    features = rng.standard_normal((len(type_idx), dim)).astype(np.float32)
    features[type_idx == 7] = features[type_idx == 7][np.arange(129) % 40]     # exact ties across a chunk edge
    for rows_per in per:
        types = np.repeat(np.arange(len(sizes)), rows_per).astype(np.int32)
        proj = rng.standard_normal((len(types), dim)).astype(np.float32)
        m = fixture_from(dim, type_idx, features, len(sizes), types, proj)
        hb = ops.half_sq_norm_bias_bf16(m.table)
        for bias in (None, hb):
            served, _ = serve(m, bias, N)
            pos = rng.integers(0, np.array(sizes)[types])                       # the target: the product served at pos
            tg = served[np.arange(len(types)), pos].astype(np.int32)
            assert (tg >= 0).all()
            keyed = [np.unique(served[r, :sizes[types[r]]][rng.random(sizes[types[r]]) < 0.3]) for r in range(len(types))]
            key = torch.arange(len(types), dtype=torch.int32, device="cuda")
            for exclude in (None, (key,) + as_csr(keyed)):
                rank, bad = ops.rank_grouped_bf16(m.dproj, m.dtypes, dev(tg), m.rowptr, m.col, m.table, bias=bias,
                                                  exclude=exclude, cand_type=None if exclude is None else m.dcand)
                rank = rank.cpu().numpy()
                assert bad.item() == 0
                if exclude is None:
                    assert (rank == pos).all(), (rows_per, bias is None)
                    continue
                for r in range(len(types)):
                    gone = np.isin(served[r, :pos[r]], keyed[r]).sum()
                    assert rank[r] == (-1 if tg[r] in keyed[r] else pos[r] - gone), (rows_per, r)


# ---- 2. exact data
@pytest.fixture(scope="module", params=[128, 256], ids=lambda d: f"D{d}")
def exact(request):
    """Integer features and queries in [-4, 4]: every product, partial sum, -|e|^2 / 2 and their sum is exact in bf16 x bf16,
    fp32 and float64 alike.  2 000 products: type 0 holds 1 100 (more than one tile of rows), the 59 others about 15 each."""
    dim, P, T, R = request.param, 2_000, 60, 150
    rng = np.random.default_rng(31)
    type_idx = rng.integers(1, T, P).astype(np.int32)
    type_idx[:1100] = 0
    features = rng.integers(-4, 5, (P, dim)).astype(np.float32)
    features[5] = features[3]                                 # exact ties inside type 0
    features[9] = features[3]
    types = rng.integers(0, T, R).astype(np.int32)
    types[:70] = 0
    types[70:74] = [-1, T, 7, 7]
    proj = rng.integers(-4, 5, (R, dim)).astype(np.float32)
    m = fixture_from(dim, type_idx, features, T, types, proj)
    assert np.array_equal(m.rounded, features)
    return m


def test_exact_data_equals_the_fp32_rank_and_the_float64_count(exact):
    from p_companion_amd import ops
    m = exact
    R = len(m.types)
    ib = np.random.default_rng(4).integers(-50, 51, m.P).astype(np.float32)
    ib[[3, 5, 9]] = 7.0                                       # the copied rows stay tied
    hb = ops.half_sq_norm_bias_bf16(m.table)
    assert (hb.cpu().numpy().astype(np.float64) == -0.5 * (m.rounded.astype(np.float64) ** 2).sum(1)).all()
    table32 = m.table.float()
    key = torch.arange(R, dtype=torch.int32, device="cuda")
    for name, bias in (("none", None), ("integer", dev(ib)), ("half_norm", hb)):
        hbias = None if bias is None else bias.cpu().numpy()
        targets = rank_case(m, hbias, seed=14)
        targets[:3] = [3, 5, 9]                               # the tied copies: the product index decides
        lists = exclusion_lists(m, seed=15)
        for exclude in (None, (key,) + as_csr(lists)):
            ct = None if exclude is None else m.dcand
            rank, bad = ops.rank_grouped_bf16(m.dproj, m.dtypes, dev(targets), m.rowptr, m.col, m.table, bias=bias,
                                              exclude=exclude, cand_type=ct)
            r32, b32 = ops.rank_grouped(m.dproj, m.dtypes, dev(targets), m.rowptr, m.col, table32, bias=bias, exclude=exclude,
                                        cand_type=ct)
            assert torch.equal(rank, r32) and bad.item() == b32.item() == 1
            rank = rank.cpu().numpy()
            for r in range(R):
                if r not in m.where:
                    assert rank[r] == (0 if 0 <= m.types[r] < m.T and exclude is None else -1), r
                    continue
                cand, s64, _ = view(m, r, hbias)
                y = targets[r]
                if exclude is not None:
                    if y in lists[r]:
                        assert rank[r] == -1, r
                        continue
                    keep = ~np.isin(cand, lists[r])
                    cand, s64 = cand[keep], s64[keep]
                g = s64[np.searchsorted(cand, y)]
                assert rank[r] == ((s64 > g) | ((s64 == g) & (cand < y))).sum(), (name, r)


# ---- 3. the float64 band
@pytest.mark.parametrize("kind", ["none", "random", "half_norm"])
def test_every_rank_lies_in_the_float64_band(mixed, kind):
    from p_companion_amd import ops
    m, bias = mixed, mixed.bias[kind]
    targets = rank_case(m, m.hbias[kind], seed=16)
    rank, _ = ops.rank_grouped_bf16(m.dproj, m.dtypes, dev(targets), m.rowptr, m.col, m.table, bias=bias)
    rank = rank.cpu().numpy()
    served, score = serve(m, bias, N)
    worst = 0.0
    for r in m.where:
        cand, s64, a = view(m, r, m.hbias[kind])
        j = np.searchsorted(cand, targets[r])
        lo = (s64 > s64[j] + a + a[j]).sum()
        hi = (s64 >= s64[j] - a - a[j]).sum()
        assert lo <= rank[r] <= hi, f"row {r}: rank {rank[r]} outside [{lo}, {hi}]"
        k = (served[r] >= 0).sum()
        pos = np.searchsorted(cand, served[r, :k])
        worst = max(worst, (np.abs(score[r, :k].astype(np.float64) - s64[pos]) / a[pos]).max())
    print(f"rank_grouped_bf16 D={m.dim} bias={kind}: worst |s - s64| / a over the 256-entry lists = {worst:.4f}")
    assert worst <= 1.0


# ---- 4. all three pieces
def three_piece_case():
    """tests/test_gpu_retrieval_bf16.py's construction (table values in {-1, 0, 1}, queries a + b 2^-9 + c 2^-18: every partial
    sum is a multiple of 2^-18 below 2^6, exact in fp32 in any order) with two pairs of products whose order one piece of the
    query alone decides.  Every query has q_0 = 1 + 2^-9 + 2^-18, q_1 = 1 + 2^-9 (equal in p0 and p1, apart in p2) and
    q_2 = 1 + 2^-9, q_3 = 1 (equal in p0, apart in p1).  In type 0, lo < hi differ in e_0, e_1 alone (hi: +1, -1; lo: -1, +1):
    hi scores 2^-17 more, a tie without p2.  lo2 < hi2 differ in e_2, e_3 alone the same way: a tie without p1.  An even row of
    type 0 ranks hi, an odd one hi2: a kernel that drops a piece counts the lower index in front."""
    c = exact_case(22)
    features = np.zeros((c.P, c.D), np.float32)
    for p in range(c.P):
        features[p, c.rng.choice(c.D, 32, replace=False)] = c.rng.choice(np.array([-1.0, 1.0], np.float32), 32)
    a, b, cc = (c.rng.integers(-1, 2, (c.R, c.D)).astype(np.float64) for _ in range(3))
    a[:, :4], b[:, :4], cc[:, :4] = 1, [1, 1, 1, 0], [1, 0, 0, 0]
    q64 = a + b * 2.0 ** -9 + cc * 2.0 ** -18
    proj = q64.astype(np.float32)
    assert (proj.astype(np.float64) == q64).all()
    lo, hi, lo2, hi2 = np.nonzero(c.type_idx == 0)[0][:4]
    features[hi, :4], features[lo, 4:], features[lo, :4] = [1, -1, 0, 0], features[hi, 4:], [-1, 1, 0, 0]
    features[hi2, :4], features[lo2, 4:], features[lo2, :4] = [0, 0, 1, -1], features[hi2, 4:], [0, 0, -1, 1]
    targets = np.array([c.rng.choice(np.nonzero(c.type_idx == t)[0]) if 0 <= t < c.T and (c.type_idx == t).any() else 0
                        for t in c.types], np.int32)
    heavy = np.nonzero(c.types == 0)[0]
    targets[heavy[0::2]], targets[heavy[1::2]] = hi, hi2

    def count(q):
        """the float64 count under the queries q; -2 for a row without candidates"""
        out = np.full(c.R, -2)
        for r, t in enumerate(c.types):
            cand = np.nonzero(c.type_idx == t)[0] if 0 <= t < c.T else np.zeros(0, np.int64)
            if not len(cand):
                continue
            sc = features[cand].astype(np.float64) @ q[r].astype(np.float64)
            g = sc[np.searchsorted(cand, targets[r])]
            out[r] = ((sc > g) | ((sc == g) & (cand < targets[r]))).sum()
        return out

    top = lambda x: (x.view(np.uint32) & np.uint32(0xffff0000)).view(np.float32)
    p0 = top(proj)
    p1 = top(proj - p0)
    full, two, one = count(proj), count((p0 + p1).astype(np.float32)), count(p0)
    # (dropping a piece moves other products too, so not every row is off by exactly one; most are off)
    even, odd = heavy[0::2], heavy[1::2]
    assert (two[even] != full[even]).sum() > len(even) // 2 and (one[odd] != full[odd]).sum() > len(odd) // 2
    return c, features, proj, targets, full


def test_all_three_pieces_of_the_query_are_used():
    from p_companion_amd import ops
    c, features, proj, targets, full = three_piece_case()
    rowptr, col, table, rounded = upload_bf16(c.type_idx, features, c.T)
    assert np.array_equal(rounded, features)
    live = full >= 0
    assert live.sum() >= 65
    lists = [np.zeros(0, np.int64)] * c.R
    key = torch.arange(c.R, dtype=torch.int32, device="cuda")
    for exclude in (None, (key,) + as_csr(lists)):            # (with empty lists the post-pass leaves the count as it is)
        rank, _ = ops.rank_grouped_bf16(dev(proj), dev(c.types), dev(targets), rowptr, col, table, exclude=exclude,
                                        cand_type=None if exclude is None else dev(c.type_idx))
        assert (rank.cpu().numpy()[live] == full[live]).all()
    # the post-pass scores through the same three pieces: lo (lo2) in the list of a row that ranks hi (hi2) stands BEHIND the
    # target and was never counted, so the rank stays; a post-pass that dropped a piece would see a tie, and take one off
    lo, _, lo2, _ = np.nonzero(c.type_idx == 0)[0][:4]
    heavy = np.nonzero(c.types == 0)[0]
    lists = [np.zeros(0, np.int64)] * c.R
    for j, r in enumerate(heavy):
        lists[r] = np.array([lo2 if j % 2 else lo])
    rank, _ = ops.rank_grouped_bf16(dev(proj), dev(c.types), dev(targets), rowptr, col, table, exclude=(key,) + as_csr(lists),
                                    cand_type=dev(c.type_idx))
    assert (rank.cpu().numpy()[heavy] == full[heavy]).all()


# ---- 5. error codes
def test_error_codes_through_ctypes():
    from p_companion_amd import _lib
    L = _lib.lib()
    R, T, P = 4, 2, 4
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32, device="cuda")
    table = torch.zeros(P + 1, 256, dtype=torch.bfloat16, device="cuda")
    b = dict(proj=torch.zeros(R, 256, device="cuda"), types=i32(0, 0, 1, 1), targets=i32(1, 0, 3, 2), row_key=i32(0, 1, -1, 0),
             rows=R, type_rowptr=i32(0, 2, 4), type_col=i32(0, 1, 2, 3), table=table, bias=torch.zeros(P, device="cuda"), n_types=T,
             num_products=P, ex_rowptr=i32(0, 1, 1), ex_col=i32(0), n_keys=2, cand_type=i32(0, 0, 1, 1), dim=128, slices=0,
             rank_out=torch.empty(R, dtype=torch.int32, device="cuda"), bad_count=torch.zeros(1, dtype=torch.int32, device="cuda"),
             ws=torch.empty(L.pc_rank_grouped_bf16_workspace_bytes(R, T, 64), dtype=torch.uint8, device="cuda"))
    b["ws_bytes"] = b["ws"].numel()
    b["stream"] = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    conv = lambda v: ctypes.c_void_p(v.data_ptr()) if torch.is_tensor(v) else v
    none = dict(row_key=None, ex_rowptr=None, ex_col=None, n_keys=0, cand_type=None)

    def rank(**kw):
        return L.pc_rank_grouped_bf16(*[conv(v) for v in {**b, **kw}.values()])

    assert rank() == 0 and rank(dim=256, slices=64) == 0 and rank(**none) == 0
    assert rank(bias=None) == 0 and rank(bias=None, **none) == 0          # the bias may be null
    torch.cuda.synchronize()
    for name in ("proj", "types", "targets", "type_rowptr", "type_col", "table", "rank_out", "bad_count", "ws", "row_key",
                 "ex_rowptr", "ex_col", "cand_type"):
        assert rank(**{name: None}) == -1, name                                   # PC_EINVAL
    assert rank(rows=0) == -1 and rank(n_types=0) == -1 and rank(num_products=0) == -1 and rank(n_keys=-1) == -1
    # lists without cand_type and the reverse
    assert rank(cand_type=None) == -1 and rank(**{**none, "cand_type": b["cand_type"]}) == -1 and rank(**{**none, "n_keys": 1}) == -1
    for kw in (dict(dim=64), dict(dim=192), dict(slices=-1), dict(slices=65)):
        assert rank(**kw) == -2 and rank(**kw, **none) == -2, kw                  # PC_ESHAPE
    off = ctypes.c_void_p(table.data_ptr() + 2)                                   # one bf16 element off: not 16-byte aligned
    assert rank(table=off) == -2 and rank(table=off, **none) == -2
    assert rank(ws_bytes=L.pc_rank_grouped_bf16_workspace_bytes(R, T, 0) - 1) == -3       # PC_EWORKSPACE
    assert L.pc_rank_grouped_bf16_workspace_bytes(R, T, 65) == 0
    for s in (0, 1, 64):
        assert L.pc_rank_grouped_bf16_workspace_bytes(R, T, s) == L.pc_rank_grouped_workspace_bytes(R, T, s) > 0
    torch.cuda.synchronize()
