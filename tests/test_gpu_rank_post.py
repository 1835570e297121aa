"""The row post-pass of the rank entries (rk_post in csrc/grouped_rank.h behind rk_exclude_kernel, nb_rank_exclude_kernel,
rb_rank_exclude_kernel, wr_post_kernel and wrb_post_kernel) at its block edges and exits.  Needs an MI355X.

The post-pass scores the target in column 0 and the row's exclusion list behind it in blocks of 16 columns, so lists of 15 | 16
and 31 | 32 entries end on either side of a block.  The other suites reach those lengths only by chance of the draw; here every
case is one hand-made row, all rows of a variant in ONE call.

The catalogue: P = 48 products in two types (0..39 and 40..47), rows, queries and bias of small integers -- every dot product,
every bias sum and the bf16 copy are exact, in both chains and in float64 -- so the oracle is a plain numpy count over the passing,
non-excluded candidates under (score descending, product index ascending).  Products 10 and 30 are copies of product 20 (row, bias
and attributes): a tie with a smaller and with a larger index.  Product 39 has the longest row by far and the `last` rows ask with
-row 39: there the target 39 is behind every other candidate in every variant, so EVERY listed candidate that passes was counted
and is taken off again, and the rank says whether the entry at a block's edge was seen.  The predicate of the _where variants is
one band on value (it fails a quarter of the products) and one deny bit (a fifth): about half of a type fails."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_gpu_nearest import as_csr, dev
from test_gpu_where_list import passes

P, P0 = 48, 40                                                # products; those of type 0 (type 1: the other 8)
LENGTHS = (0, 1, 14, 15, 16, 17, 31, 32, 33)
BAND = (1.0, 3.0, 0, 4)                                       # lo, hi, need, deny
VARIANTS = ("excluding", "biased", "bf16", "bf16_biased", "where", "where_biased", "bf16_where", "bf16_where_biased")
BIG = 2 ** 31 - 1


def catalogue(dim):
    rng = np.random.default_rng(dim)
    feats = rng.integers(-3, 4, (P, dim)).astype(np.float32)
    feats[39] = np.where(rng.random(dim) < 0.5, -4.0, 4.0)    # |row 39|^2 = 16 D: twice any other row's, and more
    feats[10] = feats[30] = feats[20]
    bias = rng.integers(-50, 51, P).astype(np.float32)
    bias[10] = bias[30] = bias[20]
    value = (np.arange(P) % 4).astype(np.float32)             # the band fails value 0
    flags = np.where(np.arange(P) % 5 == 1, 4 | 1, 1).astype(np.int32)      # the deny bit
    for p in (2, 10, 20, 30, 38, 39, 42):
        value[p], flags[p] = 2.0, 1                           # these pass
    value[7], flags[9] = 0.0, 5                               # 7 fails the band, 9 the deny bit
    type_idx = (np.arange(P) >= P0).astype(np.int32)
    return SimpleNamespace(dim=dim, rng=rng, feats=feats, bias=bias, value=value, flags=flags, type_idx=type_idx)


def rows_of(c):
    """[(name, type, target, key kind, list, query)]: one row per case.  key kind "own": the row's own list; -1, -2, "n_keys": that
    key.  A query None: a random one."""
    rng = c.rng
    ok = passes(c.value, c.flags, *BAND)
    assert ok[[2, 10, 20, 30, 38, 39, 42]].all() and not ok[7] and not ok[9] and 16 <= ok[:P0].sum() <= 26
    last = -c.feats[39]
    tie = rng.integers(-4, 5, c.dim).astype(np.float32)       # one query for the tie rows: their ranks are compared
    rows = []
    for n in LENGTHS:
        # the last entry (the largest id: the block's edge) and the first are candidates that pass; some of the rest fail
        pick = sorted(rng.choice(np.arange(3, 38), n - 2, replace=False).tolist()) if n > 2 else []
        rows.append((f"last{n}", 0, 39, "own", ([2] if n > 1 else []) + pick + ([38] if n > 0 else []), last))
        y = int(rng.choice(np.nonzero(ok[:P0])[0]))
        rows.append((f"any{n}", 0, y, "own", sorted(rng.choice(np.setdiff1d(np.arange(P0), [y]), n, replace=False).tolist()), None))
    rows += [
        ("target_in_list", 0, 20, "own", [3, 20, 25], None),
        ("target_alone_in_list", 0, 39, "own", [39], last),
        ("target_at_a_block_edge", 0, 39, "own", list(range(15)) + [39], last),            # column 16: the second block's first
        ("entries_past_P", 0, 39, "own", [5, 38, 48, 1000, BIG], last),
        ("only_entries_past_P", 0, 2, "own", [48, BIG], None),
        ("entries_of_the_other_type", 0, 39, "own", [3, 38, 41, 42, 47], last),
        ("type1_row_with_type0_entries", 1, 42, "own", [0, 2, 38, 39, 44], None),
        ("entries_that_fail", 0, 39, "own", [7, 9, 38], last),                              # 7, 9: never counted, never taken off
        ("only_entries_that_fail", 0, 39, "own", [0, 4, 7, 9], last),
        ("tie_smaller_id_listed", 0, 20, "own", [10], tie),                                # 10 precedes 20: counted, taken off
        ("tie_larger_id_listed", 0, 20, "own", [30], tie),                                 # 30 follows 20: never counted
        ("tie_both_listed", 0, 20, "own", [10, 30], tie),
        ("tie_target_first", 0, 10, "own", [20, 30], tie),
        ("tie_target_last", 0, 30, "own", [10, 20], tie),
        ("key_minus_1", 0, 39, -1, [], last),
        ("key_minus_2", 0, 39, -2, [], last),
        ("key_n_keys", 0, 20, "n_keys", [], None),
        ("target_of_the_other_type", 0, 42, "own", [3], None),
        ("target_of_the_other_type_no_list", 0, 42, -1, [], None),
        ("target_fails_its_predicate", 0, 7, "own", [3, 38], None),
        ("target_fails_its_predicate_no_list", 0, 9, -1, [], None),
        ("row_without_a_type", -1, 20, "own", [3], None),
    ]
    return rows


def build(dim):
    """The catalogue and its rows as numpy arrays."""
    c = catalogue(dim)
    rows = rows_of(c)
    R = len(rows)
    c.names = [r[0] for r in rows]
    c.types = np.array([r[1] for r in rows], np.int32)
    c.targets = np.array([r[2] for r in rows], np.int32)
    c.lists = [r[4] for r in rows if r[3] == "own"]
    n_keys = len(c.lists)
    own = iter(range(n_keys))
    c.key = np.array([next(own) if r[3] == "own" else n_keys if r[3] == "n_keys" else r[3] for r in rows], np.int32)
    c.proj = np.stack([c.rng.integers(-4, 5, c.dim).astype(np.float32) if r[5] is None else r[5] for r in rows])
    assert all(sorted(set(x)) == list(x) for x in c.lists)    # strictly ascending, as exclusion_csr builds them
    assert sorted(len(r[4]) for r in rows if r[0].startswith("last")) == sorted(LENGTHS)
    c.R = R
    return c


@pytest.fixture(scope="module", params=[128, 256], ids=lambda d: f"D{d}")
def cases(request):
    c = build(request.param)
    c.dev = SimpleNamespace(proj=dev(c.proj), types=dev(c.types), targets=dev(c.targets), rowptr=dev(np.array([0, P0, P], np.int32)),
                            col=dev(np.arange(P, dtype=np.int32)), cand_type=dev(c.type_idx), table=dev(c.feats),
                            table16=dev(c.feats).to(torch.bfloat16), bias=dev(c.bias), exclude=(dev(c.key),) + as_csr(c.lists))
    assert torch.equal(c.dev.table16.float(), c.dev.table)    # the bf16 copy is exact
    return c


def oracle(c, biased, where):
    """(rank [R], bad): the contract in numpy, exact."""
    s = c.feats.astype(np.float64) @ c.proj.astype(np.float64).T + (c.bias[:, None].astype(np.float64) if biased else 0.0)   # [P, R]
    ok = passes(c.value, c.flags, *BAND) if where else np.ones(P, bool)
    ids = np.arange(P)
    rank, bad = np.full(c.R, -1, np.int64), 0
    for r in range(c.R):
        t, y, key = c.types[r], c.targets[r], c.key[r]
        if key < -1 or key >= len(c.lists):
            bad += 1
            key = -1
        if t < 0 or c.type_idx[y] != t or not ok[y]:
            continue
        listed = np.isin(ids, c.lists[key]) if key >= 0 else np.zeros(P, bool)
        if listed[y]:
            continue
        front = (s[:, r] > s[y, r]) | ((s[:, r] == s[y, r]) & (ids < y))
        rank[r] = ((c.type_idx == t) & ok & ~listed & front).sum()
    return rank, bad


@pytest.mark.parametrize("variant", VARIANTS)
def test_post_pass_at_every_block_edge_and_exit(cases, variant):
    from p_companion_amd import ops
    c, d = cases, cases.dev
    biased, where, bf16 = "biased" in variant, "where" in variant, "bf16" in variant
    table = d.table16 if bf16 else d.table
    kw = dict(exclude=d.exclude, cand_type=d.cand_type, bias=d.bias if biased else None)
    if where:
        full = lambda x, dt: dev(np.full(c.R, x, dt))
        w = ops.RowWhere(value=dev(c.value), flags=dev(c.flags), lo=full(BAND[0], np.float32), hi=full(BAND[1], np.float32),
                         need=full(BAND[2], np.int32), deny=full(BAND[3], np.int32))
        rank, bad = ops.rank_grouped_where(d.proj, d.types, d.targets, d.rowptr, d.col, table, w, **kw)
    elif bf16:
        rank, bad = ops.rank_grouped_bf16(d.proj, d.types, d.targets, d.rowptr, d.col, table, **kw)
    else:
        rank, bad = ops.rank_grouped(d.proj, d.types, d.targets, d.rowptr, d.col, table, **kw)
    rank = rank.cpu().numpy()
    want, want_bad = oracle(c, biased, where)
    wrong = [(c.names[r], int(rank[r]), int(want[r])) for r in range(c.R) if rank[r] != want[r]]
    assert not wrong, wrong
    assert bad.item() == want_bad == 2
    what_the_rows_are_there_for(c, want, where)


def what_the_rows_are_there_for(c, want, where):
    at = {n: want[i] for i, n in enumerate(c.names)}
    ok = passes(c.value, c.flags, *BAND) if where else np.ones(P, bool)
    behind = ok[:P0].sum() - 1                                # the target 39 behind every other passing candidate of its type
    for n in LENGTHS:                                         # every listed candidate that passes is taken off, the edge's too
        assert at[f"last{n}"] == behind - ok[c.lists[c.key[c.names.index(f"last{n}")]]].sum()
    assert at["key_minus_1"] == at["key_minus_2"] == at["last0"] == behind
    assert at["entries_past_P"] == behind - 2 and at["entries_of_the_other_type"] == behind - 2
    assert at["entries_that_fail"] == (behind - 1 if where else behind - 3) and at["only_entries_that_fail"] == (behind if where else behind - 4)
    assert at["tie_larger_id_listed"] == at["tie_smaller_id_listed"] + 1 == at["tie_both_listed"] + 1      # the copy in front alone
    assert 0 <= at["tie_target_first"] <= at["tie_both_listed"] <= at["tie_target_last"]      # (equal but for other products' ties)
    for n in ("target_in_list", "target_alone_in_list", "target_at_a_block_edge", "target_of_the_other_type",
              "target_of_the_other_type_no_list", "row_without_a_type"):
        assert at[n] == -1
    assert (at["target_fails_its_predicate"] == -1) == (at["target_fails_its_predicate_no_list"] == -1) == where
    assert at["type1_row_with_type0_entries"] >= 0 and at["only_entries_past_P"] >= 0
