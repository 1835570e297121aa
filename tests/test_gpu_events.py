"""The behaviour edge lists derived from a shopper event log on the device (csrc/events.hip, ops.event_edges,
data.device_bpg_from_events) against the host twin data.event_edges_host, bit for bit: the hand-made log of
tests/test_events_host.py, every session length at which the kernels change variant, the row-count and session-id edges, times
and kinds at their limits, determinism under a permutation, fields outside their ranges, the edge limit, and a graph built end
to end.  Needs an MI355X."""
import numpy as np
import pytest
import torch

from test_events_host import (BUY, HAND_EXPECT, HAND_LOG, HAND_MAX, HAND_P, HAND_S, LISTS, LISTS_COLUMN, VIEW, assert_edges,
                              random_log)

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024)
GRAPH_ARRAYS = ("cv_rowptr", "cv_col", "similarity_pairs", "sim_rowptr", "sim_col", "complementary_pairs")
to_numpy = lambda t: t.cpu().numpy()


def on_device(log):
    return torch.from_numpy(np.ascontiguousarray(log, np.int32)).cuda()


def assert_equals_twin(log, n_products, n_sessions=None, **kw):
    """ops.event_edges over the uploaded log against the twin: the three lists and the stats.  Returns the device result."""
    from p_companion_amd import ops
    from p_companion_amd.data import event_edges_host
    want = event_edges_host(log, n_products, n_sessions, **kw)
    got = ops.event_edges(on_device(log), n_products, n_sessions, **kw)
    assert isinstance(got, ops.EventEdges) and all(getattr(got, name).is_cuda for name in LISTS)
    assert_edges(got, {name: getattr(want, name) for name in LISTS}, want.n_sessions, want.skipped_sessions, want.n_items,
                 to_numpy=to_numpy)
    return got


def assert_same_bits(a, b):
    assert all(torch.equal(getattr(a, name), getattr(b, name)) for name in LISTS) and a[3:] == b[3:]


@pytest.mark.parametrize("exclusive", [True, False])
def test_hand_made_log_gives_the_literal_lists(exclusive):
    from p_companion_amd import ops
    got = ops.event_edges(on_device(HAND_LOG), HAND_P, HAND_S, max_events=HAND_MAX, exclusive=exclusive)
    assert_edges(got, HAND_EXPECT[exclusive], 6, 1, 8, to_numpy=to_numpy)
    assert_edges(ops.event_edges(on_device(HAND_LOG), HAND_P, max_events=HAND_MAX, exclusive=exclusive), HAND_EXPECT[exclusive],
                 5, 1, 8, to_numpy=to_numpy)


def length_log(products, seed=4):
    """One session per entry of LENGTHS, in a shuffled order of rows.  products: 'distinct' (a session's rows all differ),
    'one' (every row the same product) or 'half' (drawn from half as many products as rows: about half the rows repeat);
    kinds even, times from 0..7, so equal times are common."""
    rng = np.random.default_rng(seed)
    rows = []
    for s, n in enumerate(LENGTHS):
        p = {"distinct": lambda: rng.permutation(1100)[:n], "one": lambda: np.full(n, 7),
             "half": lambda: rng.integers(0, n // 2 + 1, n)}[products]()
        rows.append(np.stack([np.full(n, s), p, rng.integers(0, 2, n), rng.integers(0, 8, n)], 1))
    log = np.concatenate(rows).astype(np.int32)
    return log[rng.permutation(len(log))]


@pytest.fixture(scope="module", params=["distinct", "one", "half"])
def lengths(request):
    return request.param, length_log(request.param)


@pytest.mark.parametrize("max_events", [1024, 64, None])
def test_session_lengths_at_every_variants_edge(lengths, max_events):
    products, log = lengths
    kw = {} if max_events is None else dict(max_events=max_events)
    got = assert_equals_twin(log, 1100, len(LENGTHS), **kw)
    assert got.skipped_sessions == sum(n > (max_events or 256) for n in LENGTHS)
    if products == "one":
        assert got.n_items == len(LENGTHS) - got.skipped_sessions and all(len(getattr(got, name)) == 0 for name in LISTS)
    elif products == "distinct":
        assert got.n_items == sum(n for n in LENGTHS if n <= (max_events or 256)) and len(got.co_view) > 0


@pytest.mark.parametrize("n_rows", [0, 1, 255, 256, 257])
def test_row_counts_at_the_launch_edges(n_rows):
    from p_companion_amd import ops
    rng = np.random.default_rng(n_rows)
    session = np.repeat(np.arange(n_rows), np.tile([1, 2, 3], n_rows // 3 + 1)[:n_rows])[:n_rows]      # sessions of 1, 2, 3, 1, ... rows
    log =np.stack([session, rng.integers(0, 9, n_rows), rng.integers(0, 2, n_rows), rng.integers(0, 4, n_rows)], 1).astype(np.int32)
    got = assert_equals_twin(log, 9)
    if n_rows == 0:
        assert all(tuple(getattr(got, name).shape) == (0, 2) and getattr(got, name).dtype == torch.int32 for name in LISTS)
        assert got[3:] == (0, 0, 0)
        assert ops.event_edges(on_device(log), 9, 3)[3:] == (3, 0, 0)
    else:
        assert_equals_twin(log, 9, n_rows + 5, exclusive=False)


def test_session_ids_with_gaps_and_empty_ends():
    log = random_log(5, n_sessions=40, longest=6)
    log[:, 0] = log[:, 0] * 3 + 2                                            # ids 2, 5, ..., 119: 0, 1 and every gap empty
    got = assert_equals_twin(log, 30, 125)                                   # ... and 120..124 empty
    assert got.n_sessions == 125 and len(got.co_view) > 0
    assert_equals_twin(log, 30)                                              # None: 120 sessions
    assert_equals_twin(log, 30, 2 ** 20, exclusive=False)


def test_times_and_kinds_at_their_limits():
    T = 2 ** 31 - 1
    log = np.array([
        (0, 1, VIEW, 5), (0, 2, BUY, 5),                                     # equal times: (1, 2) is purchased after view
        (1, 1, VIEW, 6), (1, 2, BUY, 5), (1, 2, BUY, 0),                     # the only view is later than every purchase: absent
        (2, 3, VIEW, 0), (2, 4, BUY, 0), (2, 5, VIEW, T), (2, 6, BUY, T), (2, 7, VIEW, T), (2, 7, VIEW, 0),      # times 0 and 2^31 - 1
        (3, 1, VIEW, 2), (3, 1, BUY, 1), (3, 2, VIEW, 1), (3, 2, BUY, 2), (3, 0, VIEW, 2),                      # viewed and purchased
        (4, 3, BUY, 9), (4, 3, BUY, 9), (4, 3, BUY, 9), (4, 5, VIEW, 9), (4, 5, VIEW, 9),                      # repeated identical rows
        (5, 1, VIEW, 1), (5, 2, VIEW, 2), (5, 3, VIEW, 3),                   # view-only
        (6, 1, BUY, 1), (6, 2, BUY, 2), (6, 3, BUY, 3),                      # purchase-only
    ], np.int32)
    for exclusive in (True, False):
        got = assert_equals_twin(log, 8, exclusive=exclusive)
        pv = set(map(tuple, to_numpy(got.purchase_after_view).tolist()))
        assert (1, 2) in pv and (3, 4) in pv and (3, 6) in pv and (5, 6) in pv and (7, 4) in pv and (5, 4) not in pv
        assert ((2, 1) in pv) == (not exclusive)             # session 3: item 2 was itself purchased
    got = assert_equals_twin(log[2:5], 8, exclusive=True)
    assert len(got.purchase_after_view) == 0 and got.n_items == 2


def test_a_permuted_log_and_a_second_call_give_identical_bits():
    from p_companion_amd import ops
    log = on_device(np.concatenate([random_log(6, n_sessions=300, longest=40, n_products=50), length_log("half")[:, :4] +
                                    np.array([300, 0, 0, 0], np.int32)]))
    first = ops.event_edges(log, 1100, 320, max_events=1024)
    assert len(first.co_view) > 0 and len(first.purchase_after_view) > 0 and len(first.co_purchase) > 0
    assert_same_bits(first, ops.event_edges(log, 1100, 320, max_events=1024))
    gen = torch.Generator(device="cuda").manual_seed(3)
    shuffled = log[torch.randperm(log.shape[0], device="cuda", generator=gen)].contiguous()
    assert not torch.equal(shuffled, log)
    assert_same_bits(first, ops.event_edges(shuffled, 1100, 320, max_events=1024))


def test_fields_outside_their_ranges_raise_and_the_device_stays_usable():
    from p_companion_amd import ops
    good = HAND_LOG[HAND_LOG[:, 0] != 4]
    for column, value in (("session", -1), ("session", HAND_S), ("product", -1), ("product", HAND_P), ("kind", -1), ("kind", 2),
                          ("time", -1)):
        log = good.copy()
        log[3, LISTS_COLUMN[column]] = value
        with pytest.raises(ValueError, match=column) as err:
            ops.event_edges(on_device(log), HAND_P, HAND_S)
        named = str(err.value).split(" out of range")[0]
        assert all(other not in named for other in LISTS_COLUMN if other != column)
    log = good.copy()
    log[0, 1], log[5, 3] = 2 ** 31 - 1, -(2 ** 31)
    with pytest.raises(ValueError, match="product, time"):
        ops.event_edges(on_device(log), HAND_P, HAND_S)
    with pytest.raises(ValueError, match="session"):                          # None: a negative id is still an offender
        ops.event_edges(on_device(np.array([(-2, 0, 0, 0)], np.int32)), HAND_P)
    # a valid call afterwards, on the same device
    got = ops.event_edges(on_device(HAND_LOG), HAND_P, HAND_S, max_events=HAND_MAX)
    assert_edges(got, HAND_EXPECT[True], 6, 1, 8, to_numpy=to_numpy)


def test_a_list_over_the_edge_limit_is_refused_by_name(monkeypatch):
    from p_companion_amd import ops
    monkeypatch.setattr(ops, "EVENT_EDGE_LIMIT", 10)
    log = on_device(HAND_LOG)
    assert len(ops.event_edges(log, HAND_P, HAND_S, max_events=HAND_MAX).co_view) == 10           # at the limit: served
    with pytest.raises(ValueError, match="co_view would hold 12 edges.*lower max_events"):
        ops.event_edges(log, HAND_P, HAND_S, max_events=HAND_MAX, exclusive=False)
    buys = on_device(np.array([(0, p, BUY, p) for p in range(4)] + [(1, 0, VIEW, 0), (1, 1, VIEW, 0)], np.int32))
    with pytest.raises(ValueError, match="co_purchase would hold 12 edges") as err:
        ops.event_edges(buys, HAND_P)
    assert "co_view" not in str(err.value)
    monkeypatch.undo()
    assert len(ops.event_edges(buys, HAND_P).co_purchase) == 12


def test_a_graph_from_events_equals_the_host_builders():
    from p_companion_amd.data import IntBPG, device_bpg_from_edges, device_bpg_from_events, event_edges_host
    # product 30 is co-viewed with 32 in three sessions, with 31 and 33 in one each: under degree_cap = 2 its row keeps 32 by
    # weight and, of the two of weight 1, the lower id
    extra = [(200 + s, p, VIEW, 0) for s in range(3) for p in (30, 32)] + [(203, 30, VIEW, 0), (203, 31, VIEW, 0),
                                                                          (204, 30, VIEW, 1), (204, 33, VIEW, 0)]
    log = np.concatenate([random_log(3), np.array(extra, np.int32)])
    P, S = 34, 205
    types = (np.arange(P) % 4).astype(np.int32)
    feats = np.random.default_rng(0).standard_normal((P, 8)).astype(np.float32)
    for cap, max_events, exclusive in ((2, 256, True), (5, 8, False)):
        dev = device_bpg_from_events(feats, types, 4, log, n_sessions=S, degree_cap=cap, max_events=max_events, exclusive=exclusive)
        host = IntBPG.from_events(feats, types, log, n_sessions=S, degree_cap=cap, max_events=max_events, exclusive=exclusive)
        e = event_edges_host(log, P, S, max_events=max_events, exclusive=exclusive)
        lists = device_bpg_from_edges(feats, types, 4, e.co_view, e.purchase_after_view, e.co_purchase, degree_cap=cap)
        h, l = dev.to_host(), lists.to_host()
        for k in GRAPH_ARRAYS + ("features", "type_idx"):
            a = getattr(h, k)
            assert a.dtype == getattr(host, k).dtype and np.array_equal(a, getattr(host, k)), k
            assert np.array_equal(a, getattr(l, k)), k
        assert dev.max_degree == host.max_degree == lists.max_degree == cap and dev.n_similarity_pairs > 0
        assert (dev.n_sessions, dev.skipped_sessions, dev.n_items) == (S, e.skipped_sessions, e.n_items)
        assert (dev.skipped_sessions > 0) == (max_events == 8)
        if cap == 2:
            assert h.get_neighbors(30).tolist() == [31, 32]
