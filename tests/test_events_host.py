"""The behaviour edge lists derived from a shopper event log, on the host: data.event_edges_host (the numpy twin of
ops.event_edges, csrc/events.hip) against a brute-force restatement of the semantics written here -- plain Python sets and
dicts per session, straight from the predicates -- on a hand-made log whose expected lists are written out, and on seeded
random logs; IntBPG.from_events; the C ABI's declarations; and ops.event_edges' refusals, which come before any launch (the
library is a recording stand-in).  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

VIEW, BUY = 0, 1

# ---- the hand-made log: 6 sessions over 7 products, max_events = 10 ------------------------------------------------------
# session 0 (10 rows): item 1 viewed at 5, 2, 2 (a repeated row): fv 2; item 2 purchased at 4 and 9: lp 9; item 3 viewed at 10,
#   later than every purchase; item 4 viewed at 9, purchased at 1; item 5 viewed and purchased at 3
# session 1: item 6 viewed at 7, item 0 purchased at 7 (equal times count)
# session 2: one row; sessions 3 and 5: empty; session 4: 11 rows, skipped whole
HAND_P, HAND_S, HAND_MAX = 7, 6, 10
HAND_LOG = np.array([(0, 1, VIEW, 5), (0, 1, VIEW, 2), (0, 1, VIEW, 2), (0, 2, BUY, 4), (0, 2, BUY, 9), (0, 3, VIEW, 10),
                     (0, 4, VIEW, 9), (0, 4, BUY, 1), (0, 5, VIEW, 3), (0, 5, BUY, 3),
                     (1, 6, VIEW, 7), (1, 0, BUY, 7),
                     (2, 3, VIEW, 1)] + [(4, i % 5, i % 2, i) for i in range(11)], np.int32)[
    np.random.default_rng(1).permutation(24)]
HAND_EXPECT = {
    True: dict(co_view=[(1, 3), (1, 4), (1, 5), (3, 1), (3, 4), (3, 5), (4, 1), (4, 3), (5, 1), (5, 3)],
               purchase_after_view=[(1, 2), (1, 5), (6, 0)],
               co_purchase=[(2, 4), (2, 5), (4, 2), (4, 5), (5, 2), (5, 4)]),
    False: dict(co_view=[(1, 3), (1, 4), (1, 5), (3, 1), (3, 4), (3, 5), (4, 1), (4, 3), (4, 5), (5, 1), (5, 3), (5, 4)],
                purchase_after_view=[(1, 2), (1, 5), (4, 2), (5, 2), (6, 0)],
                co_purchase=[(2, 4), (2, 5), (4, 2), (4, 5), (5, 2), (5, 4)]),
}
HAND_STATS = dict(n_sessions=6, skipped_sessions=1, n_items=8)
LISTS = ("co_view", "purchase_after_view", "co_purchase")


def brute_force(events, n_sessions, max_events, exclusive):
    """The semantics from the predicates: (lists as Python lists of (a, b) in (session, a, b) order, skipped, items)."""
    sessions = {}
    for s, p, k, t in np.asarray(events).tolist():
        sessions.setdefault(s, []).append((p, k, t))
    out = {name: [] for name in LISTS}
    skipped = items = 0
    for s in range(n_sessions):
        rows = sessions.get(s, [])
        if len(rows) > max_events:
            skipped += 1
            continue
        views, buys = {}, {}
        for p, k, t in rows:
            if k == VIEW:
                views[p] = min(t, views.get(p, t))
            else:
                buys[p] = max(t, buys.get(p, t))
        products = sorted(set(views) | set(buys))
        items += len(products)
        for a in products:
            for b in products:
                if a == b:
                    continue
                both_bought = a in buys and b in buys
                if both_bought:
                    out["co_purchase"].append((a, b))
                if a in views and b in views and not (exclusive and both_bought):
                    out["co_view"].append((a, b))
                if a in views and b in buys and views[a] <= buys[b] and not (exclusive and a in buys):
                    out["purchase_after_view"].append((a, b))
    return out, skipped, items


def assert_edges(got, want_lists, n_sessions, skipped, items, to_numpy=np.asarray):
    for name in LISTS:
        a = to_numpy(getattr(got, name))
        want = np.array(want_lists[name], np.int32).reshape(-1, 2)
        assert a.dtype == np.int32 and a.shape == want.shape and np.array_equal(a, want), name
    assert (got.n_sessions, got.skipped_sessions, got.n_items) == (n_sessions, skipped, items)


def random_log(seed, n_sessions=200, longest=12, n_products=30, times=6):
    """Sessions of 1..longest rows; few products and fewer times: repeats, view-and-purchase items and equal times are common."""
    rng = np.random.default_rng(seed)
    rows = []
    for s in range(n_sessions):
        n = int(rng.integers(1, longest + 1))
        rows.append(np.stack([np.full(n, s), rng.integers(0, n_products, n), rng.integers(0, 2, n), rng.integers(0, times, n)], 1))
    log = np.concatenate(rows).astype(np.int32)
    return log[rng.permutation(len(log))]


@pytest.mark.parametrize("exclusive", [True, False])
def test_hand_made_log_gives_the_literal_lists(exclusive):
    from p_companion_amd.data import event_edges_host
    got = event_edges_host(HAND_LOG, HAND_P, HAND_S, max_events=HAND_MAX, exclusive=exclusive)
    assert_edges(got, HAND_EXPECT[exclusive], **{"skipped": 1, "items": 8, "n_sessions": 6})
    want, skipped, items = brute_force(HAND_LOG, HAND_S, HAND_MAX, exclusive)
    assert want == HAND_EXPECT[exclusive] and (skipped, items) == (1, 8)
    # n_sessions None: the largest id + 1 (session 5 is empty: 5 sessions)
    assert_edges(event_edges_host(HAND_LOG, HAND_P, max_events=HAND_MAX, exclusive=exclusive), HAND_EXPECT[exclusive], 5, 1, 8)
    # every session kept: session 4's pairs appear
    full = event_edges_host(HAND_LOG, HAND_P, HAND_S, max_events=11, exclusive=exclusive)
    want, skipped, items = brute_force(HAND_LOG, HAND_S, 11, exclusive)
    assert_edges(full, want, HAND_S, 0, 13)
    assert len(full.co_purchase) > len(got.co_purchase) and (skipped, items) == (0, 13)


@pytest.mark.parametrize("exclusive", [True, False])
@pytest.mark.parametrize("seed,max_events", [(0, 256), (1, 8), (2, 2)])
def test_random_logs_equal_the_brute_force(seed, max_events, exclusive):
    from p_companion_amd.data import event_edges_host
    log = random_log(seed)
    want, skipped, items = brute_force(log, 200, max_events, exclusive)
    assert (skipped > 0) == (max_events < 12) and all(len(want[name]) > 0 for name in LISTS)
    assert_edges(event_edges_host(log, 30, 200, max_events=max_events, exclusive=exclusive), want, 200, skipped, items)
    # a function of the log as a multiset of rows
    again = event_edges_host(log[::-1], 30, 200, max_events=max_events, exclusive=exclusive)
    assert_edges(again, want, 200, skipped, items)


def test_the_twin_names_the_offending_columns():
    from p_companion_amd.data import event_edges_host
    good = HAND_LOG[HAND_LOG[:, 0] != 4]
    for column, value in (("session", -1), ("session", HAND_S), ("product", -1), ("product", HAND_P), ("kind", -1), ("kind", 2),
                          ("time", -1)):
        log = good.copy()
        log[3, LISTS_COLUMN[column]] = value
        with pytest.raises(ValueError, match=column) as err:
            event_edges_host(log, HAND_P, HAND_S)
        assert all(other not in str(err.value).split(" out of range")[0] for other in LISTS_COLUMN if other != column)
    for kw in (dict(max_events=1), dict(max_events=1025), dict(n_sessions=0)):
        with pytest.raises(ValueError):
            event_edges_host(good, HAND_P, **kw)
    with pytest.raises(ValueError):
        event_edges_host(good[:, :3], HAND_P)
    empty = event_edges_host(np.zeros((0, 4), np.int32), HAND_P)
    assert_edges(empty, {name: [] for name in LISTS}, 0, 0, 0)


LISTS_COLUMN = {"session": 0, "product": 1, "kind": 2, "time": 3}


def test_from_events_is_from_edges_over_the_twins_lists():
    from p_companion_amd.data import IntBPG, event_edges_host
    log = random_log(3)
    types = (np.arange(30) % 4).astype(np.int32)
    feats = np.random.default_rng(0).standard_normal((30, 8)).astype(np.float32)
    for cap, max_events, exclusive in ((None, 256, True), (2, 8, True), (3, 256, False)):
        e = event_edges_host(log, 30, 200, max_events=max_events, exclusive=exclusive)
        want = IntBPG.from_edges(feats, types, e.co_view, e.purchase_after_view, e.co_purchase, degree_cap=cap)
        got = IntBPG.from_events(feats, types, log, n_sessions=200, degree_cap=cap, max_events=max_events, exclusive=exclusive)
        for k in ("features", "type_idx", "cv_rowptr", "cv_col", "similarity_pairs", "complementary_pairs", "sim_rowptr", "sim_col"):
            assert np.array_equal(getattr(got, k), getattr(want, k)), k
        assert len(want.cv_col) > 0 and got.n_types == want.n_types
    # the session weights decide a capped row: 0 is co-viewed with 2 in three sessions, with 1 and 3 in one each
    log = np.array([(s, p, VIEW, 0) for s in range(3) for p in (0, 2)] + [(3, 0, VIEW, 0), (3, 1, VIEW, 0), (4, 0, VIEW, 1),
                                                                           (4, 3, VIEW, 0)], np.int32)
    g = IntBPG.from_events(None, np.zeros(4, np.int32), log, degree_cap=2)
    assert g.get_neighbors(0).tolist() == [1, 2]             # (2 by weight 3; of 1 and 3, both weight 1, the lower id)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------
ENTRIES = {
    "pc_events_limits": "max_events n_totals",
    "pc_events_count": "events n_events n_sessions n_products cnt bad stream",
    "pc_events_scatter": "events n_events n_sessions n_products max_events rowptr cursor bucket stream",
    "pc_events_sessions": "n_sessions rowptr bucket last_purchase max_events exclusive n_items count_cv count_pv count_cp totals "
                          "stream",
    "pc_events_emit": "n_sessions rowptr bucket last_purchase n_items max_events exclusive off_cv off_pv off_cp out_cv out_pv "
                      "out_cp stream",
}


def test_the_header_declares_the_entries_and_the_table_binds_them():
    from p_companion_amd import _lib, ops
    txt = open(os.path.join(ROOT, "include", "pcompanion_hip.h")).read()
    assert re.search(r"#define PC_ABI_VERSION 8\b", txt)
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert sorted(set(re.findall(r"\b(pc_events_[a-z0-9_]+)\s*\(", code))) == sorted(ENTRIES)
    for name, want in ENTRIES.items():
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, name
        assert [re.sub(r"\W", "", a.split()[-1]) for a in m.group(1).split(",")] == want.split(), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == len(want.split()), name
        assert _lib.SIGNATURES[name][0] is ctypes.c_int
    L = _lib.lib()                                           # binds every signature; raises on a missing symbol
    assert L.pc_abi_version() == 8
    most, words = ctypes.c_int(0), ctypes.c_int(0)
    assert L.pc_events_limits(ctypes.byref(most), ctypes.byref(words)) == 0
    assert most.value == ops.EVENT_MAX_EVENTS == 1024 and words.value == 5
    assert ops.EVENT_EDGE_LIMIT == 2 ** 31 - 1
    # argument checks come before any launch: null pointers, a max_events outside 2..1024
    assert L.pc_events_limits(None, None) == -1
    assert L.pc_events_count(None, 4, 1, 1, None, None, None) == -1
    assert L.pc_events_scatter(None, 0, 1, 1, 1, 16, 16, 16, None) == -2
    assert L.pc_events_sessions(1, 16, 16, 16, 1025, 1, 16, 16, 16, 16, 16, None) == -2
    assert L.pc_events_emit(1, 16, 16, 16, 16, 0, 1, 16, 16, 16, 16, 16, 16, None) == -2
    assert L.pc_events_emit(1, None, 16, 16, 16, 2, 1, 16, 16, 16, 16, 16, 16, None) == -1


# ---- the wrapper's refusals reach nothing -------------------------------------------------------------------------------
class OnDevice(torch.Tensor):
    """A stand-in that reports is_cuda: the checks test the device first, and this lets the ones behind it be reached."""
    is_cuda = True


class Recorder:
    """ops._lib.lib(): every attribute is an entry that records (name, arguments) and succeeds."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return 0
        return entry


@pytest.fixture
def rec(monkeypatch):
    from p_companion_amd import ops
    r = Recorder()
    monkeypatch.setattr(ops._lib, "lib", lambda: r)
    monkeypatch.setattr(ops, "_stream", lambda: ctypes.c_void_p(0x5EED0))
    return r


def test_the_refusals_come_before_any_launch(rec):
    from p_companion_amd import ops
    on = lambda t: t.as_subclass(OnDevice)
    good = on(torch.from_numpy(HAND_LOG.copy()))
    wide = on(torch.zeros(24, 8, dtype=torch.int32))
    refused = [
        (dict(events=torch.from_numpy(HAND_LOG.copy())), "on the device"),                    # a CPU tensor
        (dict(events=HAND_LOG), "on the device"),                                             # not a tensor
        (dict(events=on(torch.from_numpy(HAND_LOG.astype(np.int64)))), "int32"),
        (dict(events=on(torch.zeros(24, 3, dtype=torch.int32))), r"\[N, 4\]"),
        (dict(events=on(torch.zeros(96, dtype=torch.int32))), r"\[N, 4\]"),
        (dict(events=wide[:, :4]), "contiguous"),
        (dict(max_events=1), "max_events"), (dict(max_events=1025), "max_events"), (dict(max_events=2.5), "max_events"),
        (dict(n_sessions=0), "n_sessions"), (dict(n_sessions=-3), "n_sessions"),
        (dict(n_products=0), "n_products"),
    ]
    for kw, message in refused:
        kw = {"events": good, "n_products": HAND_P, "n_sessions": HAND_S, **kw}
        with pytest.raises(ValueError, match=message):
            ops.event_edges(**kw)
        assert rec.calls == [], message
