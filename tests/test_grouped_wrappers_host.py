"""Which C entry the grouped serving wrappers reach, and with which arguments (ops.retrieve_topk_grouped,
ops.retrieve_list_grouped, ops.rank_grouped), without a GPU and without the library: the calls are recorded, not made.

The tensors are host tensors that report is_cuda; ops._lib.lib() is an object whose every attribute records its call
(returning WS_BYTES for a *_workspace_bytes query, 0 otherwise), ops._stream gives one fixed stand-in and ops.workspace one
fixed buffer.  A recorded pointer -- a ctypes.c_void_p or the bare address, which ctypes passes alike where the entry's argtype
is c_void_p (the first test checks that it is) -- is named through data_ptr().  ARGS holds every entry's argument list in the order of
include/pcompanion_hip.h, written out here and compared with the header's text by the first test."""
import ctypes
import itertools
import os
import re

import pytest
import torch

from conftest import ROOT

R, P, T, D, KEYS = 6, 9, 3, 128, 4
WS_BYTES = 4096                          # what every recorded *_workspace_bytes query answers

FILTERED = ("proj types row_key rows type_rowptr type_col table n_types ex_rowptr ex_col n_keys n dim slices out_idx out_score "
            "bad_count ws ws_bytes stream")
ARGS = {
    "pc_retrieve_topk_grouped_workspace_bytes": "rows n_types n slices",
    "pc_retrieve_topk_grouped_excluding_workspace_bytes": "rows n_types n slices",
    "pc_retrieve_topk_grouped_bf16_workspace_bytes": "rows n_types n slices",
    "pc_retrieve_topk_grouped_biased_workspace_bytes": "rows n_types n slices",
    "pc_retrieve_list_grouped_workspace_bytes": "rows n_types n slices",
    "pc_rank_grouped_workspace_bytes": "rows n_types slices",
    "pc_rank_grouped_biased_workspace_bytes": "rows n_types slices",
    "pc_retrieve_topk_grouped": "proj types rows type_rowptr type_col table n_types n dim slices out_idx out_score ws ws_bytes "
                                "stream",
    "pc_retrieve_topk_grouped_excluding": FILTERED,
    "pc_retrieve_topk_grouped_bf16": FILTERED,
    "pc_retrieve_list_grouped": FILTERED,
    "pc_retrieve_topk_grouped_biased": "proj types row_key rows type_rowptr type_col table bias n_types ex_rowptr ex_col n_keys n "
                                       "dim slices out_idx out_score bad_count ws ws_bytes stream",
    "pc_rank_grouped": "proj types targets rows type_rowptr type_col table n_types num_products dim slices rank_out bad_count ws "
                       "ws_bytes stream",
    "pc_rank_grouped_excluding": "proj types targets row_key rows type_rowptr type_col table n_types num_products ex_rowptr ex_col "
                                 "n_keys cand_type dim slices rank_out bad_count ws ws_bytes stream",
    "pc_rank_grouped_biased": "proj types targets row_key rows type_rowptr type_col table bias n_types num_products ex_rowptr "
                              "ex_col n_keys cand_type dim slices rank_out bad_count ws ws_bytes stream",
}
# the query that belongs to an entry: its own, but pc_rank_grouped_excluding sizes its workspace as pc_rank_grouped does
QUERY = {name: name + "_workspace_bytes" for name in ARGS if not name.endswith("_workspace_bytes")}
QUERY["pc_rank_grouped_excluding"] = "pc_rank_grouped_workspace_bytes"
TAG = {name: "retrieve_grouped" for name in QUERY}
TAG.update(pc_retrieve_list_grouped="retrieve_list", pc_rank_grouped="rank_grouped", pc_rank_grouped_excluding="rank_grouped",
           pc_rank_grouped_biased="rank_grouped")
# (table, a triple given, a bias given) -> the entry retrieve_topk_grouped reaches
TOPK_ENTRY = {("fp32", False, False): "pc_retrieve_topk_grouped", ("fp32", True, False): "pc_retrieve_topk_grouped_excluding",
              ("fp32", False, True): "pc_retrieve_topk_grouped_biased", ("fp32", True, True): "pc_retrieve_topk_grouped_biased",
              ("bf16", False, False): "pc_retrieve_topk_grouped_bf16", ("bf16", True, False): "pc_retrieve_topk_grouped_bf16"}
# (a triple with cand_type given, a bias given) -> the entry rank_grouped reaches
RANK_ENTRY = {(False, False): "pc_rank_grouped", (True, False): "pc_rank_grouped_excluding",
              (False, True): "pc_rank_grouped_biased", (True, True): "pc_rank_grouped_biased"}


def test_the_argument_lists_are_the_headers():
    txt = open(os.path.join(ROOT, "include", "pcompanion_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name, want in ARGS.items():
        m = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, name
        got = [re.sub(r"\W", "", a.split()[-1]) for a in m.group(1).split(",")]
        assert [{"table_bf16": "table"}.get(a, a) for a in got] == want.split(), name
        # every pointer of the header is declared to ctypes as an address, every count as an integer
        from p_companion_amd import _lib
        declared = [ctypes.c_void_p if "*" in a else {"int": ctypes.c_int, "size_t": ctypes.c_size_t}[a.split()[0]]
                    for a in m.group(1).split(",")]
        assert _lib.SIGNATURES[name][1] == declared, name


class OnDevice(torch.Tensor):
    """A stand-in that reports is_cuda: _req tests the device first, and this lets the calls behind it be reached."""
    is_cuda = True


def dev(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype).as_subclass(OnDevice)


class Recorder:
    """ops._lib.lib(): every attribute is an entry that records (name, arguments) and succeeds."""

    def __init__(self):
        self.calls, self.workspaces = [], []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return WS_BYTES if name.endswith("_workspace_bytes") else 0
        return entry


STREAM = ctypes.c_void_p(0x5EED0)
WS = dev(2 * WS_BYTES, dtype=torch.uint8)             # (larger than asked for: ws_bytes is the buffer's size, not the query's)


@pytest.fixture
def rec(monkeypatch):
    from p_companion_amd import ops
    r = Recorder()
    monkeypatch.setattr(ops._lib, "lib", lambda: r)
    monkeypatch.setattr(ops, "_stream", lambda: STREAM)
    monkeypatch.setattr(ops, "workspace", lambda nbytes, device, tag="ws": (r.workspaces.append((nbytes, tag)), WS)[1])
    return r


def tensors(d=D, bf16=False, proj_shape=None, empty_col=False):
    i32 = torch.int32
    return dict(proj=dev(*(proj_shape or (R, d))), types=dev(R, dtype=i32), targets=dev(R, dtype=i32),
                type_rowptr=dev(T + 1, dtype=i32), type_col=dev(P, dtype=i32),
                table=dev(P, d, dtype=torch.bfloat16 if bf16 else torch.float32), bias=dev(P), cand_type=dev(P, dtype=i32),
                row_key=dev(R, dtype=i32), ex_rowptr=dev(KEYS + 1, dtype=i32), ex_col=dev(0 if empty_col else 5, dtype=i32),
                bad_count=dev(1, dtype=i32))


def triple(ts):
    return ts["row_key"], ts["ex_rowptr"], ts["ex_col"]


def recorded(rec, ts, entry, outputs, scalars, null=(), fresh=()):
    """Assert that exactly (the entry's query, the entry) were called, the query with `scalars`, the workspace fetched once under
    the entry's tag, and the entry with ARGS[entry]: a tensor of `ts` or `outputs` by its pointer, a name of `null` as a null
    pointer, a name of `fresh` as a pointer to nothing the caller holds, a scalar by its value."""
    assert [name for name, _ in rec.calls] == [QUERY[entry], entry]
    assert rec.workspaces == [(WS_BYTES, TAG[entry])]
    values = dict(scalars, ws_bytes=WS.numel())
    assert list(rec.calls[0][1]) == [values[a] for a in ARGS[QUERY[entry]].split()]
    known = {t.data_ptr(): name for name, t in {**ts, **outputs}.items() if t.numel()}
    known.update({WS.data_ptr(): "ws", STREAM.value: "stream"})
    args = rec.calls[1][1]
    assert len(args) == len(ARGS[entry].split())
    for name, arg in zip(ARGS[entry].split(), args):
        if name in values:
            assert type(arg) is int and arg == values[name], (entry, name, arg)
            continue
        assert arg is None or type(arg) in (int, ctypes.c_void_p), (entry, name, arg)
        address = arg.value if isinstance(arg, ctypes.c_void_p) else arg
        if name in null:
            assert address is None, (entry, name, arg)
        elif name in fresh:
            assert address and address not in known and address != ts[name].data_ptr(), (entry, name, arg)
        else:
            assert address is not None and known.get(address) == name, (entry, name, known.get(address))


NO_TRIPLE = ("row_key", "ex_rowptr", "ex_col", "bad_count", "cand_type")


# (a bias with a bf16 table and a counter without a triple are refused: test_the_refusals_reach_nothing)
@pytest.mark.parametrize("table,exclude,bias,bad", [c for c in itertools.product(("fp32", "bf16"), (None, "triple", "empty"),
                                                                                 (False, True), (False, True))
                                                    if not (c[2] and c[0] == "bf16") and not (c[3] and c[1] is None)])
def test_retrieve_topk_grouped_reaches_the_entry_with_the_headers_arguments(rec, monkeypatch, table, exclude, bias, bad):
    from p_companion_amd import ops
    if exclude == "empty":
        # the wrapper makes its one-entry stand-in for an empty ex_col with torch.zeros: that too has to report is_cuda
        zeros = torch.zeros
        monkeypatch.setattr(torch, "zeros", lambda *a, **kw: zeros(*a, **kw).as_subclass(OnDevice))
    entry = TOPK_ENTRY[table, exclude is not None, bias]
    for slices, n in itertools.product((0, 7), (1, 16)):
        ts = tensors(bf16=table == "bf16", empty_col=exclude == "empty")
        rec.calls.clear(), rec.workspaces.clear()
        idx, sc = ops.retrieve_topk_grouped(ts["proj"], ts["types"], ts["type_rowptr"], ts["type_col"], ts["table"], n, slices,
                                            exclude=triple(ts) if exclude else None, bad=ts["bad_count"] if bad else None,
                                            bias=ts["bias"] if bias else None)
        assert tuple(idx.shape) == (R, n) and idx.dtype == torch.int32
        assert tuple(sc.shape) == (R, n) and sc.dtype == torch.float32
        scalars = dict(rows=R, n_types=T, n=n, dim=D, slices=slices, n_keys=KEYS if exclude else 0)
        fresh = (("ex_col",) if exclude == "empty" else ()) + (("bad_count",) if exclude and not bad else ())
        recorded(rec, ts, entry, dict(out_idx=idx, out_score=sc), scalars, null=() if exclude else NO_TRIPLE, fresh=fresh)


@pytest.mark.parametrize("exclude,bad", [(False, False), (True, False), (True, True)])
def test_retrieve_list_grouped_reaches_its_entry_with_the_headers_arguments(rec, exclude, bad):
    from p_companion_amd import ops
    for n in (1, 17, 256):
        ts = tensors()
        rec.calls.clear(), rec.workspaces.clear()
        idx, sc = ops.retrieve_list_grouped(ts["proj"], ts["types"], ts["type_rowptr"], ts["type_col"], ts["table"], n,
                                            exclude=triple(ts) if exclude else None, bad=ts["bad_count"] if bad else None)
        assert tuple(idx.shape) == (R, n) and idx.dtype == torch.int32
        assert tuple(sc.shape) == (R, n) and sc.dtype == torch.float32
        scalars = dict(rows=R, n_types=T, n=n, dim=D, slices=0, n_keys=KEYS if exclude else 0)
        recorded(rec, ts, "pc_retrieve_list_grouped", dict(out_idx=idx, out_score=sc), scalars,
                 null=() if exclude else NO_TRIPLE, fresh=("bad_count",) if exclude and not bad else ())


@pytest.mark.parametrize("exclude", [False, True])
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("bad", [False, True])
def test_rank_grouped_reaches_the_entry_with_the_headers_arguments(rec, exclude, bias, bad):
    from p_companion_amd import ops
    ts = tensors()
    kw = dict(exclude=triple(ts), cand_type=ts["cand_type"]) if exclude else {}
    rank, counter = ops.rank_grouped(ts["proj"], ts["types"], ts["targets"], ts["type_rowptr"], ts["type_col"], ts["table"],
                                     bad=ts["bad_count"] if bad else None, bias=ts["bias"] if bias else None, **kw)
    assert tuple(rank.shape) == (R,) and rank.dtype == torch.int32
    assert tuple(counter.shape) == (1,) and counter.dtype == torch.int32
    assert (counter is ts["bad_count"]) == bad        # the caller's counter is passed and returned; a fresh one otherwise
    if not bad:
        assert int(counter) == 0
        ts.pop("bad_count")
    scalars = dict(rows=R, n_types=T, num_products=P, dim=D, slices=0, n_keys=KEYS if exclude else 0)
    recorded(rec, ts, RANK_ENTRY[exclude, bias], dict(rank_out=rank, bad_count=counter), scalars,
             null=() if exclude else ("row_key", "ex_rowptr", "ex_col", "cand_type"))


def test_the_width_the_slices_and_the_row_shape_travel(rec):
    """D = 256 once per wrapper (with slices = 7 for the two that were not run with it above), and proj as [2, 3, D]: 6 rows."""
    from p_companion_amd import ops
    ts = tensors(d=256)
    idx, sc = ops.retrieve_topk_grouped(ts["proj"], ts["types"], ts["type_rowptr"], ts["type_col"], ts["table"], 10,
                                        exclude=triple(ts), bad=ts["bad_count"], bias=ts["bias"])
    recorded(rec, ts, "pc_retrieve_topk_grouped_biased", dict(out_idx=idx, out_score=sc),
             dict(rows=R, n_types=T, n=10, dim=256, slices=0, n_keys=KEYS))
    rec.calls.clear(), rec.workspaces.clear()
    ts = tensors(d=256)
    idx, sc = ops.retrieve_list_grouped(ts["proj"], ts["types"], ts["type_rowptr"], ts["type_col"], ts["table"], 100, slices=7)
    recorded(rec, ts, "pc_retrieve_list_grouped", dict(out_idx=idx, out_score=sc),
             dict(rows=R, n_types=T, n=100, dim=256, slices=7, n_keys=0), null=NO_TRIPLE)
    rec.calls.clear(), rec.workspaces.clear()
    ts = tensors(d=256)
    rank, counter = ops.rank_grouped(ts["proj"], ts["types"], ts["targets"], ts["type_rowptr"], ts["type_col"], ts["table"],
                                     slices=7, bad=ts["bad_count"], exclude=triple(ts), cand_type=ts["cand_type"])
    assert counter is ts["bad_count"]
    recorded(rec, ts, "pc_rank_grouped_excluding", dict(rank_out=rank),
             dict(rows=R, n_types=T, num_products=P, dim=256, slices=7, n_keys=KEYS))
    rec.calls.clear(), rec.workspaces.clear()
    ts = tensors(proj_shape=(2, 3, D))
    idx, sc = ops.retrieve_topk_grouped(ts["proj"], ts["types"], ts["type_rowptr"], ts["type_col"], ts["table"], 5)
    assert tuple(idx.shape) == (R, 5) and tuple(sc.shape) == (R, 5)
    recorded(rec, ts, "pc_retrieve_topk_grouped", dict(out_idx=idx, out_score=sc), dict(rows=R, n_types=T, n=5, dim=D, slices=0))


def test_the_refusals_reach_nothing(rec):
    """One invalid argument at a time: the exception's type and message, and no call at all -- not even a workspace query."""
    from p_companion_amd import ops
    ts = tensors()
    bf = tensors(bf16=True)["table"]
    i32 = torch.int32
    rows = (ts["proj"], ts["types"])
    csr = (ts["type_rowptr"], ts["type_col"])
    topk = lambda table=ts["table"], n=10, **kw: ops.retrieve_topk_grouped(*rows, *csr, table, n, **kw)
    lst = lambda n=100, **kw: ops.retrieve_list_grouped(*rows, *csr, ts["table"], n, **kw)
    rank = lambda **kw: ops.rank_grouped(*rows, ts["targets"], *csr, ts["table"], **kw)
    rk, rp, cl = triple(ts)
    refused = [
        (topk, dict(bad=ts["bad_count"]),
         "retrieve_topk_grouped: bad counts keys out of range and is read with an exclude triple only"),
        (lst, dict(bad=ts["bad_count"]),
         "retrieve_list_grouped: bad counts keys out of range and is read with an exclude triple only"),
        (rank, dict(cand_type=ts["cand_type"]), "rank_grouped: cand_type is read with an exclude triple only"),
        (rank, dict(exclude=(rk, rp, cl)),
         "rank_grouped: exclude needs cand_type (the type under which each product is a candidate)"),
        (rank, dict(exclude=(rk, rp, cl), cand_type=dev(P + 1, dtype=i32)),
         "rank_grouped: cand_type must be an int32 tensor of one entry per product"),
        (topk, dict(table=bf, bias=ts["bias"]),
         "retrieve_topk_grouped: bias with a bf16 table is not supported (the biased entries read the fp32 table)"),
        (topk, dict(bias=dev(P + 1)),
         f"retrieve_topk_grouped: bias of shape ({P + 1},) is not supported: it must hold one entry per product ({P})"),
        (rank, dict(bias=dev(P, dtype=torch.float64)),
         "rank_grouped: bias of dtype torch.float64 is not supported: it must be float32"),
        (lst, dict(n=0), "retrieve_list_grouped: n must be in [1, 256], got 0"),
        (lst, dict(n=257), "retrieve_list_grouped: n must be in [1, 256], got 257"),
        (topk, dict(exclude=(rk, rp)), "retrieve_topk_grouped: exclude must be the triple (row_key, ex_rowptr, ex_col) of tensors"),
        (lst, dict(exclude="lists"), "retrieve_list_grouped: exclude must be the triple (row_key, ex_rowptr, ex_col) of tensors"),
        (rank, dict(exclude=(rk, rp, None), cand_type=ts["cand_type"]),
         "rank_grouped: exclude must be the triple (row_key, ex_rowptr, ex_col) of tensors"),
        (topk, dict(exclude=(rk.long(), rp, cl)), "retrieve_topk_grouped: exclude row_key must be int32, got torch.int64"),
        (lst, dict(exclude=(rk, rp, cl.float())), "retrieve_list_grouped: exclude ex_col must be int32, got torch.float32"),
        (topk, dict(exclude=(rk, rp.reshape(KEYS + 1, 1), cl)),
         f"retrieve_topk_grouped: exclude ex_rowptr must be 1-D, got shape ({KEYS + 1}, 1)"),
        (rank, dict(exclude=(rk[:R - 1], rp, cl), cand_type=ts["cand_type"]),
         f"rank_grouped: exclude row_key must hold one key per row ({R}), got {R - 1}"),
        (topk, dict(exclude=(rk, rp[:0], cl)), "retrieve_topk_grouped: exclude ex_rowptr must hold n_keys + 1 >= 1 entries"),
    ]
    for fn in (topk, lst, rank):
        for slices in (-1, 65):
            refused.append((fn, dict(slices=slices), f"slices must be in [0, 64] (0 = automatic), got {slices}"))
    for fn, kw, message in refused:
        with pytest.raises(ValueError) as e:
            fn(**kw)
        assert str(e.value) == message
        assert rec.calls == [] and rec.workspaces == [], message
