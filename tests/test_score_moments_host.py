"""The host side of the score moments (pc_score_moments_grouped / pc_score_moments_grouped_bf16; ops.score_moments_grouped,
ops.standardise_scores; PCompanionInference.score_moments and normalise="zscore"), without a GPU: the header and the ctypes
table, the workspace query, what the entries refuse before anything is launched, which entry the wrapper reaches per table dtype
-- recorded, not made --, every ValueError of the wrapper and of the five methods before anything is computed, and
standardise_scores against numpy on CPU tensors."""
import ctypes
import inspect
import itertools
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_grouped_wrappers_host import OnDevice, P, R, STREAM, T, WS, WS_BYTES, D, dev, rec, tensors      # noqa: F401
from test_where_list_host import Untouchable

PC_EINVAL, PC_ESHAPE, PC_EWORKSPACE = -1, -2, -3
ENTRIES = ("pc_score_moments_grouped", "pc_score_moments_grouped_bf16")
QUERY = "pc_score_moments_grouped_workspace_bytes"
ARGS = ("proj types rows type_rowptr type_col table n_types dim slices count pivot s1 s2 mean std_out bad_count ws ws_bytes "
        "stream").split()
METHODS = ("recommend_batch", "recommend_capped_batch", "recommend_page_batch", "recommend_basket_batch",
           "recommend_session_batch")


def test_header_declares_the_entries_and_the_abi_stays_8():
    from p_companion_amd import _lib
    txt = open(os.path.join(ROOT, "include", "pcompanion_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ENTRIES:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, name
        got = [re.sub(r"\W", "", a.split()[-1]) for a in m.group(1).split(",")]
        assert [{"table_bf16": "table"}.get(a, a) for a in got] == ARGS, name
        declared = [ctypes.c_void_p if "*" in a else {"int": ctypes.c_int, "size_t": ctypes.c_size_t}[a.split()[0]]
                    for a in m.group(1).split(",")]
        assert _lib.SIGNATURES[name] == (ctypes.c_int, declared), name
    assert re.search(r"\bsize_t\s+%s\s*\(\s*int rows,\s*int n_types,\s*int slices\s*\)\s*;" % QUERY, code)
    assert _lib.SIGNATURES[QUERY] == _lib.SIGNATURES["pc_rank_grouped_workspace_bytes"]
    assert re.search(r"const float \*table,", re.search(r"\bint\s+%s\s*\(([^)]*)\)" % ENTRIES[0], code).group(1))
    assert re.search(r"const uint16_t \*table_bf16,", re.search(r"\bint\s+%s\s*\(([^)]*)\)" % ENTRIES[1], code).group(1))
    assert re.search(r"#define\s+PC_ABI_VERSION\s+8\b", txt)
    assert _lib.lib().pc_abi_version() == 8


def test_the_units_are_part_of_the_build():
    from p_companion_amd import build
    assert {"score_moments.hip", "score_moments_bf16.hip"} <= set(build.sources())


def test_the_workspace_is_the_plan_and_two_sums_per_row_and_slice():
    """The rank's plan, then p1 / p2 [rows][S] and the pivots [rows] fp32, each rounded up to 256 bytes."""
    from p_companion_amd import _lib
    L = _lib.lib()
    ws, plain = getattr(L, QUERY), L.pc_rank_grouped_workspace_bytes
    assert ws.restype == ctypes.c_size_t
    up = lambda n: (n + 255) & ~255
    for rows, types, s in itertools.product((1, 17, 203, 12288), (1, 9, 100), (0, 1, 7, 64)):
        S = s or 16
        assert ws(rows, types, s) == plain(rows, types, s) + 2 * up(rows * S * 4) + up(rows * 4), (rows, types, s)
    for bad in ((0, 100, 0), (5, 0, 0), (5, 100, -1), (5, 100, 65)):
        assert ws(*bad) == 0, bad


@pytest.mark.parametrize("name", ENTRIES)
def test_the_entries_refuse_before_anything_is_launched(name):
    from p_companion_amd import _lib
    entry = getattr(_lib.lib(), name)
    buf = ctypes.create_string_buffer(96)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)      # passes every check, and no check dereferences it

    def call(**kw):
        a = dict(proj=p, types=p, rows=4, type_rowptr=p, type_col=p, table=p, n_types=3, dim=128, slices=0, count=p, pivot=p,
                 s1=p, s2=p, mean=p, std_out=p, bad_count=p, ws=p, ws_bytes=0, stream=None)
        assert list(a) == ARGS
        a.update(kw)
        return entry(*a.values())

    assert call() == PC_EWORKSPACE and call(dim=256, slices=64) == PC_EWORKSPACE           # in order: the workspace check
    for arg in ("proj", "types", "type_rowptr", "type_col", "table", "count", "pivot", "s1", "s2", "mean", "std_out", "bad_count",
                "ws"):
        assert call(**{arg: None}) == PC_EINVAL, arg
    assert call(rows=0) == PC_EINVAL and call(n_types=0) == PC_EINVAL and call(rows=-3) == PC_EINVAL
    for kw in (dict(dim=64), dict(dim=192), dict(slices=-1), dict(slices=65)):
        assert call(**kw) == PC_ESHAPE, kw
        assert call(proj=None, **kw) == PC_EINVAL, kw                                      # the pointers, then the shapes
    if "bf16" in name:
        assert call(table=ctypes.c_void_p(p.value + 8)) == PC_ESHAPE                       # the bf16 table's alignment
    assert bytes(buf) == bytes(96)                                                         # nothing was written


@pytest.mark.parametrize("table,bad", itertools.product(("fp32", "bf16"), (False, True)))
def test_the_wrapper_reaches_the_entry_of_the_tables_dtype(rec, monkeypatch, table, bad):
    from p_companion_amd import _lib, ops
    sig = inspect.signature(ops.score_moments_grouped)
    assert list(sig.parameters) == ["proj", "types", "type_rowptr", "type_col", "table", "slices", "bad"]
    assert [sig.parameters[k].default for k in ("slices", "bad")] == [0, None]
    for fn in ("zeros", "empty"):                         # the outputs the wrapper makes have to report is_cuda too
        orig = getattr(torch, fn)
        monkeypatch.setattr(torch, fn, lambda *a, _f=orig, **kw: _f(*a, **{**kw, "device": None}).as_subclass(OnDevice))
    entry = ENTRIES[table == "bf16"]
    ts = tensors(bf16=table == "bf16")
    m = ops.score_moments_grouped(ts["proj"], ts["types"], ts["type_rowptr"], ts["type_col"], ts["table"], slices=7,
                                  bad=ts["bad_count"] if bad else None)
    assert isinstance(m, ops.ScoreMoments)
    assert m.count.dtype == torch.int32 and tuple(m.count.shape) == (R,)
    for f in ("mean", "std", "pivot", "s1", "s2"):
        assert getattr(m, f).dtype == torch.float32 and tuple(getattr(m, f).shape) == (R,), f
    assert (m.bad is ts["bad_count"]) if bad else (tuple(m.bad.shape) == (1,) and m.bad.dtype == torch.int32)
    assert [name for name, _ in rec.calls] == [QUERY, entry]                               # one query for both entries
    assert list(rec.calls[0][1]) == [R, T, 7] and rec.workspaces == [(WS_BYTES, "score_moments")]
    args = [a.value if isinstance(a, ctypes.c_void_p) else a for a in rec.calls[1][1]]
    assert len(args) == len(_lib.SIGNATURES[entry][1])
    assert args == [ts["proj"].data_ptr(), ts["types"].data_ptr(), R, ts["type_rowptr"].data_ptr(), ts["type_col"].data_ptr(),
                    ts["table"].data_ptr(), T, D, 7, m.count.data_ptr(), m.pivot.data_ptr(), m.s1.data_ptr(), m.s2.data_ptr(),
                    m.mean.data_ptr(), m.std.data_ptr(), m.bad.data_ptr(), WS.data_ptr(), WS.numel(), STREAM.value]
    assert len({m.count.data_ptr(), m.pivot.data_ptr(), m.s1.data_ptr(), m.s2.data_ptr(), m.mean.data_ptr(),
                m.std.data_ptr()}) == 6


def test_the_wrapper_refuses_before_anything_is_reached(rec):
    from p_companion_amd import ops
    for ts in (tensors(), tensors(bf16=True)):
        base = (ts["proj"], ts["types"], ts["type_rowptr"], ts["type_col"])
        # the table: fp32 or bf16, [P, 128 or 256]
        for table in (ts["table"].double(), ts["table"].half(), ts["table"].int(), ts["table"][0], [0.0] * P, None):
            with pytest.raises(ValueError, match="table must be a"):
                ops.score_moments_grouped(*base, table)
        for table in (ts["table"][:, :64], ts["table"][:0], dev(P, 192, dtype=ts["table"].dtype)):
            with pytest.raises(ValueError, match="128 or 256 columns"):
                ops.score_moments_grouped(*base, table)
        # types: int32, one per row
        for types in (ts["types"][:-1], dev(R + 1, dtype=torch.int32), ts["types"].long(), dev(R, 1, dtype=torch.int32), None):
            with pytest.raises(ValueError, match="types must be an int32 tensor of one entry per row"):
                ops.score_moments_grouped(ts["proj"], types, ts["type_rowptr"], ts["type_col"], ts["table"])
        with pytest.raises(ValueError, match="proj must be"):
            ops.score_moments_grouped(dev(R, D + 1), ts["types"], ts["type_rowptr"], ts["type_col"], ts["table"])
        with pytest.raises(ValueError, match="type_rowptr"):
            ops.score_moments_grouped(ts["proj"], ts["types"], dev(1, dtype=torch.int32), ts["type_col"], ts["table"])
        for slices in (-1, 65, 1000):
            with pytest.raises(ValueError, match="slices must be in"):
                ops.score_moments_grouped(*base, ts["table"], slices=slices)
        with pytest.raises(ValueError, match="bad"):
            ops.score_moments_grouped(*base, ts["table"], bad=dev(2, dtype=torch.int32))
    assert rec.calls == [] and rec.workspaces == []


def test_the_methods_refuse_an_unknown_normalise_before_the_model_runs():
    from p_companion_amd.inference import CompactInference, PCompanionInference
    inf = object.__new__(PCompanionInference)
    inf.__dict__.update(model=Untouchable(), features=Untouchable(), bpg=Untouchable(), exclusions=Untouchable(),
                        config=Untouchable(), type_idx=Untouchable(), type_rowptr=Untouchable(), type_col=Untouchable(),
                        device="cpu")
    q = torch.zeros(2, dtype=torch.int32)
    for name in METHODS:
        assert getattr(CompactInference, name) is getattr(PCompanionInference, name)       # inherited, not restated
        for unknown in ("minmax", "ZSCORE", "", 0, True, ("zscore",)):
            with pytest.raises(ValueError, match=rf"{name}: normalise must be None or 'zscore'"):
                getattr(inf, name)(q, normalise=unknown)
        assert "normalise" in getattr(PCompanionInference, name).__doc__
    assert inf._normalise is None and "_normalise" not in inf.__dict__
    # "zscore" passes the check and reaches the method's own checks, and the mode does not outlive a call that raises
    inf.__dict__["config"] = type("C", (), {"NUM_COMP_TYPES": 3})()
    with pytest.raises(ValueError, match="need 1 <= per_type"):
        inf.recommend_page_batch(q, per_type=0, normalise="zscore")
    assert inf._normalise is None
    assert list(inspect.signature(PCompanionInference.score_moments).parameters) == ["self", "query_idx"]
    assert "exclusion" in PCompanionInference.score_moments.__doc__


def reference_z(score, mean, std, count):
    s, m, d = score.astype(np.float32), mean.astype(np.float32), std.astype(np.float32)
    flat = np.broadcast_to((count < 2) | (d == 0), s.shape)
    with np.errstate(all="ignore"):
        z = ((s - m) / np.where(d == 0, np.float32(1), d)).astype(np.float32)
    z = np.where(flat, np.float32(0), z)
    return np.where(np.isneginf(s), np.float32(-np.inf), z).astype(np.float32)


def test_standardise_scores_against_numpy_on_every_branch():
    from p_companion_amd import ops
    rng = np.random.default_rng(11)
    rows, n = 64, 9
    score = (rng.standard_normal((rows, n)) * 30 + 100).astype(np.float32)
    mean = (rng.standard_normal((rows, 1)) * 30 + 100).astype(np.float32)
    std = (rng.random((rows, 1)) * 20 + 0.01).astype(np.float32)
    count = rng.integers(2, 10_000, (rows, 1)).astype(np.int32)
    count[:6, 0] = [0, 1, 1, 0, 2, 2]                         # count < 2: z = 0 -- and count == 2 on the other side of the edge
    std[6:10, 0] = 0                                          # std == 0: z = 0
    std[1, 0] = 0
    score[::5, -2:] = -np.inf                                 # the padding of a short list, in every kind of row
    score[0, :] = -np.inf
    z = ops.standardise_scores(torch.from_numpy(score), torch.from_numpy(mean), torch.from_numpy(std), torch.from_numpy(count))
    assert z.dtype == torch.float32 and tuple(z.shape) == (rows, n)
    want = reference_z(score, mean, std, count)
    assert (z.numpy().view(np.int32) == want.view(np.int32)).all()
    assert (z.numpy()[:4][np.isfinite(score[:4])] == 0).all() and (z.numpy()[6:10][np.isfinite(score[6:10])] == 0).all()
    assert np.isneginf(z.numpy()[np.isneginf(score)]).all() and np.isfinite(z.numpy()[np.isfinite(score)]).all()
    assert (z.numpy()[4:6] != 0).any()
    # monotone inside a row: a list keeps its order
    order = np.argsort(-score[21])
    assert np.isfinite(score[21]).all() and (np.diff(z.numpy()[21][order]) <= 0).all()
    # the refusals
    t = torch.from_numpy
    with pytest.raises(ValueError, match="float32"):
        ops.standardise_scores(t(score).double(), t(mean), t(std), t(count))
    with pytest.raises(ValueError, match="tensors"):
        ops.standardise_scores(score, t(mean), t(std), t(count))
