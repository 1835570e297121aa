"""The host side of the long and diversified lists over the bf16 catalogue (pc_retrieve_list_grouped_bf16,
pc_diversify_lists_bf16, pc_inv_norm_bf16; ops.retrieve_list_grouped on a bf16 table, ops.diversify_lists_bf16,
ops.inv_norm_bf16, ops.CompactCatalogue; PCompanionInference(catalogue=ops.CompactCatalogue(...))), without a GPU: the header
and the ctypes table, the workspace query, what the entries refuse before anything is launched, the call that
ops.retrieve_list_grouped records for a bf16 table (the recorder of tests/test_grouped_wrappers_host.py), and every refusal
of the wrappers, the class and the constructor before the library, the model or the graph is read."""
import ctypes
import inspect
import os
import re
from types import SimpleNamespace

import pytest
import torch

from conftest import ROOT
from test_grouped_wrappers_host import (ARGS, D, FILTERED, KEYS, NO_TRIPLE, OnDevice, P, QUERY, R, T, TAG, dev, rec, recorded,
                                        tensors, triple)

PC_EINVAL, PC_ESHAPE, PC_EWORKSPACE = -1, -2, -3
LIST = "pc_retrieve_list_grouped_bf16"
ENTRIES = (LIST, LIST + "_workspace_bytes", "pc_diversify_lists_bf16", "pc_inv_norm_bf16")


def _prototype(name):
    txt = open(os.path.join(ROOT, "include", "pcompanion_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\b(?:int|size_t)\s+%s\s*\(([^)]*)\)\s*;" % name, code)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def test_header_prototypes_match_the_ctypes_table_and_the_abi_stays_8():
    from p_companion_amd import _lib
    kinds = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "float": ctypes.c_float}
    for name in ENTRIES:
        declared = [ctypes.c_void_p if "*" in a else kinds[a.split()[0]] for a in _prototype(name)]
        assert _lib.SIGNATURES[name][1] == declared, name
    sig = _lib.SIGNATURES
    assert sig[LIST] == sig["pc_retrieve_list_grouped"] and sig[LIST + "_workspace_bytes"] == sig["pc_retrieve_list_grouped_workspace_bytes"]
    assert sig["pc_diversify_lists_bf16"] == sig["pc_diversify_lists"] and sig["pc_inv_norm_bf16"] == sig["pc_inv_norm"]
    for name in (LIST, "pc_diversify_lists_bf16", "pc_inv_norm_bf16"):
        assert any(re.fullmatch(r"const\s+uint16_t\s*\*\s*table_bf16", a) for a in _prototype(name)), name
    txt = open(os.path.join(ROOT, "include", "pcompanion_hip.h")).read()
    assert re.search(r"#define\s+PC_ABI_VERSION\s+8\b", txt)
    L = _lib.lib()
    assert L.pc_abi_version() == 8
    assert L.pc_retrieve_list_grouped_bf16_workspace_bytes.restype == ctypes.c_size_t


def test_the_list_entrys_argument_order_is_the_fp32_list_entrys():
    names = lambda entry: [{"table_bf16": "table"}.get(n, n) for n in (re.sub(r"\W", "", a.split()[-1]) for a in _prototype(entry))]
    assert names(LIST) == names("pc_retrieve_list_grouped") == FILTERED.split()
    assert names(LIST + "_workspace_bytes") == "rows n_types n slices".split()
    strip = lambda entry: [re.sub(r"\btable_bf16\b", "table", re.sub(r"uint16_t", "float", a)) for a in _prototype(entry)]
    assert strip("pc_diversify_lists_bf16") == strip("pc_diversify_lists") and strip("pc_inv_norm_bf16") == strip("pc_inv_norm")


def test_the_unit_is_part_of_the_build():
    from p_companion_amd import build
    assert "retrieve_list_bf16.hip" in build.sources()


def test_the_workspace_query_is_the_fp32_list_entrys():
    from p_companion_amd import _lib
    L = _lib.lib()
    ws, ws32 = L.pc_retrieve_list_grouped_bf16_workspace_bytes, L.pc_retrieve_list_grouped_workspace_bytes
    for rows in (1, 17, 12288):
        for types in (1, 100, 34_800):
            for n in (1, 16, 17, 100, 256):
                for s in (0, 1, 7, 64):
                    assert ws(rows, types, n, s) == ws32(rows, types, n, s) > 0, (rows, types, n, s)
    rows, types = 12288, 100
    for bad in ((0, types, 10, 0), (rows, 0, 10, 0), (rows, types, 0, 0), (rows, types, 257, 0), (rows, types, 10, -1),
                (rows, types, 10, 65)):
        assert ws(*bad) == 0, bad


def _aligned():
    buf = ctypes.create_string_buffer(4096 + 16)
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)


def test_the_list_entry_refuses_before_anything_is_launched():
    """(the pointers are one aligned host buffer, which no check dereferences)"""
    from p_companion_amd import _lib
    entry = _lib.lib().pc_retrieve_list_grouped_bf16
    buf, p = _aligned()

    def call(**kw):
        a = dict(proj=p, types=p, row_key=p, rows=4, type_rowptr=p, type_col=p, table=p, n_types=3, ex_rowptr=p, ex_col=p, n_keys=2,
                 n=100, dim=128, slices=0, out_idx=p, out_score=p, bad_count=p, ws=p, ws_bytes=0, stream=None)
        a.update(kw)
        return entry(*a.values())

    for name in ("proj", "types", "type_rowptr", "type_col", "table", "out_idx", "out_score", "ws", "ex_rowptr", "ex_col",
                 "bad_count"):
        assert call(**{name: None}) == PC_EINVAL, name
    assert call(rows=0) == PC_EINVAL and call(n_types=0) == PC_EINVAL and call(n_keys=-1) == PC_EINVAL
    assert call(row_key=None) == PC_EINVAL and call(row_key=None, ex_rowptr=None, ex_col=None) == PC_EINVAL
    none = dict(row_key=None, ex_rowptr=None, ex_col=None, n_keys=0, bad_count=None)
    for kw in (dict(n=0), dict(n=257), dict(dim=64), dict(dim=192), dict(slices=-1), dict(slices=65)):
        assert call(**kw) == PC_ESHAPE, kw
        assert call(**kw, **none) == PC_ESHAPE, kw
    for off in (2, 4, 8):                                                          # a table that is not 16-byte aligned
        assert call(table=ctypes.c_void_p(p.value + off)) == PC_ESHAPE, off
        assert call(table=ctypes.c_void_p(p.value + off), **none) == PC_ESHAPE, off
    for n in (1, 16, 17, 256):
        assert call(n=n) == PC_EWORKSPACE and call(n=n, dim=256, **none) == PC_EWORKSPACE


def test_the_diversify_entries_refuse_before_anything_is_launched():
    from p_companion_amd import _lib
    L = _lib.lib()
    buf, p = _aligned()

    def call(**kw):
        a = dict(idx=p, score=p, rows=3, m=20, table=p, scale=None, num_products=7, dim=128, n=5, lam=0.5, out_idx=p,
                 out_score=p, bad=None, stream=None)
        a.update(kw)
        return L.pc_diversify_lists_bf16(*a.values())

    odd = [ctypes.c_void_p(p.value + off) for off in (2, 4, 8)]
    for kw in (dict(m=0), dict(m=-1), dict(m=257), dict(n=0), dict(n=21), dict(m=256, n=257), dict(dim=0), dict(dim=64),
               dict(dim=192), dict(dim=512), dict(lam=-1e-6), dict(lam=1.0 + 1e-6), dict(lam=float("nan")), dict(lam=float("inf")),
               dict(rows=-1), dict(num_products=0), dict(idx=None), dict(score=None), dict(table=None), dict(out_idx=None),
               dict(out_score=None)) + tuple(dict(table=o) for o in odd):
        assert call(**kw) == PC_ESHAPE, kw
    assert call(rows=0) == 0 and call(rows=0, idx=None, score=None, table=None, out_idx=None, out_score=None) == 0
    assert call(rows=0, m=257) == PC_ESHAPE and call(rows=0, lam=2.0) == PC_ESHAPE
    entry = L.pc_inv_norm_bf16
    assert entry(None, 4, 128, p, None) == PC_EINVAL and entry(p, 4, 128, None, None) == PC_EINVAL
    assert entry(p, 0, 128, p, None) == PC_EINVAL and entry(p, -3, 256, p, None) == PC_EINVAL
    for dim in (0, 64, 192, 512):
        assert entry(p, 4, dim, p, None) == PC_ESHAPE, dim
    for o in odd:
        assert entry(o, 4, 128, p, None) == PC_ESHAPE


# ---- the call ops.retrieve_list_grouped records for a bf16 table
@pytest.mark.parametrize("exclude,bad", [(False, False), (True, False), (True, True)])
def test_retrieve_list_grouped_reaches_the_bf16_entry_with_the_headers_arguments(rec, monkeypatch, exclude, bad):
    from p_companion_amd import ops
    monkeypatch.setitem(ARGS, LIST, FILTERED)
    monkeypatch.setitem(ARGS, LIST + "_workspace_bytes", "rows n_types n slices")
    monkeypatch.setitem(QUERY, LIST, LIST + "_workspace_bytes")                   # its own query
    monkeypatch.setitem(TAG, LIST, "retrieve_list")
    for n, d, slices in ((1, D, 0), (16, D, 0), (17, D, 7), (256, 256, 0)):
        ts = tensors(d=d, bf16=True)
        rec.calls.clear(), rec.workspaces.clear()
        idx, sc = ops.retrieve_list_grouped(ts["proj"], ts["types"], ts["type_rowptr"], ts["type_col"], ts["table"], n, slices,
                                            exclude=triple(ts) if exclude else None, bad=ts["bad_count"] if bad else None)
        assert tuple(idx.shape) == (R, n) and idx.dtype == torch.int32
        assert tuple(sc.shape) == (R, n) and sc.dtype == torch.float32
        scalars = dict(rows=R, n_types=T, n=n, dim=d, slices=slices, n_keys=KEYS if exclude else 0)
        recorded(rec, ts, LIST, dict(out_idx=idx, out_score=sc), scalars, null=() if exclude else NO_TRIPLE,
                 fresh=("bad_count",) if exclude and not bad else ())
    # an fp32 table beside it: the fp32 entry, as before
    ts = tensors()
    rec.calls.clear(), rec.workspaces.clear()
    ops.retrieve_list_grouped(ts["proj"], ts["types"], ts["type_rowptr"], ts["type_col"], ts["table"], 100)
    assert [name for name, _ in rec.calls] == ["pc_retrieve_list_grouped_workspace_bytes", "pc_retrieve_list_grouped"]


def test_retrieve_list_grouped_refusals_with_a_bf16_table_reach_nothing(rec):
    from p_companion_amd import ops
    ts = tensors(bf16=True)
    lst = lambda n=100, table=ts["table"], **kw: ops.retrieve_list_grouped(ts["proj"], ts["types"], ts["type_rowptr"], ts["type_col"],
                                                                           table, n, **kw)
    for kw, message in ((dict(n=0), "retrieve_list_grouped: n must be in [1, 256], got 0"),
                        (dict(n=257), "retrieve_list_grouped: n must be in [1, 256], got 257"),
                        (dict(bad=ts["bad_count"]), "retrieve_list_grouped: bad counts keys out of range and is read with an exclude triple only"),
                        (dict(slices=65), "slices must be in [0, 64] (0 = automatic), got 65")):
        with pytest.raises(ValueError) as e:
            lst(**kw)
        assert str(e.value) == message
    for dtype in (torch.float16, torch.float64):                                  # any other dtype: the fp32 entry's TypeError
        with pytest.raises(TypeError, match="table: expected torch.float32"):
            lst(table=dev(P, D, dtype=dtype))
    with pytest.raises(ValueError, match="width"):
        lst(table=dev(P, 64, dtype=torch.bfloat16))
    assert rec.calls == [] and rec.workspaces == []


# ---- the wrappers, the class and the constructor refuse before anything is read
def _untouched():
    raise AssertionError("the library was touched before the arguments were refused")


def test_diversify_lists_bf16_and_inv_norm_bf16_check_their_arguments_before_the_library_is_touched(monkeypatch):
    from p_companion_amd import _lib, ops
    monkeypatch.setattr(_lib, "lib", _untouched)
    assert list(inspect.signature(ops.diversify_lists_bf16).parameters) == list(inspect.signature(ops.diversify_lists).parameters)
    on = lambda t: t.as_subclass(OnDevice)
    idx, sc, table = torch.zeros(4, 20, dtype=torch.int32), torch.zeros(4, 20), torch.zeros(7, 128, dtype=torch.bfloat16)
    with pytest.raises(TypeError, match="idx: expected a CUDA/ROCm"):
        ops.diversify_lists_bf16(idx, on(sc), on(table), 5, 0.5)
    with pytest.raises(TypeError, match="score: expected a CUDA/ROCm"):
        ops.diversify_lists_bf16(on(idx), sc, on(table), 5, 0.5)
    with pytest.raises(TypeError, match="table: expected a CUDA/ROCm"):
        ops.diversify_lists_bf16(on(idx), on(sc), table, 5, 0.5)
    with pytest.raises(TypeError, match="scale: expected a CUDA/ROCm"):
        ops.diversify_lists_bf16(on(idx), on(sc), on(table), 5, 0.5, scale=torch.zeros(7))
    with pytest.raises(TypeError, match="bad: expected a CUDA/ROCm"):
        ops.diversify_lists_bf16(on(idx), on(sc), on(table), 5, 0.5, bad=torch.zeros(1, dtype=torch.int32))
    call = lambda **kw: ops.diversify_lists_bf16(on(kw.pop("idx", idx)), on(kw.pop("score", sc)), on(kw.pop("table", table)),
                                                 kw.pop("n", 5), kw.pop("lam", 0.5), **kw)
    with pytest.raises(TypeError, match="idx: expected torch.int32"):
        call(idx=idx.long())
    with pytest.raises(TypeError, match="score: expected torch.float32"):
        call(score=sc.double())
    for bad_idx, bad_sc in ((torch.zeros(80, dtype=torch.int32), torch.zeros(80)), (idx, torch.zeros(4, 21))):
        with pytest.raises(ValueError, match=r"diversify_lists_bf16: expected idx and score of one shape \[R, m\]"):
            call(idx=bad_idx, score=bad_sc)
    for m in (0, 257):
        with pytest.raises(ValueError, match=r"pool m must be in \[1, 256\], got %d" % m):
            call(idx=torch.zeros(2, m, dtype=torch.int32), score=torch.zeros(2, m))
    for n in (0, -1, 21, 256):
        with pytest.raises(ValueError, match=r"n must be in \[1, m = 20\], got %d" % n):
            call(n=n)
    for lam in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"lam must be in \[0, 1\]"):
            call(lam=lam)
    for dtype in (torch.float32, torch.float16):                                  # the fp32 table belongs to diversify_lists
        with pytest.raises(TypeError, match="table: expected torch.bfloat16"):
            call(table=torch.zeros(7, 128, dtype=dtype))
    with pytest.raises(ValueError, match=r"\[P, D\]"):
        call(table=torch.zeros(7 * 128, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="width"):
        call(table=torch.zeros(7, 64, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="at least one row"):
        call(table=torch.zeros(0, 128, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="scale must be"):
        call(scale=[1.0] * 7)
    with pytest.raises(TypeError, match="scale: expected torch.float32"):
        call(scale=on(torch.zeros(7, dtype=torch.bfloat16)))
    for shape in ((6,), (8,), (7, 1)):
        with pytest.raises(ValueError, match=r"scale: expected shape \(7,\)"):
            call(scale=on(torch.zeros(shape)))
    with pytest.raises(TypeError, match="bad: expected torch.int32"):
        call(bad=on(torch.zeros(1)))
    with pytest.raises(ValueError, match=r"bad: expected shape \(1,\)"):
        call(bad=on(torch.zeros(2, dtype=torch.int32)))
    # ... and diversify_lists keeps refusing the bf16 table
    with pytest.raises(TypeError, match="table: expected torch.float32"):
        ops.diversify_lists(on(idx), on(sc), on(table), 5, 0.5)
    # inv_norm_bf16: inv_norm's checks
    with pytest.raises(TypeError, match="CUDA/ROCm"):
        ops.inv_norm_bf16(table)
    with pytest.raises(TypeError, match="table: expected torch.bfloat16"):
        ops.inv_norm_bf16(on(torch.zeros(5, 128)))
    with pytest.raises(ValueError, match=r"\[P, D\]"):
        ops.inv_norm_bf16(on(torch.zeros(128, dtype=torch.bfloat16)))
    with pytest.raises(ValueError, match="width"):
        ops.inv_norm_bf16(on(torch.zeros(5, 64, dtype=torch.bfloat16)))
    with pytest.raises(ValueError, match="at least one row"):
        ops.inv_norm_bf16(on(torch.zeros(0, 128, dtype=torch.bfloat16)))
    with pytest.raises(TypeError, match="table: expected torch.float32"):
        ops.inv_norm(on(table))


def test_compact_catalogue_checks_its_table_before_the_library_is_touched(monkeypatch):
    from p_companion_amd import _lib, ops
    monkeypatch.setattr(_lib, "lib", _untouched)
    on = lambda t: t.as_subclass(OnDevice)
    for bad, what in ((None, "float32 or bfloat16"), ([[0.0] * 128], "float32 or bfloat16"), (torch.bfloat16, "float32 or bfloat16"),
                      (on(torch.zeros(7, 128, dtype=torch.float16)), "float32 or bfloat16"),
                      (on(torch.zeros(7, 128, dtype=torch.float64)), "float32 or bfloat16"),
                      (on(torch.zeros(7 * 128)), r"\[P >= 1, 128 or 256\]"), (on(torch.zeros(7, 64)), r"\[P >= 1, 128 or 256\]"),
                      (on(torch.zeros(0, 128, dtype=torch.bfloat16)), r"\[P >= 1, 128 or 256\]"),
                      (torch.zeros(7, 128, dtype=torch.bfloat16), "contiguous device tensor"),
                      (on(torch.zeros(7, 256, dtype=torch.bfloat16))[:, :128], "contiguous device tensor")):
        with pytest.raises(ValueError, match=what):
            ops.CompactCatalogue(bad)
    # a bf16 table is taken as it is, an fp32 table is rounded once (to nearest even); neither touches the library
    t16 = on(torch.zeros(7, 128, dtype=torch.bfloat16))
    assert ops.CompactCatalogue(t16).table is t16
    t32 = on(torch.tensor([[1.0 + 2.0 ** -8 + 2.0 ** -20] * 256, [1.0 + 2.0 ** -8] * 256]))
    cc = ops.CompactCatalogue(t32)
    assert cc.table.dtype == torch.bfloat16 and tuple(cc.table.shape) == (2, 256) and cc.table.is_contiguous()
    assert cc.table[0, 0].item() == 1.0 + 2.0 ** -7 and cc.table[1, 0].item() == 1.0
    with pytest.raises(AssertionError, match="the library was touched"):          # .inv_norm is formed on first use, not before
        cc.inv_norm


class Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"read .{name} before refusing")


def test_inference_checks_a_compact_catalogue_before_the_model_or_the_graph_is_touched():
    from p_companion_amd import ops
    from p_companion_amd.inference import PCompanionInference
    cfg = SimpleNamespace(DEVICE="cuda")
    bpg = SimpleNamespace(num_products=7)                             # (no arrays, no cuda(): reading them is an error)
    on = lambda t: t.as_subclass(OnDevice)
    for table, what in ((on(torch.zeros(6, 128, dtype=torch.bfloat16)), r"\[7, 128 or 256\]"),
                        (on(torch.zeros(8, 256)), r"\[7, 128 or 256\]")):
        with pytest.raises(ValueError, match=what):
            PCompanionInference(Untouchable(), cfg, bpg, catalogue=ops.CompactCatalogue(table))
    cc = ops.CompactCatalogue(on(torch.zeros(7, 128, dtype=torch.bfloat16)))
    cc.table = torch.zeros(7, 128, dtype=torch.bfloat16)              # (moved off the device behind the class's back)
    with pytest.raises(ValueError, match="device tensor"):
        PCompanionInference(Untouchable(), cfg, bpg, catalogue=cc)
    # the signatures stay
    assert list(inspect.signature(PCompanionInference.__init__).parameters) == ["self", "model", "config", "bpg", "product_ids",
                                                                               "catalogue"]
    assert list(inspect.signature(PCompanionInference.recommend_batch).parameters) == ["self", "query_idx", "num_recommendations"]
    assert list(inspect.signature(PCompanionInference.recommend_diverse_batch).parameters) == [
        "self", "query_idx", "num_recommendations", "pool", "diversity", "similarity"]
    assert list(inspect.signature(PCompanionInference.recommend).parameters) == ["self", "query_id", "num_recommendations"]


def test_a_compact_object_refuses_before_the_model_runs_and_a_bare_tensor_refuses_what_it_refused():
    from p_companion_amd.inference import PCompanionInference
    assert PCompanionInference.compact is None                         # objects built without the attribute take today's branches
    q = torch.zeros(2, dtype=torch.int32)
    inf = object.__new__(PCompanionInference)                          # (no graph, no model, no device)
    inf.__dict__.update(model=Untouchable(), bpg=Untouchable(), features=None, _graph=Untouchable(), exclusions=Untouchable(),
                        catalogue=torch.zeros(3, 128, dtype=torch.bfloat16), compact=Untouchable())
    with pytest.raises(ValueError, match="at most 256"):
        inf.recommend_batch(q, 257)
    for n, pool in ((0, 64), (65, 64), (10, 257), (10, 0)):
        with pytest.raises(ValueError, match="num_recommendations <= pool <= 256"):
            inf.recommend_diverse_batch(q, n, pool=pool)
    with pytest.raises(ValueError, match=r"diversity must be in \[0, 1\]"):
        inf.recommend_diverse_batch(q, 10, pool=200, diversity=1.5)
    with pytest.raises(ValueError, match="'cosine' or 'dot'"):
        inf.recommend_diverse_batch(q, 10, pool=200, similarity="l2")
    with pytest.raises(ValueError, match="fp32 catalogue"):
        inf.rank_targets(q, q)
    with pytest.raises(ValueError, match="fp32 catalogue"):
        inf.evaluate_catalogue(Untouchable())
    # a long list gets past the length check and goes on to the device (which this object does not have)
    with pytest.raises(AttributeError, match="device"):
        inf.recommend_batch(q, 100)
    # the bare tensor: no `compact` in the object -- the two pinned refusals
    bare = object.__new__(PCompanionInference)
    bare.__dict__.update(model=Untouchable(), bpg=Untouchable(), features=None, _graph={},
                         catalogue=torch.zeros(3, 128, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="bf16 catalogue serves at most 16"):
        bare.recommend_batch(q, 17)
    with pytest.raises(ValueError, match="without them"):
        bare.recommend_diverse_batch(q, 10, pool=16)
