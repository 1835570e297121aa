"""The host side of the per-query attribute filters (pc_retrieve_list_grouped_where and its bf16 / biased twins; ops.RowWhere,
ops.retrieve_list_grouped_where; recommend_where_batch / similar_where_batch), without a GPU: the header and the ctypes table,
the workspace query, what the entries refuse before anything is launched, the checks of the holder, and which entry the wrapper
reaches per table dtype and bias -- recorded, not made, as tests/test_grouped_wrappers_host.py records them."""
import ctypes
import inspect
import itertools
import os
import re

import pytest
import torch

from conftest import ROOT
from test_grouped_wrappers_host import KEYS, OnDevice, P, R, STREAM, T, WS, WS_BYTES, D, dev, rec, tensors, triple      # noqa: F401

PC_EINVAL, PC_ESHAPE, PC_EWORKSPACE = -1, -2, -3
TWINS = {"pc_retrieve_list_grouped_where": "pc_retrieve_list_grouped",
         "pc_retrieve_list_grouped_bf16_where": "pc_retrieve_list_grouped_bf16",
         "pc_retrieve_list_grouped_biased_where": "pc_retrieve_list_grouped_biased",
         "pc_retrieve_list_grouped_bf16_biased_where": "pc_retrieve_list_grouped_bf16_biased"}
FIELDS = ["value", "lo", "hi", "flags", "need", "deny"]


def test_header_declares_the_entries_and_the_abi_stays_8():
    from p_companion_amd import _lib
    txt = open(os.path.join(ROOT, "include", "pcompanion_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    arg_names = lambda name: [a.split("*")[-1].split()[-1] for a in
                              re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, code).group(1).split(",")]
    sig = _lib.SIGNATURES
    for name, twin in TWINS.items():
        assert name in sig and name + "_workspace_bytes" in sig
        got, plain = arg_names(name), arg_names(twin)
        assert got == plain[:-3] + ["where"] + plain[-3:] and plain[-3:] == ["ws", "ws_bytes", "stream"]      # in front of ws
        ret, args = sig[twin]
        assert sig[name] == (ret, args[:-3] + [ctypes.POINTER(_lib.RowWhere)] + args[-3:])
        assert sig[name + "_workspace_bytes"] == sig[twin + "_workspace_bytes"]
    # the struct: six pointers in the header's order
    body = re.search(r"typedef\s+struct\s+pc_row_where\s*\{(.*?)\}\s*pc_row_where\s*;", code, flags=re.S).group(1)
    assert re.findall(r"\*\s*(\w+)", body) == FIELDS
    assert [f for f, _ in _lib.RowWhere._fields_] == FIELDS and ctypes.sizeof(_lib.RowWhere) == 6 * ctypes.sizeof(ctypes.c_void_p)
    assert re.search(r"#define\s+PC_ABI_VERSION\s+8\b", txt)
    assert _lib.lib().pc_abi_version() == 8


def test_the_units_are_part_of_the_build():
    from p_companion_amd import build
    assert {"where_list.hip", "where_list_bf16.hip"} <= set(build.sources())


def test_the_workspace_is_the_list_entrys():
    from p_companion_amd import _lib
    L = _lib.lib()
    plain = L.pc_retrieve_list_grouped_workspace_bytes
    for name in TWINS:
        ws = getattr(L, name + "_workspace_bytes")
        assert ws.restype == ctypes.c_size_t
        for rows, types, n, s in itertools.product((1, 17, 12288), (1, 100), (1, 16, 17, 32, 33, 96, 97, 256), (0, 7, 64)):
            assert ws(rows, types, n, s) == plain(rows, types, n, s) > 0, (name, rows, types, n, s)
        for bad in ((0, 100, 10, 0), (5, 0, 10, 0), (5, 100, 0, 0), (5, 100, 257, 0), (5, 100, 10, -1), (5, 100, 10, 65)):
            assert ws(*bad) == 0, (name, bad)


def _aligned():
    """One 16-byte aligned host buffer: a pointer that passes every check, and that no check dereferences."""
    buf = ctypes.create_string_buffer(96)
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)


@pytest.mark.parametrize("name", list(TWINS))
def test_the_entries_refuse_before_anything_is_launched(name):
    from p_companion_amd import _lib
    entry = getattr(_lib.lib(), name)
    buf, p = _aligned()
    biased = "biased" in name

    def call(where="all", **kw):
        a = dict(proj=p, types=p, row_key=p, rows=4, type_rowptr=p, type_col=p, table=p)
        if biased:
            a["bias"] = p
        a.update(n_types=3, ex_rowptr=p, ex_col=p, n_keys=2, n=100, dim=128, slices=0, out_idx=p, out_score=p, bad_count=p,
                 where=None, ws=p, ws_bytes=0, stream=None)
        a.update(kw)
        if where is not None:
            st = _lib.RowWhere(**{f: p.value for f in (FIELDS if where == "all" else where)})
            a["where"] = ctypes.byref(st)
        return entry(*a.values())

    none = dict(row_key=None, ex_rowptr=None, ex_col=None, n_keys=0, bad_count=None)
    # a filter that is in order reaches the workspace check, with and without lists, whatever parts it holds
    ok = ("all", (), ("value", "lo", "hi"), ("flags",), ("flags", "need"), ("flags", "deny"), ("flags", "need", "deny"),
          ("value", "lo", "hi", "flags"))
    for where in ok:
        assert call(where) == PC_EWORKSPACE and call(where, **none) == PC_EWORKSPACE, where
    # the pairing rules, and the null filter
    assert call(None) == PC_EINVAL and call(None, **none) == PC_EINVAL
    bad = (("lo",), ("hi",), ("lo", "hi"), ("value",), ("value", "lo"), ("value", "hi"), ("need",), ("deny",), ("need", "deny"),
           ("value", "lo", "hi", "need"), ("flags", "need", "lo"), ("flags", "value"), ("lo", "hi", "flags", "need", "deny"))
    for where in bad:
        assert call(where) == PC_EINVAL and call(where, **none) == PC_EINVAL, where
    # everything else as the twin refuses it
    for arg in ("proj", "types", "type_rowptr", "type_col", "table", "out_idx", "out_score", "ws", "ex_rowptr", "ex_col",
                "bad_count") + (("bias",) if biased else ()):
        assert call(**{arg: None}) == PC_EINVAL, arg
    assert call(rows=0) == PC_EINVAL and call(n_types=0) == PC_EINVAL and call(n_keys=-1) == PC_EINVAL
    assert call(row_key=None) == PC_EINVAL and call(row_key=None, ex_col=None, n_keys=0) == PC_EINVAL
    for kw in (dict(n=0), dict(n=257), dict(n=-1), dict(dim=64), dict(dim=192), dict(slices=-1), dict(slices=65)):
        assert call(**kw) == PC_ESHAPE and call(**kw, **none) == PC_ESHAPE, kw
        assert call(("lo",), **kw) == PC_EINVAL and call(None, **kw) == PC_EINVAL, kw      # the pointers, then the shapes
    if "bf16" in name:
        assert call(table=ctypes.c_void_p(p.value + 8)) == PC_ESHAPE                       # the bf16 table's alignment
    for n in (1, 16, 17, 32, 33, 96, 97, 256):                                             # every buffer size, both widths
        assert call(n=n) == PC_EWORKSPACE and call(n=n, dim=256, **none) == PC_EWORKSPACE


def test_row_where_checks_its_parts_on_the_host_side():
    from p_companion_amd import ops
    sig = inspect.signature(ops.RowWhere)
    assert list(sig.parameters) == ["value", "flags", "lo", "hi", "need", "deny"]
    assert all(p.default is None for p in sig.parameters.values())
    f32, i32 = (lambda n: torch.zeros(n)), (lambda n: torch.zeros(n, dtype=torch.int32))
    # in order: nothing, a band, masks (one or both), everything -- host tensors too: the device is the call's business
    w = ops.RowWhere()
    assert all(getattr(w, f) is None for f in FIELDS)
    full = dict(value=f32(P), flags=i32(P), lo=f32(R), hi=f32(R), need=i32(R), deny=i32(R))
    w = ops.RowWhere(**full)
    assert all(getattr(w, f) is full[f] for f in FIELDS)
    for keep in (("value", "lo", "hi"), ("flags",), ("flags", "need"), ("flags", "deny"), ("flags", "need", "deny")):
        ops.RowWhere(**{k: full[k] for k in keep})
    # dtypes, shapes, kinds
    for name in FIELDS:
        wrong = torch.int32 if full[name].dtype == torch.float32 else torch.float32
        for other in (wrong, torch.float64, torch.int64, torch.bfloat16, torch.bool):
            with pytest.raises(ValueError, match=f"{name} of dtype"):
                ops.RowWhere(**{**full, name: full[name].to(other)})
        for shape in ((), (3, 1), (1, 3)):
            with pytest.raises(ValueError, match=f"{name} must be 1-D"):
                ops.RowWhere(**{**full, name: torch.zeros(shape, dtype=full[name].dtype)})
        for no_tensor in ([0] * 3, 1.0, "x"):
            with pytest.raises(ValueError, match=f"{name} must be None or"):
                ops.RowWhere(**{**full, name: no_tensor})
    with pytest.raises(ValueError, match="one device"):
        ops.RowWhere(**{**full, "lo": torch.zeros(R, device="meta")})
    # the pairing rule
    for keep in (("lo",), ("hi",), ("lo", "hi"), ("flags", "lo", "hi")):
        with pytest.raises(ValueError, match="lo / hi bound"):
            ops.RowWhere(**{k: full[k] for k in keep})
    for keep in (("value",), ("value", "lo"), ("value", "hi"), ("value", "flags", "need")):
        with pytest.raises(ValueError, match="value needs both lo and hi"):
            ops.RowWhere(**{k: full[k] for k in keep})
    for keep in (("need",), ("deny",), ("need", "deny"), ("value", "lo", "hi", "need")):
        with pytest.raises(ValueError, match="need / deny test"):
            ops.RowWhere(**{k: full[k] for k in keep})


def where_tensors(keep=FIELDS, p=P, r=R):
    sizes = dict(value=p, flags=p, lo=r, hi=r, need=r, deny=r)
    return {f: dev(sizes[f], dtype=torch.float32 if f in ("value", "lo", "hi") else torch.int32) + i
            for i, f in enumerate(FIELDS) if f in keep}


ENTRY = {("fp32", False): "pc_retrieve_list_grouped_where", ("bf16", False): "pc_retrieve_list_grouped_bf16_where",
         ("fp32", True): "pc_retrieve_list_grouped_biased_where", ("bf16", True): "pc_retrieve_list_grouped_bf16_biased_where"}


@pytest.mark.parametrize("table,bias,exclude", itertools.product(("fp32", "bf16"), (False, True), (False, True)))
def test_the_wrapper_reaches_the_entry_of_the_tables_dtype_and_the_bias(rec, table, bias, exclude):
    from p_companion_amd import _lib, ops
    sig = inspect.signature(ops.retrieve_list_grouped_where)
    assert list(sig.parameters) == ["proj", "types", "type_rowptr", "type_col", "table", "n", "where", "slices", "exclude", "bad",
                                    "bias"]
    assert [sig.parameters[k].default for k in ("slices", "exclude", "bad", "bias")] == [0, None, None, None]
    entry = ENTRY[table, bias]
    for n, keep in ((1, FIELDS), (17, ("value", "lo", "hi")), (256, ("flags", "deny")), (40, ())):
        ts, ws = tensors(bf16=table == "bf16"), where_tensors(keep)
        rec.calls.clear(), rec.workspaces.clear()
        idx, sc = ops.retrieve_list_grouped_where(ts["proj"], ts["types"], ts["type_rowptr"], ts["type_col"], ts["table"], n,
                                                  ops.RowWhere(**ws), slices=7, exclude=triple(ts) if exclude else None,
                                                  bias=ts["bias"] if bias else None)
        assert tuple(idx.shape) == tuple(sc.shape) == (R, n) and idx.dtype == torch.int32 and sc.dtype == torch.float32
        assert [name for name, _ in rec.calls] == [entry + "_workspace_bytes", entry]
        assert list(rec.calls[0][1]) == [R, T, n, 7] and rec.workspaces == [(WS_BYTES, "retrieve_list")]
        args = list(rec.calls[1][1])
        ptr = lambda a: a.value if isinstance(a, ctypes.c_void_p) else a
        assert len(args) == len(_lib.SIGNATURES[entry][1])
        # the tail: where, ws, ws_bytes, stream; the head: the twin's list
        assert [ptr(a) for a in args[-3:]] == [WS.data_ptr(), WS.numel(), STREAM.value]
        head = [ptr(a) for a in args[:-4]]
        at = 7 + bias
        assert head[:7] == [ts["proj"].data_ptr(), ts["types"].data_ptr(), ts["row_key"].data_ptr() if exclude else None, R,
                            ts["type_rowptr"].data_ptr(), ts["type_col"].data_ptr(), ts["table"].data_ptr()]
        assert not bias or head[7] == ts["bias"].data_ptr()
        assert head[at] == T and head[at + 3:at + 7] == [KEYS if exclude else 0, n, D, 7]
        assert head[at + 7:at + 9] == [idx.data_ptr(), sc.data_ptr()]
        st = args[-4]._obj
        assert isinstance(st, _lib.RowWhere)
        assert {f: getattr(st, f) for f in FIELDS} == {f: ws[f].data_ptr() if f in ws else None for f in FIELDS}


def test_the_wrapper_refuses_before_anything_is_reached(rec):
    from p_companion_amd import ops
    ts = tensors()
    base = (ts["proj"], ts["types"], ts["type_rowptr"], ts["type_col"])
    where = ops.RowWhere(**where_tensors())
    for n in (0, 257, -1):
        with pytest.raises(ValueError, match=r"n must be in \[1, 256\]"):
            ops.retrieve_list_grouped_where(*base, ts["table"], n, where)
    for no_holder in (None, {}, where_tensors()):
        with pytest.raises(ValueError, match="where must be an ops.RowWhere"):
            ops.retrieve_list_grouped_where(*base, ts["table"], 10, no_holder)
    # the lengths against P and R, at the call
    for f in FIELDS:
        short = where_tensors()
        short[f] = short[f][:-1].contiguous().as_subclass(OnDevice)
        with pytest.raises(ValueError, match=rf"where\.{f} must hold one entry per (product|row)"):
            ops.retrieve_list_grouped_where(*base, ts["table"], 10, ops.RowWhere(**short))
    # a host tensor in the holder: the device check of the call
    cpu = where_tensors()
    cpu["lo"] = torch.zeros(R)
    with pytest.raises(TypeError, match="CUDA/ROCm"):
        ops.retrieve_list_grouped_where(*base, ts["table"], 10, ops.RowWhere(**cpu))
    # the bias checks are the existing biased functions', per dtype
    with pytest.raises(ValueError, match="float32"):
        ops.retrieve_list_grouped_where(*base, ts["table"], 10, where, bias=ts["bias"].double())
    with pytest.raises(ValueError, match="one entry per product"):
        ops.retrieve_list_grouped_where(*base, ts["table"], 10, where, bias=dev(P + 1))
    bf = tensors(bf16=True)
    with pytest.raises(ValueError, match="one entry per product"):
        ops.retrieve_list_grouped_where(*base, bf["table"], 10, where, bias=dev(P - 1))
    with pytest.raises(ValueError, match="bias must be"):
        ops.retrieve_list_grouped_where(*base, bf["table"], 10, where, bias=[0.0] * P)
    with pytest.raises(ValueError, match="bad counts keys"):
        ops.retrieve_list_grouped_where(*base, ts["table"], 10, where, bad=ts["bad_count"])
    with pytest.raises(ValueError, match="exclude"):
        ops.retrieve_list_grouped_where(*base, ts["table"], 10, where, exclude=(ts["row_key"].long(), ts["ex_rowptr"], ts["ex_col"]))
    assert rec.calls == []


class Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"read .{name} before refusing")


def test_the_methods_refuse_before_the_model_runs():
    from p_companion_amd.inference import (CompactSimilarProducts, IndexedSimilarProducts, PCompanionInference,
                                           SimilarProducts)
    sig = inspect.signature(PCompanionInference.recommend_where_batch)
    assert list(sig.parameters) == ["self", "query_idx", "num_recommendations", "lo", "hi", "need", "deny"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [10, None, None, None, None]
    sig = inspect.signature(SimilarProducts.similar_where_batch)
    assert list(sig.parameters) == ["self", "query_idx", "n", "lo", "hi", "need", "deny"]
    assert CompactSimilarProducts.similar_where_batch is SimilarProducts.similar_where_batch
    q = torch.zeros(2, dtype=torch.int32)
    f32, i32 = torch.zeros(2), torch.zeros(2, dtype=torch.int32)
    value, flags = torch.arange(9.0), torch.arange(9, dtype=torch.int32)
    inf = object.__new__(PCompanionInference)
    inf.__dict__.update(model=Untouchable(), features=Untouchable(), bpg=Untouchable(), exclusions=Untouchable(),
                        type_idx=torch.zeros(9, dtype=torch.int32), device="cpu")
    sp = object.__new__(SimilarProducts)
    sp.__dict__.update(table=Untouchable(), bpg=Untouchable(), exclusions=Untouchable(), bias=Untouchable(),
                       type_idx=torch.zeros(9, dtype=torch.int32), device="cpu")
    for obj, call in ((inf, inf.recommend_where_batch), (sp, sp.similar_where_batch)):
        with pytest.raises(ValueError, match="no per-product attributes are installed"):
            call(q, 10, lo=f32, hi=f32)
        assert obj.set_attributes(value=value, flags=flags) is obj and obj.attributes[0] is not None
        with pytest.raises(ValueError, match="at least one of lo, hi, need, deny"):
            call(q, 10)
        for kw in (dict(lo=f32.double()), dict(hi=torch.zeros(3)), dict(need=f32), dict(deny=torch.zeros(2, 1, dtype=torch.int32)),
                   dict(lo=1.0)):
            with pytest.raises(ValueError, match="one entry per query"):
                call(q, 10, **kw)
        obj.set_attributes(flags=flags)
        with pytest.raises(ValueError, match="lo / hi bound the per-product value"):
            call(q, 10, lo=f32)
        with pytest.raises(ValueError, match="band_around: no per-product value"):
            obj.band_around(q)
        obj.set_attributes(value=value)
        with pytest.raises(ValueError, match="need / deny test the per-product flags"):
            call(q, 10, deny=i32)
        lo, hi = obj.band_around(torch.tensor([2, 8]), 0.5, 2.0)
        assert lo.tolist() == [1.0, 4.0] and hi.tolist() == [4.0, 16.0] and lo.dtype == hi.dtype == torch.float32
        for bad in (dict(value=value.double()), dict(value=value[:8]), dict(flags=flags.long()), dict(flags=[0] * 9)):
            with pytest.raises(ValueError, match="set_attributes"):
                obj.set_attributes(**bad)
        assert obj.set_attributes().attributes is None
    for n in (0, 257):
        with pytest.raises(ValueError, match="1 to 256"):
            sp.similar_where_batch(q, n, lo=f32)
    with pytest.raises(ValueError, match="at most 256"):
        inf.recommend_where_batch(q, 257, lo=f32)
    # a bare bf16 catalogue stops at 16
    inf.__dict__.update(catalogue=torch.zeros(1, dtype=torch.bfloat16), compact=None)
    with pytest.raises(ValueError, match="at most 16"):
        inf.recommend_where_batch(q, 17, lo=f32)
    ix = object.__new__(IndexedSimilarProducts)
    with pytest.raises(NotImplementedError, match="cell index"):
        ix.similar_where_batch(q, 10, lo=f32)
