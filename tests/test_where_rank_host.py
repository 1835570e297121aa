"""The host side of the ranks under a per-query predicate (pc_rank_grouped_where / pc_rank_grouped_bf16_where;
ops.rank_grouped_where; rank_targets_where / evaluate_catalogue_where, rank_pairs_where / evaluate_pairs_where), without a GPU:
the header and the ctypes table, the workspace query, what the entries refuse before anything is launched, which entry the
wrapper reaches per table dtype -- recorded, not made, as tests/test_where_list_host.py records the lists' -- and every ValueError
of the wrapper and of the four methods before anything is computed."""
import ctypes
import inspect
import itertools
import os
import re

import pytest
import torch

from conftest import ROOT
from test_grouped_wrappers_host import KEYS, OnDevice, P, R, STREAM, T, WS, WS_BYTES, D, dev, rec, tensors, triple      # noqa: F401
from test_where_list_host import FIELDS, Untouchable, where_tensors

PC_EINVAL, PC_ESHAPE, PC_EWORKSPACE = -1, -2, -3
ENTRIES = ("pc_rank_grouped_where", "pc_rank_grouped_bf16_where")
TWIN = "pc_rank_grouped_bf16"


def test_header_declares_the_entries_and_the_abi_stays_8():
    from p_companion_amd import _lib
    txt = open(os.path.join(ROOT, "include", "pcompanion_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    arg_names = lambda name: [a.split("*")[-1].split()[-1] for a in
                              re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, code).group(1).split(",")]
    arg_types = lambda name: [" ".join(a.replace("*", " * ").split()[:-1]) for a in
                              re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, code).group(1).split(",")]
    sig = _lib.SIGNATURES
    plain = arg_names(TWIN)
    for name in ENTRIES:
        assert name in sig and name + "_workspace_bytes" in sig
        got = [{"table": "table_bf16"}.get(a, a) for a in arg_names(name)]
        assert got == plain[:-3] + ["where"] + plain[-3:] and plain[-3:] == ["ws", "ws_bytes", "stream"]          # in front of ws
        ret, args = sig[TWIN]
        assert sig[name] == (ret, args[:-3] + [ctypes.POINTER(_lib.RowWhere)] + args[-3:])
        assert sig[name + "_workspace_bytes"] == sig["pc_rank_grouped_workspace_bytes"]
        assert re.search(r"\bsize_t\s+%s_workspace_bytes\s*\(\s*int rows,\s*int n_types,\s*int slices\s*\)\s*;" % name, code)
        assert arg_types(name)[arg_names(name).index("where")] == "const pc_row_where *"
    # the fp32 entry reads a float table, the bf16 entry the 16-bit copy; both take a nullable bias behind it
    assert arg_types(ENTRIES[0])[7:9] == ["const float *", "const float *"] and arg_names(ENTRIES[0])[7:9] == ["table", "bias"]
    assert arg_types(ENTRIES[1])[7:9] == ["const uint16_t *", "const float *"] and arg_names(ENTRIES[1])[7:9] == ["table_bf16", "bias"]
    assert re.search(r"#define\s+PC_ABI_VERSION\s+8\b", txt)
    assert _lib.lib().pc_abi_version() == 8


def test_the_units_are_part_of_the_build():
    from p_companion_amd import build
    assert {"where_rank.hip", "where_rank_bf16.hip"} <= set(build.sources())


def test_the_workspace_is_the_rank_entrys():
    from p_companion_amd import _lib
    L = _lib.lib()
    plain = L.pc_rank_grouped_workspace_bytes
    for name in ENTRIES:
        ws = getattr(L, name + "_workspace_bytes")
        assert ws.restype == ctypes.c_size_t
        for rows, types, s in itertools.product((1, 17, 203, 12288), (1, 9, 100), (0, 1, 7, 64)):
            assert ws(rows, types, s) == plain(rows, types, s) > 0, (name, rows, types, s)
        for bad in ((0, 100, 0), (5, 0, 0), (5, 100, -1), (5, 100, 65)):
            assert ws(*bad) == 0, (name, bad)


def _aligned():
    """One 16-byte aligned host buffer: a pointer that passes every check, and that no check dereferences."""
    buf = ctypes.create_string_buffer(96)
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)


@pytest.mark.parametrize("name", ENTRIES)
def test_the_entries_refuse_before_anything_is_launched(name):
    from p_companion_amd import _lib
    entry = getattr(_lib.lib(), name)
    buf, p = _aligned()

    def call(where="all", **kw):
        a = dict(proj=p, types=p, targets=p, row_key=p, rows=4, type_rowptr=p, type_col=p, table=p, bias=p, n_types=3,
                 num_products=9, ex_rowptr=p, ex_col=p, n_keys=2, cand_type=p, dim=128, slices=0, rank_out=p, bad_count=p,
                 where=None, ws=p, ws_bytes=0, stream=None)
        a.update(kw)
        if where is not None:
            st = _lib.RowWhere(**{f: p.value for f in (FIELDS if where == "all" else where)})
            a["where"] = ctypes.byref(st)
        return entry(*a.values())

    none = dict(row_key=None, ex_rowptr=None, ex_col=None, n_keys=0, cand_type=None)
    # a filter that is in order reaches the workspace check, with and without lists, with and without a bias
    ok = ("all", (), ("value", "lo", "hi"), ("flags",), ("flags", "need"), ("flags", "deny"), ("flags", "need", "deny"),
          ("value", "lo", "hi", "flags"))
    for where in ok:
        assert call(where) == PC_EWORKSPACE and call(where, **none) == PC_EWORKSPACE, where
        assert call(where, bias=None) == PC_EWORKSPACE and call(where, bias=None, dim=256, **none) == PC_EWORKSPACE, where
    # the pairing rules, and the null filter
    assert call(None) == PC_EINVAL and call(None, **none) == PC_EINVAL
    bad = (("lo",), ("hi",), ("lo", "hi"), ("value",), ("value", "lo"), ("value", "hi"), ("need",), ("deny",), ("need", "deny"),
           ("value", "lo", "hi", "need"), ("flags", "need", "lo"), ("flags", "value"), ("lo", "hi", "flags", "need", "deny"))
    for where in bad:
        assert call(where) == PC_EINVAL and call(where, **none) == PC_EINVAL, where
    # everything else as the twin refuses it
    for arg in ("proj", "types", "targets", "type_rowptr", "type_col", "table", "rank_out", "bad_count", "ws", "ex_rowptr", "ex_col",
                "cand_type", "row_key"):
        assert call(**{arg: None}) == PC_EINVAL, arg
    assert call(**{**none, "cand_type": p}) == PC_EINVAL                                   # the products' types without lists
    assert call(rows=0) == PC_EINVAL and call(n_types=0) == PC_EINVAL and call(num_products=0) == PC_EINVAL
    assert call(n_keys=-1) == PC_EINVAL
    for kw in (dict(dim=64), dict(dim=192), dict(slices=-1), dict(slices=65)):
        assert call(**kw) == PC_ESHAPE and call(**kw, **none) == PC_ESHAPE, kw
        assert call(("lo",), **kw) == PC_EINVAL and call(None, **kw) == PC_EINVAL, kw      # the pointers, then the shapes
    if "bf16" in name:
        assert call(table=ctypes.c_void_p(p.value + 8)) == PC_ESHAPE                       # the bf16 table's alignment


@pytest.mark.parametrize("table,bias,exclude", itertools.product(("fp32", "bf16"), (False, True), (False, True)))
def test_the_wrapper_reaches_the_entry_of_the_tables_dtype(rec, table, bias, exclude):
    from p_companion_amd import _lib, ops
    sig = inspect.signature(ops.rank_grouped_where)
    assert list(sig.parameters) == ["proj", "types", "targets", "type_rowptr", "type_col", "table", "where", "slices", "bad",
                                    "exclude", "cand_type", "bias"]
    assert [sig.parameters[k].default for k in ("slices", "bad", "exclude", "cand_type", "bias")] == [0, None, None, None, None]
    entry = "pc_rank_grouped_bf16_where" if table == "bf16" else "pc_rank_grouped_where"
    for keep in (FIELDS, ("value", "lo", "hi"), ("flags", "deny"), ()):
        ts, ws = tensors(bf16=table == "bf16"), where_tensors(keep)
        rec.calls.clear(), rec.workspaces.clear()
        rank, bad = ops.rank_grouped_where(ts["proj"], ts["types"], ts["targets"], ts["type_rowptr"], ts["type_col"], ts["table"],
                                           ops.RowWhere(**ws), slices=7, bad=ts["bad_count"],
                                           exclude=triple(ts) if exclude else None, cand_type=ts["cand_type"] if exclude else None,
                                           bias=ts["bias"] if bias else None)
        assert tuple(rank.shape) == (R,) and rank.dtype == torch.int32 and bad is ts["bad_count"]
        assert [name for name, _ in rec.calls] == [entry + "_workspace_bytes", entry]
        assert list(rec.calls[0][1]) == [R, T, 7] and rec.workspaces == [(WS_BYTES, "rank_grouped")]
        args = list(rec.calls[1][1])
        ptr = lambda a: a.value if isinstance(a, ctypes.c_void_p) else a
        assert len(args) == len(_lib.SIGNATURES[entry][1])
        # the tail: where, ws, ws_bytes, stream; the head: pc_rank_grouped_bf16's list
        assert [ptr(a) for a in args[-3:]] == [WS.data_ptr(), WS.numel(), STREAM.value]
        head = [ptr(a) for a in args[:-4]]
        lists = [ts["ex_rowptr"].data_ptr(), ts["ex_col"].data_ptr(), KEYS, ts["cand_type"].data_ptr()] if exclude \
            else [None, None, 0, None]
        assert head == [ts["proj"].data_ptr(), ts["types"].data_ptr(), ts["targets"].data_ptr(),
                        ts["row_key"].data_ptr() if exclude else None, R, ts["type_rowptr"].data_ptr(), ts["type_col"].data_ptr(),
                        ts["table"].data_ptr(), ts["bias"].data_ptr() if bias else None, T, P] + lists + \
            [D, 7, rank.data_ptr(), ts["bad_count"].data_ptr()]
        st = args[-4]._obj
        assert isinstance(st, _lib.RowWhere)
        assert {f: getattr(st, f) for f in FIELDS} == {f: ws[f].data_ptr() if f in ws else None for f in FIELDS}


def test_the_wrapper_refuses_before_anything_is_reached(rec):
    from p_companion_amd import ops
    ts, bf = tensors(), tensors(bf16=True)
    base = (ts["proj"], ts["types"], ts["targets"], ts["type_rowptr"], ts["type_col"])
    where = ops.RowWhere(**where_tensors())
    for no_holder in (None, {}, where_tensors()):
        with pytest.raises(ValueError, match="where must be an ops.RowWhere"):
            ops.rank_grouped_where(*base, ts["table"], no_holder)
    # the lengths against P and R, at the call
    for f in FIELDS:
        short = where_tensors()
        short[f] = short[f][:-1].contiguous().as_subclass(OnDevice)
        with pytest.raises(ValueError, match=rf"where\.{f} must hold one entry per (product|row)"):
            ops.rank_grouped_where(*base, ts["table"], ops.RowWhere(**short))
    # the table: fp32 or bf16, [P, D]
    for table in (ts["table"].double(), ts["table"].half(), ts["table"][0], [0.0] * P):
        with pytest.raises(ValueError, match="table"):
            ops.rank_grouped_where(*base, table, where)
    # the bias checks are rank_grouped's and rank_grouped_bf16's
    for t in (ts, bf):
        with pytest.raises(ValueError, match="float32"):
            ops.rank_grouped_where(*base, t["table"], where, bias=ts["bias"].double())
        with pytest.raises(ValueError, match="one entry per product"):
            ops.rank_grouped_where(*base, t["table"], where, bias=dev(P + 1))
        with pytest.raises(ValueError, match="bias must be"):
            ops.rank_grouped_where(*base, t["table"], where, bias=[0.0] * P)
        # the lists and the products' types: all or none
        with pytest.raises(ValueError, match="cand_type is read with an exclude triple only"):
            ops.rank_grouped_where(*base, t["table"], where, cand_type=ts["cand_type"])
        with pytest.raises(ValueError, match="exclude needs cand_type"):
            ops.rank_grouped_where(*base, t["table"], where, exclude=triple(ts))
        for cand in (ts["cand_type"].long(), dev(P + 1, dtype=torch.int32), dev(P, 1, dtype=torch.int32)):
            with pytest.raises(ValueError, match="cand_type must be an int32 tensor"):
                ops.rank_grouped_where(*base, t["table"], where, exclude=triple(ts), cand_type=cand)
        with pytest.raises(ValueError, match="exclude"):
            ops.rank_grouped_where(*base, t["table"], where, exclude=(ts["row_key"].long(), ts["ex_rowptr"], ts["ex_col"]),
                                   cand_type=ts["cand_type"])
        with pytest.raises(ValueError, match="slices"):
            ops.rank_grouped_where(*base, t["table"], where, slices=65)
    assert rec.calls == []


F32, I32 = torch.zeros(2), torch.zeros(2, dtype=torch.int32)
VALUE, FLAGS = torch.arange(9.0), torch.arange(9, dtype=torch.int32)


def _refusals(obj, call):
    """_row_predicate's refusals through a method: no attributes, none of the four, wrong dtype or shape, a band without value,
    masks without flags"""
    with pytest.raises(ValueError, match="no per-product attributes are installed"):
        call(lo=F32, hi=F32)
    obj.set_attributes(value=VALUE, flags=FLAGS)
    with pytest.raises(ValueError, match="at least one of lo, hi, need, deny"):
        call()
    for kw in (dict(lo=F32.double()), dict(hi=torch.zeros(3)), dict(need=F32), dict(deny=torch.zeros(2, 1, dtype=torch.int32)),
               dict(lo=1.0)):
        with pytest.raises(ValueError, match="one entry per query"):
            call(**kw)
    obj.set_attributes(flags=FLAGS)
    with pytest.raises(ValueError, match="lo / hi bound the per-product value"):
        call(lo=F32)
    obj.set_attributes(value=VALUE)
    with pytest.raises(ValueError, match="need / deny test the per-product flags"):
        call(deny=I32)
    obj.set_attributes()


def test_the_complement_methods_refuse_before_the_model_runs():
    from p_companion_amd.data import ComplementaryIndexDataset
    from p_companion_amd.inference import CompactInference, PCompanionInference
    sig = inspect.signature(PCompanionInference.rank_targets_where)
    assert list(sig.parameters) == ["self", "query_idx", "target_idx", "lo", "hi", "need", "deny", "take"]
    assert all(p.default is None for p in list(sig.parameters.values())[3:])
    sig = inspect.signature(PCompanionInference.evaluate_catalogue_where)
    assert list(sig.parameters) == ["self", "dataset", "predicate", "ks", "chunk"]
    assert [sig.parameters[k].default for k in ("ks", "chunk")] == [(1, 3, 10, 100), 65536]
    assert CompactInference.rank_targets_where is PCompanionInference.rank_targets_where
    assert CompactInference.evaluate_catalogue_where is PCompanionInference.evaluate_catalogue_where
    q = torch.zeros(2, dtype=torch.int32)
    bpg = object()
    inf = object.__new__(PCompanionInference)
    inf.__dict__.update(model=Untouchable(), features=Untouchable(), bpg=bpg, exclusions=Untouchable(),
                        type_idx=torch.zeros(9, dtype=torch.int32), device="cpu")
    _refusals(inf, lambda **kw: inf.rank_targets_where(q, q, **kw))
    ds = object.__new__(ComplementaryIndexDataset)
    ds.__dict__.update(bpg=bpg, pairs=torch.tensor([[0, 1, 1], [2, 3, 1]], dtype=torch.int32))
    with pytest.raises(ValueError, match="no per-product attributes are installed"):
        inf.evaluate_catalogue_where(ds, lambda qi: dict(lo=F32))
    _refusals(inf, lambda **kw: inf.evaluate_catalogue_where(ds, lambda qi: kw))
    inf.set_attributes(value=VALUE)
    for no_callable in (None, dict(lo=F32), 3):
        with pytest.raises(ValueError, match="predicate must be a callable"):
            inf.evaluate_catalogue_where(ds, no_callable)
    for no_dict in ((F32, F32), dict(low=F32), None):
        with pytest.raises(ValueError, match="must return a dict with any of lo, hi, need, deny"):
            inf.evaluate_catalogue_where(ds, lambda qi: no_dict)
    with pytest.raises(ValueError, match="chunk must be positive"):
        inf.evaluate_catalogue_where(ds, lambda qi: dict(lo=F32), chunk=0)
    with pytest.raises(ValueError, match="another graph"):
        inf.evaluate_catalogue_where(object(), lambda qi: dict(lo=F32))
    # a bare bf16 catalogue stays refused: the rank kernels of this class read the fp32 catalogue
    inf.__dict__.update(catalogue=torch.zeros(1, dtype=torch.bfloat16), compact=None)
    with pytest.raises(ValueError, match="the rank kernels read the fp32 catalogue"):
        inf.rank_targets_where(q, q, lo=F32)
    with pytest.raises(ValueError, match="the rank kernels read the fp32 catalogue"):
        inf.evaluate_catalogue_where(ds, lambda qi: dict(lo=F32))


def test_the_substitute_methods_refuse_before_anything_is_computed():
    from p_companion_amd.inference import (CompactSimilarProducts, IndexedCompactSimilarProducts, IndexedSimilarProducts,
                                           SimilarProducts)
    sig = inspect.signature(SimilarProducts.rank_pairs_where)
    assert list(sig.parameters) == ["self", "anchor_idx", "target_idx", "lo", "hi", "need", "deny"]
    assert all(p.default is None for p in list(sig.parameters.values())[3:])
    sig = inspect.signature(SimilarProducts.evaluate_pairs_where)
    assert list(sig.parameters) == ["self", "pairs", "predicate", "ks", "chunk"]
    assert [sig.parameters[k].default for k in ("ks", "chunk")] == [(1, 3, 10, 100), 65536]
    for cls in (CompactSimilarProducts, IndexedSimilarProducts, IndexedCompactSimilarProducts):      # the exact ones, inherited
        assert cls.rank_pairs_where is SimilarProducts.rank_pairs_where
        assert cls.evaluate_pairs_where is SimilarProducts.evaluate_pairs_where
    q = torch.zeros(2, dtype=torch.int32)
    pairs = torch.tensor([[0, 1], [2, 3]], dtype=torch.int32)
    sp = object.__new__(SimilarProducts)
    sp.__dict__.update(table=Untouchable(), bpg=Untouchable(), exclusions=Untouchable(), bias=Untouchable(),
                       type_idx=torch.zeros(9, dtype=torch.int32), device="cpu")
    _refusals(sp, lambda **kw: sp.rank_pairs_where(q, q, **kw))
    with pytest.raises(ValueError, match="no per-product attributes are installed"):
        sp.evaluate_pairs_where(pairs, lambda a: dict(lo=F32))
    _refusals(sp, lambda **kw: sp.evaluate_pairs_where(pairs, lambda a: kw))
    sp.set_attributes(value=VALUE)
    for no_callable in (None, dict(lo=F32), 3):
        with pytest.raises(ValueError, match="predicate must be a callable"):
            sp.evaluate_pairs_where(pairs, no_callable)
    for no_dict in ((F32, F32), dict(low=F32), None):
        with pytest.raises(ValueError, match="must return a dict with any of lo, hi, need, deny"):
            sp.evaluate_pairs_where(pairs, lambda a: no_dict)
    with pytest.raises(ValueError, match="chunk must be positive"):
        sp.evaluate_pairs_where(pairs, lambda a: dict(lo=F32), chunk=0)
    with pytest.raises(ValueError, match=r"non-empty \[M, 2\]"):
        sp.evaluate_pairs_where(torch.zeros(0, 2, dtype=torch.int32), lambda a: dict(lo=F32))
