"""The host side of the long substitute lists (pc_retrieve_list_grouped_biased; ops.retrieve_list_grouped_biased;
SimilarProducts / IndexedSimilarProducts.similar_list_batch and similar_capped_list_batch), without a GPU: the header and the
ctypes table, the workspace query, what the entry refuses before anything is launched, and the argument checks of the wrapper and
the methods that need no device."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT

PC_EINVAL, PC_ESHAPE, PC_EWORKSPACE = -1, -2, -3
ENTRIES = ("pc_retrieve_list_grouped_biased", "pc_retrieve_list_grouped_biased_workspace_bytes")


def test_header_declares_the_entries_and_the_abi_stays_8():
    from p_companion_amd import _lib
    txt = open(os.path.join(ROOT, "include", "pcompanion_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES
    decl = re.search(r"\bpc_retrieve_list_grouped_biased\s*\(([^;]*)\)\s*;", code).group(1)
    names = [a.split("*")[-1].split()[-1] for a in decl.split(",")]
    plain = re.search(r"\bpc_retrieve_list_grouped\s*\(([^;]*)\)\s*;", code).group(1)
    plain = [a.split("*")[-1].split()[-1] for a in plain.split(",")]
    assert names == plain[:7] + ["bias"] + plain[7:] and plain[6] == "table"     # the bias directly behind the table
    assert re.search(r"#define\s+PC_ABI_VERSION\s+8\b", txt)
    sig = _lib.SIGNATURES
    ret, args = sig["pc_retrieve_list_grouped"]
    assert sig["pc_retrieve_list_grouped_biased"] == (ret, args[:7] + [ctypes.c_void_p] + args[7:])
    assert sig["pc_retrieve_list_grouped_biased"] == sig["pc_retrieve_topk_grouped_biased"]
    assert sig["pc_retrieve_list_grouped_biased_workspace_bytes"] == sig["pc_retrieve_list_grouped_workspace_bytes"]
    L = _lib.lib()
    assert L.pc_abi_version() == 8
    assert L.pc_retrieve_list_grouped_biased_workspace_bytes.restype == ctypes.c_size_t


def test_the_unit_is_part_of_the_build():
    from p_companion_amd import build
    assert "nearest_list.hip" in build.sources()


def test_the_workspace_is_the_unbiased_list_entrys():
    from p_companion_amd import _lib
    L = _lib.lib()
    ws, plain = L.pc_retrieve_list_grouped_biased_workspace_bytes, L.pc_retrieve_list_grouped_workspace_bytes
    for rows in (1, 17, 12288):
        for types in (1, 100, 34_800):
            for n in (1, 16, 17, 32, 33, 96, 97, 255, 256):
                for s in (0, 1, 7, 64):
                    assert ws(rows, types, n, s) == plain(rows, types, n, s) > 0, (rows, types, n, s)
    rows, types = 12288, 100
    assert ws(rows, types, 256, 0) == ws(rows, types, 256, 16) >= rows * 16 * 256 * 8
    for bad in ((0, types, 10, 0), (rows, 0, 10, 0), (rows, types, 0, 0), (rows, types, 257, 0), (rows, types, 10, -1),
                (rows, types, 10, 65), (-1, types, 10, 0)):
        assert ws(*bad) == 0, bad


def _aligned():
    """One 16-byte aligned host buffer: a pointer that passes every check, and that no check dereferences."""
    buf = ctypes.create_string_buffer(96)
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)


def test_the_entry_refuses_before_anything_is_launched():
    from p_companion_amd import _lib
    entry = _lib.lib().pc_retrieve_list_grouped_biased
    buf, p = _aligned()

    def call(**kw):
        a = dict(proj=p, types=p, row_key=p, rows=4, type_rowptr=p, type_col=p, table=p, bias=p, n_types=3, ex_rowptr=p,
                 ex_col=p, n_keys=2, n=100, dim=128, slices=0, out_idx=p, out_score=p, bad_count=p, ws=p, ws_bytes=0, stream=None)
        a.update(kw)
        return entry(*a.values())

    for name in ("proj", "types", "type_rowptr", "type_col", "table", "bias", "out_idx", "out_score", "ws", "ex_rowptr", "ex_col",
                 "bad_count"):
        assert call(**{name: None}) == PC_EINVAL, name
    assert call(rows=0) == PC_EINVAL and call(n_types=0) == PC_EINVAL and call(n_keys=-1) == PC_EINVAL
    # the exclusion arguments: all or none
    assert call(row_key=None) == PC_EINVAL and call(row_key=None, ex_rowptr=None, ex_col=None) == PC_EINVAL
    assert call(row_key=None, ex_col=None, n_keys=0) == PC_EINVAL
    none = dict(row_key=None, ex_rowptr=None, ex_col=None, n_keys=0, bad_count=None)
    assert call(bias=None, **none) == PC_EINVAL
    for kw in (dict(n=0), dict(n=257), dict(n=-1), dict(dim=64), dict(dim=192), dict(slices=-1), dict(slices=65)):
        assert call(**kw) == PC_ESHAPE, kw
        assert call(**kw, **none) == PC_ESHAPE, kw
        assert call(bias=None, **kw) == PC_EINVAL, kw                   # the family's order: the pointers, then the shapes
    for n in (1, 16, 17, 32, 33, 96, 97, 256):                          # every buffer size, both widths
        assert call(n=n) == PC_EWORKSPACE and call(n=n, **none) == PC_EWORKSPACE and call(n=n, dim=256, **none) == PC_EWORKSPACE


class OnDevice(torch.Tensor):
    """A stand-in that reports is_cuda: _req tests the device first, and this lets the checks behind it be reached."""
    is_cuda = True


def test_the_wrapper_refuses_cpu_tensors_an_unsupported_bias_and_n_out_of_range():
    from p_companion_amd import ops
    sig = inspect.signature(ops.retrieve_list_grouped_biased)
    assert list(sig.parameters) == ["proj", "types", "type_rowptr", "type_col", "table", "bias", "n", "slices", "exclude", "bad"]
    assert [sig.parameters[k].default for k in ("slices", "exclude", "bad")] == [0, None, None]
    assert "bias" not in inspect.signature(ops.retrieve_list_grouped).parameters
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)
    proj, table, bias = torch.zeros(4, 128), torch.zeros(5, 128), torch.zeros(5)
    fn = lambda n=20, **kw: ops.retrieve_list_grouped_biased(proj, i32(4), i32(3), i32(5), kw.pop("table", table),
                                                             kw.pop("bias", bias), n, **kw)
    # a well-formed call: it goes on to the device check of its tensors
    for n in (1, 16, 17, 256):
        with pytest.raises(TypeError, match="CUDA/ROCm"):
            fn(n)
    # the refusals of the bias itself: _check_bias's, whatever else the call holds
    with pytest.raises(ValueError, match="bf16 table"):
        fn(table=torch.zeros(5, 128, dtype=torch.bfloat16))
    for dtype in (torch.float64, torch.float16, torch.bfloat16, torch.int32):
        with pytest.raises(ValueError, match="float32"):
            fn(bias=bias.to(dtype))
    for shape in ((4,), (6,), (5, 1), (1, 5), ()):
        with pytest.raises(ValueError, match="one entry per product"):
            fn(bias=torch.zeros(shape))
    for no_tensor in ([0.0] * 5, None):
        with pytest.raises(ValueError, match="bias must be"):
            fn(bias=no_tensor)
    for n in (0, 257, -1, 1000):
        with pytest.raises(ValueError, match=r"n must be in \[1, 256\]"):
            fn(n)
        with pytest.raises(ValueError, match=r"n must be in \[1, 256\]"):
            fn(n, bias=bias.as_subclass(OnDevice), table=table.as_subclass(OnDevice))
    # the exclusion checks are the unbiased call's
    with pytest.raises(ValueError, match="exclude"):
        fn(exclude=(i32(4).long(), i32(3), i32(0)))
    with pytest.raises(ValueError, match="bad counts keys"):
        fn(bad=i32(1))


class Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"read .{name} before refusing")


def test_the_methods_refuse_before_anything_is_touched():
    from p_companion_amd.inference import IndexedSimilarProducts, SimilarProducts
    assert SimilarProducts.MAX_LIST == 256 and SimilarProducts.MAX_N == 16 and IndexedSimilarProducts.MAX_LIST == 256
    sig = inspect.signature(SimilarProducts.similar_list_batch)
    assert list(sig.parameters) == ["self", "query_idx", "n"] and sig.parameters["n"].default == 64
    sig = inspect.signature(IndexedSimilarProducts.similar_list_batch)
    assert list(sig.parameters) == ["self", "query_idx", "n", "nprobe"]
    assert [sig.parameters[k].default for k in ("n", "nprobe")] == [64, None]
    sig = inspect.signature(SimilarProducts.similar_capped_list_batch)
    assert list(sig.parameters) == ["self", "query_idx", "n", "group", "cap", "own_group", "pool"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [10, None, 1, False, 64]
    # inherited, not restated: the subclass's similar_list_batch serves the pool
    assert IndexedSimilarProducts.similar_capped_list_batch is SimilarProducts.similar_capped_list_batch
    q = torch.zeros(2, dtype=torch.int32)
    bad_groups = (torch.zeros(9), torch.zeros(9, dtype=torch.int64), torch.zeros(3, 3, dtype=torch.int32), [0] * 9, "group")
    for cls in (SimilarProducts, IndexedSimilarProducts):
        sp = object.__new__(cls)                                       # (no table, no graph, no device)
        sp.__dict__.update(table=Untouchable(), bpg=Untouchable(), exclusions=Untouchable(), type_idx=Untouchable(),
                           bias=Untouchable(), index=Untouchable(), n_cells=Untouchable(), nprobe=Untouchable())
        for n in (0, -1, 257, 1000):
            with pytest.raises(ValueError, match="1 to 256"):
                sp.similar_list_batch(q, n)
        for n, pool in ((0, 64), (-1, 64), (65, 64), (10, 9), (10, 257), (300, 300), (10, 0)):
            with pytest.raises(ValueError, match="1 <= n <= pool <= 256"):
                sp.similar_capped_list_batch(q, n, pool=pool)
        with pytest.raises(ValueError, match="cap must be at least 1"):
            sp.similar_capped_list_batch(q, 10, cap=0)
        for g in bad_groups:
            with pytest.raises(ValueError, match=r"group must be None or a \[P\] int32"):
                sp.similar_capped_list_batch(q, 10, group=g)
        sp.__dict__.update(type_idx=torch.zeros(9, dtype=torch.int32))
        with pytest.raises(ValueError, match=r"one entry per product \(9\), got 7"):
            sp.similar_capped_list_batch(q, 10, group=torch.zeros(7, dtype=torch.int32), pool=256)
    doc = " ".join(SimilarProducts.similar_capped_batch.__doc__.split())
    assert "pool is 16" in doc and "SHORT" in doc and "similar_capped_list_batch" in doc
