"""pc_retrieve_topk_grouped_bf16's host side (a bf16 copy of the catalogue), without a GPU: the header and the ctypes table,
the workspace query, what the entry refuses before anything is launched, and the argument checks of ops.catalogue_bf16,
ops.retrieve_topk_grouped and PCompanionInference(catalogue=) that need no device."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

from conftest import ROOT

PC_EINVAL, PC_ESHAPE, PC_EWORKSPACE = -1, -2, -3


def test_header_declares_the_entries_and_the_abi_stays_8():
    from p_companion_amd import _lib
    txt = open(os.path.join(ROOT, "include", "pcompanion_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("pc_retrieve_topk_grouped_bf16", "pc_retrieve_topk_grouped_bf16_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES
    assert re.search(r"const\s+uint16_t\s*\*\s*table_bf16", code)
    assert re.search(r"#define\s+PC_ABI_VERSION\s+8\b", txt)
    sig = _lib.SIGNATURES
    # the filtered entry's argument list (the table pointer is the one difference, and a pointer is a pointer)
    assert sig["pc_retrieve_topk_grouped_bf16"] == sig["pc_retrieve_topk_grouped_excluding"]
    assert sig["pc_retrieve_topk_grouped_bf16_workspace_bytes"] == sig["pc_retrieve_topk_grouped_workspace_bytes"]
    L = _lib.lib()
    assert L.pc_abi_version() == 8
    assert L.pc_retrieve_topk_grouped_bf16_workspace_bytes.restype == ctypes.c_size_t


def test_workspace_bytes_depend_on_the_plan_only():
    from p_companion_amd import _lib
    L = _lib.lib()
    ws = L.pc_retrieve_topk_grouped_bf16_workspace_bytes
    rows, types = 12288, 100
    full = ws(rows, types, 16, 16)
    partials = rows * 16 * 16 * 8
    assert partials <= full < partials + 8 * (rows + types) * 4 + 8 * 256
    assert ws(rows, types, 16, 0) == full                               # 0 = automatic = 16 slices
    assert ws(rows, types, 16, 1) < ws(rows, types, 16, 7) < full < ws(rows, types, 16, 64)
    assert ws(rows, 34_800, 10, 0) > ws(rows, 100, 10, 0)
    for bad in ((0, types, 10, 0), (rows, 0, 10, 0), (rows, types, 0, 0), (rows, types, 17, 0), (rows, types, 10, -1),
                (rows, types, 10, 65)):
        assert ws(*bad) == 0, bad
    # the fp32 entry's plan and partial lists: the same size
    for n, s in ((1, 1), (10, 0), (16, 64)):
        assert ws(rows, types, n, s) == L.pc_retrieve_topk_grouped_workspace_bytes(rows, types, n, s)


def _entry_args(**kw):
    """Arguments that would pass every check: the pointers are one 16-byte aligned host buffer, which no check dereferences."""
    buf = ctypes.create_string_buffer(96)
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p((base + 15) & ~15)
    a = dict(proj=p, types=p, row_key=p, rows=4, type_rowptr=p, type_col=p, table=p, n_types=3, ex_rowptr=p, ex_col=p, n_keys=2,
             n=10, dim=128, slices=0, out_idx=p, out_score=p, bad_count=p, ws=p, ws_bytes=0, stream=None)
    a.update(kw)
    return buf, p, list(a.values())


def test_entry_refuses_before_anything_is_launched():
    from p_companion_amd import _lib
    entry = _lib.lib().pc_retrieve_topk_grouped_bf16

    def call(**kw):
        buf, _, args = _entry_args(**kw)
        return entry(*args)

    for name in ("proj", "types", "type_rowptr", "type_col", "table", "out_idx", "out_score", "ws", "ex_rowptr", "ex_col",
                 "bad_count"):
        assert call(**{name: None}) == PC_EINVAL, name
    assert call(rows=0) == PC_EINVAL and call(n_types=0) == PC_EINVAL and call(n_keys=-1) == PC_EINVAL
    # the exclusion arguments are nullable as a group only
    assert call(row_key=None) == PC_EINVAL and call(row_key=None, ex_rowptr=None, ex_col=None) == PC_EINVAL
    none = dict(row_key=None, ex_rowptr=None, ex_col=None, n_keys=0, bad_count=None)
    for kw in (dict(n=0), dict(n=17), dict(dim=64), dict(dim=192), dict(slices=-1), dict(slices=65)):
        assert call(**kw) == PC_ESHAPE, kw
        assert call(**kw, **none) == PC_ESHAPE, kw
    buf, p, _ = _entry_args()
    for off in (2, 4, 8):                                                          # a table that is not 16-byte aligned
        assert call(table=ctypes.c_void_p(p.value + off)) == PC_ESHAPE, off
        assert call(table=ctypes.c_void_p(p.value + off), **none) == PC_ESHAPE, off
    assert call() == PC_EWORKSPACE and call(**none) == PC_EWORKSPACE and call(n=16, dim=256, **none) == PC_EWORKSPACE


def test_wrappers_refuse_cpu_tensors_and_other_dtypes():
    from p_companion_amd import ops
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)
    proj = torch.zeros(4, 128)
    bf = torch.zeros(5, 128, dtype=torch.bfloat16)
    rk, rp, cl = i32(4), i32(3), i32(0)
    for kw in ({}, {"exclude": (rk, rp, cl)}):
        with pytest.raises(TypeError, match="CUDA/ROCm"):
            ops.retrieve_topk_grouped(proj, i32(4), i32(3), i32(5), bf, 5, **kw)
    with pytest.raises(ValueError, match="bad"):
        ops.retrieve_topk_grouped(proj, i32(4), i32(3), i32(5), bf, 5, bad=i32(1))
    with pytest.raises(ValueError, match="exclude"):
        ops.retrieve_topk_grouped(proj, i32(4), i32(3), i32(5), bf, 5, exclude=(rk.long(), rp, cl))
    with pytest.raises(ValueError, match="width"):
        ops.retrieve_topk_grouped(torch.zeros(4, 64), i32(4), i32(3), i32(5), torch.zeros(5, 64, dtype=torch.bfloat16), 5)
    with pytest.raises(TypeError, match="CUDA/ROCm"):
        ops.catalogue_bf16(torch.zeros(5, 128))
    # the other serving wrappers keep refusing anything but fp32 (on the host the device check comes first: a TypeError either way)
    for fn in (ops.retrieve_topk, ops.retrieve_list_grouped):
        with pytest.raises(TypeError):
            fn(proj, i32(4), i32(3), i32(5), bf, 5)
    with pytest.raises(TypeError):
        ops.rank_grouped(proj, i32(4), i32(4), i32(3), i32(5), bf)


def test_catalogue_bf16_refuses_a_non_fp32_input():
    """_req tests the device first; a stand-in that reports is_cuda lets the dtype test be reached without a device."""
    from p_companion_amd import ops

    class OnDevice(torch.Tensor):
        is_cuda = True

    for dtype in (torch.float64, torch.float16, torch.bfloat16, torch.int32):
        t = torch.zeros(5, 128, dtype=dtype).as_subclass(OnDevice)
        with pytest.raises(TypeError, match="float32"):
            ops.catalogue_bf16(t)
    with pytest.raises(TypeError):
        ops.catalogue_bf16([[0.0] * 128])
    with pytest.raises(ValueError, match=r"\[P, D\]"):
        ops.catalogue_bf16(torch.zeros(128).as_subclass(OnDevice))
    with pytest.raises(ValueError, match="width"):
        ops.catalogue_bf16(torch.zeros(5, 64).as_subclass(OnDevice))
    # any other table dtype gets retrieve_topk_grouped's TypeError, as before
    i32 = lambda n: torch.zeros(n, dtype=torch.int32).as_subclass(OnDevice)
    proj = torch.zeros(4, 128).as_subclass(OnDevice)
    for dtype in (torch.float16, torch.float64):
        with pytest.raises(TypeError, match="float32"):
            ops.retrieve_topk_grouped(proj, i32(4), i32(3), i32(5), torch.zeros(5, 128, dtype=dtype).as_subclass(OnDevice), 5)


class Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"read .{name} before refusing")


def test_inference_refuses_a_bad_catalogue_before_the_model_or_the_graph_is_touched():
    from p_companion_amd.inference import PCompanionInference
    cfg = SimpleNamespace(DEVICE="cuda")
    bpg = SimpleNamespace(num_products=7)                             # (no arrays, no cuda(): reading them is an error)
    for bad, what in ((torch.float16, "catalogue must be"), ("bf16", "catalogue must be"), (16, "catalogue must be"),
                      (torch.float32, "catalogue must be"),
                      (torch.zeros(7, 128), "bfloat16"), (torch.zeros(7, 128, dtype=torch.float16), "bfloat16"),
                      (torch.zeros(6, 128, dtype=torch.bfloat16), r"\[7, 128 or 256\]"),
                      (torch.zeros(7, 64, dtype=torch.bfloat16), r"\[7, 128 or 256\]"),
                      (torch.zeros(7 * 128, dtype=torch.bfloat16), r"\[7, 128 or 256\]"),
                      (torch.zeros(7, 128, dtype=torch.bfloat16), "device tensor")):
        with pytest.raises(ValueError, match=what):
            PCompanionInference(Untouchable(), cfg, bpg, catalogue=bad)


def test_a_bf16_catalogue_names_the_fp32_catalogue_before_the_model_runs():
    from p_companion_amd.inference import PCompanionInference
    inf = object.__new__(PCompanionInference)                          # (no graph, no model, no device)
    inf.__dict__.update(model=Untouchable(), bpg=Untouchable(), features=None,
                        catalogue=torch.zeros(3, 128, dtype=torch.bfloat16))
    q = torch.zeros(2, dtype=torch.int32)
    for n in (17, 100, 256):
        with pytest.raises(ValueError, match="fp32 catalogue"):
            inf.recommend_batch(q, n)
    with pytest.raises(ValueError, match="256"):
        inf.recommend_batch(q, 257)
    with pytest.raises(ValueError, match="fp32 catalogue"):
        inf.rank_targets(q, q)
    with pytest.raises(ValueError, match="fp32 catalogue"):
        inf.evaluate_catalogue(Untouchable())
