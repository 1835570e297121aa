"""pc_retrieve_list_grouped's host side (long lists, up to 256 products per (query, type)), without a GPU: the header and the
bindings, the workspace query, the refusals of the C entry before anything is launched, and the Python wrappers' own checks --
every tensor here lives on the host, so a call that reached a device check would raise TypeError (no CPU fallback)."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

PC_EINVAL, PC_ESHAPE = -1, -2


def test_header_declares_both_entries_and_the_abi_stays_8():
    txt = open(os.path.join(ROOT, "include", "pcompanion_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("pc_retrieve_list_grouped", "pc_retrieve_list_grouped_workspace_bytes"):
        assert re.search(r"\b" + name + r"\s*\(", txt), name
    assert re.search(r"#define PC_ABI_VERSION 8\b", txt)
    from p_companion_amd import _lib
    sig = _lib.SIGNATURES
    # the filtered 16-entry's arguments, one for one
    assert sig["pc_retrieve_list_grouped"] == sig["pc_retrieve_topk_grouped_excluding"]
    assert sig["pc_retrieve_list_grouped_workspace_bytes"] == sig["pc_retrieve_topk_grouped_workspace_bytes"]
    L = _lib.lib()
    assert L.pc_retrieve_list_grouped.argtypes == sig["pc_retrieve_list_grouped"][1]
    assert L.pc_retrieve_list_grouped_workspace_bytes.restype == ctypes.c_size_t


def test_workspace_bytes():
    from p_companion_amd import _lib
    ws = _lib.lib().pc_retrieve_list_grouped_workspace_bytes
    rows, types = 12288, 100
    for bad in ((0, types, 64, 0), (rows, 0, 64, 0), (rows, types, 0, 0), (rows, types, 257, 0), (rows, types, 64, -1),
                (rows, types, 64, 65)):
        assert ws(*bad) == 0, bad
    sizes = [ws(rows, types, n, 0) for n in (1, 16, 17, 256)]
    assert sizes[0] > 0 and sizes == sorted(sizes) and sizes[1] < sizes[3]
    partials = rows * 16 * 256 * 8                                     # [rows][S][n] of (score, id)
    assert partials <= sizes[3] < partials + 8 * (rows + types) * 4 + 8 * 256
    assert ws(rows, types, 256, 16) == sizes[3]                        # 0 = automatic = 16 slices
    assert ws(rows, types, 256, 1) < ws(rows, types, 256, 7) < sizes[3] < ws(rows, types, 256, 64)
    # at n <= 16 the partial lists are the existing entry's
    assert ws(rows, types, 16, 0) == _lib.lib().pc_retrieve_topk_grouped_workspace_bytes(rows, types, 16, 0)


def _entry_args(**kw):
    """Arguments that would pass every check: the pointers are host buffers, which no check dereferences."""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    a = dict(proj=p, types=p, row_key=p, rows=4, type_rowptr=p, type_col=p, table=p, n_types=3, ex_rowptr=p, ex_col=p, n_keys=2,
             n=64, dim=128, slices=0, out_idx=p, out_score=p, bad_count=p, ws=p, ws_bytes=0, stream=None)
    a.update(kw)
    return buf, list(a.values())


def test_entry_refuses_before_anything_is_launched():
    from p_companion_amd import _lib
    entry = _lib.lib().pc_retrieve_list_grouped

    def call(**kw):
        buf, args = _entry_args(**kw)
        return entry(*args)

    for name in ("proj", "types", "type_rowptr", "type_col", "table", "out_idx", "out_score", "ws", "ex_rowptr", "ex_col",
                 "bad_count"):
        assert call(**{name: None}) == PC_EINVAL, name
    assert call(rows=0) == PC_EINVAL and call(n_types=0) == PC_EINVAL and call(n_keys=-1) == PC_EINVAL
    # without keys there is no list (and no counter is needed)
    assert call(row_key=None) == PC_EINVAL and call(row_key=None, ex_rowptr=None, ex_col=None) == PC_EINVAL
    none = dict(row_key=None, ex_rowptr=None, ex_col=None, n_keys=0, bad_count=None)
    for kw in (dict(n=0), dict(n=257), dict(dim=64), dict(slices=-1), dict(slices=65)):
        assert call(**kw) == PC_ESHAPE, kw
        assert call(**kw, **none) == PC_ESHAPE, kw
    assert call() == -3 and call(**none) == -3 and call(n=256, **none) == -3       # PC_EWORKSPACE: ws_bytes = 0


def test_wrapper_refuses_on_the_host():
    from p_companion_amd import ops
    assert ops.RETRIEVE_LIST_MAX_N == 256
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)
    proj, table = torch.zeros(4, 128), torch.zeros(5, 128)
    call = lambda n, **kw: ops.retrieve_list_grouped(proj, i32(4), i32(3), i32(5), table, n, **kw)
    for n in (0, 257, -1):
        with pytest.raises(ValueError, match="256"):
            call(n)
    with pytest.raises(ValueError, match="slices"):
        call(100, slices=65)
    rk, rp, cl = i32(4), i32(3), i32(0)
    for bad in ((rk, rp), "lists", (rk, rp, None), (rk.long(), rp, cl), (rk[:3], rp, cl), (rk, rp.reshape(3, 1), cl), (rk, rp[:0], cl)):
        with pytest.raises(ValueError, match="exclude"):
            call(100, exclude=bad)
    with pytest.raises(ValueError, match="bad"):
        call(100, bad=i32(1))
    # well-formed arguments pass these checks and meet the device check
    for kw in ({}, {"exclude": (rk, rp, cl)}):
        with pytest.raises(TypeError, match="CUDA/ROCm"):
            call(100, **kw)
        with pytest.raises(TypeError, match="CUDA/ROCm"):
            call(256, **kw)
    # the 16-entries keep their limit
    with pytest.raises(TypeError, match="CUDA/ROCm"):
        ops.retrieve_topk_grouped(proj, i32(4), i32(3), i32(5), table, 17)


def test_recommend_batch_names_the_limit_before_the_model_runs():
    from p_companion_amd.inference import PCompanionInference

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"recommend_batch read .{name} before refusing the length")

    inf = object.__new__(PCompanionInference)                          # (no graph, no model, no device)
    inf.__dict__.update(model=Untouchable(), bpg=Untouchable(), features=Untouchable())
    q = torch.zeros(2, dtype=torch.int32)
    for n in (257, 1000):
        with pytest.raises(ValueError, match="256"):
            inf.recommend_batch(q, n)
    assert PCompanionInference._list_length(256) == 256 and PCompanionInference._list_length(17) == 17
    with pytest.raises(ValueError, match="256"):
        PCompanionInference._list_length(257)
