"""The host side of the biased grouped retrieval and rank (pc_retrieve_topk_grouped_biased, pc_rank_grouped_biased,
pc_half_sq_norm_bias) and of inference.SimilarProducts, without a GPU: the header and the ctypes table, the workspace queries,
what the entries refuse before anything is launched, and the argument checks of the wrappers and the class that need no device."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

PC_EINVAL, PC_ESHAPE, PC_EWORKSPACE = -1, -2, -3
ENTRIES = ("pc_half_sq_norm_bias", "pc_retrieve_topk_grouped_biased", "pc_retrieve_topk_grouped_biased_workspace_bytes",
           "pc_rank_grouped_biased", "pc_rank_grouped_biased_workspace_bytes")


def test_header_declares_the_entries_and_the_abi_stays_8():
    from p_companion_amd import _lib
    txt = open(os.path.join(ROOT, "include", "pcompanion_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES
    assert len(re.findall(r"const\s+float\s*\*\s*bias\b", code)) >= 2
    assert re.search(r"#define\s+PC_ABI_VERSION\s+8\b", txt)
    sig = _lib.SIGNATURES
    vp = ctypes.c_void_p
    # the neighbouring entries' argument lists with the bias pointer behind the table
    ret, args = sig["pc_retrieve_topk_grouped_bf16"]
    assert sig["pc_retrieve_topk_grouped_biased"] == (ret, args[:7] + [vp] + args[7:])
    ret, args = sig["pc_rank_grouped_excluding"]
    assert sig["pc_rank_grouped_biased"] == (ret, args[:8] + [vp] + args[8:])
    assert sig["pc_retrieve_topk_grouped_biased_workspace_bytes"] == sig["pc_retrieve_topk_grouped_workspace_bytes"]
    assert sig["pc_rank_grouped_biased_workspace_bytes"] == sig["pc_rank_grouped_workspace_bytes"]
    L = _lib.lib()
    assert L.pc_abi_version() == 8
    assert L.pc_retrieve_topk_grouped_biased_workspace_bytes.restype == ctypes.c_size_t
    assert L.pc_rank_grouped_biased_workspace_bytes.restype == ctypes.c_size_t


def test_the_unit_is_part_of_the_build():
    from p_companion_amd import build
    assert "nearest.hip" in build.sources()


def test_workspace_bytes_depend_on_the_plan_only():
    from p_companion_amd import _lib
    L = _lib.lib()
    ws = L.pc_retrieve_topk_grouped_biased_workspace_bytes
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
    for n, s in ((1, 1), (10, 0), (16, 64)):                            # the unbiased entry's plan and partial lists
        assert ws(rows, types, n, s) == L.pc_retrieve_topk_grouped_workspace_bytes(rows, types, n, s)
    rk = L.pc_rank_grouped_biased_workspace_bytes
    for s in (0, 1, 64):                                                # the plan alone: no partial lists, whatever the slices
        assert rk(rows, types, s) == L.pc_rank_grouped_workspace_bytes(rows, types, s) == rk(rows, types, 0) > 0
    assert rk(rows, 34_800, 0) > rk(rows, types, 0)
    for bad in ((0, types, 0), (rows, 0, 0), (rows, types, -1), (rows, types, 65)):
        assert rk(*bad) == 0, bad


def _aligned():
    """One 16-byte aligned host buffer: a pointer that passes every check, and that no check dereferences."""
    buf = ctypes.create_string_buffer(96)
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)


def test_the_retrieval_refuses_before_anything_is_launched():
    from p_companion_amd import _lib
    entry = _lib.lib().pc_retrieve_topk_grouped_biased
    buf, p = _aligned()

    def call(**kw):
        a = dict(proj=p, types=p, row_key=p, rows=4, type_rowptr=p, type_col=p, table=p, bias=p, n_types=3, ex_rowptr=p,
                 ex_col=p, n_keys=2, n=10, dim=128, slices=0, out_idx=p, out_score=p, bad_count=p, ws=p, ws_bytes=0, stream=None)
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
    for kw in (dict(n=0), dict(n=17), dict(dim=64), dict(dim=192), dict(slices=-1), dict(slices=65)):
        assert call(**kw) == PC_ESHAPE, kw
        assert call(**kw, **none) == PC_ESHAPE, kw
    assert call() == PC_EWORKSPACE and call(**none) == PC_EWORKSPACE and call(n=16, dim=256, **none) == PC_EWORKSPACE


def test_the_rank_refuses_before_anything_is_launched():
    from p_companion_amd import _lib
    entry = _lib.lib().pc_rank_grouped_biased
    buf, p = _aligned()

    def call(**kw):
        a = dict(proj=p, types=p, targets=p, row_key=p, rows=4, type_rowptr=p, type_col=p, table=p, bias=p, n_types=3,
                 num_products=9, ex_rowptr=p, ex_col=p, n_keys=2, cand_type=p, dim=128, slices=0, rank_out=p, bad_count=p, ws=p,
                 ws_bytes=0, stream=None)
        a.update(kw)
        return entry(*a.values())

    for name in ("proj", "types", "targets", "type_rowptr", "type_col", "table", "bias", "rank_out", "bad_count", "ws", "row_key",
                 "ex_rowptr", "ex_col", "cand_type"):
        assert call(**{name: None}) == PC_EINVAL, name
    for kw in (dict(rows=0), dict(n_types=0), dict(num_products=0), dict(n_keys=-1)):
        assert call(**kw) == PC_EINVAL, kw
    none = dict(row_key=None, ex_rowptr=None, ex_col=None, n_keys=0, cand_type=None)
    # the exclusion triple and cand_type: all or none
    for half in (dict(none, cand_type=p), dict(none, ex_rowptr=p), dict(none, ex_col=p), dict(none, n_keys=2)):
        assert call(**half) == PC_EINVAL, half
    for kw in (dict(dim=64), dict(dim=192), dict(slices=-1), dict(slices=65)):
        assert call(**kw) == PC_ESHAPE, kw
        assert call(**kw, **none) == PC_ESHAPE, kw
    assert call() == PC_EWORKSPACE and call(**none) == PC_EWORKSPACE and call(dim=256, slices=64, **none) == PC_EWORKSPACE


def test_the_bias_entry_refuses_before_anything_is_launched():
    from p_companion_amd import _lib
    entry = _lib.lib().pc_half_sq_norm_bias
    buf, p = _aligned()
    assert entry(None, 4, 128, p, None) == PC_EINVAL and entry(p, 4, 128, None, None) == PC_EINVAL
    assert entry(p, 0, 128, p, None) == PC_EINVAL and entry(p, -3, 256, p, None) == PC_EINVAL
    for dim in (0, 64, 192, 512):
        assert entry(p, 4, dim, p, None) == PC_ESHAPE, dim


class OnDevice(torch.Tensor):
    """A stand-in that reports is_cuda: _req tests the device first, and this lets the checks behind it be reached."""
    is_cuda = True


def test_the_wrappers_refuse_cpu_tensors_and_an_unsupported_bias():
    from p_companion_amd import ops
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)
    proj, table, bias = torch.zeros(4, 128), torch.zeros(5, 128), torch.zeros(5)
    with pytest.raises(TypeError, match="CUDA/ROCm"):
        ops.half_sq_norm_bias(table)
    with pytest.raises(TypeError, match="float32"):
        ops.half_sq_norm_bias(torch.zeros(5, 128, dtype=torch.float64).as_subclass(OnDevice))
    with pytest.raises(ValueError, match=r"\[P, D\]"):
        ops.half_sq_norm_bias(torch.zeros(128).as_subclass(OnDevice))
    with pytest.raises(ValueError, match="width"):
        ops.half_sq_norm_bias(torch.zeros(5, 64).as_subclass(OnDevice))
    retrieve = lambda **kw: ops.retrieve_topk_grouped(proj, i32(4), i32(3), i32(5), kw.pop("table", table), 5, **kw)
    rank = lambda **kw: ops.rank_grouped(proj, i32(4), i32(4), i32(3), i32(5), kw.pop("table", table), **kw)
    for fn in (retrieve, rank):
        # a well-formed bias: the call goes on to the device check of its tensors
        with pytest.raises(TypeError, match="CUDA/ROCm"):
            fn(bias=bias)
        # the refusals of the bias itself: ValueError, naming what is unsupported, whatever else the call holds
        with pytest.raises(ValueError, match="bf16 table"):
            fn(bias=bias, table=torch.zeros(5, 128, dtype=torch.bfloat16))
        for dtype in (torch.float64, torch.float16, torch.bfloat16, torch.int32):
            with pytest.raises(ValueError, match="float32"):
                fn(bias=bias.to(dtype))
        for shape in ((4,), (6,), (5, 1), (1, 5), ()):
            with pytest.raises(ValueError, match="one entry per product"):
                fn(bias=torch.zeros(shape))
        with pytest.raises(ValueError, match="bias must be"):
            fn(bias=[0.0] * 5)
    # the exclusion checks are the unbiased call's
    with pytest.raises(ValueError, match="exclude"):
        retrieve(bias=bias, exclude=(i32(4).long(), i32(3), i32(0)))
    with pytest.raises(ValueError, match="cand_type"):
        rank(bias=bias, exclude=(i32(4), i32(3), i32(0)))
    with pytest.raises(ValueError, match="cand_type"):
        rank(bias=bias, cand_type=i32(5))
    # lists above 16 take no bias
    with pytest.raises(TypeError, match="bias"):
        ops.retrieve_list_grouped(proj, i32(4), i32(3), i32(5), table, 20, bias=bias)


class Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"read .{name} before refusing")


def test_similar_products_refuses_a_bad_table_before_the_graph_is_touched():
    from p_companion_amd.inference import SimilarProducts
    for bad, what in ((torch.zeros(7, 128, dtype=torch.bfloat16), "float32"), (torch.zeros(7, 128, dtype=torch.float64), "float32"),
                      ([[0.0] * 128] * 7, "float32"), (torch.zeros(7, 64), r"\[P, 128 or 256\]"),
                      (torch.zeros(7 * 128), r"\[P, 128 or 256\]"), (torch.zeros(0, 128), r"\[P, 128 or 256\]"),
                      (torch.zeros(7, 128), "device tensor")):
        with pytest.raises(ValueError, match=what):
            SimilarProducts(bad, Untouchable())
    with pytest.raises(ValueError, match="scope"):
        SimilarProducts(torch.zeros(7, 128), Untouchable(), scope="category")


def test_similar_batch_refuses_more_than_16_before_anything_is_touched():
    from p_companion_amd.inference import SimilarProducts
    sp = object.__new__(SimilarProducts)                              # (no table, no graph, no device)
    sp.__dict__.update(table=Untouchable(), bpg=Untouchable(), exclusions=Untouchable())
    q = torch.zeros(2, dtype=torch.int32)
    for n in (17, 100, 0, -1):
        with pytest.raises(ValueError, match="1 to 16"):
            sp.similar_batch(q, n)


def test_the_serving_classes_share_their_filters():
    """set_exclusions / set_eligible are one implementation for both classes, not a copy."""
    from p_companion_amd.inference import PCompanionInference, SimilarProducts
    for name in ("set_exclusions", "set_eligible", "_excluded"):
        assert getattr(PCompanionInference, name) is getattr(SimilarProducts, name), name
