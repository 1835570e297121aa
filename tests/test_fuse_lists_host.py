"""The host side of the basket recommendations (pc_fuse_lists; ops.fuse_lists; PCompanionInference.recommend_basket_batch),
without a GPU: the header and the ctypes table, what the entry refuses before anything is launched, and the argument checks of
the wrapper and the method that need no device."""
import ctypes
import inspect
import os
import re
from types import SimpleNamespace

import pytest
import torch

from conftest import ROOT

PC_ESHAPE = -2


def test_header_declares_the_entry_and_the_abi_stays_8():
    from p_companion_amd import _lib
    txt = open(os.path.join(ROOT, "include", "pcompanion_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+pc_fuse_lists\s*\(", code)
    assert re.search(r"#define\s+PC_ABI_VERSION\s+8\b", txt)
    # the declaration, argument by argument, against the ctypes table
    decl = re.search(r"\bint\s+pc_fuse_lists\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
    args = [" ".join(a.split()) for a in decl.split(",")]
    assert args == ["const int32_t *idx", "const float *score", "const int32_t *source", "int baskets", "int sources", "int w",
                    "const int32_t *ex_rowptr", "const int32_t *ex_col", "int num_products", "int n", "int combine",
                    "int32_t *out_idx", "float *out_score", "int32_t *out_support", "int32_t *bad_count", "void *stream"]
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert _lib.SIGNATURES["pc_fuse_lists"] == (i, [vp if "*" in a else i for a in args])
    L = _lib.lib()
    assert L.pc_abi_version() == 8
    assert L.pc_fuse_lists.argtypes == _lib.SIGNATURES["pc_fuse_lists"][1] and L.pc_fuse_lists.restype == i
    # the contract stands in the header and above the kernel
    for path in (os.path.join(ROOT, "include", "pcompanion_hip.h"), os.path.join(ROOT, "p_companion_amd", "csrc", "fuse_lists.hip")):
        words = " ".join(w for w in open(path).read().split() if w not in ("//", "*"))       # (across the comment's lines)
        for phrase in ("the largest first", "ban set", "support"):
            assert phrase in words, (path, phrase)


def test_the_unit_is_part_of_the_build():
    from p_companion_amd import build
    assert "fuse_lists.hip" in build.sources()


def _aligned():
    """One 16-byte aligned host buffer: a pointer that passes every check, and that no check dereferences."""
    buf = ctypes.create_string_buffer(96)
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)


def test_the_entry_refuses_before_anything_is_launched():
    from p_companion_amd import _lib
    entry = _lib.lib().pc_fuse_lists
    buf, p = _aligned()

    def call(**kw):
        a = dict(idx=p, score=p, source=p, baskets=3, sources=4, w=5, ex_rowptr=p, ex_col=p, num_products=7, n=5, combine=0,
                 out_idx=p, out_score=p, out_support=p, bad=None, stream=None)
        a.update(kw)
        return entry(*a.values())

    refused = (dict(baskets=-1), dict(sources=0), dict(sources=-1), dict(w=0), dict(w=-2), dict(sources=1025, w=1),
               dict(sources=1, w=1025), dict(sources=33, w=32), dict(sources=2 ** 16, w=2 ** 16),       # (the product wraps an int)
               dict(n=0), dict(n=-1), dict(n=21), dict(sources=16, w=64, n=257), dict(sources=1, w=1, n=2),
               dict(num_products=0), dict(num_products=-1), dict(combine=2), dict(combine=-1),
               dict(idx=None), dict(score=None), dict(out_idx=None), dict(out_score=None), dict(out_support=None),
               dict(ex_rowptr=None), dict(ex_col=None),                                               # half an exclusion set
               dict(source=None), dict(source=None, bad=p))                                           # ... a set without sources
    for kw in refused:
        assert call(**kw) == PC_ESHAPE, kw
        assert call(**kw, stream=ctypes.c_void_p(1)) == PC_ESHAPE, kw           # (... whatever the stream: it is never used)
    # no baskets: success without a launch, whatever the pointers -- but a refused shape is refused first
    assert call(baskets=0) == 0 and call(baskets=0, ex_rowptr=None, ex_col=None) == 0
    assert call(baskets=0, source=None, ex_rowptr=None, ex_col=None, combine=1) == 0
    assert call(baskets=0, idx=None, score=None, source=None, ex_rowptr=None, ex_col=None, out_idx=None, out_score=None,
                out_support=None) == 0
    assert call(baskets=0, sources=16, w=64, n=256) == 0 and call(baskets=0, sources=1, w=1, n=1) == 0
    for kw in (dict(sources=1025, w=1), dict(n=21), dict(combine=2), dict(num_products=0), dict(source=None), dict(ex_col=None)):
        assert call(baskets=0, **kw) == PC_ESHAPE, kw


class OnDevice(torch.Tensor):
    """A stand-in that reports is_cuda: _req tests the device first, and this lets the checks behind it be reached."""
    is_cuda = True


def dev(t):
    return t.as_subclass(OnDevice)


def test_the_wrapper_checks_its_arguments_before_the_library_is_touched(monkeypatch):
    from p_companion_amd import _lib, ops

    def untouched():
        raise AssertionError("the library was touched before the arguments were refused")

    monkeypatch.setattr(_lib, "lib", untouched)
    assert ops.FUSE_LISTS_MAX_POOL == 1024
    sig = inspect.signature(ops.fuse_lists)
    assert list(sig.parameters) == ["idx", "score", "n", "combine", "source", "exclude", "num_products", "bad"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[3:]] == ["sum", None, None, None, None]
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    idx, sc, source, ex = i32(4, 3, 20), torch.zeros(4, 3, 20), i32(4, 3), (i32(8), i32(5))
    # CPU tensors are refused, argument by argument
    with pytest.raises(TypeError, match="idx: expected a CUDA/ROCm"):
        ops.fuse_lists(idx, dev(sc), 5)
    with pytest.raises(TypeError, match="score: expected a CUDA/ROCm"):
        ops.fuse_lists(dev(idx), sc, 5)
    with pytest.raises(TypeError, match="source: expected a CUDA/ROCm"):
        ops.fuse_lists(dev(idx), dev(sc), 5, source=source)
    with pytest.raises(TypeError, match="ex_rowptr: expected a CUDA/ROCm"):
        ops.fuse_lists(dev(idx), dev(sc), 5, source=dev(source), exclude=(ex[0], dev(ex[1])))
    with pytest.raises(TypeError, match="ex_col: expected a CUDA/ROCm"):
        ops.fuse_lists(dev(idx), dev(sc), 5, source=dev(source), exclude=(dev(ex[0]), ex[1]))
    with pytest.raises(TypeError, match="bad: expected a CUDA/ROCm"):
        ops.fuse_lists(dev(idx), dev(sc), 5, bad=i32(1))
    call = lambda **kw: ops.fuse_lists(dev(kw.pop("idx", idx)), dev(kw.pop("score", sc)), kw.pop("n", 5), **kw)
    # dtypes and shapes
    with pytest.raises(TypeError, match="idx: expected torch.int32"):
        call(idx=idx.long())
    with pytest.raises(TypeError, match="score: expected torch.float32"):
        call(score=sc.double())
    for bad_idx, bad_sc in ((i32(4, 60), torch.zeros(4, 60)), (idx, torch.zeros(4, 3, 21)), (idx, torch.zeros(4, 20, 3)),
                            (i32(2, 2, 3, 20), torch.zeros(2, 2, 3, 20))):
        with pytest.raises(ValueError, match=r"one shape \[B, S, w\]"):
            call(idx=bad_idx, score=bad_sc)
    for s, w in ((1025, 1), (1, 1025), (33, 32), (0, 5), (5, 0)):
        with pytest.raises(ValueError, match=r"pool S \* w must be in \[1, 1024\], got %d \* %d" % (s, w)):
            call(idx=i32(2, s, w), score=torch.zeros(2, s, w))
    for n in (0, -1, 61, 256):
        with pytest.raises(ValueError, match=r"n must be in \[1, min\(S \* w, 256\) = 60\], got %d" % n):
            call(n=n)
    with pytest.raises(ValueError, match=r"n must be in \[1, min\(S \* w, 256\) = 256\], got 257"):
        call(idx=i32(2, 16, 64), score=torch.zeros(2, 16, 64), n=257)
    for combine in ("mean", "Sum", None, 0):
        with pytest.raises(ValueError, match="combine must be 'sum' or 'max'"):
            call(combine=combine)
    # source: int32, one entry per row
    with pytest.raises(ValueError, match="source must be"):
        call(source=[[0] * 3] * 4)
    with pytest.raises(TypeError, match="source: expected torch.int32"):
        call(source=dev(source.long()))
    for shape in ((4,), (3, 4), (4, 3, 1), (5, 3)):
        with pytest.raises(ValueError, match=r"source: expected shape \(4, 3\)"):
            call(source=dev(i32(*shape)))
    # exclude: needs source, a pair of int32 tensors, keyed by the products
    with pytest.raises(ValueError, match="exclude .* needs source"):
        call(exclude=(dev(ex[0]), dev(ex[1])))
    for pair in (dev(ex[0]), (dev(ex[0]),), (dev(ex[0]), None), [1, 2]):
        with pytest.raises(ValueError, match=r"exclude must be the pair"):
            call(source=dev(source), exclude=pair)
    with pytest.raises(TypeError, match="ex_rowptr: expected torch.int32"):
        call(source=dev(source), exclude=(dev(ex[0].long()), dev(ex[1])))
    with pytest.raises(TypeError, match="ex_col: expected torch.int32"):
        call(source=dev(source), exclude=(dev(ex[0]), dev(ex[1].long())))
    for rowptr, col in ((i32(1), i32(5)), (i32(2, 4), i32(5)), (i32(8), i32(5, 1))):
        with pytest.raises(ValueError, match=r"ex_rowptr \[P \+ 1\]"):
            call(source=dev(source), exclude=(dev(rowptr), dev(col)))
    with pytest.raises(ValueError, match="num_products 9 does not match the exclusion set's 7 keys"):
        call(source=dev(source), exclude=(dev(ex[0]), dev(ex[1])), num_products=9)
    for p in (0, -1, 2 ** 31):
        with pytest.raises(ValueError, match=r"num_products must be in \[1, 2\^31 - 1\]"):
            call(num_products=p)
    with pytest.raises(TypeError, match="bad: expected torch.int32"):
        call(bad=dev(torch.zeros(1)))
    with pytest.raises(ValueError, match=r"bad: expected shape \(1,\)"):
        call(bad=dev(i32(2)))
    # no baskets: empty outputs without a call (the library is still untouchable)
    out = call(idx=i32(0, 3, 20), score=torch.zeros(0, 3, 20), n=7, source=dev(i32(0, 3)), combine="max")
    assert [tuple(t.shape) for t in out] == [(0, 7)] * 3
    assert [t.dtype for t in out] == [torch.int32, torch.float32, torch.int32]


class Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"read .{name} before refusing")


def _inference(k=3):
    from p_companion_amd.inference import PCompanionInference
    inf = object.__new__(PCompanionInference)                          # (no graph, no model, no device)
    inf.__dict__.update(model=Untouchable(), bpg=Untouchable(), features=Untouchable(), _graph=Untouchable(),
                        exclusions=Untouchable(), type_idx=Untouchable(), config=SimpleNamespace(NUM_COMP_TYPES=k))
    return inf


def test_recommend_basket_batch_refuses_before_the_model_or_the_graph_is_touched():
    from p_companion_amd.inference import CompactInference, PCompanionInference
    sig = inspect.signature(PCompanionInference.recommend_basket_batch)
    assert list(sig.parameters) == ["self", "basket", "num_recommendations", "per_item", "combine"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [10, 8, "sum"]
    assert CompactInference.recommend_basket_batch is PCompanionInference.recommend_basket_batch         # inherited, not restated
    inf = _inference(k=3)
    basket = torch.zeros(2, 4, dtype=torch.int32)
    for bad in (basket.long(), basket.reshape(-1), basket.reshape(2, 2, 2), torch.zeros(2, 0, dtype=torch.int32), [[0, 1]]):
        with pytest.raises(ValueError, match=r"basket must be a \[B, I\] int32 tensor"):
            inf.recommend_basket_batch(bad)
    for per_item in (0, -1, 86, 1024):                                  # I K per_item > 1024: 4 x 3 x 86 = 1032
        with pytest.raises(ValueError, match=r"I \* K \* per_item <= 1024, got I = 4, K = 3 and per_item %d" % per_item):
            inf.recommend_basket_batch(basket, 10, per_item=per_item)
    with pytest.raises(ValueError, match=r"I \* K \* per_item <= 1024, got I = 4, K = 5 and per_item 52"):
        _inference(k=5).recommend_basket_batch(basket, 10, per_item=52)
    for n, per_item, most in ((0, 8, 96), (-1, 8, 96), (97, 8, 96), (13, 1, 12), (257, 85, 256), (300, 40, 256)):
        with pytest.raises(ValueError, match=r"num_recommendations <= min\(I \* K \* per_item, 256\) = %d, got %d" % (most, n)):
            inf.recommend_basket_batch(basket, n, per_item=per_item)
    for combine in ("mean", None, 1):
        with pytest.raises(ValueError, match="combine must be 'sum' or 'max'"):
            inf.recommend_basket_batch(basket, 10, combine=combine)
    doc = " ".join(PCompanionInference.recommend_basket_batch.__doc__.split())
    assert "bucket baskets by length" in doc and "Nothing is read back" in doc
    # a bare bf16 catalogue bounds per_item at what it serves: recommend_batch's own message, before the model runs
    inf.__dict__.update(device="cpu", type_idx=torch.zeros(9, dtype=torch.int32), compact=None,
                        catalogue=torch.zeros(9, 128, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="bf16 catalogue serves at most 16"):
        inf.recommend_basket_batch(basket, 10, per_item=17)
