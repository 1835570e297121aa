"""The host side of the session recommendations (pc_fuse_sessions; ops.fuse_sessions;
PCompanionInference.recommend_session_batch), without a GPU: the header and the ctypes table, what the entry refuses before
anything is launched, and the argument checks of the wrapper and the method that need no device."""
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
    assert re.search(r"\bint\s+pc_fuse_sessions\s*\(", code)
    assert re.search(r"#define\s+PC_ABI_VERSION\s+8\b", txt)
    # the declaration, argument by argument, against the ctypes table
    decl = re.search(r"\bint\s+pc_fuse_sessions\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
    args = [" ".join(a.split()) for a in decl.split(",")]
    assert args == ["const int32_t *idx", "const float *score", "const int32_t *source", "const float *weight",
                    "const int32_t *seg_rowptr", "int rows", "int sessions", "int w", "int max_items",
                    "const int32_t *ex_rowptr", "const int32_t *ex_col", "int num_products", "int n", "int combine",
                    "int32_t *out_idx", "float *out_score", "int32_t *out_support", "int32_t *bad_count",
                    "int32_t *truncated_count", "void *stream"]
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert _lib.SIGNATURES["pc_fuse_sessions"] == (i, [vp if "*" in a else i for a in args])
    L = _lib.lib()
    assert L.pc_abi_version() == 8
    assert L.pc_fuse_sessions.argtypes == _lib.SIGNATURES["pc_fuse_sessions"][1] and L.pc_fuse_sessions.restype == i
    # the parent entry's line in the table is what it was
    assert _lib.SIGNATURES["pc_fuse_lists"] == (i, [vp, vp, vp, i, i, i, vp, vp, i, i, i, vp, vp, vp, vp, vp])
    # the contract stands in the header and above the kernel
    for path in (os.path.join(ROOT, "include", "pcompanion_hip.h"),
                 os.path.join(ROOT, "p_companion_amd", "csrc", "fuse_sessions.hip")):
        words = " ".join(w for w in open(path).read().split() if w not in ("//", "*"))       # (across the comment's lines)
        for phrase in ("the largest first", "ban set", "support", "live rows", "offering row", "never contracted with an addition",
                       "subnormal range are outside the contract", "an overflowed term is no candidate", "truncated_count",
                       "one truncation status"):
            assert phrase in words, (path, phrase)


def test_the_unit_is_part_of_the_build():
    from p_companion_amd import build
    assert "fuse_sessions.hip" in build.sources() and "fuse_lists.hip" in build.sources()


def _aligned():
    """One 16-byte aligned host buffer: a pointer that passes every check, and that no check dereferences."""
    buf = ctypes.create_string_buffer(96)
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)


def test_the_entry_refuses_before_anything_is_launched():
    from p_companion_amd import _lib
    entry = _lib.lib().pc_fuse_sessions
    buf, p = _aligned()
    buf.raw = b"\x5a" * 96                                 # pre-filled: a refusal writes through no pointer
    before = buf.raw

    def call(**kw):
        a = dict(idx=p, score=p, source=p, weight=p, seg_rowptr=p, rows=12, sessions=3, w=5, max_items=0, ex_rowptr=p, ex_col=p,
                 num_products=7, n=5, combine=0, out_idx=p, out_score=p, out_support=p, bad=p, truncated=p, stream=None)
        a.update(kw)
        return entry(*a.values())

    refused = (dict(rows=-1), dict(sessions=-1), dict(w=0), dict(w=-2), dict(w=1025), dict(w=2 ** 31 - 1),
               dict(n=0), dict(n=-1), dict(n=257), dict(max_items=-1), dict(max_items=-2 ** 31),
               dict(num_products=0), dict(num_products=-1), dict(combine=2), dict(combine=-1),
               dict(idx=None), dict(score=None), dict(seg_rowptr=None), dict(out_idx=None), dict(out_score=None),
               dict(out_support=None),
               dict(ex_rowptr=None), dict(ex_col=None),                                               # half an exclusion set
               dict(source=None), dict(source=None, bad=None, truncated=None))                        # ... a set without sources
    for kw in refused:
        assert call(**kw) == PC_ESHAPE, kw
        assert call(**kw, stream=ctypes.c_void_p(1)) == PC_ESHAPE, kw           # (... whatever the stream: it is never used)
    # no sessions: success without a launch, whatever the pointers -- but a refused shape is refused first
    assert call(sessions=0) == 0 and call(sessions=0, ex_rowptr=None, ex_col=None) == 0
    assert call(sessions=0, source=None, weight=None, ex_rowptr=None, ex_col=None, combine=1) == 0
    assert call(sessions=0, idx=None, score=None, source=None, weight=None, seg_rowptr=None, ex_rowptr=None, ex_col=None,
                out_idx=None, out_score=None, out_support=None, bad=None, truncated=None) == 0
    assert call(sessions=0, w=1024, n=256, max_items=2 ** 31 - 1) == 0 and call(sessions=0, rows=0, w=1, n=1) == 0
    for kw in (dict(w=1025), dict(n=257), dict(combine=2), dict(num_products=0), dict(source=None), dict(ex_col=None),
               dict(max_items=-1), dict(rows=-1)):
        assert call(sessions=0, **kw) == PC_ESHAPE, kw
    assert buf.raw == before                               # nothing was written: not an output, not a counter


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
    assert ops.FUSE_SESSIONS_MAX_POOL == 1024 and ops.FUSE_SESSIONS_MAX_N == 256
    sig = inspect.signature(ops.fuse_sessions)
    assert list(sig.parameters) == ["idx", "score", "seg_rowptr", "n", "combine", "source", "weight", "exclude", "num_products",
                                    "max_items", "bad", "truncated"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[4:]] == ["sum"] + [None] * 7
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    idx, sc, ptr, source, wt, ex = i32(12, 20), torch.zeros(12, 20), i32(5), i32(12), torch.ones(12), (i32(8), i32(5))
    # CPU tensors are refused, argument by argument
    with pytest.raises(TypeError, match="idx: expected a CUDA/ROCm"):
        ops.fuse_sessions(idx, dev(sc), dev(ptr), 5)
    with pytest.raises(TypeError, match="score: expected a CUDA/ROCm"):
        ops.fuse_sessions(dev(idx), sc, dev(ptr), 5)
    with pytest.raises(TypeError, match="seg_rowptr: expected a CUDA/ROCm"):
        ops.fuse_sessions(dev(idx), dev(sc), ptr, 5)
    with pytest.raises(TypeError, match="source: expected a CUDA/ROCm"):
        ops.fuse_sessions(dev(idx), dev(sc), dev(ptr), 5, source=source)
    with pytest.raises(TypeError, match="weight: expected a CUDA/ROCm"):
        ops.fuse_sessions(dev(idx), dev(sc), dev(ptr), 5, weight=wt)
    with pytest.raises(TypeError, match="ex_rowptr: expected a CUDA/ROCm"):
        ops.fuse_sessions(dev(idx), dev(sc), dev(ptr), 5, source=dev(source), exclude=(ex[0], dev(ex[1])))
    with pytest.raises(TypeError, match="ex_col: expected a CUDA/ROCm"):
        ops.fuse_sessions(dev(idx), dev(sc), dev(ptr), 5, source=dev(source), exclude=(dev(ex[0]), ex[1]))
    with pytest.raises(TypeError, match="bad: expected a CUDA/ROCm"):
        ops.fuse_sessions(dev(idx), dev(sc), dev(ptr), 5, bad=i32(1))
    with pytest.raises(TypeError, match="truncated: expected a CUDA/ROCm"):
        ops.fuse_sessions(dev(idx), dev(sc), dev(ptr), 5, truncated=i32(1))
    call = lambda **kw: ops.fuse_sessions(dev(kw.pop("idx", idx)), dev(kw.pop("score", sc)), dev(kw.pop("seg_rowptr", ptr)),
                                          kw.pop("n", 5), **kw)
    # dtypes and shapes
    with pytest.raises(TypeError, match="idx: expected torch.int32"):
        call(idx=idx.long())
    with pytest.raises(TypeError, match="score: expected torch.float32"):
        call(score=sc.double())
    with pytest.raises(TypeError, match="seg_rowptr: expected torch.int32"):
        call(seg_rowptr=ptr.long())
    for bad_idx, bad_sc in ((i32(240), torch.zeros(240)), (idx, torch.zeros(12, 21)), (idx, torch.zeros(20, 12)),
                            (i32(4, 3, 20), torch.zeros(4, 3, 20))):
        with pytest.raises(ValueError, match=r"one shape \[R, w\]"):
            call(idx=bad_idx, score=bad_sc)
    for w in (0, 1025):
        with pytest.raises(ValueError, match=r"row width w must be in \[1, 1024\], got %d" % w):
            call(idx=i32(2, w), score=torch.zeros(2, w))
    for bad_ptr in (i32(0), i32(2, 3)):
        with pytest.raises(ValueError, match=r"seg_rowptr \[B \+ 1\]"):
            call(seg_rowptr=bad_ptr)
    for n in (0, -1, 257):
        with pytest.raises(ValueError, match=r"n must be in \[1, 256\], got %d" % n):
            call(n=n)
    for combine in ("mean", "Sum", None, 0):
        with pytest.raises(ValueError, match="combine must be 'sum' or 'max'"):
            call(combine=combine)
    # source and weight: one entry per row
    with pytest.raises(ValueError, match="source must be"):
        call(source=[0] * 12)
    with pytest.raises(TypeError, match="source: expected torch.int32"):
        call(source=dev(source.long()))
    for shape in ((11,), (12, 1), (4, 3)):
        with pytest.raises(ValueError, match=r"source: expected shape \(12,\)"):
            call(source=dev(i32(*shape)))
    with pytest.raises(ValueError, match="weight must be"):
        call(weight=[1.0] * 12)
    with pytest.raises(TypeError, match="weight: expected torch.float32"):
        call(weight=dev(wt.double()))
    for shape in ((11,), (12, 1), (4, 3)):
        with pytest.raises(ValueError, match=r"weight: expected shape \(12,\)"):
            call(weight=dev(torch.ones(*shape)))
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
    for cap in (-1, 2 ** 31):
        with pytest.raises(ValueError, match=r"max_items must be None or in \[0, 2\^31 - 1\]"):
            call(max_items=cap)
    with pytest.raises(TypeError, match="bad: expected torch.int32"):
        call(bad=dev(torch.zeros(1)))
    with pytest.raises(ValueError, match=r"bad: expected shape \(1,\)"):
        call(bad=dev(i32(2)))
    with pytest.raises(TypeError, match="truncated: expected torch.int32"):
        call(truncated=dev(torch.zeros(1)))
    with pytest.raises(ValueError, match=r"truncated: expected shape \(1,\)"):
        call(truncated=dev(i32(2)))
    # no sessions: empty outputs without a call (the library is still untouchable)
    out = call(seg_rowptr=i32(1), n=7, source=dev(source), weight=dev(wt), combine="max", max_items=3)
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


def test_recommend_session_batch_refuses_before_the_model_or_the_graph_is_touched():
    from p_companion_amd.inference import CompactInference, PCompanionInference
    sig = inspect.signature(PCompanionInference.recommend_session_batch)
    assert list(sig.parameters) == ["self", "items", "seg_rowptr", "num_recommendations", "per_item", "weight", "combine",
                                    "max_items"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[3:]] == [10, 8, None, "sum", None]
    assert CompactInference.recommend_session_batch is PCompanionInference.recommend_session_batch      # inherited, not restated
    # the basket method is what it was
    assert list(inspect.signature(PCompanionInference.recommend_basket_batch).parameters) == [
        "self", "basket", "num_recommendations", "per_item", "combine"]
    inf = _inference(k=3)
    items, ptr = torch.zeros(8, dtype=torch.int32), torch.tensor([0, 3, 3, 8], dtype=torch.int32)
    for bad in (items.long(), items.reshape(2, 4), items.float(), [0, 1]):
        with pytest.raises(ValueError, match=r"items must be a \[R\] int32 tensor"):
            inf.recommend_session_batch(bad, ptr)
    for bad in (ptr.long(), ptr.reshape(2, 2), torch.zeros(0, dtype=torch.int32), [0, 8]):
        with pytest.raises(ValueError, match=r"seg_rowptr must be a \[B \+ 1\] int32 tensor"):
            inf.recommend_session_batch(items, bad)
    for bad in (torch.ones(7), torch.ones(8, 1), torch.ones(8, dtype=torch.float64), [1.0] * 8):
        with pytest.raises(ValueError, match=r"weight must be a \[R = 8\] float32 tensor"):
            inf.recommend_session_batch(items, ptr, weight=bad)
    for per_item in (0, -1, 342, 1025):                                 # K per_item > 1024: 3 x 342 = 1026
        with pytest.raises(ValueError, match=r"K \* per_item <= 1024, got K = 3 and per_item %d" % per_item):
            inf.recommend_session_batch(items, ptr, 10, per_item=per_item)
    with pytest.raises(ValueError, match=r"K \* per_item <= 1024, got K = 5 and per_item 205"):
        _inference(k=5).recommend_session_batch(items, ptr, 10, per_item=205)
    for n in (0, -1, 257):
        with pytest.raises(ValueError, match=r"num_recommendations <= 256, got %d" % n):
            inf.recommend_session_batch(items, ptr, n)
    for combine in ("mean", None, 1):
        with pytest.raises(ValueError, match="combine must be 'sum' or 'max'"):
            inf.recommend_session_batch(items, ptr, combine=combine)
    with pytest.raises(ValueError, match="max_items must be None or at least 0"):
        inf.recommend_session_batch(items, ptr, max_items=-1)
    doc = " ".join(PCompanionInference.recommend_session_batch.__doc__.split())
    assert "repeat_interleave(length, output_size=R)" in doc and "Nothing is read back" in doc
    assert "no padding rows" in doc
    # a bare bf16 catalogue bounds per_item at what it serves: recommend_batch's own message, before the model runs
    inf.__dict__.update(device="cpu", type_idx=torch.zeros(9, dtype=torch.int32), compact=None,
                        catalogue=torch.zeros(9, 128, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="bf16 catalogue serves at most 16"):
        inf.recommend_session_batch(items, ptr, 10, per_item=17)


def test_the_recency_weights_of_the_docstring_are_what_it_says():
    """the one-liner on CPU tensors: weight 1 for a session's last item, halved per step back; empty sessions cost nothing"""
    seg_rowptr = torch.tensor([0, 3, 3, 4, 8], dtype=torch.int32)
    R = 8
    length = (seg_rowptr[1:] - seg_rowptr[:-1]).long()
    age = seg_rowptr[1:].repeat_interleave(length, output_size=R) - 1 - torch.arange(R, device=length.device)
    weight = torch.pow(0.5, age.float())
    assert weight.tolist() == [0.25, 0.5, 1.0, 1.0, 0.125, 0.25, 0.5, 1.0] and weight.dtype == torch.float32
