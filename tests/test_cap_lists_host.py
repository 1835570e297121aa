"""The host side of the group caps and the merged page (pc_cap_lists; ops.cap_lists; PCompanionInference.recommend_capped_batch /
recommend_page_batch; SimilarProducts.similar_capped_batch), without a GPU: the header and the ctypes table, what the entry
refuses before anything is launched, and the argument checks of the wrapper and the three methods that need no device."""
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
    assert re.search(r"\bint\s+pc_cap_lists\s*\(", code)
    assert re.search(r"#define\s+PC_ABI_VERSION\s+8\b", txt)
    # the declaration, argument by argument, against the ctypes table
    decl = re.search(r"\bint\s+pc_cap_lists\s*\((.*?)\)\s*;", code, flags=re.S).group(1)
    args = [" ".join(a.split()) for a in decl.split(",")]
    assert args == ["const int32_t *idx", "const float *score", "int rows", "int m", "const int32_t *group",
                    "const int32_t *row_ban", "int num_products", "int n", "int cap", "int32_t *out_idx", "float *out_score",
                    "int32_t *bad_count", "void *stream"]
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert _lib.SIGNATURES["pc_cap_lists"] == (i, [vp if "*" in a else i for a in args])
    L = _lib.lib()
    assert L.pc_abi_version() == 8
    assert L.pc_cap_lists.argtypes == _lib.SIGNATURES["pc_cap_lists"][1] and L.pc_cap_lists.restype == i


def test_the_unit_is_part_of_the_build():
    from p_companion_amd import build
    assert "cap_lists.hip" in build.sources()


def _aligned():
    """One 16-byte aligned host buffer: a pointer that passes every check, and that no check dereferences."""
    buf = ctypes.create_string_buffer(96)
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)


def test_the_entry_refuses_before_anything_is_launched():
    from p_companion_amd import _lib
    entry = _lib.lib().pc_cap_lists
    buf, p = _aligned()

    def call(**kw):
        a = dict(idx=p, score=p, rows=3, m=20, group=p, row_ban=p, num_products=7, n=5, cap=1, out_idx=p, out_score=p, bad=None,
                 stream=None)
        a.update(kw)
        return entry(*a.values())

    for kw in (dict(rows=-1), dict(m=0), dict(m=-1), dict(m=257), dict(n=0), dict(n=-1), dict(n=21), dict(m=256, n=257),
               dict(cap=0), dict(cap=-3), dict(num_products=0), dict(num_products=-1), dict(idx=None), dict(score=None),
               dict(out_idx=None), dict(out_score=None), dict(group=None), dict(group=None, bad=p)):      # (row_ban without group)
        assert call(**kw) == PC_ESHAPE, kw
        assert call(**kw, stream=ctypes.c_void_p(1)) == PC_ESHAPE, kw           # (... whatever the stream: it is never used)
    # no rows: success without a launch, whatever the pointers -- but a refused shape is refused first
    assert call(rows=0) == 0 and call(rows=0, group=None, row_ban=None) == 0
    assert call(rows=0, idx=None, score=None, out_idx=None, out_score=None, group=None, row_ban=None) == 0
    for kw in (dict(m=257), dict(n=21), dict(cap=0), dict(num_products=0), dict(group=None)):
        assert call(rows=0, **kw) == PC_ESHAPE, kw


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
    assert ops.CAP_LISTS_MAX_POOL == 256
    sig = inspect.signature(ops.cap_lists)
    assert list(sig.parameters) == ["idx", "score", "n", "group", "cap", "row_ban", "bad"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[3:]] == [None, 1, None, None]
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    idx, sc, group = i32(4, 20), torch.zeros(4, 20), i32(7)
    # CPU tensors are refused, argument by argument
    with pytest.raises(TypeError, match="idx: expected a CUDA/ROCm"):
        ops.cap_lists(idx, dev(sc), 5)
    with pytest.raises(TypeError, match="score: expected a CUDA/ROCm"):
        ops.cap_lists(dev(idx), sc, 5)
    with pytest.raises(TypeError, match="group: expected a CUDA/ROCm"):
        ops.cap_lists(dev(idx), dev(sc), 5, group=group)
    with pytest.raises(TypeError, match="row_ban: expected a CUDA/ROCm"):
        ops.cap_lists(dev(idx), dev(sc), 5, group=dev(group), row_ban=i32(4))
    with pytest.raises(TypeError, match="bad: expected a CUDA/ROCm"):
        ops.cap_lists(dev(idx), dev(sc), 5, bad=i32(1))
    call = lambda **kw: ops.cap_lists(dev(kw.pop("idx", idx)), dev(kw.pop("score", sc)), kw.pop("n", 5), **kw)
    # dtypes and shapes
    with pytest.raises(TypeError, match="idx: expected torch.int32"):
        call(idx=idx.long())
    with pytest.raises(TypeError, match="score: expected torch.float32"):
        call(score=sc.double())
    for bad_idx, bad_sc in ((i32(80), torch.zeros(80)), (idx, torch.zeros(4, 21)), (idx, torch.zeros(5, 20)),
                            (i32(2, 2, 20), torch.zeros(2, 2, 20))):
        with pytest.raises(ValueError, match=r"one shape \[R, m\]"):
            call(idx=bad_idx, score=bad_sc)
    with pytest.raises(ValueError, match=r"pool m must be in \[1, 256\], got 257"):
        call(idx=i32(2, 257), score=torch.zeros(2, 257))
    with pytest.raises(ValueError, match=r"pool m must be in \[1, 256\], got 0"):
        call(idx=i32(2, 0), score=torch.zeros(2, 0))
    for n in (0, -1, 21, 256):
        with pytest.raises(ValueError, match=r"n must be in \[1, m = 20\], got %d" % n):
            call(n=n)
    for cap in (0, -1):
        with pytest.raises(ValueError, match="cap must be at least 1, got %d" % cap):
            call(cap=cap, group=dev(group))
        with pytest.raises(ValueError, match="cap must be at least 1"):
            call(cap=cap)
    with pytest.raises(ValueError, match="group must be"):
        call(group=[0] * 7)
    with pytest.raises(TypeError, match="group: expected torch.int32"):
        call(group=dev(group.long()))
    for shape in ((0,), (7, 1), ()):
        with pytest.raises(ValueError, match=r"group must be \[P\]"):
            call(group=dev(i32(*shape) if shape else torch.zeros((), dtype=torch.int32)))
    # row_ban: needs group, int32, one entry per row
    with pytest.raises(ValueError, match="row_ban .* needs group"):
        call(row_ban=dev(i32(4)))
    with pytest.raises(ValueError, match="row_ban must be"):
        call(group=dev(group), row_ban=[0] * 4)
    with pytest.raises(TypeError, match="row_ban: expected torch.int32"):
        call(group=dev(group), row_ban=dev(i32(4).long()))
    for shape in ((3,), (5,), (4, 1)):
        with pytest.raises(ValueError, match=r"row_ban: expected shape \(4,\)"):
            call(group=dev(group), row_ban=dev(i32(*shape)))
    with pytest.raises(TypeError, match="bad: expected torch.int32"):
        call(bad=dev(torch.zeros(1)))
    with pytest.raises(ValueError, match=r"bad: expected shape \(1,\)"):
        call(bad=dev(i32(2)))
    # no rows: empty outputs without a call (the library is still untouchable)
    e_i, e_s = call(idx=i32(0, 20), score=torch.zeros(0, 20), n=7, group=dev(group), cap=3)
    assert e_i.shape == (0, 7) and e_i.dtype == torch.int32 and e_s.shape == (0, 7) and e_s.dtype == torch.float32


class Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"read .{name} before refusing")


def _inference(k=3):
    from p_companion_amd.inference import PCompanionInference
    inf = object.__new__(PCompanionInference)                          # (no graph, no model, no device)
    inf.__dict__.update(model=Untouchable(), bpg=Untouchable(), features=Untouchable(), _graph=Untouchable(),
                        exclusions=Untouchable(), type_idx=Untouchable(), config=SimpleNamespace(NUM_COMP_TYPES=k))
    return inf


BAD_GROUPS = (torch.zeros(7, dtype=torch.int64), torch.zeros(7), torch.zeros(7, 1, dtype=torch.int32), [0] * 7)


def test_recommend_capped_batch_refuses_before_the_model_or_the_graph_is_touched():
    from p_companion_amd.inference import PCompanionInference
    sig = inspect.signature(PCompanionInference.recommend_capped_batch)
    assert list(sig.parameters) == ["self", "query_idx", "num_recommendations", "group", "cap", "pool", "diversity", "similarity"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [10, None, 1, 64, None, "cosine"]
    inf = _inference()
    q = torch.zeros(2, dtype=torch.int32)
    for n, pool in ((0, 64), (-1, 64), (65, 64), (10, 257), (300, 300), (10, 0), (11, 10)):
        with pytest.raises(ValueError, match="num_recommendations <= pool <= 256"):
            inf.recommend_capped_batch(q, n, pool=pool)
    for cap in (0, -2):
        with pytest.raises(ValueError, match="cap must be at least 1"):
            inf.recommend_capped_batch(q, 10, cap=cap)
    for g in BAD_GROUPS:
        with pytest.raises(ValueError, match=r"group must be None or a \[P\] int32"):
            inf.recommend_capped_batch(q, 10, group=g)
    for d in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError, match=r"diversity must be None or in \[0, 1\]"):
            inf.recommend_capped_batch(q, 10, diversity=d)
    for s in ("l2", "Cosine", None, 1):
        with pytest.raises(ValueError, match="'cosine' or 'dot'"):
            inf.recommend_capped_batch(q, 10, diversity=0.3, similarity=s)
    # a group that does not cover the catalogue
    inf.__dict__.update(type_idx=torch.zeros(9, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"one entry per product \(9\), got 7"):
        inf.recommend_capped_batch(q, 10, group=torch.zeros(7, dtype=torch.int32))
    # a diversity over a graph without the fp32 features: recommend_diverse_batch's refusal, before the model runs
    inf.__dict__.update(features=None, _graph={}, catalogue=torch.zeros(3, 128, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="recommend_capped_batch.*without them"):
        inf.recommend_capped_batch(q, 10, pool=16, diversity=0.3)
    # ... and a bf16 catalogue bounds the pool at what it serves: recommend_batch's own message
    with pytest.raises(ValueError, match="bf16 catalogue serves at most 16"):
        inf.recommend_capped_batch(q, 10, pool=17)
    # the neighbours keep their signatures
    assert list(inspect.signature(PCompanionInference.recommend_batch).parameters) == ["self", "query_idx", "num_recommendations"]
    assert list(inspect.signature(PCompanionInference.recommend_diverse_batch).parameters) == [
        "self", "query_idx", "num_recommendations", "pool", "diversity", "similarity"]


def test_recommend_page_batch_refuses_before_the_model_or_the_graph_is_touched():
    from p_companion_amd.inference import PCompanionInference
    sig = inspect.signature(PCompanionInference.recommend_page_batch)
    assert list(sig.parameters) == ["self", "query_idx", "num_recommendations", "per_type", "group", "cap"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [10, 4, None, 1]
    q = torch.zeros(2, dtype=torch.int32)
    inf = _inference(k=3)
    for per_type in (0, -1, 86, 256):                                   # K per_type > 256: 3 x 86 = 258
        with pytest.raises(ValueError, match=r"K \* per_type <= 256, got K = 3 and per_type %d" % per_type):
            inf.recommend_page_batch(q, 10, per_type=per_type)
    with pytest.raises(ValueError, match=r"K \* per_type <= 256, got K = 5 and per_type 52"):
        _inference(k=5).recommend_page_batch(q, 10, per_type=52)
    for n, per_type in ((0, 4), (-1, 4), (13, 4), (256, 85), (4, 1)):
        with pytest.raises(ValueError, match=r"num_recommendations <= K \* per_type = %d, got %d" % (3 * per_type, n)):
            inf.recommend_page_batch(q, n, per_type=per_type)
    with pytest.raises(ValueError, match="cap must be at least 1"):
        inf.recommend_page_batch(q, 10, cap=0)
    for g in BAD_GROUPS:
        with pytest.raises(ValueError, match=r"group must be None or a \[P\] int32"):
            inf.recommend_page_batch(q, 10, group=g)
    inf.__dict__.update(type_idx=torch.zeros(9, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"one entry per product \(9\), got 7"):
        inf.recommend_page_batch(q, 10, group=torch.zeros(7, dtype=torch.int32))
    assert "as they are" in PCompanionInference.recommend_page_batch.__doc__.lower()


def test_similar_capped_batch_refuses_before_anything_is_touched():
    from p_companion_amd.inference import IndexedSimilarProducts, SimilarProducts
    sig = inspect.signature(SimilarProducts.similar_capped_batch)
    assert list(sig.parameters) == ["self", "query_idx", "n", "group", "cap", "own_group"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [10, None, 1, False]
    assert IndexedSimilarProducts.similar_capped_batch is SimilarProducts.similar_capped_batch       # inherited, not restated
    q = torch.zeros(2, dtype=torch.int32)
    for cls in (SimilarProducts, IndexedSimilarProducts):
        sp = object.__new__(cls)                                       # (no table, no graph, no device)
        sp.__dict__.update(table=Untouchable(), bpg=Untouchable(), exclusions=Untouchable(), type_idx=Untouchable())
        for n in (17, 100, 0, -1):
            with pytest.raises(ValueError, match="1 to 16"):
                sp.similar_capped_batch(q, n)
        with pytest.raises(ValueError, match="cap must be at least 1"):
            sp.similar_capped_batch(q, 10, cap=0)
        for g in BAD_GROUPS:
            with pytest.raises(ValueError, match=r"group must be None or a \[P\] int32"):
                sp.similar_capped_batch(q, 10, group=g)
        sp.__dict__.update(type_idx=torch.zeros(9, dtype=torch.int32))
        with pytest.raises(ValueError, match=r"one entry per product \(9\), got 7"):
            sp.similar_capped_batch(q, 10, group=torch.zeros(7, dtype=torch.int32))
    doc = " ".join(SimilarProducts.similar_capped_batch.__doc__.split())
    assert "pool is 16" in doc and "SHORT" in doc
