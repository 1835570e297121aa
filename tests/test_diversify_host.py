"""The host side of the diversified lists (pc_diversify_lists, pc_inv_norm; ops.diversify_lists, ops.inv_norm;
PCompanionInference.recommend_diverse_batch), without a GPU: the header and the ctypes table, what the entries refuse before
anything is launched, and the argument checks of the wrappers and the method that need no device."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from conftest import ROOT

PC_EINVAL, PC_ESHAPE = -1, -2
ENTRIES = ("pc_diversify_lists", "pc_inv_norm")


def test_header_declares_the_entries_and_the_abi_stays_8():
    from p_companion_amd import _lib
    txt = open(os.path.join(ROOT, "include", "pcompanion_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES
    assert re.search(r"#define\s+PC_ABI_VERSION\s+8\b", txt)
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert _lib.SIGNATURES["pc_diversify_lists"] == (i, [vp, vp, i, i, vp, vp, i, i, i, f, vp, vp, vp, vp])
    assert _lib.SIGNATURES["pc_inv_norm"] == _lib.SIGNATURES["pc_half_sq_norm_bias"]
    L = _lib.lib()
    assert L.pc_abi_version() == 8
    assert L.pc_diversify_lists.argtypes == _lib.SIGNATURES["pc_diversify_lists"][1]


def test_the_unit_is_part_of_the_build():
    from p_companion_amd import build
    assert "diversify.hip" in build.sources()


def _aligned():
    buf = ctypes.create_string_buffer(4096 + 16)
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)


def test_the_entries_refuse_before_anything_is_launched():
    from p_companion_amd import _lib
    L = _lib.lib()
    buf, p = _aligned()
    odd = ctypes.c_void_p(p.value + 4)

    def call(**kw):
        a = dict(idx=p, score=p, rows=3, m=20, table=p, scale=None, num_products=7, dim=128, n=5, lam=0.5, out_idx=p,
                 out_score=p, bad=None, stream=None)
        a.update(kw)
        return L.pc_diversify_lists(*a.values())

    for kw in (dict(m=0), dict(m=-1), dict(m=257), dict(n=0), dict(n=21), dict(m=256, n=257), dict(dim=0), dict(dim=64),
               dict(dim=192), dict(dim=512), dict(lam=-1e-6), dict(lam=1.0 + 1e-6), dict(lam=float("nan")), dict(lam=float("inf")),
               dict(rows=-1), dict(num_products=0), dict(idx=None), dict(score=None), dict(table=None), dict(out_idx=None),
               dict(out_score=None), dict(table=odd)):
        assert call(**kw) == PC_ESHAPE, kw
    # no rows: success without a launch, whatever the pointers -- but a refused shape is refused first
    assert call(rows=0) == 0 and call(rows=0, idx=None, score=None, table=None, out_idx=None, out_score=None) == 0
    assert call(rows=0, m=257) == PC_ESHAPE and call(rows=0, lam=2.0) == PC_ESHAPE
    entry = L.pc_inv_norm
    assert entry(None, 4, 128, p, None) == PC_EINVAL and entry(p, 4, 128, None, None) == PC_EINVAL
    assert entry(p, 0, 128, p, None) == PC_EINVAL and entry(p, -3, 256, p, None) == PC_EINVAL
    for dim in (0, 64, 192, 512):
        assert entry(p, 4, dim, p, None) == PC_ESHAPE, dim
    assert entry(odd, 4, 128, p, None) == PC_ESHAPE


class OnDevice(torch.Tensor):
    """A stand-in that reports is_cuda: _req tests the device first, and this lets the checks behind it be reached."""
    is_cuda = True


def test_the_wrappers_check_their_arguments_before_the_library_is_touched(monkeypatch):
    from p_companion_amd import _lib, ops

    def untouched():
        raise AssertionError("the library was touched before the arguments were refused")

    monkeypatch.setattr(_lib, "lib", untouched)
    assert ops.DIVERSIFY_MAX_POOL == 256
    dev = lambda t: t.as_subclass(OnDevice)
    idx, sc, table = torch.zeros(4, 20, dtype=torch.int32), torch.zeros(4, 20), torch.zeros(7, 128)
    # CPU tensors are refused, argument by argument
    with pytest.raises(TypeError, match="idx: expected a CUDA/ROCm"):
        ops.diversify_lists(idx, dev(sc), dev(table), 5, 0.5)
    with pytest.raises(TypeError, match="score: expected a CUDA/ROCm"):
        ops.diversify_lists(dev(idx), sc, dev(table), 5, 0.5)
    with pytest.raises(TypeError, match="table: expected a CUDA/ROCm"):
        ops.diversify_lists(dev(idx), dev(sc), table, 5, 0.5)
    with pytest.raises(TypeError, match="scale: expected a CUDA/ROCm"):
        ops.diversify_lists(dev(idx), dev(sc), dev(table), 5, 0.5, scale=torch.zeros(7))
    with pytest.raises(TypeError, match="bad: expected a CUDA/ROCm"):
        ops.diversify_lists(dev(idx), dev(sc), dev(table), 5, 0.5, bad=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(TypeError, match="CUDA/ROCm"):
        ops.inv_norm(table)
    call = lambda **kw: ops.diversify_lists(dev(kw.pop("idx", idx)), dev(kw.pop("score", sc)), dev(kw.pop("table", table)),
                                            kw.pop("n", 5), kw.pop("lam", 0.5), **kw)
    # dtypes and shapes
    with pytest.raises(TypeError, match="idx: expected torch.int32"):
        call(idx=idx.long())
    with pytest.raises(TypeError, match="score: expected torch.float32"):
        call(score=sc.double())
    for bad_idx, bad_sc in ((torch.zeros(80, dtype=torch.int32), torch.zeros(80)), (idx, torch.zeros(4, 21)),
                            (torch.zeros(2, 2, 20, dtype=torch.int32), torch.zeros(2, 2, 20))):
        with pytest.raises(ValueError, match=r"one shape \[R, m\]"):
            call(idx=bad_idx, score=bad_sc)
    with pytest.raises(ValueError, match=r"pool m must be in \[1, 256\], got 257"):
        call(idx=torch.zeros(2, 257, dtype=torch.int32), score=torch.zeros(2, 257))
    with pytest.raises(ValueError, match=r"pool m must be in \[1, 256\], got 0"):
        call(idx=torch.zeros(2, 0, dtype=torch.int32), score=torch.zeros(2, 0))
    for n in (0, -1, 21, 256):
        with pytest.raises(ValueError, match=r"n must be in \[1, m = 20\], got %d" % n):
            call(n=n)
    for lam in (-0.1, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"lam must be in \[0, 1\]"):
            call(lam=lam)
    with pytest.raises(TypeError, match="table: expected torch.float32"):
        call(table=torch.zeros(7, 128, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match=r"\[P, D\]"):
        call(table=torch.zeros(7 * 128))
    with pytest.raises(ValueError, match="width"):
        call(table=torch.zeros(7, 64))
    with pytest.raises(ValueError, match="at least one row"):
        call(table=torch.zeros(0, 128))
    with pytest.raises(ValueError, match="scale must be"):
        call(scale=[1.0] * 7)
    with pytest.raises(TypeError, match="scale: expected torch.float32"):
        call(scale=dev(torch.zeros(7, dtype=torch.float64)))
    for shape in ((6,), (8,), (7, 1)):
        with pytest.raises(ValueError, match=r"scale: expected shape \(7,\)"):
            call(scale=dev(torch.zeros(shape)))
    with pytest.raises(TypeError, match="bad: expected torch.int32"):
        call(bad=dev(torch.zeros(1)))
    with pytest.raises(ValueError, match=r"bad: expected shape \(1,\)"):
        call(bad=dev(torch.zeros(2, dtype=torch.int32)))
    # inv_norm: half_sq_norm_bias's checks
    with pytest.raises(TypeError, match="float32"):
        ops.inv_norm(dev(torch.zeros(5, 128, dtype=torch.float64)))
    with pytest.raises(ValueError, match=r"\[P, D\]"):
        ops.inv_norm(dev(torch.zeros(128)))
    with pytest.raises(ValueError, match="width"):
        ops.inv_norm(dev(torch.zeros(5, 64)))
    with pytest.raises(ValueError, match="at least one row"):
        ops.inv_norm(dev(torch.zeros(0, 128)))


class Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"read .{name} before refusing")


def test_recommend_diverse_batch_refuses_before_the_model_or_the_graph_is_touched():
    from p_companion_amd.inference import PCompanionInference
    sig = inspect.signature(PCompanionInference.recommend_diverse_batch)
    assert list(sig.parameters) == ["self", "query_idx", "num_recommendations", "pool", "diversity", "similarity"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [10, 64, 0.3, "cosine"]
    inf = object.__new__(PCompanionInference)                          # (no graph, no model, no device)
    inf.__dict__.update(model=Untouchable(), bpg=Untouchable(), features=Untouchable(), _graph=Untouchable(),
                        exclusions=Untouchable())
    q = torch.zeros(2, dtype=torch.int32)
    for n, pool in ((0, 64), (-1, 64), (65, 64), (10, 257), (300, 300), (10, 0)):
        with pytest.raises(ValueError, match="num_recommendations <= pool <= 256"):
            inf.recommend_diverse_batch(q, n, pool=pool)
    for d in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError, match=r"diversity must be in \[0, 1\]"):
            inf.recommend_diverse_batch(q, 10, diversity=d)
    for s in ("l2", "Cosine", None, 1):
        with pytest.raises(ValueError, match="'cosine' or 'dot'"):
            inf.recommend_diverse_batch(q, 10, similarity=s)
    # a bf16 catalogue over a graph without the fp32 features: refused, and it says so, before the model runs
    inf.__dict__.update(features=None, _graph={}, catalogue=torch.zeros(3, 128, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="without them"):
        inf.recommend_diverse_batch(q, 10, pool=16)
    # ... and with them, the pool is bounded by what the bf16 catalogue serves: recommend_batch's own message
    inf.__dict__.update(_graph={"features": Untouchable()})
    with pytest.raises(ValueError, match="bf16 catalogue serves at most 16"):
        inf.recommend_diverse_batch(q, 10, pool=17)
    # recommend_batch and recommend keep their signatures
    assert list(inspect.signature(PCompanionInference.recommend_batch).parameters) == ["self", "query_idx", "num_recommendations"]


def test_intra_list_similarity_on_the_host():
    """Metrics.intra_list_similarity is torch: its arithmetic is checked here on CPU tensors."""
    from p_companion_amd.metrics import Metrics
    table = torch.tensor([[1.0, 0.0], [0.0, 2.0], [3.0, 3.0], [1.0, 1.0]])
    idx = torch.tensor([[0, 1, 2], [3, -1, 2], [1, -1, -1], [-1, -1, -1]], dtype=torch.int32)
    # list 0: pairs (0,1) 0, (0,2) 3, (1,2) 6 -> 3; list 1: pair (3,2) 6 -> 6; lists 2 and 3 hold fewer than two products
    assert float(Metrics.intra_list_similarity(idx, table)) == pytest.approx(4.5)
    scale = 1.0 / table.norm(dim=1)
    c02, c12 = 3 / (18 ** 0.5), 6 / (2 * 18 ** 0.5)
    assert float(Metrics.intra_list_similarity(idx, table, scale)) == pytest.approx(((0 + c02 + c12) / 3 + 1.0) / 2, rel=1e-6)
    assert float(Metrics.intra_list_similarity(idx[2:], table)) == 0.0            # no list with two products
    assert float(Metrics.intra_list_similarity(idx.reshape(2, 2, 3), table)) == pytest.approx(4.5)
