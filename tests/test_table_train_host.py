"""The host side of the trainable product table (pc_joint_query_grad, pc_sparse_adam_rows, ops.joint_query_grad,
ops.sparse_adam_rows, table_optim.ProductTableAdam, train.train with TRAIN_PRODUCT_EMBEDDINGS) without a GPU: the header and
the ctypes table, the workspace queries, what the entries and the wrappers refuse before anything is launched."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

from conftest import ROOT

PC_EINVAL, PC_ESHAPE, PC_EWORKSPACE = -1, -2, -3
ENTRIES = ("pc_joint_query_grad", "pc_joint_query_grad_workspace_bytes", "pc_sparse_adam_rows",
           "pc_sparse_adam_rows_workspace_bytes")


def test_header_declares_the_entries_and_the_abi_stays_8():
    from p_companion_amd import _lib
    txt = open(os.path.join(ROOT, "include", "pcompanion_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES
    assert re.search(r"#define\s+PC_ABI_VERSION\s+8\b", txt)
    L = _lib.lib()                                                    # binds every signature
    assert L.pc_abi_version() == 8
    assert L.pc_joint_query_grad_workspace_bytes.restype == ctypes.c_size_t
    assert L.pc_sparse_adam_rows_workspace_bytes.restype == ctypes.c_size_t


def test_the_unit_is_part_of_the_build():
    from p_companion_amd import build
    assert "table_train.hip" in build.sources()


def test_workspace_queries():
    from p_companion_amd import _lib
    L = _lib.lib()
    sa = L.pc_sparse_adam_rows_workspace_bytes
    assert sa(0) == 0 and sa(-1) == 0 and sa((1 << 20) + 1) == 0
    for r in (1, 1000, 8192, 8193, 70_000, 1 << 20):
        # two (key, value) buffer pairs of R words and the digit counts of every 4096-key chunk
        chunks = (r + 4095) // 4096
        assert 16 * r + 1024 * chunks <= sa(r) <= 16 * r + 1024 * chunks + 5 * 256, r
    qg = L.pc_joint_query_grad_workspace_bytes
    for bad in ((0, 3, 128), (16, 0, 128), (16, 9, 128), (16, 3, 64), (16, 3, 192)):
        assert qg(*bad) == 0, bad
    for b, k, d in ((1, 1, 128), (4096, 3, 128), (130, 3, 256)):
        floats = b * d * 2 + b * k * d + d * d
        assert 4 * (floats + 2 * b + b * k) <= qg(b, k, d) <= 4 * (floats + 2 * b + b * k) + 7 * 256, (b, k, d)


def _aligned():
    """One 16-byte aligned host buffer: a pointer that passes every check, and that no check dereferences."""
    buf = ctypes.create_string_buffer(256)
    return buf, (ctypes.addressof(buf) + 15) & ~15


def test_the_sparse_adam_refuses_before_anything_is_launched():
    from p_companion_amd import _lib
    entry = _lib.lib().pc_sparse_adam_rows
    buf, a = _aligned()
    p = ctypes.c_void_p(a)

    def call(**kw):
        args = dict(table=p, exp_avg=p, exp_avg_sq=p, P=10, dim=128, idx=p, grad=p, R=4, t=1, lr=1e-3, beta1=0.9, beta2=0.999,
                    eps=1e-8, bad=p, ws=p, ws_bytes=0, stream=None)
        args.update(kw)
        return entry(*args.values())

    for name in ("table", "exp_avg", "exp_avg_sq", "idx", "grad", "bad", "ws"):
        assert call(**{name: None}) == PC_EINVAL, name
    for kw in (dict(P=0), dict(P=1 << 31), dict(R=0), dict(R=(1 << 20) + 1), dict(t=0), dict(t=-3)):
        assert call(**kw) == PC_EINVAL, kw
    for dim in (0, 64, 192, 512):
        assert call(dim=dim) == PC_ESHAPE, dim
    off = ctypes.c_void_p(a + 4)
    for name in ("table", "exp_avg", "exp_avg_sq", "grad", "ws"):
        assert call(**{name: off}) == PC_ESHAPE, name
    for name in ("idx", "bad"):
        assert call(**{name: off}) == PC_EWORKSPACE, name            # (4-byte alignment is enough for those)
        assert call(**{name: ctypes.c_void_p(a + 2)}) == PC_ESHAPE, name
    assert call() == PC_EWORKSPACE and call(dim=256, R=1 << 20, ws_bytes=1 << 20) == PC_EWORKSPACE


def test_the_query_gradient_refuses_before_anything_is_launched():
    from p_companion_amd import _lib
    entry = _lib.lib().pc_joint_query_grad
    buf, a = _aligned()
    p = ctypes.c_void_p(a)
    st = _lib.JointTensors()
    for f, _ in _lib.JointTensors._fields_[:11]:
        setattr(st, f, a)

    def call(params=st, **kw):
        args = dict(query_idx=p, topk=p, pos=p, neg=p, B=4, P=9, T=7, K=3, dim=128, margin=1.0, alpha=0.8, dq=p, bad=p, ws=p,
                    ws_bytes=0, stream=None)
        args.update(kw)
        return entry(ctypes.byref(params) if params is not None else None, *args.values())

    assert call(params=None) == PC_EINVAL
    for field in ("product_table", "itm_w", "itm_b", "typ_w", "typ_b", "comp_types"):
        holed = _lib.JointTensors()
        for f, _ in _lib.JointTensors._fields_[:11]:
            setattr(holed, f, None if f == field else a)
        assert call(params=holed) == PC_EINVAL, field
    for name in ("query_idx", "topk", "pos", "neg", "dq", "bad", "ws"):
        assert call(**{name: None}) == PC_EINVAL, name
    for kw in (dict(B=0), dict(T=0), dict(P=0)):
        assert call(**kw) == PC_EINVAL, kw
    for kw in (dict(K=0), dict(K=9), dict(K=8), dict(dim=64), dict(dim=192)):       # (K = 8 > T = 7)
        assert call(**kw) == PC_ESHAPE, kw
    for name in ("pos", "neg", "dq", "ws"):
        assert call(**{name: ctypes.c_void_p(a + 4)}) == PC_ESHAPE, name
    assert call() == PC_EWORKSPACE and call(dim=256, K=7) == PC_EWORKSPACE


class OnDevice(torch.Tensor):
    """A stand-in that reports is_cuda: _req tests the device first, and this lets the checks behind it be reached."""
    is_cuda = True


def _dev(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype).as_subclass(OnDevice)


def test_sparse_adam_rows_wrapper_refusals():
    from p_companion_amd import ops
    table, m, v = _dev(9, 128), _dev(9, 128), _dev(9, 128)
    idx, grad = _dev(4, dtype=torch.int32), _dev(4, 128)
    with pytest.raises(TypeError, match="CUDA/ROCm"):
        ops.sparse_adam_rows(torch.zeros(9, 128), m, v, idx, grad, 1)
    with pytest.raises(TypeError, match="float32"):
        ops.sparse_adam_rows(_dev(9, 128, dtype=torch.float64), m, v, idx, grad, 1)
    with pytest.raises(TypeError, match="int32"):
        ops.sparse_adam_rows(table, m, v, _dev(4, dtype=torch.int64), grad, 1)
    with pytest.raises(TypeError, match="float32"):
        ops.sparse_adam_rows(table, m, v, idx, _dev(4, 128, dtype=torch.bfloat16), 1)
    with pytest.raises(ValueError, match="width"):
        ops.sparse_adam_rows(_dev(9, 64), _dev(9, 64), _dev(9, 64), idx, _dev(4, 64), 1)
    # moments of another shape than the table
    with pytest.raises(ValueError, match="exp_avg:"):
        ops.sparse_adam_rows(table, _dev(8, 128), v, idx, grad, 1)
    with pytest.raises(ValueError, match="exp_avg_sq:"):
        ops.sparse_adam_rows(table, m, _dev(9 * 128), idx, grad, 1)
    # idx [R] against grad [R, D]
    with pytest.raises(ValueError, match="grad:"):
        ops.sparse_adam_rows(table, m, v, idx, _dev(5, 128), 1)
    with pytest.raises(ValueError, match="grad:"):
        ops.sparse_adam_rows(table, m, v, idx, _dev(4, 256), 1)
    with pytest.raises(ValueError, match=r"\[R\]"):
        ops.sparse_adam_rows(table, m, v, _dev(2, 2, dtype=torch.int32), grad, 1)
    with pytest.raises(ValueError, match=r"\[R\]"):
        ops.sparse_adam_rows(table, m, v, _dev(0, dtype=torch.int32), _dev(0, 128), 1)
    for t in (0, -1):
        with pytest.raises(ValueError, match="step number"):
            ops.sparse_adam_rows(table, m, v, idx, grad, t)
    with pytest.raises(TypeError, match="bad"):
        ops.sparse_adam_rows(table, m, v, idx, grad, 1, bad=_dev(1, dtype=torch.int64))


def test_joint_query_grad_wrapper_refusals():
    from p_companion_amd import ops
    b, k, d = 4, 3, 128
    params = {"product_embeddings.weight": _dev(9, d), "complementary_type_embeddings.weight": _dev(7, 64)}
    qi, topk = _dev(b, dtype=torch.int32), _dev(b, k, dtype=torch.int32)
    pos, neg = _dev(b, d), _dev(b, d)
    call = lambda **kw: ops.joint_query_grad(kw.pop("params", params), kw.pop("qi", qi), kw.pop("topk", topk), kw.pop("pos", pos),
                                             kw.pop("neg", neg), 1.0, 0.8)
    with pytest.raises(TypeError, match="CUDA/ROCm"):
        call(qi=torch.zeros(b, dtype=torch.int32))
    with pytest.raises(TypeError, match="int32"):
        call(qi=_dev(b, dtype=torch.int64))
    with pytest.raises(TypeError, match="int32"):
        call(topk=_dev(b, k, dtype=torch.int64))
    with pytest.raises(TypeError, match="float32"):
        call(pos=_dev(b, d, dtype=torch.float64))
    with pytest.raises(TypeError, match="float32"):
        call(params=dict(params, **{"product_embeddings.weight": _dev(9, d, dtype=torch.bfloat16)}))
    with pytest.raises(ValueError, match="width"):
        call(params=dict(params, **{"product_embeddings.weight": _dev(9, 64)}))
    # [B, K] against [B] and [B, D]
    with pytest.raises(ValueError, match=r"\[B, K\]"):
        call(topk=_dev(b + 1, k, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"\[B, K\]"):
        call(topk=_dev(b * k, dtype=torch.int32))
    with pytest.raises(ValueError, match="K = 9"):
        call(topk=_dev(b, 9, dtype=torch.int32))
    with pytest.raises(ValueError, match="positive_items"):
        call(pos=_dev(b + 1, d))
    with pytest.raises(ValueError, match="negative_items"):
        call(neg=_dev(b, 256))
    with pytest.raises(ValueError, match=r"\[B\]"):
        call(qi=_dev(b, 1, dtype=torch.int32))


def test_product_table_adam_state_dict_layout_without_a_step():
    from p_companion_amd.table_optim import ProductTableAdam
    model = SimpleNamespace(product_embeddings=SimpleNamespace(weight=torch.zeros(5, 128)))
    opt = ProductTableAdam(model, lr=3e-4)
    sd = opt.state_dict()
    assert sd["state"] == {} and len(sd["param_groups"]) == 1
    g = sd["param_groups"][0]
    assert g["lr"] == 3e-4 and g["betas"] == (0.9, 0.999) and g["eps"] == 1e-8 and g["params"] == [0]
    ref = torch.optim.SparseAdam([torch.nn.Parameter(torch.zeros(5, 128))], lr=3e-4).state_dict()
    assert set(g) == set(ref["param_groups"][0])
    with pytest.raises(ValueError):
        ProductTableAdam(model, lr=-1.0)
    with pytest.raises(ValueError):
        ProductTableAdam(SimpleNamespace(product_embeddings=SimpleNamespace(weight=torch.zeros(5, 128, dtype=torch.float64))))
    # a saved state comes back: the step count and both moments, in torch.optim.SparseAdam's layout
    opt.load_state_dict({"state": {0: {"step": 7, "exp_avg": torch.ones(5, 128), "exp_avg_sq": torch.full((5, 128), 2.0)}},
                         "param_groups": [dict(g, lr=1e-2)]})
    back = opt.state_dict()
    assert back["state"][0]["step"] == 7 and back["param_groups"][0]["lr"] == 1e-2
    assert torch.equal(back["state"][0]["exp_avg"], torch.ones(5, 128))
    assert torch.equal(back["state"][0]["exp_avg_sq"], torch.full((5, 128), 2.0))
    with pytest.raises(ValueError, match="shape"):
        opt.load_state_dict({"state": {0: {"step": 1, "exp_avg": torch.ones(4, 128), "exp_avg_sq": torch.ones(4, 128)}},
                             "param_groups": [g]})


def test_train_refuses_the_dense_route_with_the_flag():
    from p_companion_amd import train as drv

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError(f"read .{name} before refusing")

    cfg = SimpleNamespace(TRAIN_PRODUCT_EMBEDDINGS=True)
    with pytest.raises(ValueError, match="fused=False"):
        drv.train(cfg, Untouchable(), Untouchable(), Untouchable(), fused=False)


def test_train_step_keyword_defaults_to_todays_behaviour():
    import inspect
    from p_companion_amd.p_companion import PCompanion
    sig = inspect.signature(PCompanion.train_step)
    assert list(sig.parameters) == ["self", "batch", "optimizer", "table_optimizer"]
    assert sig.parameters["table_optimizer"].default is None and sig.parameters["optimizer"].default is None
