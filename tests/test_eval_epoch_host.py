"""Evaluation over a device-resident split (pc_eval_batch_stats, pc_joint_eval_workspace_bytes, pc_joint_eval_epoch) on the host
side only: the symbols, the argument checks that come before any launch, the workspace's size and growth, and the refusal of
Metrics.evaluate_model(fused=True) for a loader the one-call form does not serve.  No GPU, no compute calls."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

NAMES = ("pc_eval_batch_stats", "pc_joint_eval_workspace_bytes", "pc_joint_eval_epoch")
EINVAL, ESHAPE, EWORKSPACE = -1, -2, -3


def test_symbols_in_header_library_and_ctypes_table():
    from p_companion_amd import _lib
    txt = open(os.path.join(ROOT, "include", "pcompanion_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = _lib.lib()
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, txt), n
        assert n in _lib.SIGNATURES and hasattr(L, n), n
    assert L.pc_abi_version() == 8                                    # additive: the version stays


def _dummy():
    """Non-null host addresses: the calls below must fail their checks before anything could dereference them."""
    buf = ctypes.create_string_buffer(4096)
    return buf, ctypes.c_void_p(ctypes.addressof(buf))


def _tensors(ptr, skip=None):
    from p_companion_amd._lib import JointTensors
    st = JointTensors()
    for name, _ in JointTensors._fields_:
        if name != "dropout" and name != skip:
            setattr(st, name, ptr.value)
    return st


def test_stats_argument_checks_come_before_any_launch():
    from p_companion_amd import _lib
    L = _lib.lib()
    keep, p = _dummy()
    ok = [p, p, p, p, 64, 3, 128, p, p, p, 1 << 30, None]
    assert L.pc_eval_batch_stats(None, p, p, p, 64, 3, 128, p, p, p, 1 << 30, None) == EINVAL
    for i in (1, 2, 3, 7, 8, 9):                                      # every pointer
        a = list(ok); a[i] = None
        assert L.pc_eval_batch_stats(*a) == EINVAL, i
    for i in (4, 5):                                                  # batch, k
        a = list(ok); a[i] = 0
        assert L.pc_eval_batch_stats(*a) == EINVAL, i
    a = list(ok); a[6] = 192
    assert L.pc_eval_batch_stats(*a) == ESHAPE
    a = list(ok); a[5] = 9
    assert L.pc_eval_batch_stats(*a) == ESHAPE
    a = list(ok); a[10] = 16
    assert L.pc_eval_batch_stats(*a) == EWORKSPACE


def test_epoch_argument_checks_come_before_any_launch():
    from p_companion_amd import _lib
    L = _lib.lib()
    keep, p = _dummy()
    st = _tensors(p)

    def call(st=st, pairs=p, n_pairs=1000, features=p, type_idx=p, n_types=100, dim=128, batch=100, num_types=100, k=3,
             num_products=5000, stats=p, cos=p, metrics=p, ws=p, ws_bytes=1 << 40):
        return L.pc_joint_eval_epoch(ctypes.byref(st) if st is not None else None, pairs, n_pairs, features, type_idx, n_types,
                                     dim, 1, 0, batch, num_types, k, num_products, stats, cos, metrics, None, ws, ws_bytes, None)

    assert call(st=None) == EINVAL
    assert call(st=_tensors(p, skip="itm_w")) == EINVAL and call(st=_tensors(p, skip="product_table")) == EINVAL
    for kw in ("pairs", "features", "type_idx", "stats", "cos", "metrics", "ws"):
        assert call(**{kw: None}) == EINVAL, kw
    for kw in ("n_pairs", "batch", "num_types", "n_types", "num_products"):
        assert call(**{kw: 0}) == EINVAL, kw
    assert call(dim=64) == ESHAPE and call(k=0) == ESHAPE and call(k=9) == ESHAPE and call(k=3, num_types=2) == ESHAPE
    # a ragged rest of 1..9 pairs (metrics.py:103: its key min(10, cols) is not 'hit@10'): refused; 10 and more are served
    assert call(n_pairs=1005) == ESHAPE and call(n_pairs=1001) == ESHAPE and call(n_pairs=1009) == ESHAPE
    assert call(n_pairs=45, batch=8) == ESHAPE                        # full batches of fewer than 10 rows
    need = L.pc_joint_eval_workspace_bytes(100, 100, 3, 128)
    assert need > 0
    assert call(n_pairs=1010, ws_bytes=need - 1) == EWORKSPACE and call(n_pairs=1000, ws_bytes=0) == EWORKSPACE


def test_workspace_fits_beside_the_catalogue_and_grows_no_faster_than_T():
    from p_companion_amd import _lib
    L = _lib.lib()
    T, B, K = 34_800, 4096, 3
    for dim in (128, 256):
        one, two = L.pc_joint_eval_workspace_bytes(B, T, K, dim), L.pc_joint_eval_workspace_bytes(B, 2 * T, K, dim)
        assert one >= T * K * dim * 4                                 # holds the [T, K, D] table
        assert two <= 2.1 * one, (dim, one, two)
    assert L.pc_joint_eval_workspace_bytes(B, T, K, 128) < 1_000_000_000
    assert L.pc_joint_eval_workspace_bytes(0, T, K, 128) == 0 and L.pc_joint_eval_workspace_bytes(B, T, K, 96) == 0
    assert L.pc_joint_eval_workspace_bytes(B, T, 9, 128) == 0


def test_fused_true_refuses_a_plain_list_of_batches_before_anything_is_touched():
    from p_companion_amd.metrics import Metrics

    class Untouchable:
        def __getattr__(self, name):
            raise AssertionError("the model was touched: " + name)

    with pytest.raises(ValueError, match="ComplementaryIndexLoader"):
        Metrics.evaluate_model(Untouchable(), [{"query_idx": None}], "cuda", fused=True)


def test_ops_refuse_cpu_tensors():
    import torch
    from p_companion_amd import ops
    with pytest.raises(TypeError):
        ops.eval_batch_stats(torch.zeros(16, 3, 128), torch.zeros(16, 128), torch.zeros(16, 128),
                             torch.zeros(16, 3, dtype=torch.int32))
