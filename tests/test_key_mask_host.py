"""The key-padding mask's host side, without a GPU: the four _masked entries are declared, exported and bound with the
argument lists the header states, the ABI stays 8, NULL or inconsistent arguments are refused before any launch, and
ops.p2v_train_step(masked=True) refuses the split (cross-replica) step."""
import ctypes
import os
import re

import pytest
import torch

from conftest import ROOT

ENTRIES = ("pc_p2v_attention_forward_masked", "pc_p2v_attention_backward_masked", "pc_p2v_train_step_compact_masked",
           "pc_p2v_train_step_unique_masked")
PC_EINVAL, PC_EBATCHNORM = -1, -4


def test_header_declares_library_exports_and_ctypes_binds_the_entries():
    from p_companion_amd import _lib
    txt = open(os.path.join(ROOT, "include", "pcompanion_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(L, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES, name
        proto = re.search(r"int\s+" + name + r"\s*\((.*?)\)\s*;", txt, flags=re.S)
        assert proto, f"{name} is not declared in the header"
        args = [a.strip() for a in proto.group(1).split(",")]
        res, sig = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == len(sig), (name, len(args), len(sig))
        for a, ct in zip(args, sig):
            if "*" in a:
                assert ct is ctypes.c_void_p or issubclass(ct, ctypes._Pointer), (name, a, ct)
            else:
                want = {"size_t": ctypes.c_size_t, "float": ctypes.c_float, "int": ctypes.c_int}[a.split()[0]]
                assert ct is want, (name, a, ct)
    assert L.pc_abi_version() == 8                                      # additive entries: the ABI stays 8
    assert _lib.lib().pc_abi_version() == 8


def _structs():
    from p_companion_amd import _lib
    return _lib.P2VTensors(), _lib.P2VTensors(), _lib.AttnSaved()


def test_masked_attention_entries_refuse_bad_arguments_before_any_launch():
    from p_companion_amd import _lib
    lib = _lib.lib()
    p, g, sv = _structs()
    x = ctypes.c_void_p(4096)                      # stands for a device pointer: never dereferenced on the way to the refusal
    none = None
    fwd, bwd = lib.pc_p2v_attention_forward_masked, lib.pc_p2v_attention_backward_masked
    assert fwd(ctypes.byref(p), x, x, none, 4, 3, x, ctypes.byref(sv), x, 1 << 30, None) == PC_EINVAL        # no key_pad
    assert fwd(ctypes.byref(p), x, x, x, 0, 3, x, ctypes.byref(sv), x, 1 << 30, None) == PC_EINVAL           # B = 0
    assert fwd(ctypes.byref(p), x, x, x, 4, 0, x, ctypes.byref(sv), x, 1 << 30, None) == PC_EINVAL           # N = 0
    assert fwd(None, x, x, x, 4, 3, x, ctypes.byref(sv), x, 1 << 30, None) == PC_EINVAL                      # no parameters
    assert fwd(ctypes.byref(p), x, x, x, 4, 3, x, ctypes.byref(sv), x, 1 << 30, None) == PC_EINVAL           # NULL weights / saved
    assert bwd(ctypes.byref(p), ctypes.byref(g), x, x, none, 4, 3, x, ctypes.byref(sv), x, x, 0, x, 1 << 30, None) == PC_EINVAL
    assert bwd(ctypes.byref(p), ctypes.byref(g), x, x, x, -1, 3, x, ctypes.byref(sv), x, x, 0, x, 1 << 30, None) == PC_EINVAL
    assert bwd(None, ctypes.byref(g), x, x, x, 4, 3, x, ctypes.byref(sv), x, x, 0, x, 1 << 30, None) == PC_EINVAL


def test_masked_step_entries_refuse_bad_arguments_before_any_launch():
    from p_companion_amd import _lib
    lib = _lib.lib()
    p, g, _ = _structs()
    P, G = ctypes.byref(p), ctypes.byref(g)
    x = ctypes.c_void_p(4096)
    B, N, K = 8, 4, 5
    tail = (x, x, x, x, None, x, 1 << 30)          # loss, d_pos, d_neg, anchor_emb, profile, ws, ws_bytes
    compact = lib.pc_p2v_train_step_compact_masked

    def cm(nb_rows=x, n_real=6, slot_row=x, b=B, n=N, k=K, table=x):
        return compact(P, G, table, x, x, x, nb_rows, n_real, slot_row, b, n, k, 1.0, *tail, None)
    assert cm(nb_rows=None) == PC_EINVAL and cm(slot_row=None) == PC_EINVAL
    assert cm(n_real=-1) == PC_EINVAL and cm(n_real=B * N + 1) == PC_EINVAL
    assert cm(n=0) == PC_EINVAL and cm(b=0) == PC_EINVAL and cm(k=0) == PC_EINVAL and cm(table=None) == PC_EINVAL
    assert cm(n_real=1) == PC_EBATCHNORM                                 # one real slot: a BatchNorm call of one row
    unique = lib.pc_p2v_train_step_unique_masked

    def um(step_rows=None, anchor=x, nb_weight=x, n_unique=5, n_slots=9, ref_off=x, ref_slot=x, b=B):
        return unique(P, G, x, anchor, x, x, step_rows, x, nb_weight, n_unique, n_slots, x, ref_off, ref_slot, b, N, K, 1.0,
                      *tail, None, None)
    assert um(nb_weight=None) == PC_EINVAL and um(ref_off=None) == PC_EINVAL and um(ref_slot=None) == PC_EINVAL
    assert um(anchor=None) == PC_EINVAL                                  # neither index arrays nor step_rows
    assert um(n_slots=-1) == PC_EINVAL
    assert um(n_slots=4) == PC_EINVAL                                    # fewer real slots than real rows
    assert um(n_slots=B * N + 1) == PC_EINVAL
    assert um(b=0) == PC_EINVAL
    assert um(n_unique=1, n_slots=1) == PC_EBATCHNORM
    assert um(n_unique=1, n_slots=1, step_rows=x, anchor=None) == PC_EBATCHNORM


def test_masked_with_sync_reduce_raises():
    from p_companion_amd import ops
    with pytest.raises(ValueError, match="sync_reduce"):
        ops.p2v_train_step({}, {}, None, None, None, None, None, 1.0, sync_reduce=lambda t: t, masked=True)


def test_wrappers_refuse_cpu_tensors_and_bad_masks():
    from p_companion_amd import ops
    with pytest.raises(TypeError):
        ops._key_pad(torch.zeros(2, 3, dtype=torch.bool), 2, 3)          # no CPU fallback
    with pytest.raises(ValueError, match="counts"):
        ops.make_segments([0, 4], 8, counts=[3])
    with pytest.raises(ValueError, match="Expected more than 1 value"):
        ops.make_segments([0], 8, counts=[1])                            # a logical count of one row
    s = ops.make_segments([0, 4], 8, counts=[0, 3])
    assert (s.count[0], s.count[1], s.nseg) == (0, 3, 2)


def test_unique_neighbors_counts_the_real_slots():
    from p_companion_amd import ops
    nb = torch.tensor([[3, -1, 5], [-1, -1, -1], [5, 5, 7]], dtype=torch.int32)
    uq = ops.unique_neighbors(nb)
    assert uq["n_real"] == 5 and uq["n_unique"] == 3 and float(uq["weight"][:3].sum()) == 5.0 and float(uq["weight"][3]) == 4.0
