"""pc_rank_grouped's host side and the catalogue metrics, without a GPU: the two entries are declared, exported and bound;
the workspace query depends on rows and n_types only; ops.rank_grouped refuses CPU tensors; evaluate_catalogue refuses what
it cannot serve before it touches the device; Metrics.catalogue_metrics against hand-written cases."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT

ENTRIES = ("pc_rank_grouped_workspace_bytes", "pc_rank_grouped")


def test_header_declares_library_exports_and_ctypes_binds_the_two_entries():
    from p_companion_amd import _lib
    txt = open(os.path.join(ROOT, "include", "pcompanion_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    declared = set(re.findall(r"\b(pc_[a-z0-9_]+)\s*\(", txt))
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in declared, name
        assert hasattr(L, name), f"{name} declared in the header but not exported"
        assert name in _lib.SIGNATURES, name
    # the argument lists as the header states them
    proto = re.search(r"int\s+pc_rank_grouped\s*\((.*?)\)\s*;", txt, flags=re.S).group(1)
    args = [a.strip() for a in proto.split(",")]
    assert len(args) == 16 == len(_lib.SIGNATURES["pc_rank_grouped"][1])
    for a, ct in zip(args, _lib.SIGNATURES["pc_rank_grouped"][1]):
        want = ctypes.c_void_p if "*" in a else ctypes.c_size_t if a.startswith("size_t") else ctypes.c_int
        assert ct is want, (a, ct)
    assert _lib.SIGNATURES["pc_rank_grouped_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 3)
    assert L.pc_abi_version() == 8                                      # additive entries: the ABI stays 8


def test_workspace_bytes_depend_on_rows_and_types_only():
    from p_companion_amd import _lib
    ws = _lib.lib().pc_rank_grouped_workspace_bytes
    rows, types = 12288, 100
    full = ws(rows, types, 0)
    # cnt [T] + pos [R] + row_start [T+1] + item_start [T+1] x 8 + order [R], each on a 256-byte boundary: no partial lists
    exact = sum((n + 255) // 256 * 256 for n in (types * 4, rows * 4, (types + 1) * 4, (types + 1) * 8, rows * 4))
    assert full == exact
    assert all(ws(rows, types, s) == full for s in (1, 7, 16, 64))
    assert ws(rows, 34_800, 0) > full and ws(2 * rows, types, 0) > full
    assert full < _lib.lib().pc_retrieve_topk_grouped_workspace_bytes(rows, types, 1, 1)
    for bad in ((0, types, 0), (rows, 0, 0), (-1, types, 0), (rows, types, -1), (rows, types, 65)):
        assert ws(*bad) == 0, bad


def test_rank_grouped_refuses_cpu_tensors():
    from p_companion_amd import ops
    proj = torch.zeros(2, 128)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    with pytest.raises(TypeError):
        ops.rank_grouped(proj, i32(0, 0), i32(0, 0), i32(0, 1), i32(0), torch.zeros(1, 128))
    with pytest.raises(ValueError):
        ops.rank_grouped(proj, i32(0, 0), i32(0, 0), i32(0, 1), i32(0), torch.zeros(1, 96))      # no kernel for this width


def _inference_over(bpg):
    """A PCompanionInference that holds its graph and nothing else: what evaluate_catalogue looks at before the device."""
    from p_companion_amd.inference import PCompanionInference
    inf = object.__new__(PCompanionInference)
    inf.bpg, inf.device, inf.grouped = bpg, torch.device("cpu"), False
    return inf


def _host_bpg(comp):
    from p_companion_amd.data import IntBPG
    P = 12
    z = np.zeros(0, np.int32)
    return IntBPG(features=np.zeros((P, 128), np.float32), type_idx=np.zeros(P, np.int32), category=np.zeros(P, np.int32),
                  cv_rowptr=np.zeros(P + 1, np.int32), cv_col=z,
                  similarity_pairs=np.array([[i, (i + 1) % P] for i in range(P)] * 4, np.int32),
                  complementary_pairs=np.asarray(comp, np.int32).reshape(-1, 2), n_types=1)


def test_evaluate_catalogue_refusals():
    from p_companion_amd.data import ComplementaryIndexDataset, DeviceBPG
    bpg = _host_bpg([[0, 1], [2, 3], [4, 5], [6, 7]] * 5)
    other = _host_bpg([[0, 1], [2, 3], [4, 5], [6, 7]] * 5)
    ds = ComplementaryIndexDataset(bpg, "test")
    # a dataset over another graph
    with pytest.raises(ValueError, match="another graph"):
        _inference_over(other).evaluate_catalogue(ds)
    with pytest.raises(ValueError, match="another graph"):
        _inference_over(bpg).evaluate_catalogue(SimpleNamespace(bpg=bpg, pairs=ds.pairs))
    # an empty +1 set: a graph without complementary pairs, and a split that happens to hold none
    none = _host_bpg(np.zeros((0, 2)))
    with pytest.raises(ValueError, match=r"no \+1 pair"):
        _inference_over(none).evaluate_catalogue(ComplementaryIndexDataset(none, "test"))
    ds.pairs = ds.pairs[ds.pairs[:, 2] == -1]
    assert len(ds.pairs)
    with pytest.raises(ValueError, match=r"no \+1 pair"):
        _inference_over(bpg).evaluate_catalogue(ds)
    # a sharded DeviceBPG (refused whatever the dataset)
    shard = DeviceBPG({"n_products": 12, "max_degree": 1}, 1, 128, rank=1, world=2)
    with pytest.raises(ValueError, match="shard"):
        _inference_over(shard).evaluate_catalogue(SimpleNamespace(bpg=shard, pairs=ds.pairs))
    with pytest.raises(ValueError, match="chunk"):
        _inference_over(bpg).evaluate_catalogue(ComplementaryIndexDataset(bpg, "test"), chunk=0)


def test_catalogue_metrics_hand_cases():
    from p_companion_amd.metrics import Metrics
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    # six pairs: ranks 0, 2, 9, 150 under slots 0 / 1 / 2 / 0, two pairs whose type no slot predicted
    slot, rank = i32([0, 1, 2, 0, -1, -1]), i32([0, 2, 9, 150, -1, -1])
    m = Metrics.catalogue_metrics(slot, rank)
    assert list(m) == ["pairs", "type_hit", "hit@1", "hit@3", "hit@10", "hit@100", "mrr", "median_rank"]
    assert m["pairs"] == 6 and m["type_hit"] == 4 / 6
    assert (m["hit@1"], m["hit@3"], m["hit@10"], m["hit@100"]) == (1 / 6, 2 / 6, 3 / 6, 3 / 6)
    assert m["mrr"] == pytest.approx((1 + 1 / 3 + 1 / 10 + 1 / 151) / 6, rel=1e-15)
    assert m["median_rank"] == 0.5 * (2 + 9)
    # `take`: the pairs that do not count change nothing, whatever they hold
    take = torch.tensor([True, False, True, True, False, True, True, True, False])
    slot2, rank2 = i32([0, 2, 1, 2, 0, 0, -1, -1, -1]), i32([0, 0, 2, 9, 5, 150, -1, -1, 7])
    assert Metrics.catalogue_metrics(slot2, rank2, take=take) == m
    # an odd number of ranked pairs, other ks, every pair ranked
    m = Metrics.catalogue_metrics(i32([2, 2, 2]), i32([4, 0, 16]), ks=(5, 16, 17))
    assert m == {"pairs": 3, "type_hit": 1.0, "hit@5": 2 / 3, "hit@16": 2 / 3, "hit@17": 1.0,
                 "mrr": pytest.approx((1 / 5 + 1 + 1 / 17) / 3, rel=1e-15), "median_rank": 4.0}
    # nothing matched: zeros, and the median says so
    m = Metrics.catalogue_metrics(i32([-1, -1]), i32([-1, -1]), ks=(1,))
    assert m == {"pairs": 2, "type_hit": 0.0, "hit@1": 0.0, "mrr": 0.0, "median_rank": -1.0}
    # a matched slot whose rank is missing (an id the kernel refused) counts as a type hit and as no hit@k
    m = Metrics.catalogue_metrics(i32([1, 0]), i32([-1, 3]), ks=(10,))
    assert m == {"pairs": 2, "type_hit": 1.0, "hit@10": 0.5, "mrr": 0.125, "median_rank": 3.0}
    with pytest.raises(ValueError):
        Metrics.catalogue_metrics(i32([]), i32([]))
    with pytest.raises(ValueError):
        Metrics.catalogue_metrics(i32([0, 1]), i32([0, 1]), take=torch.tensor([False, False]))
    with pytest.raises(ValueError):
        Metrics.catalogue_metrics(i32([0]), i32([0]), ks=(0,))
