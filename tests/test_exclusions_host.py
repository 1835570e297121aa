"""The host side of the exclusion lists (ops.retrieve_topk_grouped / ops.rank_grouped with `exclude`, ops.exclusion_csr,
Metrics.catalogue_metrics with filtered targets, the header): no GPU, no device call."""
import os
import re

import pytest
import torch

from conftest import ROOT


def _triple(rows=4, dtype=torch.int32):
    return (torch.zeros(rows, dtype=dtype), torch.zeros(3, dtype=dtype), torch.zeros(0, dtype=dtype))


def _call(fn, exclude, **kw):
    from p_companion_amd import ops
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)
    proj, table = torch.zeros(4, 128), torch.zeros(5, 128)
    if fn == "retrieve":
        return ops.retrieve_topk_grouped(proj, i32(4), i32(3), i32(5), table, 10, exclude=exclude, **kw)
    return ops.rank_grouped(proj, i32(4), i32(4), i32(3), i32(5), table, exclude=exclude, **kw)


@pytest.mark.parametrize("fn", ["retrieve", "rank"])
def test_a_malformed_exclude_triple_is_a_value_error_before_any_device_call(fn):
    """Every tensor here lives on the host: a call that reached the device checks would raise TypeError (no CPU fallback)."""
    kw = {"cand_type": torch.zeros(5, dtype=torch.int32)} if fn == "rank" else {}
    rk, rp, cl = _triple()
    for bad in ((rk, rp), (rk, rp, cl, cl), "lists", (rk, rp, None),
                (rk.long(), rp, cl), (rk, rp.long(), cl), (rk, rp, cl.float()),
                (rk[:3], rp, cl), (rk.reshape(2, 2), rp, cl), (rk, rp.reshape(3, 1), cl), (rk, rp[:0], cl)):
        with pytest.raises(ValueError, match="exclude"):
            _call(fn, bad, **kw)
    # a well-formed triple passes these checks and meets the device check
    with pytest.raises(TypeError, match="CUDA/ROCm"):
        _call(fn, (rk, rp, cl), **kw)


def test_rank_grouped_needs_cand_type_with_exclude_and_only_then():
    with pytest.raises(ValueError, match="cand_type"):
        _call("rank", _triple())
    for wrong in (torch.zeros(5, dtype=torch.int64), torch.zeros(4, dtype=torch.int32), torch.zeros(5, 1, dtype=torch.int32), [0] * 5):
        with pytest.raises(ValueError, match="cand_type"):
            _call("rank", _triple(), cand_type=wrong)
    with pytest.raises(ValueError, match="cand_type"):
        _call("rank", None, cand_type=torch.zeros(5, dtype=torch.int32))


def test_exclusion_csr_refuses_on_the_host():
    from p_companion_amd import ops
    rp, cl = torch.zeros(3, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    for a, b in ((rp.long(), cl), (rp, cl.long()), (rp.reshape(3, 1), cl), (rp[:0], cl)):
        with pytest.raises(ValueError, match="exclusion_csr"):
            ops.exclusion_csr(a, b)
    with pytest.raises(ValueError, match="31 bits"):
        ops.exclusion_csr(rp, cl, num_products=2 ** 31 - 2)
    with pytest.raises(ValueError, match="31 bits"):
        ops.exclusion_csr(rp, torch.zeros(1, dtype=torch.int32).expand(2 ** 31 - 2), num_products=2)   # (no memory behind it)


def test_catalogue_metrics_counts_a_filtered_target_as_a_miss_and_keeps_its_slot():
    from p_companion_amd.metrics import Metrics
    slot = torch.tensor([0, 2, 1, -1, 0, 1], dtype=torch.int32)
    rank = torch.tensor([0, -1, 4, -1, -1, 120], dtype=torch.int32)      # pairs 1 and 4: a slot, no rank -- filtered targets
    got = Metrics.catalogue_metrics(slot, rank, ks=(1, 10))
    assert got["pairs"] == 6 and got["type_hit"] == 5 / 6
    assert got["hit@1"] == 1 / 6 and got["hit@10"] == 2 / 6
    assert got["mrr"] == pytest.approx((1 + 1 / 5 + 1 / 121) / 6, rel=1e-15)
    assert got["median_rank"] == 4.0
    # the same pairs with their targets not filtered: type_hit is what it was
    unfiltered = Metrics.catalogue_metrics(slot, torch.tensor([0, 7, 4, -1, 30, 120], dtype=torch.int32), ks=(1, 10))
    assert unfiltered["type_hit"] == got["type_hit"] and unfiltered["hit@10"] == 3 / 6


def test_header_declares_both_entries():
    txt = open(os.path.join(ROOT, "include", "pcompanion_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    for name in ("pc_retrieve_topk_grouped_excluding", "pc_retrieve_topk_grouped_excluding_workspace_bytes",
                 "pc_rank_grouped_excluding"):
        assert re.search(r"\b" + name + r"\s*\(", txt), name
    from p_companion_amd import _lib
    sig = _lib.SIGNATURES
    assert len(sig["pc_retrieve_topk_grouped_excluding"][1]) == len(sig["pc_retrieve_topk_grouped"][1]) + 5
    assert len(sig["pc_rank_grouped_excluding"][1]) == len(sig["pc_rank_grouped"][1]) + 5
    assert re.search(r"#define PC_ABI_VERSION 8\b", txt)


def test_inference_methods_exist():
    from p_companion_amd.inference import PCompanionInference
    assert callable(PCompanionInference.set_exclusions) and callable(PCompanionInference.set_eligible)
