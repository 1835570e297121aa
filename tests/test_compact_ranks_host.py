"""The host side of the ranks and substitutes over the bf16 catalogue (pc_rank_grouped_bf16,
pc_retrieve_list_grouped_bf16_biased, pc_half_sq_norm_bias_bf16; ops.rank_grouped_bf16, ops.retrieve_list_grouped_bf16_biased,
ops.half_sq_norm_bias_bf16; inference.CompactSimilarProducts, inference.CompactInference), without a GPU: the header and the
ctypes table, what the entries and the wrappers refuse before anything is launched, the refusals of the fp32 names that stay
pinned, and that neither class reads the fp32 features of a graph."""
import ctypes
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import ROOT

PC_EINVAL, PC_ESHAPE, PC_EWORKSPACE = -1, -2, -3
ENTRIES = ("pc_half_sq_norm_bias_bf16", "pc_retrieve_list_grouped_bf16_biased",
           "pc_retrieve_list_grouped_bf16_biased_workspace_bytes", "pc_rank_grouped_bf16", "pc_rank_grouped_bf16_workspace_bytes")


def declared(code, name):
    """the parameter list of `name` in the header, one normalised 'type name' string per parameter"""
    m = re.search(r"\b%s\s*\(([^)]*)\)\s*;" % name, code)
    assert m, name
    return [" ".join(p.replace("*", " * ").split()) for p in m.group(1).split(",")]


def test_header_declares_the_entries_and_the_abi_stays_8():
    from p_companion_amd import _lib
    txt = open(os.path.join(ROOT, "include", "pcompanion_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    sig = _lib.SIGNATURES
    for name in ENTRIES:
        assert name in sig and len(declared(code, name)) == len(sig[name][1]), name
    assert re.search(r"#define\s+PC_ABI_VERSION\s+8\b", txt)
    # the fp32 biased entries' argument lists with the bf16 table in the place of the fp32 one
    bf16 = lambda params: [p.replace("const float * table", "const uint16_t * table_bf16") for p in params]
    assert declared(code, "pc_rank_grouped_bf16") == bf16(declared(code, "pc_rank_grouped_biased"))
    assert declared(code, "pc_retrieve_list_grouped_bf16_biased") == bf16(declared(code, "pc_retrieve_list_grouped_biased"))
    assert declared(code, "pc_half_sq_norm_bias_bf16") == bf16(declared(code, "pc_half_sq_norm_bias"))
    assert "const uint16_t * table_bf16" in declared(code, "pc_rank_grouped_bf16")
    assert sig["pc_rank_grouped_bf16"] == sig["pc_rank_grouped_biased"]
    assert sig["pc_retrieve_list_grouped_bf16_biased"] == sig["pc_retrieve_list_grouped_biased"]
    assert sig["pc_half_sq_norm_bias_bf16"] == sig["pc_half_sq_norm_bias"]
    assert sig["pc_rank_grouped_bf16_workspace_bytes"] == sig["pc_rank_grouped_workspace_bytes"]
    assert sig["pc_retrieve_list_grouped_bf16_biased_workspace_bytes"] == sig["pc_retrieve_list_grouped_workspace_bytes"]
    L = _lib.lib()
    assert L.pc_abi_version() == 8
    assert L.pc_rank_grouped_bf16_workspace_bytes.restype == ctypes.c_size_t


def test_the_units_are_part_of_the_build():
    from p_companion_amd import build
    assert {"rank_bf16.hip", "nearest_list_bf16.hip", "retrieve_list_bf16.hip"} <= set(build.sources())
    csrc = os.path.join(ROOT, "p_companion_amd", "csrc")
    # the bf16 chain is one text, in the header both list units include
    assert "struct RlChainBf16" in open(os.path.join(csrc, "grouped_list_bf16.h")).read()
    for unit in ("retrieve_list_bf16.hip", "nearest_list_bf16.hip"):
        text = open(os.path.join(csrc, unit)).read()
        assert '#include "grouped_list_bf16.h"' in text and "struct RlChainBf16" not in text, unit


def test_workspace_bytes_are_the_fp32_entries():
    from p_companion_amd import _lib
    L = _lib.lib()
    rows, types = 12288, 100
    for s in (0, 1, 64):
        assert L.pc_rank_grouped_bf16_workspace_bytes(rows, types, s) == L.pc_rank_grouped_workspace_bytes(rows, types, s) > 0
        for n in (1, 16, 17, 256):
            assert L.pc_retrieve_list_grouped_bf16_biased_workspace_bytes(rows, types, n, s) \
                == L.pc_retrieve_list_grouped_workspace_bytes(rows, types, n, s) > 0
    for bad in ((0, types, 0), (rows, 0, 0), (rows, types, -1), (rows, types, 65)):
        assert L.pc_rank_grouped_bf16_workspace_bytes(*bad) == 0, bad
    for bad in ((0, types, 10, 0), (rows, 0, 10, 0), (rows, types, 0, 0), (rows, types, 257, 0), (rows, types, 10, 65)):
        assert L.pc_retrieve_list_grouped_bf16_biased_workspace_bytes(*bad) == 0, bad


def _aligned():
    """One 16-byte aligned host buffer: a pointer that passes every check, and that no check dereferences."""
    buf = ctypes.create_string_buffer(96)
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)


def test_the_rank_refuses_before_anything_is_launched():
    from p_companion_amd import _lib
    entry = _lib.lib().pc_rank_grouped_bf16
    buf, p = _aligned()

    def call(**kw):
        a = dict(proj=p, types=p, targets=p, row_key=p, rows=4, type_rowptr=p, type_col=p, table=p, bias=p, n_types=3,
                 num_products=9, ex_rowptr=p, ex_col=p, n_keys=2, cand_type=p, dim=128, slices=0, rank_out=p, bad_count=p, ws=p,
                 ws_bytes=0, stream=None)
        a.update(kw)
        return entry(*a.values())

    for name in ("proj", "types", "targets", "type_rowptr", "type_col", "table", "rank_out", "bad_count", "ws", "row_key",
                 "ex_rowptr", "ex_col", "cand_type"):
        assert call(**{name: None}) == PC_EINVAL, name
    for kw in (dict(rows=0), dict(n_types=0), dict(num_products=0), dict(n_keys=-1)):
        assert call(**kw) == PC_EINVAL, kw
    none = dict(row_key=None, ex_rowptr=None, ex_col=None, n_keys=0, cand_type=None)
    for half in (dict(none, cand_type=p), dict(none, ex_rowptr=p), dict(none, ex_col=p), dict(none, n_keys=2)):
        assert call(**half) == PC_EINVAL, half
    for kw in (dict(dim=64), dict(dim=192), dict(slices=-1), dict(slices=65), dict(table=ctypes.c_void_p(p.value + 2)),
               dict(table=ctypes.c_void_p(p.value + 8))):
        assert call(**kw) == PC_ESHAPE, kw
        assert call(**kw, **none) == PC_ESHAPE, kw
    # the bias may be null: the call goes on to the workspace check
    for kw in ({}, none, dict(bias=None), dict(none, bias=None), dict(none, dim=256, slices=64)):
        assert call(**kw) == PC_EWORKSPACE, kw


def test_the_biased_list_refuses_before_anything_is_launched():
    from p_companion_amd import _lib
    entry = _lib.lib().pc_retrieve_list_grouped_bf16_biased
    buf, p = _aligned()

    def call(**kw):
        a = dict(proj=p, types=p, row_key=p, rows=4, type_rowptr=p, type_col=p, table=p, bias=p, n_types=3, ex_rowptr=p,
                 ex_col=p, n_keys=2, n=100, dim=128, slices=0, out_idx=p, out_score=p, bad_count=p, ws=p, ws_bytes=0, stream=None)
        a.update(kw)
        return entry(*a.values())

    for name in ("proj", "types", "type_rowptr", "type_col", "table", "bias", "out_idx", "out_score", "ws", "ex_rowptr", "ex_col",
                 "bad_count"):
        assert call(**{name: None}) == PC_EINVAL, name
    assert call(rows=0) == PC_EINVAL and call(n_types=0) == PC_EINVAL and call(n_keys=-1) == PC_EINVAL
    assert call(row_key=None) == PC_EINVAL
    none = dict(row_key=None, ex_rowptr=None, ex_col=None, n_keys=0, bad_count=None)
    for kw in (dict(n=0), dict(n=257), dict(dim=64), dict(slices=-1), dict(slices=65), dict(table=ctypes.c_void_p(p.value + 2))):
        assert call(**kw) == PC_ESHAPE, kw
        assert call(**kw, **none) == PC_ESHAPE, kw
    for kw in ({}, none, dict(none, n=1), dict(none, n=16), dict(none, n=256, dim=256)):
        assert call(**kw) == PC_EWORKSPACE, kw


def test_the_bias_entry_refuses_before_anything_is_launched():
    from p_companion_amd import _lib
    entry = _lib.lib().pc_half_sq_norm_bias_bf16
    buf, p = _aligned()
    assert entry(None, 4, 128, p, None) == PC_EINVAL and entry(p, 4, 128, None, None) == PC_EINVAL
    assert entry(p, 0, 128, p, None) == PC_EINVAL and entry(p, -3, 256, p, None) == PC_EINVAL
    for dim in (0, 64, 192, 512):
        assert entry(p, 4, dim, p, None) == PC_ESHAPE, dim
    assert entry(ctypes.c_void_p(p.value + 2), 4, 128, p, None) == PC_ESHAPE


class OnDevice(torch.Tensor):
    """A stand-in that reports is_cuda: _req tests the device first, and this lets the checks behind it be reached."""
    is_cuda = True


def test_the_wrappers_refuse_on_the_host_side():
    from p_companion_amd import ops
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)
    proj, bias = torch.zeros(4, 128), torch.zeros(5)
    table = torch.zeros(5, 128, dtype=torch.bfloat16)
    # the bias function
    with pytest.raises(TypeError, match="CUDA/ROCm"):
        ops.half_sq_norm_bias_bf16(table)
    with pytest.raises(ValueError, match="half_sq_norm_bias's"):
        ops.half_sq_norm_bias_bf16(table.float())
    with pytest.raises(TypeError, match="bfloat16"):
        ops.half_sq_norm_bias_bf16(torch.zeros(5, 128, dtype=torch.float16).as_subclass(OnDevice))
    with pytest.raises(ValueError, match=r"\[P, D\]"):
        ops.half_sq_norm_bias_bf16(torch.zeros(128, dtype=torch.bfloat16).as_subclass(OnDevice))
    with pytest.raises(ValueError, match="width"):
        ops.half_sq_norm_bias_bf16(torch.zeros(5, 64, dtype=torch.bfloat16).as_subclass(OnDevice))
    retrieve = lambda **kw: ops.retrieve_list_grouped_bf16_biased(proj, i32(4), i32(3), i32(5), kw.pop("table", table),
                                                                  kw.pop("bias", bias), kw.pop("n", 100), **kw)
    rank = lambda **kw: ops.rank_grouped_bf16(proj, i32(4), i32(4), i32(3), i32(5), kw.pop("table", table), **kw)
    for fn, fp32 in ((retrieve, "retrieve_list_grouped_biased"), (rank, "rank_grouped")):
        # well formed: the call goes on to the device check of its tensors
        with pytest.raises(TypeError, match="CUDA/ROCm"):
            fn(bias=bias)
        # an fp32 table: the message names the fp32 function
        with pytest.raises(ValueError, match=fp32 + "'s"):
            fn(bias=bias, table=table.float())
        for bad in (torch.zeros(5, 128, dtype=torch.float16), [[0.0] * 128] * 5, torch.zeros(128, dtype=torch.bfloat16)):
            with pytest.raises(ValueError, match="table"):
                fn(bias=bias, table=bad)
        for dtype in (torch.float64, torch.float16, torch.bfloat16, torch.int32):
            with pytest.raises(ValueError, match="float32"):
                fn(bias=bias.to(dtype))
        for shape in ((4,), (6,), (5, 1), (1, 5), ()):
            with pytest.raises(ValueError, match="one entry per product"):
                fn(bias=torch.zeros(shape))
        with pytest.raises(ValueError, match="bias must be"):
            fn(bias=[0.0] * 5)
        with pytest.raises(ValueError, match="exclude"):
            fn(bias=bias, exclude=(i32(4).long(), i32(3), i32(0)))
        with pytest.raises(ValueError, match="slices"):
            fn(bias=bias, slices=65)
    for n in (0, 257, -1):
        with pytest.raises(ValueError, match=r"\[1, 256\]"):
            retrieve(n=n)
    with pytest.raises(ValueError, match="bad counts keys"):
        retrieve(bad=i32(1))
    with pytest.raises(TypeError, match="CUDA/ROCm"):          # the rank's bias may be absent
        rank()
    with pytest.raises(ValueError, match="cand_type"):
        rank(exclude=(i32(4), i32(3), i32(0)))
    with pytest.raises(ValueError, match="cand_type"):
        rank(cand_type=i32(5))
    with pytest.raises(ValueError, match="cand_type"):
        rank(exclude=(i32(4), i32(3), i32(0)), cand_type=i32(4))


def test_the_pinned_refusals_of_the_fp32_names_still_fire():
    from p_companion_amd import ops
    from p_companion_amd.inference import PCompanionInference, SimilarProducts
    i32 = lambda n: torch.zeros(n, dtype=torch.int32)
    proj, bias = torch.zeros(4, 128).as_subclass(OnDevice), torch.zeros(5)
    bf16 = torch.zeros(5, 128, dtype=torch.bfloat16).as_subclass(OnDevice)
    dev = lambda t: t.as_subclass(OnDevice)
    with pytest.raises(TypeError, match="float32"):
        ops.rank_grouped(proj, dev(i32(4)), dev(i32(4)), dev(i32(3)), dev(i32(5)), bf16)
    with pytest.raises(ValueError, match="bf16 table"):
        ops.retrieve_topk_grouped(proj, i32(4), i32(3), i32(5), bf16, 5, bias=bias)
    with pytest.raises(ValueError, match="bf16 table"):
        ops.retrieve_list_grouped_biased(proj, i32(4), i32(3), i32(5), bf16, bias, 100)
    with pytest.raises(ValueError, match="bf16 table"):
        ops.rank_grouped(proj, i32(4), i32(4), i32(3), i32(5), bf16, bias=bias)
    with pytest.raises(ValueError, match="float32"):
        SimilarProducts(torch.zeros(7, 128, dtype=torch.bfloat16), Untouchable())
    for catalogue in (bf16, object.__new__(ops.CompactCatalogue)):
        inf = object.__new__(PCompanionInference)
        inf.__dict__.update(catalogue=catalogue, features=Untouchable(), model=Untouchable(), bpg=Untouchable())
        with pytest.raises(ValueError, match="rank_targets: .*fp32 catalogue"):
            inf.rank_targets(i32(2), i32(2))
        with pytest.raises(ValueError, match="evaluate_catalogue: .*fp32 catalogue"):
            inf.evaluate_catalogue(None)
    assert _lib_abi() == 8


def _lib_abi():
    from p_companion_amd import _lib
    return _lib.lib().pc_abi_version()


class Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"read .{name} before refusing")


def test_the_classes_refuse_before_the_graph_is_touched():
    from p_companion_amd.inference import CompactInference, CompactSimilarProducts
    for bad, what in ((torch.zeros(7, 128), "bfloat16"), (torch.zeros(7, 128, dtype=torch.float64), "bfloat16"),
                      ([[0.0] * 128] * 7, "CompactCatalogue"), (None, "CompactCatalogue"),
                      (torch.zeros(7, 64, dtype=torch.bfloat16), r"\[P >= 1, 128 or 256\]"),
                      (torch.zeros(7 * 128, dtype=torch.bfloat16), r"\[P >= 1, 128 or 256\]"),
                      (torch.zeros(0, 128, dtype=torch.bfloat16), r"\[P >= 1, 128 or 256\]"),
                      (torch.zeros(7, 128, dtype=torch.bfloat16), "device tensor")):
        with pytest.raises(ValueError, match=what):
            CompactSimilarProducts(bad, Untouchable())
    with pytest.raises(ValueError, match="scope"):
        CompactSimilarProducts(torch.zeros(7, 128, dtype=torch.bfloat16), Untouchable(), scope="category")
    for bad in (None, torch.bfloat16, torch.zeros(7, 128, dtype=torch.bfloat16), torch.zeros(7, 128)):
        with pytest.raises(ValueError, match="ops.CompactCatalogue"):
            CompactInference(Untouchable(), Untouchable(), Untouchable(), catalogue=bad)
    sp = object.__new__(CompactSimilarProducts)                       # (no table, no graph, no device)
    sp.__dict__.update(table=Untouchable(), bpg=Untouchable(), exclusions=Untouchable(), compact=Untouchable())
    q = torch.zeros(2, dtype=torch.int32)
    for n in (17, 0):
        with pytest.raises(ValueError, match="1 to 16"):
            sp.similar_batch(q, n)
    for n in (257, 0):
        with pytest.raises(ValueError, match="1 to 256"):
            sp.similar_list_batch(q, n)


class NoFeatures(dict):
    """the arrays of a graph generated without features: asking for them is the failure"""
    def __getitem__(self, key):
        assert key != "features", "read the fp32 features"
        return dict.__getitem__(self, key)

    def get(self, key, default=None):
        assert key != "features", "read the fp32 features"
        return dict.get(self, key, default)

    def __contains__(self, key):
        return key != "features" and dict.__contains__(self, key)


def test_neither_class_touches_the_features_of_a_graph_without_them(monkeypatch):
    """Both classes built and driven on the host, the device entries replaced by recorders: the graph's arrays answer every key
    but "features", and every table the entries are handed is the bf16 copy."""
    from p_companion_amd import ops
    from p_companion_amd.inference import CompactInference, CompactSimilarProducts
    P, T, D, K = 12, 3, 128, 2
    type_idx = torch.arange(P, dtype=torch.int32) % T
    arrays = NoFeatures(type_idx=type_idx, cv_rowptr=torch.zeros(P + 1, dtype=torch.int32), cv_col=torch.zeros(0, dtype=torch.int32))
    bpg = SimpleNamespace(num_products=P, n_types=T, type_idx=type_idx.numpy(), cuda=lambda device=None: arrays)
    cc = object.__new__(ops.CompactCatalogue)
    cc.table = torch.randn(P, D).to(torch.bfloat16).as_subclass(OnDevice)
    cc._half_sq_norm = torch.zeros(P)
    seen = []

    def lists(proj, types, rowptr, col, table, *rest, **kw):
        n = next(x for x in rest if isinstance(x, int))
        seen.append(table)
        return torch.zeros(proj.shape[0], n, dtype=torch.int32), torch.zeros(proj.shape[0], n)

    def ranks(proj, types, targets, rowptr, col, table, **kw):
        seen.append(table)
        return torch.zeros(proj.shape[0], dtype=torch.int32), torch.zeros(1, dtype=torch.int32)

    def host_csr(t, n):
        order = torch.argsort(t, stable=True).to(torch.int32)
        return torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(torch.bincount(t, minlength=n), 0)]).to(torch.int32), order

    monkeypatch.setattr(ops, "retrieve_list_grouped_bf16_biased", lists)
    monkeypatch.setattr(ops, "retrieve_list_grouped", lists)
    monkeypatch.setattr(ops, "retrieve_topk_grouped", lists)
    monkeypatch.setattr(ops, "rank_grouped_bf16", ranks)
    monkeypatch.setattr(ops, "type_csr", host_csr)
    monkeypatch.setattr(ops, "cap_lists", lambda idx, score, n, *a, **k: (idx[:, :n], score[:, :n]))
    monkeypatch.setattr(ops, "exclusion_csr", lambda rowptr, col, include_self=True, num_products=None: (rowptr, col))
    for name in ("rank_grouped", "retrieve_list_grouped_biased", "half_sq_norm_bias", "half_sq_norm_bias_bf16"):
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("an fp32 entry, or a bias formed twice"))
    q = torch.tensor([0, 5, 7], dtype=torch.int32)
    for scope in ("type", "catalogue"):
        sp = CompactSimilarProducts(cc, bpg, scope=scope)
        assert sp.table is cc.table and sp.bias is cc._half_sq_norm
        sp.similar_batch(q, 4), sp.similar_list_batch(q, 40), sp.similar_capped_batch(q, 4), sp.similar_capped_list_batch(q, 4, pool=40)
        slot, rank = sp.rank_pairs(q, torch.tensor([3, 4, 7], dtype=torch.int32))
        assert slot.tolist() == ([0, -1, 0] if scope == "type" else [0, 0, 0])
        assert sp.evaluate_pairs(np.array([[0, 3], [5, 8]]))["pairs"] == 2
    assert len(seen) == 2 * 6 and all(t is cc.table for t in seen)

    class Model(torch.nn.Module):
        def forward(self, batch):
            b = batch["query_idx"].shape[0]
            return {"complementary_types": torch.arange(K).repeat(b, 1), "projected_embeddings": torch.zeros(b, K, D)}

    del seen[:]
    config = SimpleNamespace(DEVICE=torch.device("cpu"), NUM_COMP_TYPES=K)
    inf = CompactInference(Model(), config, bpg, catalogue=cc)
    assert inf.features is None and inf.catalogue is cc.table
    inf.recommend_batch(q, 10), inf.recommend_batch(q, 100)
    slot, rank = inf.rank_targets(q, torch.tensor([3, 4, 8], dtype=torch.int32))
    assert slot.tolist() == [0, 1, -1]
    inf.set_exclusions()
    inf.set_eligible(torch.ones(P, dtype=torch.bool))
    inf.rank_targets(q, torch.tensor([3, 4, 8], dtype=torch.int32))
    assert len(seen) == 4 and all(t is cc.table for t in seen)
