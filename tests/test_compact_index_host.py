"""The host side of the cell index over the bf16 catalogue (pc_cell_means_bf16; ops.cell_means_bf16, ops.build_cell_index_bf16;
inference.IndexedCompactSimilarProducts) without a GPU: the header and the ctypes table, what the entry refuses before anything
is launched, and the argument checks of the wrappers and the class that need no device."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

from conftest import ROOT
from test_cell_index_host import OnDevice, Untouchable, dev

PC_EINVAL, PC_ESHAPE = -1, -2
BF16 = torch.bfloat16


def test_header_declares_the_entry_and_the_abi_stays_8():
    from p_companion_amd import _lib
    txt = open(os.path.join(ROOT, "include", "pcompanion_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"#define\s+PC_ABI_VERSION\s+8\b", txt)
    m = re.search(r"\bint\s+pc_cell_means_bf16\s*\(([^)]*)\)\s*;", code)
    assert m
    # the header's argument list -> ctypes: every pointer travels as an address, every count as an int
    want = [ctypes.c_void_p if "*" in a else {"int": ctypes.c_int}[a.split()[0]] for a in m.group(1).split(",")]
    assert _lib.SIGNATURES["pc_cell_means_bf16"] == (ctypes.c_int, want)
    assert len(want) == 8
    assert _lib.SIGNATURES["pc_cell_means_bf16"] == _lib.SIGNATURES["pc_cell_means"]
    L = _lib.lib()
    assert L.pc_abi_version() == 8
    assert L.pc_cell_means_bf16.restype == ctypes.c_int


def test_the_unit_is_part_of_the_build():
    from p_companion_amd import build
    assert "cells_bf16.hip" in build.sources() and "cells.hip" in build.sources()


def test_cell_means_bf16_refuses_before_anything_is_launched():
    from p_companion_amd import _lib
    entry = _lib.lib().pc_cell_means_bf16
    buf = ctypes.create_string_buffer(96)                               # (a pointer that passes every check; none dereferences it)
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)

    def call(**kw):
        a = dict(table=p, cell_rowptr=p, cell_col=p, n_cells=3, num_products=9, dim=128, centroids=p, stream=None)
        a.update(kw)
        return entry(*a.values())

    for name in ("table", "cell_rowptr", "cell_col", "centroids"):
        assert call(**{name: None}) == PC_EINVAL, name
    for kw in (dict(n_cells=0), dict(n_cells=-1), dict(num_products=0), dict(num_products=-5)):
        assert call(**kw) == PC_EINVAL, kw
    # the family's order: a null pointer or a bad count is reported before a bad shape
    for name in ("table", "cell_rowptr", "cell_col", "centroids"):
        assert call(**{name: None}, dim=64) == PC_EINVAL, name
    assert call(n_cells=0, dim=64) == PC_EINVAL and call(num_products=0, dim=512) == PC_EINVAL
    for dim in (0, 64, 192, 512):
        assert call(dim=dim) == PC_ESHAPE, dim
    off = ctypes.c_void_p(p.value + 4)                                  # 8-byte loads of the rows, 16-byte stores of the centroids
    assert call(table=off) == PC_ESHAPE and call(table=off, dim=256) == PC_ESHAPE
    assert call(centroids=off) == PC_ESHAPE and call(centroids=off, dim=256) == PC_ESHAPE


def test_cell_means_bf16_refuses_cpu_tensors_wrong_dtypes_and_wrong_shapes():
    """cell_means' checks and messages with the table's dtype swapped."""
    from p_companion_amd import ops
    i32 = torch.int32
    good = dict(table=dev(9, 128, dtype=BF16), cell_rowptr=dev(4, dtype=i32), cell_col=dev(9, dtype=i32), centroids=dev(3, 128))
    for name in good:
        with pytest.raises(TypeError, match="CUDA/ROCm"):
            ops.cell_means_bf16(**{**good, name: torch.zeros_like(good[name]).as_subclass(torch.Tensor)})
    for name, dtype in (("table", torch.float64), ("table", torch.float16), ("centroids", BF16), ("cell_rowptr", torch.int64),
                        ("cell_col", torch.int64)):
        with pytest.raises(TypeError, match="expected torch"):
            ops.cell_means_bf16(**{**good, name: dev(*good[name].shape, dtype=dtype)})
    with pytest.raises(ValueError, match=r"cell_means's"):               # an fp32 table is pointed at the fp32 function
        ops.cell_means_bf16(**{**good, "table": dev(9, 128)})
    b = lambda *shape: dev(*shape, dtype=BF16)
    for kw, what in ((dict(table=b(9 * 128)), r"\[P, D\]"), (dict(table=b(9, 64)), "width"), (dict(table=b(0, 128)), "one row"),
                     (dict(centroids=dev(3, 256)), "centroids"), (dict(centroids=dev(3 * 128)), "centroids"),
                     (dict(centroids=dev(0, 128)), "centroids"), (dict(cell_rowptr=dev(3, dtype=i32)), "cell_rowptr"),
                     (dict(cell_rowptr=dev(5, dtype=i32)), "cell_rowptr"), (dict(cell_col=dev(3, 3, dtype=i32)), "cell_col")):
        with pytest.raises(ValueError, match=what):
            ops.cell_means_bf16(**{**good, **kw})
    # the fp32 wrapper still refuses the bf16 table
    with pytest.raises(TypeError, match="expected torch"):
        ops.cell_means(**good)


def test_build_cell_index_bf16_refuses_bad_arguments():
    """build_cell_index's checks and messages with the table's dtype swapped."""
    from p_companion_amd import ops
    table = dev(7, 128, dtype=BF16)
    with pytest.raises(TypeError, match="CUDA/ROCm"):
        ops.build_cell_index_bf16(torch.zeros(7, 128, dtype=BF16), 3)
    with pytest.raises(TypeError, match="expected torch"):
        ops.build_cell_index_bf16(dev(7, 128, dtype=torch.float64), 3)
    with pytest.raises(ValueError, match=r"build_cell_index's"):         # an fp32 table is pointed at the fp32 function
        ops.build_cell_index_bf16(dev(7, 128), 3)
    with pytest.raises(ValueError, match="width"):
        ops.build_cell_index_bf16(dev(7, 64, dtype=BF16), 3)
    with pytest.raises(ValueError, match=r"\[P, D\]"):
        ops.build_cell_index_bf16(dev(7 * 128, dtype=BF16), 3)
    for n_cells in (0, -1, 8, 100):
        with pytest.raises(ValueError, match="n_cells"):
            ops.build_cell_index_bf16(table, n_cells)
    for shape in ((3, 256), (4, 128), (2, 128), (3 * 128,)):
        with pytest.raises(ValueError, match="init"):
            ops.build_cell_index_bf16(table, 3, init=dev(*shape))
    with pytest.raises(TypeError, match="CUDA/ROCm"):
        ops.build_cell_index_bf16(table, 3, init=torch.zeros(3, 128))
    with pytest.raises(TypeError, match="expected torch"):               # init is fp32, as the centroids are
        ops.build_cell_index_bf16(table, 3, init=dev(3, 128, dtype=BF16))
    with pytest.raises(ValueError, match="iters"):
        ops.build_cell_index_bf16(table, 3, iters=-1)
    with pytest.raises(ValueError, match="chunk_rows"):
        ops.build_cell_index_bf16(table, 3, chunk_rows=0)
    # new names only: the fp32 build still refuses a bf16 table
    with pytest.raises(TypeError, match="expected torch"):
        ops.build_cell_index(table, 3)


def test_the_methods_refuse_their_limits_before_anything_is_touched():
    from p_companion_amd.inference import IndexedCompactSimilarProducts, IndexedSimilarProducts
    assert IndexedCompactSimilarProducts.MAX_NPROBE == 64 and IndexedSimilarProducts.MAX_NPROBE == 16
    q = torch.zeros(2, dtype=torch.int32)
    for cells, too_many in ((12, (13, 17, 65, 100)), (40, (41, 65)), (64, (65, 100)), (5000, (65, 4096))):
        sp = object.__new__(IndexedCompactSimilarProducts)            # (no catalogue, no graph, no index, no device)
        sp.__dict__.update(table=Untouchable(), compact=Untouchable(), bpg=Untouchable(), exclusions=Untouchable(),
                           index=Untouchable(), cell_rowptr=Untouchable(), cell_col=Untouchable(), n_cells=cells, nprobe=8)
        for n in (0, 17, -1, 100):
            with pytest.raises(ValueError, match="1 to 16"):
                sp.similar_batch(q, n)
        for n in (0, 257, -1, 1000):
            with pytest.raises(ValueError, match="1 to 256"):
                sp.similar_list_batch(q, n)
        for nprobe in (0, -1) + too_many:
            with pytest.raises(ValueError, match="nprobe"):
                sp.similar_batch(q, 10, nprobe=nprobe)
            with pytest.raises(ValueError, match="nprobe"):
                sp.similar_list_batch(q, 64, nprobe=nprobe)
            with pytest.raises(ValueError, match="nprobe"):
                sp.probe_cells(q, nprobe)
            with pytest.raises(ValueError, match="nprobe"):
                sp.recall(q, 10, nprobe)
        sp.nprobe = 0                                                 # None takes the object's value
        with pytest.raises(ValueError, match="nprobe"):
            sp.similar_batch(q, 10)
        with pytest.raises(NotImplementedError, match="IndexedCompactSimilarProducts.similar_where_batch"):
            sp.similar_where_batch(q, 10)


def test_the_constructor_refuses_before_anything_is_touched():
    from p_companion_amd.inference import IndexedCompactSimilarProducts as ICSP
    table = torch.zeros(7, 128, dtype=BF16)
    index = lambda p, d, c=3: SimpleNamespace(num_products=p, dim=d, n_cells=c)
    with pytest.raises(ValueError, match="IndexedCompactSimilarProducts: pass an index, or n_cells"):
        ICSP(table, Untouchable())
    with pytest.raises(ValueError, match="index, or n_cells"):
        ICSP(table, Untouchable(), index=index(7, 128), n_cells=3)
    for bad in (index(8, 128), index(7, 256), index(6, 64)):          # an index over another P or D
        with pytest.raises(ValueError, match="the index is over"):
            ICSP(table, Untouchable(), index=bad)
    for kw in (dict(n_cells=3, nprobe=0), dict(n_cells=3, nprobe=-1), dict(n_cells=3, nprobe=4), dict(n_cells=100, nprobe=65),
               dict(index=index(7, 128, 5), nprobe=6), dict(index=index(7, 128, 80), nprobe=65)):
        with pytest.raises(ValueError, match="nprobe"):
            ICSP(table, Untouchable(), **kw)
    # the table's own checks are the compact parent's, still ahead of the graph
    with pytest.raises(ValueError, match="device tensor"):
        ICSP(table, Untouchable(), n_cells=3, nprobe=2)
    with pytest.raises(ValueError, match="128 or 256"):
        ICSP(torch.zeros(7, 64, dtype=BF16), Untouchable(), n_cells=3, nprobe=2)
    with pytest.raises(ValueError, match="must be torch.bfloat16"):
        ICSP(torch.zeros(7, 128), Untouchable(), n_cells=3, nprobe=2)


def test_the_exact_paths_and_the_steps_are_the_parents():
    """rank_pairs / evaluate_pairs are SimilarProducts' own functions (their device calls go through the compact hooks); the
    indexed steps are IndexedSimilarProducts' own; what differs is the index build and the scan."""
    from p_companion_amd.inference import (CompactSimilarProducts, IndexedCompactSimilarProducts as ICSP, IndexedSimilarProducts,
                                           SimilarProducts)
    for name in ("rank_pairs", "evaluate_pairs", "set_exclusions", "_excluded", "similar_capped_batch",
                 "similar_capped_list_batch"):
        assert getattr(ICSP, name) is getattr(SimilarProducts, name), name
    for name in ("similar_batch", "similar_list_batch", "probe_cells", "recall", "set_eligible", "similar_where_batch", "_search",
                 "_probe", "__init__"):
        assert getattr(ICSP, name) is getattr(IndexedSimilarProducts, name), name
    for name in ("_rank", "_rows", "_check_table", "_half_sq_norm", "_retrieve", "_retrieve_list"):
        assert getattr(ICSP, name) is getattr(CompactSimilarProducts, name), name
    assert ICSP._scan is not IndexedSimilarProducts._scan and ICSP._build_index is not IndexedSimilarProducts._build_index
