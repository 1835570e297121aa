"""The host side of the k-means cell index (pc_cell_means, pc_merge_lists; ops.cell_means, ops.merge_lists,
ops.build_cell_index; inference.IndexedSimilarProducts) without a GPU: the header and the ctypes table, what the entries refuse
before anything is launched, and the argument checks of the wrappers and the class that need no device."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

from conftest import ROOT

PC_EINVAL, PC_ESHAPE = -1, -2
ENTRIES = ("pc_cell_means", "pc_merge_lists")


def test_header_declares_the_entries_and_the_abi_stays_8():
    from p_companion_amd import _lib
    txt = open(os.path.join(ROOT, "include", "pcompanion_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"#define\s+PC_ABI_VERSION\s+8\b", txt)
    for name in ENTRIES:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, code)
        assert m, name
        # the header's argument list -> ctypes: every pointer travels as an address, every count as an int
        want = [ctypes.c_void_p if "*" in a else {"int": ctypes.c_int}[a.split()[0]] for a in m.group(1).split(",")]
        assert _lib.SIGNATURES[name] == (ctypes.c_int, want), name
    assert len(_lib.SIGNATURES["pc_cell_means"][1]) == 8 and len(_lib.SIGNATURES["pc_merge_lists"][1]) == 8
    L = _lib.lib()
    assert L.pc_abi_version() == 8
    for name in ENTRIES:
        assert getattr(L, name).restype == ctypes.c_int


def test_the_unit_is_part_of_the_build():
    from p_companion_amd import build
    assert "cells.hip" in build.sources()


def _aligned():
    """One 16-byte aligned host buffer: a pointer that passes every check, and that no check dereferences."""
    buf = ctypes.create_string_buffer(96)
    return buf, ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)


def test_cell_means_refuses_before_anything_is_launched():
    from p_companion_amd import _lib
    entry = _lib.lib().pc_cell_means
    buf, p = _aligned()

    def call(**kw):
        a = dict(table=p, cell_rowptr=p, cell_col=p, n_cells=3, num_products=9, dim=128, centroids=p, stream=None)
        a.update(kw)
        return entry(*a.values())

    for name in ("table", "cell_rowptr", "cell_col", "centroids"):
        assert call(**{name: None}) == PC_EINVAL, name
    for kw in (dict(n_cells=0), dict(n_cells=-1), dict(num_products=0), dict(num_products=-5)):
        assert call(**kw) == PC_EINVAL, kw
    # the family's order: a null pointer or a bad count is reported before a bad shape
    assert call(table=None, dim=64) == PC_EINVAL and call(n_cells=0, dim=64) == PC_EINVAL
    for dim in (0, 64, 192, 512):
        assert call(dim=dim) == PC_ESHAPE, dim
    off = ctypes.c_void_p(p.value + 4)                                   # 16-byte loads and stores
    assert call(table=off) == PC_ESHAPE and call(centroids=off, dim=256) == PC_ESHAPE


def test_merge_lists_refuses_before_anything_is_launched():
    from p_companion_amd import _lib
    entry = _lib.lib().pc_merge_lists
    buf, p = _aligned()

    def call(**kw):
        a = dict(idx=p, score=p, rows=4, L=8, n=10, out_idx=p, out_score=p, stream=None)
        a.update(kw)
        return entry(*a.values())

    for name in ("idx", "score", "out_idx", "out_score"):
        assert call(**{name: None}) == PC_EINVAL, name
    assert call(rows=0) == PC_EINVAL and call(rows=-2) == PC_EINVAL
    assert call(idx=None, L=0) == PC_EINVAL and call(rows=0, n=257) == PC_EINVAL
    for kw in (dict(L=0), dict(L=65), dict(L=-1), dict(n=0), dict(n=257), dict(n=-1)):
        assert call(**kw) == PC_ESHAPE, kw


class OnDevice(torch.Tensor):
    """A stand-in that reports is_cuda: _req tests the device first, and this lets the checks behind it be reached."""
    is_cuda = True


def dev(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype).as_subclass(OnDevice)


def test_the_wrappers_refuse_cpu_tensors_wrong_dtypes_and_wrong_shapes():
    from p_companion_amd import ops
    i32 = torch.int32
    good = dict(table=dev(9, 128), cell_rowptr=dev(4, dtype=i32), cell_col=dev(9, dtype=i32), centroids=dev(3, 128))
    for name in good:
        with pytest.raises(TypeError, match="CUDA/ROCm"):
            ops.cell_means(**{**good, name: torch.zeros_like(good[name]).as_subclass(torch.Tensor)})
    for name, dtype in (("table", torch.float64), ("centroids", torch.bfloat16), ("cell_rowptr", torch.int64),
                        ("cell_col", torch.int64)):
        with pytest.raises(TypeError, match="expected torch"):
            ops.cell_means(**{**good, name: dev(*good[name].shape, dtype=dtype)})
    for kw, what in ((dict(table=dev(9 * 128)), r"\[P, D\]"), (dict(table=dev(9, 64)), "width"), (dict(table=dev(0, 128)), "one row"),
                     (dict(centroids=dev(3, 256)), "centroids"), (dict(centroids=dev(3 * 128)), "centroids"),
                     (dict(centroids=dev(0, 128)), "centroids"), (dict(cell_rowptr=dev(3, dtype=i32)), "cell_rowptr"),
                     (dict(cell_rowptr=dev(5, dtype=i32)), "cell_rowptr"), (dict(cell_col=dev(3, 3, dtype=i32)), "cell_col")):
        with pytest.raises(ValueError, match=what):
            ops.cell_means(**{**good, **kw})

    with pytest.raises(TypeError, match="CUDA/ROCm"):
        ops.merge_lists(torch.zeros(4, 2, 10, dtype=i32), torch.zeros(4, 2, 10))
    with pytest.raises(TypeError, match="expected torch"):
        ops.merge_lists(dev(4, 2, 10, dtype=torch.int64), dev(4, 2, 10))
    with pytest.raises(TypeError, match="expected torch"):
        ops.merge_lists(dev(4, 2, 10, dtype=i32), dev(4, 2, 10, dtype=torch.float64))
    for ishape, sshape, what in (((4, 20), (4, 20), r"\[R, L, n\]"), ((4, 2, 10), (4, 2, 9), r"\[R, L, n\]"),
                                 ((4, 0, 10), (4, 0, 10), "L must be"), ((4, 65, 10), (4, 65, 10), "L must be"),
                                 ((4, 2, 0), (4, 2, 0), "n must be"), ((4, 2, 257), (4, 2, 257), "n must be")):
        with pytest.raises(ValueError, match=what):
            ops.merge_lists(dev(*ishape, dtype=i32), dev(*sshape))


def test_build_cell_index_refuses_bad_arguments():
    from p_companion_amd import ops
    table = dev(7, 128)
    with pytest.raises(TypeError, match="CUDA/ROCm"):
        ops.build_cell_index(torch.zeros(7, 128), 3)
    with pytest.raises(TypeError, match="expected torch"):
        ops.build_cell_index(dev(7, 128, dtype=torch.float64), 3)
    with pytest.raises(ValueError, match="width"):
        ops.build_cell_index(dev(7, 64), 3)
    for n_cells in (0, -1, 8, 100):
        with pytest.raises(ValueError, match="n_cells"):
            ops.build_cell_index(table, n_cells)
    for shape in ((3, 256), (4, 128), (2, 128), (3 * 128,)):
        with pytest.raises(ValueError, match="init"):
            ops.build_cell_index(table, 3, init=dev(*shape))
    with pytest.raises(TypeError, match="CUDA/ROCm"):
        ops.build_cell_index(table, 3, init=torch.zeros(3, 128))
    with pytest.raises(ValueError, match="iters"):
        ops.build_cell_index(table, 3, iters=-1)
    with pytest.raises(ValueError, match="chunk_rows"):
        ops.build_cell_index(table, 3, chunk_rows=0)


class Untouchable:
    def __getattr__(self, name):
        raise AssertionError(f"read .{name} before refusing")


def test_similar_batch_refuses_its_limits_before_anything_is_touched():
    from p_companion_amd.inference import IndexedSimilarProducts
    q = torch.zeros(2, dtype=torch.int32)
    for cells, too_many in ((12, (13, 17, 100)), (64, (17, 65))):
        sp = object.__new__(IndexedSimilarProducts)                   # (no table, no graph, no index, no device)
        sp.__dict__.update(table=Untouchable(), bpg=Untouchable(), exclusions=Untouchable(), index=Untouchable(),
                           cell_rowptr=Untouchable(), cell_col=Untouchable(), n_cells=cells, nprobe=8)
        for n in (0, 17, -1, 100):
            with pytest.raises(ValueError, match="1 to 16"):
                sp.similar_batch(q, n)
        for nprobe in (0, -1) + too_many:
            with pytest.raises(ValueError, match="nprobe"):
                sp.similar_batch(q, 10, nprobe=nprobe)
            with pytest.raises(ValueError, match="nprobe"):
                sp.probe_cells(q, nprobe)
            with pytest.raises(ValueError, match="nprobe"):
                sp.recall(q, 10, nprobe)
        sp.nprobe = 0                                                 # None takes the object's value
        with pytest.raises(ValueError, match="nprobe"):
            sp.similar_batch(q, 10)


def test_the_constructor_refuses_before_anything_is_touched():
    from p_companion_amd.inference import IndexedSimilarProducts
    table = torch.zeros(7, 128)
    index = lambda p, d, c=3: SimpleNamespace(num_products=p, dim=d, n_cells=c)
    with pytest.raises(ValueError, match="index, or n_cells"):
        IndexedSimilarProducts(table, Untouchable())
    with pytest.raises(ValueError, match="index, or n_cells"):
        IndexedSimilarProducts(table, Untouchable(), index=index(7, 128), n_cells=3)
    for bad in (index(8, 128), index(7, 256), index(6, 64)):          # an index over another P or D
        with pytest.raises(ValueError, match="the index is over"):
            IndexedSimilarProducts(table, Untouchable(), index=bad)
    for kw in (dict(n_cells=3, nprobe=0), dict(n_cells=3, nprobe=4), dict(n_cells=100, nprobe=17),
               dict(index=index(7, 128, 5), nprobe=6)):
        with pytest.raises(ValueError, match="nprobe"):
            IndexedSimilarProducts(table, Untouchable(), **kw)
    # the table's own checks are the parent's, still ahead of the graph
    with pytest.raises(ValueError, match="device tensor"):
        IndexedSimilarProducts(table, Untouchable(), n_cells=3, nprobe=2)
    with pytest.raises(ValueError, match=r"\[P, 128 or 256\]"):
        IndexedSimilarProducts(torch.zeros(7, 64), Untouchable(), n_cells=3, nprobe=2)


def test_the_exact_paths_are_the_parents():
    """rank_pairs / evaluate_pairs are inherited, not re-implemented; the filters stay the shared ones but for set_eligible,
    which also filters the cell CSR."""
    from p_companion_amd.inference import IndexedSimilarProducts, SimilarProducts
    for name in ("rank_pairs", "evaluate_pairs", "set_exclusions", "_excluded"):
        assert getattr(IndexedSimilarProducts, name) is getattr(SimilarProducts, name), name
    assert IndexedSimilarProducts.set_eligible is not SimilarProducts.set_eligible
