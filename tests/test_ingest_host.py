"""Ingestion of behaviour edge lists, the host side (no GPU): IntBPG.from_edges -- the numpy twin of ops.build_catalogue /
csrc/ingest.hip -- against the reference's own graph and a hand-made one whose expected arrays are written out, the header
and the bindings, the C entries' refusals before anything is launched and build_catalogue's own argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT

PC_EINVAL, PC_ESHAPE, PC_EWORKSPACE = -1, -2, -3


def _keys(pairs, P):
    pairs = np.asarray(pairs).reshape(-1, 2).astype(np.int64)
    return set((pairs[:, 0] * P + pairs[:, 1]).tolist())


# ---- a hand-made graph of 12 products, degree_cap = 3 ----------------------------------------------------------------------
# co_view row 0: weights 5:3, 2:2, 4:2, 7:2, 9:1, 1:1 and a self-loop -> keeps 5, then two of the three ids of weight 2: the
#   lower ones, 2 and 4 (7 loses the tie by id)
# co_view row 4: four targets of weight 1 -> the three lowest ids (10 is dropped); row 10: one edge given twice
# product 11 has no edge at all; every list holds a self-loop
HAND_P, HAND_CAP = 12, 3
HAND_TYPES = np.array([0, 1, 2] * 4, np.int32)
HAND_CV = np.array([(0, 5), (0, 2), (0, 7), (4, 0), (0, 4), (0, 9), (0, 5), (3, 8), (0, 0), (0, 7), (4, 9), (10, 4), (0, 2),
                    (6, 3), (0, 1), (0, 5), (4, 10), (3, 6), (0, 4), (10, 4), (4, 3)], np.int32)
# (0, 7) and (4, 10): co-viewed but dropped by the cap -> no similarity pair; (1, 2): not co-viewed; (6, 6): self-loop
HAND_PV = np.array([(0, 2), (0, 5), (0, 7), (0, 5), (3, 8), (4, 10), (4, 3), (6, 6), (6, 3), (1, 2), (10, 4)], np.int32)
# (0, 5) and (6, 3) take their similarity pairs away; (0, 9): its co-view twin was dropped by the cap, still no complement;
# (1, 2) and (4, 10): purchased after view; (1, 7) twice; (5, 5): self-loop
HAND_CP = np.array([(0, 5), (0, 9), (0, 3), (1, 2), (1, 7), (1, 7), (5, 5), (8, 0), (4, 10), (6, 3), (2, 1)], np.int32)
HAND_EXPECT = dict(
    cv_rowptr=[0, 3, 3, 3, 5, 8, 8, 9, 9, 9, 9, 10, 10], cv_col=[2, 4, 5, 6, 8, 0, 3, 9, 3, 4], max_degree=3,
    sim_pairs=[[0, 2], [3, 8], [4, 3], [10, 4]], sim_rowptr=[0, 1, 1, 1, 2, 3, 3, 3, 3, 3, 3, 4, 4], sim_col=[2, 8, 3, 4],
    pair_deg=[3, 2, 3, 1], complementary_pairs=[[0, 3], [1, 7], [2, 1], [8, 0]])
# the same with an EMPTY purchase_after_view: no similarity pair, and (1, 2) becomes a complement
HAND_EXPECT_NO_PV = dict(
    cv_rowptr=HAND_EXPECT["cv_rowptr"], cv_col=HAND_EXPECT["cv_col"], max_degree=3, sim_pairs=np.zeros((0, 2), np.int32),
    sim_rowptr=[0] * 13, sim_col=[], pair_deg=[], complementary_pairs=[[0, 3], [1, 2], [1, 7], [2, 1], [8, 0]])


def check_against(expect, bpg, pair_deg=None):
    """bpg: an IntBPG (built on the host, or DeviceBPG.to_host()); pair_deg: the device's array, where there is one."""
    for k in ("cv_rowptr", "cv_col", "sim_rowptr", "sim_col", "complementary_pairs"):
        got = getattr(bpg, k)
        assert got.dtype == np.int32 and np.array_equal(got, np.asarray(expect[k], np.int32).reshape(got.shape)), k
    assert np.array_equal(bpg.similarity_pairs, np.asarray(expect["sim_pairs"], np.int32).reshape(-1, 2))
    assert bpg.max_degree == expect["max_degree"]
    deg = bpg.degree(bpg.similarity_pairs[:, 0]) if pair_deg is None else pair_deg
    assert np.array_equal(deg, np.asarray(expect["pair_deg"], np.int32))


def test_golden_graph_gives_the_references_pairs_and_rows(golden):
    """The reference's own three edge lists -> its own derived pairs and neighbour rows (no duplicates, no self-loops, maximum
    degree 48, 32 empty rows: without a cap nothing is dropped)."""
    from p_companion_amd.data import IntBPG
    z = golden("g2_bpg1000.npz")
    P = 1000
    b = IntBPG.from_edges(z["features"], z["type_idx"], z["co_view"], z["purchase_after_view"], z["co_purchase"],
                          category=z["category"])
    assert len(z["similarity_pairs"]) == 2949 and len(z["complementary_pairs"]) == 4523
    assert len(b.similarity_pairs) == 2949 and _keys(b.similarity_pairs, P) == _keys(z["similarity_pairs"], P)
    assert len(b.complementary_pairs) == 4523 and _keys(b.complementary_pairs, P) == _keys(z["complementary_pairs"], P)
    deg = np.diff(b.cv_rowptr)
    assert np.array_equal(deg, np.diff(z["cv_rowptr"])) and deg.max() == 48 == b.max_degree and int((deg == 0).sum()) == 32
    for i in range(P):
        row = b.get_neighbors(i)
        assert np.all(np.diff(row) > 0)                                    # strictly ascending
        assert set(row.tolist()) == set(z["cv_col"][z["cv_rowptr"][i]:z["cv_rowptr"][i + 1]].tolist()), i
    # both pair arrays sorted by (s, t); the positives' CSR is the similarity pairs in that order
    for p in (b.similarity_pairs, b.complementary_pairs):
        k = p[:, 0].astype(np.int64) * P + p[:, 1]
        assert np.all(np.diff(k) > 0)
    assert np.array_equal(b.sim_col, b.similarity_pairs[:, 1])
    assert np.array_equal(np.repeat(np.arange(P), np.diff(b.sim_rowptr)), b.similarity_pairs[:, 0])
    assert np.array_equal(b.category, z["category"]) and b.n_types == int(z["type_idx"].max()) + 1
    # a cap of 64 is above the maximum degree: the same graph
    c = IntBPG.from_edges(z["features"], z["type_idx"], z["co_view"], z["purchase_after_view"], z["co_purchase"], degree_cap=64)
    for k in ("cv_rowptr", "cv_col", "similarity_pairs", "complementary_pairs"):
        assert np.array_equal(getattr(b, k), getattr(c, k)), k
    assert not c.category.any()                                            # category defaults to zeros


def test_hand_made_graph():
    from p_companion_amd.data import IntBPG
    b = IntBPG.from_edges(None, HAND_TYPES, HAND_CV, HAND_PV, HAND_CP, degree_cap=HAND_CAP)
    check_against(HAND_EXPECT, b)
    assert b.features.shape == (12, 0) and b.num_products == 12 and b.n_types == 3
    check_against(HAND_EXPECT_NO_PV, IntBPG.from_edges(None, HAND_TYPES, HAND_CV, np.zeros((0, 2), np.int32), HAND_CP,
                                                       degree_cap=HAND_CAP))
    # the result is a function of the lists as (multi)sets: any order of the edges gives the same arrays
    rng = np.random.default_rng(0)
    s = IntBPG.from_edges(None, HAND_TYPES, HAND_CV[rng.permutation(len(HAND_CV))], HAND_PV[rng.permutation(len(HAND_PV))],
                          HAND_CP[rng.permutation(len(HAND_CP))], degree_cap=HAND_CAP)
    check_against(HAND_EXPECT, s)
    # without a cap the dropped edges are neighbours again, and (0, 7), (4, 10) similarity pairs
    u = IntBPG.from_edges(None, HAND_TYPES, HAND_CV, HAND_PV, HAND_CP)
    assert u.get_neighbors(0).tolist() == [1, 2, 4, 5, 7, 9] and u.get_neighbors(4).tolist() == [0, 3, 9, 10]
    assert u.similarity_pairs.tolist() == [[0, 2], [0, 7], [3, 8], [4, 3], [10, 4]]
    assert u.complementary_pairs.tolist() == HAND_EXPECT["complementary_pairs"]


def test_host_builder_names_the_list_of_a_bad_id():
    from p_companion_amd.data import IntBPG
    lists = dict(co_view=HAND_CV, purchase_after_view=HAND_PV, co_purchase=HAND_CP)
    for name in lists:
        for bad in ((3, 12), (-1, 3)):
            kw = dict(lists)
            kw[name] = np.concatenate([lists[name], np.array([bad], np.int32)])
            with pytest.raises(ValueError, match=name):
                IntBPG.from_edges(None, HAND_TYPES, degree_cap=3, **kw)


def test_header_bindings_and_limits():
    txt = open(os.path.join(ROOT, "include", "pcompanion_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    from p_companion_amd import _lib, ops
    names = ("pc_ingest_count", "pc_ingest_scatter", "pc_ingest_row_limits", "pc_ingest_rows_workspace_bytes", "pc_ingest_rows",
             "pc_ingest_flag", "pc_ingest_emit")
    for name in names:
        assert re.search(r"\b" + name + r"\s*\(", txt), name
        assert name in _lib.SIGNATURES, name
    assert re.search(r"#define PC_ABI_VERSION 8\b", txt)
    L = _lib.lib()
    w, l = ctypes.c_int(), ctypes.c_int()
    assert L.pc_ingest_row_limits(ctypes.byref(w), ctypes.byref(l)) == 0
    assert (w.value, l.value) == (ops.INGEST_WAVE_ROW_MAX, ops.INGEST_LDS_ROW_MAX) == (128, 4096)
    assert L.pc_ingest_row_limits(None, ctypes.byref(l)) == PC_EINVAL
    ws = L.pc_ingest_rows_workspace_bytes
    assert ws(0) == 0 and ws(-1) == 0 and ws(2 ** 31) == 0
    assert 4 * 1000 <= ws(1000) <= 4 * 1000 + 1024 and ws(10_000_000) < 41_000_000


def test_entries_refuse_before_anything_is_launched():
    """The pointers are host buffers, which no check dereferences: every call below returns from its argument checks."""
    from p_companion_amd import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.pc_ingest_count(p, 0, 10, 1, p, p, None) == 0                  # an empty list: nothing to launch
    assert L.pc_ingest_scatter(p, 0, 10, p, p, p, None) == 0
    for args in ((None, 5, 10, 1, p, p), (p, -1, 10, 1, p, p), (p, 2 ** 31, 10, 1, p, p), (p, 5, 0, 1, p, p),
                 (p, 5, 2 ** 31, 1, p, p), (p, 5, 10, 0, p, p), (p, 5, 10, 1, None, p), (p, 5, 10, 1, p, None)):
        assert L.pc_ingest_count(*args, None) == PC_EINVAL, args
    for args in ((None, 5, 10, p, p, p), (p, 5, 10, None, p, p), (p, 5, 10, p, None, p), (p, 5, 10, p, p, None),
                 (p, 2 ** 31, 10, p, p, p), (p, 5, 0, p, p, p)):
        assert L.pc_ingest_scatter(*args, None) == PC_EINVAL, args
    rows = dict(n=10, rowptr=p, bucket=p, scratch=p, cap=3, full=p, kept=p, mx=p, ws=p, ws_bytes=1 << 20)
    call = lambda **kw: L.pc_ingest_rows(*{**rows, **kw}.values(), None)
    for name in ("rowptr", "bucket", "scratch", "full", "kept", "mx", "ws"):
        assert call(**{name: None}) == PC_EINVAL, name
    assert call(n=0) == PC_EINVAL and call(n=2 ** 31) == PC_EINVAL
    assert call(cap=-1) == PC_ESHAPE and call(cap=65) == PC_ESHAPE
    assert call(ws_bytes=0) == PC_EWORKSPACE and call(cap=0, kept=None, mx=None, ws_bytes=0) == PC_EWORKSPACE
    flag = [10, p, p, None, p, p, None, None, None, None, None, None, None, p]
    for i, v in ((0, 0), (1, None), (2, None), (13, None), (5, None)):       # (5: a set's buffer without its offsets)
        a = list(flag)
        a[i] = v
        assert L.pc_ingest_flag(*a, None) == PC_EINVAL, i
    emit = [10, p, p, None, p, p, None, None, None, 0]
    for i, v in ((0, 0), (1, None), (2, None), (4, None), (5, None)):       # (5: no output at all)
        a = list(emit)
        a[i] = v
        assert L.pc_ingest_emit(*a, None) == PC_EINVAL, i
    assert L.pc_ingest_emit(10, p, p, None, p, None, None, p, None, 0, None) == PC_EINVAL      # pair degrees without their offsets


def test_build_catalogue_refuses_on_the_host():
    """dtype, shape, degree_cap and the list length are checked in Python; well-formed HOST tensors then meet the device check
    (no CPU fallback) -- all of it before the library is asked for anything."""
    from p_companion_amd import ops
    t = torch.from_numpy(HAND_TYPES)
    cv, pv, cp = (torch.from_numpy(a) for a in (HAND_CV, HAND_PV, HAND_CP))
    for cap in (0, 65, -1, 2.5, None, True):
        with pytest.raises(ValueError, match="degree_cap"):
            ops.build_catalogue(t, cv, pv, cp, degree_cap=cap)
    with pytest.raises(ValueError, match="type_idx"):
        ops.build_catalogue(t.long(), cv, pv, cp)
    with pytest.raises(ValueError, match="type_idx"):
        ops.build_catalogue(t.reshape(3, 4), cv, pv, cp)
    with pytest.raises(ValueError, match="type_idx"):
        ops.build_catalogue(t[:0], cv, pv, cp)
    with pytest.raises(ValueError, match="n_types"):
        ops.build_catalogue(t, cv, pv, cp, n_types=0)
    for k, name in enumerate(ops.INGEST_LISTS):
        for bad in (cv.long(), cv.reshape(-1), cv.reshape(-1, 3), cv.numpy(), None,
                    torch.empty((2 ** 31, 2), dtype=torch.int32, device="meta")):
            lists = [cv, pv, cp]
            lists[k] = bad
            with pytest.raises(ValueError, match=name):
                ops.build_catalogue(t, *lists)
    for bad in (torch.zeros(12, 8, dtype=torch.float64), torch.zeros(11, 8), torch.zeros(12)):
        with pytest.raises(ValueError, match="features"):
            ops.build_catalogue(t, cv, pv, cp, features=bad)
    with pytest.raises(TypeError, match="CUDA/ROCm"):
        ops.build_catalogue(t, cv, pv, cp, degree_cap=3)
    with pytest.raises(TypeError, match="CUDA/ROCm"):
        ops.build_catalogue(t, cv, torch.zeros(0, 2, dtype=torch.int32), cp, degree_cap=64, features=torch.zeros(12, 8))
