"""CPU checks behind tests/test_gpu_building_blocks.py: the case lists reach the kernel forms and switches they are
named after, and the bounds the GPU tests assert cannot reject a correct kernel -- the plainest correct evaluation
order (one sequential fp32 chain per output element) stays inside the 4e-7 |x| |w|^T term alone."""
import numpy as np
import pytest

import building_block_cases as bb


# ------------------------------------------------------------------ the lists cover what they claim
@pytest.mark.parametrize("form", bb.NT_FORMS)
def test_nt_case_list_covers_its_form(form):
    cases = bb.NT_CASES[form]
    assert 8 <= len(cases) <= 12
    for m, k, n, act, bias, gather in cases:
        assert k % 4 == 0 and bb.nt_form(m, k, n) == form, (form, m, k, n)
    ms, ks, ns = bb.NT_LISTED[form]
    assert set(ms) <= {c[0] for c in cases} and set(ks) <= {c[1] for c in cases} and set(ns) <= {c[2] for c in cases}
    assert {c[3] for c in cases} == {0, 1, 2}
    assert {c[4] for c in cases} == {True, False}
    gathers = [c for c in cases if c[5]]
    assert gathers and all(c[3] != 1 for c in gathers)      # -1 rows are compared bit for bit with act(b): none / ReLU
    for m, k, n, *_ in gathers:
        tile = bb.NT_TILE.get(form, 128)
        idx = bb.gather_idx(m, bb.GATHER_TABLE_ROWS, tile)
        assert m > tile and idx[tile - 1] == -1 and idx[m - 1] == -1            # last row of a full and of the ragged tile
        live = idx[idx >= 0]
        assert len(live) > len(set(live.tolist())) and int(live.max()) < bb.GATHER_TABLE_ROWS
    if form != "few_row":                                   # the K-pipelined kernels meet a zero-filled K tail
        bk = 16 if "four_wave" in form else 32
        assert any(k % bk for _, k, *_ in cases) and any(n % 4 for _, _, n, *_ in cases)


def test_nt_switches_are_straddled():
    f = bb.nt_form
    # 191 | 192 row tiles (M = 24448 | 24449), at a narrow, a ragged and a full width
    assert (f(24448, 36, 3), f(24449, 4, 6)) == ("few_row", "four_wave")
    assert (f(129, 36, 256), f(24449, 128, 256)) == ("eight_wave_1", "paired_four_wave")
    # K = 256 | 260
    assert (f(33, 256, 128), f(65, 260, 128)) == ("few_row", "two_wave")
    # N = 128 | 129, 256 | 257, 512 | 513
    assert (f(128, 260, 128), f(128, 260, 129)) == ("two_wave", "eight_wave_1")
    assert (f(129, 36, 256), f(129, 36, 257), f(129, 36, 512), f(130, 36, 513)) == \
        ("eight_wave_1", "eight_wave_2", "eight_wave_2", "eight_wave_3plus")
    # the paired numbering without and with padding tiles
    assert bb.nt_paired_tiles(24449) == (192, 384) and bb.nt_paired_tiles(24577) == (193, 400)
    every = {c[:3] for cases in bb.NT_CASES.values() for c in cases}
    for shape in ((24448, 36, 3), (24449, 4, 6), (129, 36, 256), (24449, 128, 256), (33, 256, 128), (65, 260, 128),
                  (129, 36, 512), (130, 36, 513), (24449, 36, 257)):
        assert shape in every, shape
    assert {n for _, _, n in every} >= {128, 129, 256, 257, 512, 513}
    for m, k, n, *_ in bb.NT_PADDED_K:
        assert k % 4 != 0


def test_dx_cases_reach_every_nt_form():
    forms = {bb.dx_form(*c) for c in bb.DX_CASES}
    assert forms >= {"few_row", "two_wave", "four_wave", "paired_four_wave", "eight_wave_3plus"}
    assert any(o % 4 for _, o, _ in bb.DX_CASES) and any(i % 4 for _, _, i in bb.DX_CASES)
    assert any(o % 32 and i % 32 and o > 32 and i > 32 for _, o, i in bb.DX_CASES)       # ragged multi-tile transpose
    assert (200, 256, 128) in bb.DX_CASES


def test_tn_cases_sit_on_their_side_of_the_switch():
    assert all(not bb.tn_full_tile(*c) for c in bb.DW_PLAIN_CASES + bb.DW_PADDED_CASES)
    assert all(bb.tn_full_tile(*c) for c in bb.DW_FULL_CASES)
    assert not bb.tn_full_tile(8191, 256, 256) and bb.tn_full_tile(8192, 256, 256)
    assert (8191, 256, 256) in bb.DW_PLAIN_CASES and (8192, 256, 256) in bb.DW_FULL_CASES
    assert (8191, 192, 64) in bb.DW_PLAIN_CASES and (8192, 192, 64) in bb.DW_FULL_CASES
    # the plan is not monotone in R: 19969 rows are cut into fewer slices than 16384
    assert bb.tn_plan(16384, 256, 256)[0] == 256 and bb.tn_plan(19969, 256, 256) == (209, 96)
    assert bb.tn_plan(8192, 256, 256) == (128, 64) and bb.tn_plan(8193, 256, 256) == (129, 64)
    assert {c[1:] for c in bb.DW_FULL_CASES} == set(bb.DW_FULL_SHAPES)
    assert {64, 192} <= {no for _, no, _ in bb.DW_FULL_CASES} & {ni for _, _, ni in bb.DW_FULL_CASES}
    kinds = [bb.tn_full_tile(*c) for c in bb.DW_GATHER_CASES]
    assert True in kinds and False in kinds
    assert all(no % 4 or ni % 4 for _, no, ni in bb.DW_PADDED_CASES)


# ------------------------------------------------------------------ the bounds cannot reject a correct kernel
def _sequential_fp32(a, b, bias=None):
    """C[i][j] = sum_k a[i][k] b[j][k], one fp32 product and one fp32 addition per k, in the order of k"""
    a, b = a.numpy().astype(np.float32), b.numpy().astype(np.float32)
    acc = np.zeros((a.shape[0], b.shape[0]), dtype=np.float32)
    for k in range(a.shape[1]):
        acc += a[:, k, None] * b[None, :, k]
    if bias is not None:
        acc += bias.numpy().astype(np.float32)[None, :]
    return acc


@pytest.mark.parametrize("family,shape", [("nt", (200, 1028, 128)), ("nt", (64, 36, 130)), ("tn", (19969, 64, 64))])
def test_plain_fp32_order_stays_inside_the_magnitude_term(family, shape):
    """The longest contraction of each family.  The GPU tests allow 1.25 x torch's fp32 error + 4e-7 mag; a plain
    sequential fp32 chain must fit into 4e-7 mag alone, so a correct kernel in any sensible order does too.
    (Measured: 1.96e-7, 1.65e-7 and 1.96e-7 mag for the three -- the bound leaves about 2x over the plainest order.)"""
    if family == "nt":
        m, k, n = shape
        x, w, b = bb.linear_inputs(m, k, n, bias=True)
        got = _sequential_fp32(x, w, b)
        ref = x.double() @ w.double().T + b.double()
        mag = x.double().abs() @ w.double().abs().T + b.double().abs()
    else:
        r, no, ni = shape
        dy, x = bb.dw_inputs(r, no, ni)
        got = _sequential_fp32(dy.T.contiguous(), x.T.contiguous())
        ref = dy.double().T @ x.double()
        mag = dy.double().abs().T @ x.double().abs()
    ratio = float((np.abs(got.astype(np.float64) - ref.numpy()) / mag.numpy()).max())
    print(f"sequential fp32 {family} {shape}: max err / mag = {ratio:.3e} (allowed {bb.MAG_COEF:.1e})")
    assert ratio <= bb.MAG_COEF


@pytest.mark.parametrize("case", bb.SCATTER_INT_CASES + bb.SCATTER_SMALL_CASES, ids=str)
def test_integer_scatter_sums_are_exact_in_fp32(case):
    table_rows, width, rows, mode = case
    table, idx, src = bb.scatter_int_inputs(*case)
    assert int(table.abs().max()) <= bb.INT_RANGE and int(src.abs().max()) <= bb.INT_RANGE
    assert bb.scatter_int_worst_partial(table_rows, idx) < 2 ** 24
    assert int(idx.max()) < table_rows


def test_scatter_case_lists_cover_the_issue():
    assert {c[1] for c in bb.SCATTER_INT_CASES} == {1, 3, 64, 130}
    assert {c[0] for c in bb.SCATTER_INT_CASES} == {1, 7, 100, 5000}
    assert {c[2] for c in bb.SCATTER_INT_CASES} == {1, 255, 257, 12288}
    assert {c[2] for c in bb.SCATTER_SMALL_CASES} == {1, 127, 128, 129, 32769}
    lds_bytes = {c[0] * c[1] * 4 for c in bb.SCATTER_SMALL_CASES}
    assert 65536 in lds_bytes and max(lds_bytes) > 65536 and 3 in {c[1] for c in bb.SCATTER_SMALL_CASES}
    assert 32769 > 256 * 128
