"""The exported building-block ops (pc_linear_*, pc_gather_rows, pc_scatter_*_rows, pc_act_backward, pc_hadamard_*_dim;
ops.py '# building blocks') against plain fp64 / exact references at every dispatch edge of the two shared GEMM
families: each kernel form of launch_gemm_nt with K tails and N % 4 != 0, the 191|192 row-tile, K 256|260 and
N 128|129, 256|257, 512|513 switches, the paired numbering with and without padding tiles; launch_gemm_tn's plain and
full-tile kernels at the 8191|8192 switch, the partly filled 64 / 192-wide images and the non-monotone plan; the row
and elementwise ops bit for bit.  The case lists and what each one targets: tests/building_block_cases.py (their
coverage and the bounds used here are checked on the CPU by test_building_block_bounds_host.py).  Needs an MI355X."""
import ctypes

import pytest
import torch

import building_block_cases as bb
from test_gpu_ops import close, dev, rnd

pytestmark = pytest.mark.gpu

U = 2.0 ** -24            # fp32 unit roundoff


@pytest.fixture(scope="module")
def ops():
    from p_companion_amd import ops as o
    assert torch.cuda.is_available()
    return o


@pytest.fixture(scope="module")
def lib():
    from p_companion_amd import _lib
    return _lib.lib()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def within(got, ref, tol, family, what):
    """|got - ref| <= tol per element (fp64 on the device); prints the worst err / bound for the record"""
    assert torch.isfinite(got).all(), f"{what}: not finite"
    err = (got.double() - ref).abs()
    tol = torch.as_tensor(tol, dtype=torch.float64, device=err.device).expand_as(err)
    worst = float((err / tol.clamp_min(1e-300)).max())          # (a zero bound: any error at all is far above 1)
    print(f"BB_RATIO {family} {what} {worst:.4f} max_err {float(err.max()):.3e}")
    assert worst <= 1.0, f"{what}: error / bound = {worst:.3f} (max err {float(err.max()):.3e})"


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _act64(t, act):
    return torch.tanh(t) if act == 1 else torch.relu(t) if act == 2 else t


def _nt_check(y, xr, w, b, act, family, what):
    """y against act(xr w^T + b) in fp64 under the fp32-grade bound (xr: the rows the product read, on the device)"""
    pre = xr.double() @ w.double().T
    mag = xr.double().abs() @ w.double().abs().T
    t32 = xr @ w.T
    if b is not None:
        pre, mag, t32 = pre + b.double(), mag + b.double().abs(), t32 + b
    e32 = (t32.double() - pre).abs().max()
    within(y, _act64(pre, act), bb.fp32_grade_tol(e32, mag, act), family, what)


# ------------------------------------------------------------------ linear_forward, one list per kernel form
ALL_NT = [c for form in bb.NT_FORMS for c in bb.NT_CASES[form]] + bb.NT_PADDED_K


@pytest.mark.parametrize("case", ALL_NT, ids=bb.nt_id)
def test_linear_forward_forms(ops, case):
    m, k, n, act, bias, gather = case
    x, w, b = bb.linear_inputs(bb.GATHER_TABLE_ROWS if gather else m, k, n, bias)
    x, w, b = dev(x), dev(w), (dev(b) if bias else None)
    if not gather:
        y = ops.linear_forward(x, w, b, act=act)
        assert y.shape == (m, n)
        _nt_check(y, x, w, b, act, "nt_forward", bb.nt_id(case))
        return
    form = bb.nt_form(m, k, n)
    idx = dev(bb.gather_idx(m, bb.GATHER_TABLE_ROWS, bb.NT_TILE.get(form, 128)))
    y = ops.linear_forward(x, w, b, idx=idx, act=act)
    assert y.shape == (m, n)
    _nt_check(y, bb.gathered(x, idx), w, b, act, "nt_forward", bb.nt_id(case))
    # a -1 row is a zero row: its output is act(b) exactly (exact zero without bias)
    want = torch.zeros(n, device="cuda") if b is None else (torch.relu(b) if act == 2 else b)
    dead = y[idx < 0]
    assert dead.shape[0] >= 2 and bits_equal(dead, want.expand_as(dead))


@pytest.mark.parametrize("xrows,rows,k,n", bb.NT_ROWS_ARG)
def test_linear_forward_rows_argument(ops, lib, xrows, rows, k, n):
    """rows= smaller than x: the result has `rows` rows; through the C entry with a larger sentinel-filled output, the
    rows past `rows` are never written (the last tile is ragged, N % 4 != 0: the scalar store path)."""
    x, w, b = (dev(t) for t in bb.linear_inputs(xrows, k, n))
    y = ops.linear_forward(x, w, b, rows=rows)
    assert y.shape == (rows, n)
    _nt_check(y, x[:rows], w, b, 0, "nt_forward", f"rows_arg-{rows}of{xrows}-K{k}-N{n}")
    big = torch.full((xrows, n), -7.25, device="cuda")
    assert lib.pc_linear_forward(_ptr(x), None, rows, k, _ptr(w), _ptr(b), n, 0, _ptr(big), _stream()) == 0
    assert bits_equal(big[:rows], y)
    assert bool((big[rows:] == -7.25).all())


# ------------------------------------------------------------------ linear_backward_input
@pytest.mark.parametrize("rows,out_dim,in_dim", bb.DX_CASES, ids=lambda v: str(v))
def test_linear_backward_input_forms(ops, rows, out_dim, in_dim):
    dy, w = (dev(t) for t in bb.dx_inputs(rows, out_dim, in_dim))
    dx = ops.linear_backward_input(dy, w)
    assert dx.shape == (rows, in_dim)
    _nt_check(dx, dy, w.T.contiguous(), None, 0, "dx", f"{bb.dx_form(rows, out_dim, in_dim)}-{rows}x{out_dim}x{in_dim}")


# ------------------------------------------------------------------ linear_backward_weight
def _tn_check(ops, rows, no, ni, kind, gather=False):
    dy, x = bb.dw_inputs(rows, no, ni, x_rows=bb.TN_TABLE_ROWS if gather else None)
    dy, x = dev(dy), dev(x)
    idx = dev(bb.sparse_idx(rows, bb.TN_TABLE_ROWS)) if gather else None
    dw, db = ops.linear_backward_weight(dy, x, no, ni, idx=idx)
    assert dw.shape == (no, ni) and db.shape == (no,)           # exactly [out_dim, in_dim] and [out_dim]
    xr = bb.gathered(x, idx) if gather else x
    ref = dy.double().T @ xr.double()
    mag = dy.double().abs().T @ xr.double().abs()
    e32 = ((dy.T @ xr).double() - ref).abs().max()
    what = f"R{rows}-{no}x{ni}" + ("-gather" if gather else "")
    within(dw, ref, bb.fp32_grade_tol(e32, mag), f"dw_{kind}", what)
    refb = dy.double().sum(0)
    e32b = (dy.sum(0).double() - refb).abs().max()
    within(db, refb, bb.fp32_grade_tol(e32b, dy.double().abs().sum(0)), f"db_{kind}", what)
    dw2, db2 = ops.linear_backward_weight(dy, x, no, ni, idx=idx)
    assert bits_equal(dw, dw2) and bits_equal(db, db2)          # fixed-order split-K: bitwise reproducible


@pytest.mark.parametrize("rows,no,ni", bb.DW_PLAIN_CASES + bb.DW_PADDED_CASES, ids=lambda v: str(v))
def test_linear_backward_weight_plain_tiles(ops, rows, no, ni):
    assert not bb.tn_full_tile(rows, no, ni)
    _tn_check(ops, rows, no, ni, "plain")


@pytest.mark.parametrize("rows,no,ni", bb.DW_FULL_CASES, ids=lambda v: str(v))
def test_linear_backward_weight_full_tile(ops, rows, no, ni):
    assert bb.tn_full_tile(rows, no, ni)
    _tn_check(ops, rows, no, ni, "full_tile")


@pytest.mark.parametrize("rows,no,ni", bb.DW_GATHER_CASES, ids=lambda v: str(v))
def test_linear_backward_weight_gather(ops, rows, no, ni):
    _tn_check(ops, rows, no, ni, "full_tile" if bb.tn_full_tile(rows, no, ni) else "plain", gather=True)


@pytest.mark.parametrize("rows,no,ni", bb.DW_NO_BIAS_CASES, ids=lambda v: str(v))
def test_linear_backward_weight_without_bias(ops, rows, no, ni):
    dy, x = (dev(t) for t in bb.dw_inputs(rows, no, ni))
    dw, db = ops.linear_backward_weight(dy, x, no, ni)
    dw0, db0 = ops.linear_backward_weight(dy, x, no, ni, want_bias=False)
    assert db0 is None and db is not None
    assert bits_equal(dw, dw0)


# ------------------------------------------------------------------ row ops: exact
@pytest.mark.parametrize("rows", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("width", [4, 64, 128, 260])
def test_gather_rows(ops, rows, width):
    table = dev(rnd(77, width, seed=11))
    idx = bb.sparse_idx(rows, 77, seed=rows)
    if rows > 1:
        idx[rows - 1] = -1
        idx[0] = 76
    out = ops.gather_rows(table, dev(idx))
    assert bits_equal(out, bb.gathered(table, dev(idx)))
    if rows > 1:
        assert bits_equal(out[rows - 1], torch.zeros(width, device="cuda"))       # -1: an exact (+0) zero row


@pytest.mark.parametrize("rows", [1, 63, 64, 65, 1000])
@pytest.mark.parametrize("width", [4, 64, 128, 260])
def test_scatter_rows(ops, rows, width):
    out_rows = rows + 37
    g = torch.Generator().manual_seed(rows * 1000 + width)
    idx = torch.randperm(out_rows, generator=g)[:rows].to(torch.int32)           # distinct targets
    skip = torch.rand(rows, generator=g) < 0.1
    idx[skip] = -1
    src = rnd(rows, width, seed=12)
    out = torch.full((out_rows, width), -7.25)
    ref = out.clone()
    ref[idx[~skip].long()] = src[~skip]
    got = ops.scatter_rows(dev(out), dev(idx), dev(src))
    assert bits_equal(got.cpu(), ref)                                             # untouched rows keep the sentinel


def _scatter_int_check(case, run):
    table_rows, width, rows, mode = case
    table, idx, src = bb.scatter_int_inputs(*case)
    assert bb.scatter_int_worst_partial(table_rows, idx) < 2 ** 24
    ref = table.clone()
    live = idx >= 0
    ref.index_add_(0, idx[live].long(), src[live])                               # int64: exact
    t = dev(table, torch.float32)
    run(t, dev(idx), dev(src, torch.float32))
    close(t, ref.float(), 0.0, what=f"scatter_add {case}")                         # (|ref| < 2^24: exact in fp32)
    assert torch.equal(t.cpu().long(), ref)


@pytest.mark.parametrize("case", bb.SCATTER_INT_CASES, ids=str)
def test_scatter_add_rows_integer_data(ops, case):
    _scatter_int_check(case, lambda t, idx, src: ops.scatter_add_rows(t, idx, src))


@pytest.mark.parametrize("case", bb.SCATTER_SMALL_CASES, ids=str)
def test_scatter_add_rows_small_integer_data(lib, case):
    """pc_scatter_add_rows_small: the LDS-table form (table <= 64 KB) and its fall-back for larger tables"""
    def run(t, idx, src):
        rc = lib.pc_scatter_add_rows_small(_ptr(t), t.shape[0], _ptr(idx), idx.numel(), t.shape[1], _ptr(src), _stream())
        assert rc == 0
    _scatter_int_check(case, run)


def test_scatter_add_rows_normal_data(ops):
    """Standard-normal sources onto a non-zero table (+=, not =) against an fp64 index_add.  Per element the textbook
    bound of a c-term fp32 sum in any order, (c - 1) 2^-24 sum|src|, c the number of sources on the row."""
    table_rows, width, rows = 100, 64, 12288
    table, src = rnd(table_rows, width, seed=13), rnd(rows, width, seed=14)
    idx = bb.sparse_idx(rows, table_rows, seed=5)
    live = idx >= 0
    ref = table.double().index_add_(0, idx[live].long(), src[live].double())
    mag = torch.zeros(table_rows, width, dtype=torch.float64).index_add_(0, idx[live].long(), src[live].double().abs())
    c = torch.bincount(idx[live].long(), minlength=table_rows).double()
    assert int(c.min()) >= 2
    got = ops.scatter_add_rows(dev(table), dev(idx), dev(src))
    # (a plain assignment instead of += would miss by |table| ~ 1, a thousand bounds)
    within(got.cpu(), ref, (c[:, None] - 1) * U * mag, "scatter_add", "normal-100x64-12288")


# ------------------------------------------------------------------ act_backward, Hadamard
@pytest.mark.parametrize("n", [1, 255, 256, 257, 100003])
def test_act_backward(ops, n):
    dy = rnd(n, seed=15)
    y = torch.tanh(rnd(n, seed=16, scale=2.0))                  # |y| <= 1
    if n >= 255:
        y[3], y[4], y[5], y[6], y[n - 1] = 0.0, -0.0, 1.0, -1.0, 0.0
    else:
        y[0] = -0.0
    dyd, yd = dev(dy), dev(y)
    relu = ops.act_backward(dyd, yd, 2)
    assert bits_equal(relu, torch.where(yd > 0, dyd, torch.zeros_like(dyd)))     # y = 0 and y = -0.0 give (+)0
    tanh = ops.act_backward(dyd, yd, 1)
    ref = dyd.double() * (1.0 - yd.double() ** 2)
    # two roundings in 1 - y^2, one in the product (fewer with fma contraction)
    within(tanh, ref, 3 * U * dyd.double().abs(), "act_backward", f"tanh-n{n}")


@pytest.mark.parametrize("B,K", [(1, 1), (3, 3), (4, 3), (5, 8), (257, 3)])
@pytest.mark.parametrize("D", [128, 256])
def test_hadamard(ops, D, B, K):
    pi, tp, dproj = dev(rnd(B, D, seed=17)), dev(rnd(B * K, D, seed=18)), dev(rnd(B, K, D, seed=19))
    proj = ops.hadamard_forward(pi, tp, K)
    assert bits_equal(proj, pi[:, None, :] * tp.view(B, K, D))                   # single fp32 products
    dpi, dtp = ops.hadamard_backward(dproj, pi, tp)
    assert bits_equal(dtp, (dproj * pi[:, None, :]).view(B * K, D))
    terms = dproj.double() * tp.view(B, K, D).double()
    within(dpi, terms.sum(1), (K + 1) * U * terms.abs().sum(1), "hadamard", f"dpi-D{D}-B{B}-K{K}")


def test_hadamard_refuses_other_widths(ops, lib):
    pi, tp, dproj = dev(rnd(4, 64, seed=20)), dev(rnd(12, 64, seed=21)), dev(rnd(4, 3, 64, seed=22))
    with pytest.raises(ValueError):
        ops.hadamard_forward(pi, tp, 3)
    with pytest.raises(ValueError):
        ops.hadamard_backward(dproj, pi, tp)
    out = torch.full((4, 3, 64), -7.25, device="cuda")
    dpi, dtp = torch.full((4, 64), -7.25, device="cuda"), torch.full((12, 64), -7.25, device="cuda")
    PC_ESHAPE = -2
    assert lib.pc_hadamard_forward_dim(_ptr(pi), _ptr(tp), 4, 3, 64, _ptr(out), _stream()) == PC_ESHAPE
    assert lib.pc_hadamard_backward_dim(_ptr(dproj), _ptr(pi), _ptr(tp), 4, 3, 64, _ptr(dpi), _ptr(dtp), _stream()) == PC_ESHAPE
    torch.cuda.synchronize()
    assert bool((out == -7.25).all()) and bool((dpi == -7.25).all()) and bool((dtp == -7.25).all())   # nothing launched
