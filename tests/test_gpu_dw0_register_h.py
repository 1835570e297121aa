"""dW0's loader with H0 through registers (gemm_tn.hip, the ZPRO form of gemm_tn8_kernel with 32-row chunks) against the form
that stages H0 through LDS beside dZ1 (PC_OPT_DW0_STAGED_H = 1): the same expression on the same rows in the same order, so every
output keeps its bits; and dW0 / db0 against fp64 under the building blocks' fp32-grade bound.

Two entries reach the loader: ops.ffn_backward without a dx consumer (the BatchNorm backward of dZ1 is then applied inside the
dW0 kernel), and Product2Vec.train_step_indexed on the hand-built unique-layout batches of test_gpu_tn_riders.py.

Row counts (tn_plan(R, 256, 128), restated in building_block_cases.tn_plan and asserted below):
  8192     128 slices of 64 rows: two whole 32-row chunks each, the ring's steady state is one step long
  8193     129 slices, the last one owns ONE row: a single ragged chunk, prologue and epilogue with nothing in flight ahead
  8229     129 slices, the last one ends mid-chunk (37 rows: one whole chunk and five rows)
  19969    the non-monotone plan of gemm_tn_workspace_floats: 209 slices of 96 rows (three chunks), the last one of a single row
Segment boundaries are no multiples of 32, so chunks straddle segments and the loader reloads its coefficients inside a chunk.
The neighbour segment carries row multiplicities != 1 (pc_segments.row_weight over a sub-range), its last row is the weighted
pad row (pc_segments.weighted_row, weight 0 or 3, gather index -1), and every 10th gather index is -1: the A row is zero and Z
is still transformed.

The fp64 reference recomputes dZ1 from the inputs (the kernels' own dZ1 never leaves the workspace): autograd through
Linear0 -> BatchNorm with weighted statistics -> tanh -> Linear3 -> tanh -> Linear5 in fp64, and once more in fp32 for the error
a plain fp32 computation makes (the e32 term of building_block_cases.fp32_grade_tol).  Needs an MI355X."""
import ctypes

import pytest
import torch

import building_block_cases as bb
import test_gpu_tn_riders as riders
from test_gpu_building_blocks import bits_equal, within

pytestmark = pytest.mark.gpu

H = 256
TABLE_ROWS = 3000
FFN_KEYS = ("ffn.0.weight", "ffn.0.bias", "ffn.1.weight", "ffn.1.bias", "ffn.3.weight", "ffn.3.bias", "ffn.5.weight", "ffn.5.bias")


def set_staged(v):
    from p_companion_amd import _lib
    assert _lib.lib().pc_set_option(_lib.PC_OPT_DW0_STAGED_H, v) == 0


def test_option_default_and_refusals():
    from p_companion_amd import _lib
    L = _lib.lib()
    v = ctypes.c_int(-1)
    assert L.pc_get_option(_lib.PC_OPT_DW0_STAGED_H, ctypes.byref(v)) == 0 and v.value == 0
    assert L.pc_set_option(_lib.PC_OPT_DW0_STAGED_H, 2) == -1
    try:
        set_staged(1)
        assert L.pc_get_option(_lib.PC_OPT_DW0_STAGED_H, ctypes.byref(v)) == 0 and v.value == 1
    finally:
        set_staged(0)


# ------------------------------------------------------------------ the FFN backward without a dx consumer
def seg_starts(R, nseg):
    starts = [0, 1001, 1001 + (R // 2 | 1), R - 1203][:nseg]
    assert all(s % 32 for s in starts[1:]) and all(a < b for a, b in zip(starts, starts[1:] + [R]))
    return starts


def ffn_inputs(R, nseg, dim, wmult):
    """Everything a case feeds the kernels (on the device) and the per-row multiplicities the reference needs."""
    from p_companion_amd import ops
    g = torch.Generator().manual_seed(R * 10 + nseg + dim)
    rn = lambda *shape, scale=1.0: (torch.randn(*shape, generator=g) * scale).cuda()
    params = {k: rn(*shape, scale=0.1) for k, shape in zip(ops.P2V_KEYS, ops.p2v_shapes(dim))}
    params["ffn.1.weight"] = 1.0 + rn(H, scale=0.1)
    params["ffn.1.running_mean"] = torch.zeros(H, device="cuda")
    params["ffn.1.running_var"] = torch.ones(H, device="cuda")
    params["ffn.1.num_batches_tracked"] = torch.zeros((), dtype=torch.int64, device="cuda")
    starts = seg_starts(R, nseg)
    w0, wrow = starts[1], starts[2] - 1                      # multiplicities over [w0, wrow), the pad row behind them
    idx = torch.randint(0, TABLE_ROWS, (R,), generator=g, dtype=torch.int32)
    idx[::10] = -1
    idx[wrow] = -1
    roww = torch.tensor([1.0, 2.0, 3.0, 5.0])[torch.randint(0, 4, (wrow - w0,), generator=g)]
    assert float((roww != 1).float().mean()) > 0.5
    m = torch.ones(R)
    m[w0:wrow] = roww
    m[wrow] = wmult
    bounds = starts + [R]
    counts = [int(m[a:b].sum()) for a, b in zip(bounds, bounds[1:])]
    return dict(R=R, dim=dim, starts=starts, params=params, table=rn(TABLE_ROWS, dim), idx=idx.cuda(), dy=rn(R, dim, scale=0.1),
                roww=roww.cuda(), w0=w0, wrow=wrow, wmult=wmult, m=m.cuda(), counts=counts)


def patched_segments(ops, c):
    """ops.make_segments with the multiplicities of case c: row_weight over the sub-range [w0, wrow) and the weighted row."""
    orig = ops.make_segments

    def make(starts, rows, row_weight=None, counts=None):
        s = orig(starts, rows, None, c["counts"])
        s.row_weight, s.row_weight_start, s.row_weight_rows = c["roww"].data_ptr(), c["w0"], c["wrow"] - c["w0"]
        s.weighted_row, s.weight = c["wrow"], c["wmult"]
        return s
    return make


def ffn_reference(c, dtype):
    """(dW0, db0, dH0) by autograd in `dtype` on the device, BatchNorm statistics weighted by the row multiplicities."""
    p = {k: c["params"][k].to(dtype) for k in FFN_KEYS}
    w0, b0 = p["ffn.0.weight"].clone().requires_grad_(True), p["ffn.0.bias"].clone().requires_grad_(True)
    x = bb.gathered(c["table"], c["idx"]).to(dtype)
    h0 = x @ w0.T + b0
    h0.retain_grad()
    a1 = []
    bounds = c["starts"] + [c["R"]]
    for s, (a, b) in enumerate(zip(bounds, bounds[1:])):
        hs, ms, n = h0[a:b], c["m"][a:b, None].to(dtype), c["counts"][s]
        mean = (ms * hs).sum(0) / n
        var = (ms * (hs - mean) ** 2).sum(0) / n
        a1.append(torch.tanh(p["ffn.1.weight"] * (hs - mean) / torch.sqrt(var + 1e-5) + p["ffn.1.bias"]))
    a2 = torch.tanh(torch.cat(a1) @ p["ffn.3.weight"].T + p["ffn.3.bias"])
    y = a2 @ p["ffn.5.weight"].T + p["ffn.5.bias"]
    (y * c["dy"].to(dtype)).sum().backward()
    return w0.grad, b0.grad, h0.grad, x


# (R, segments, weight of the pad row, accumulate, PRODUCT_EMB_DIM); at 256 the loader keeps its staged form (128 accumulator
# registers: the register form spills), whatever the option says -- that case asserts it still runs and matches
FFN_CASES = [(8192, 4, 0.0, False, 128), (8193, 4, 3.0, False, 128), (8229, 4, 0.0, False, 128), (19969, 4, 3.0, False, 128),
             (8229, 3, 3.0, False, 128), (8193, 4, 0.0, True, 128), (8193, 4, 3.0, False, 256)]
PLANS = {8192: (128, 64), 8193: (129, 64), 8229: (129, 64), 19969: (209, 96)}


@pytest.mark.parametrize("R,nseg,wmult,accumulate,dim", FFN_CASES, ids=lambda v: str(v))
def test_ffn_backward_without_dx(monkeypatch, R, nseg, wmult, accumulate, dim):
    from p_companion_amd import ops
    assert bb.tn_full_tile(R, H, dim) and (dim == 256 or bb.tn_plan(R, H, dim) == PLANS[R])
    c = ffn_inputs(R, nseg, dim, wmult)
    monkeypatch.setattr(ops, "make_segments", patched_segments(ops, c))
    _, sv = ops.ffn_forward_train(c["params"], c["table"], c["idx"], R, c["starts"], update_running=False)
    init = {k: torch.randn(v.shape, generator=torch.Generator().manual_seed(7)).cuda() for k, v in c["params"].items() if k in ops.P2V_KEYS}
    got = {}
    try:
        for staged in (0, 1):
            set_staged(staged)
            grads = {k: v.clone() for k, v in init.items()} if accumulate else None
            got[staged], dx = ops.ffn_backward(c["params"], c["table"], c["idx"], c["dy"], sv, grads=grads, accumulate=accumulate)
            assert dx is None
        torch.cuda.synchronize()
    finally:
        set_staged(0)
    for k in FFN_KEYS:
        assert bits_equal(got[0][k], got[1][k]), k
    dw_ref, db_ref, dh0, x = ffn_reference(c, torch.float64)
    dw32, db32, _, _ = ffn_reference(c, torch.float32)
    mag_w, mag_b = dh0.abs().T @ x.abs(), dh0.abs().sum(0)
    e32_w, e32_b = (dw32.double() - dw_ref).abs().max(), (db32.double() - db_ref).abs().max()
    if accumulate:                                              # (one more addition: the start value enters the magnitude)
        iw, ib = init["ffn.0.weight"].double(), init["ffn.0.bias"].double()
        dw_ref, db_ref, mag_w, mag_b = dw_ref + iw, db_ref + ib, mag_w + iw.abs(), mag_b + ib.abs()
    what = f"R{R}-seg{nseg}-w{wmult}-acc{int(accumulate)}-D{dim}"
    within(got[0]["ffn.0.weight"], dw_ref, bb.fp32_grade_tol(e32_w, mag_w), "dw0_register_h", what)
    within(got[0]["ffn.0.bias"], db_ref, bb.fp32_grade_tol(e32_b, mag_b), "db0_register_h", what)


# ------------------------------------------------------------------ the fused step
def steps(batches, dim, staged, **kw):
    try:
        set_staged(staged)
        return riders.run_steps(batches, dim, 1, **kw)
    finally:
        set_staged(0)


@pytest.mark.parametrize("B,n_unique,R", [(1024, 1023, 8192), (1024, 1024, 8193), (1024, 1060, 8229), (2048, 5632, 19969)])
def test_steps_keep_their_bits(B, n_unique, R):
    """Two steps with the optimizer riding, and one without it (the gradients themselves): loss, parameters, BatchNorm buffers,
    both Adam moments and the step count, bit for bit between the two forms of the loader."""
    made = [riders.make_batch(B, 8, n_unique, seed=90 + i) for i in range(2)]
    assert all(r == R for _, r in made)
    batches = [b for b, _ in made]
    riders.assert_same_bits(steps(batches, 128, 0), steps(batches, 128, 1), "adam riding")
    g0, g1 = steps(batches, 128, 0, riding=False, steps=1), steps(batches, 128, 1, riding=False, steps=1)
    assert float(g0["grad0"].abs().max()) > 0
    riders.assert_same_bits(g0, g1, "gradients only")


def test_steps_dim_256_still_run_and_match():
    """PRODUCT_EMB_DIM = 256: the 256 x 256 loader stays staged under either setting."""
    b, R = riders.make_batch(1024, 4, 1300, seed=70)
    assert R == 8469
    riders.assert_same_bits(steps([b], 256, 0), steps([b], 256, 1), "dim 256")
