"""accumulate = 1 through the stand-alone FFN and attention backward entries: the gradients are ADDED to what the gradient
tensors hold.  The flag travels through the launchers' call blocks into every weight-gradient product, the column-sum rider's
value-bias output and the BatchNorm-backward finalize.  Reference: G0 + the gradient of the oracle evaluated in fp64.
Needs an MI355X."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import p2v_oracle, philox_oracle

ULP = 2.0 ** -23


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _state(d, seed=11):
    st = p2v_oracle.init_state(seed, d=d)
    st["ffn.1.weight"] = 1.0 + 0.1 * rnd(256, seed=seed + 1)
    st["ffn.1.bias"] = 0.1 * rnd(256, seed=seed + 2)
    st["attention.in_proj_bias"] = 0.05 * rnd(3 * d, seed=seed + 3)
    st["attention.out_proj.bias"] = 0.05 * rnd(d, seed=seed + 4)
    return st


def _f64(st):
    return {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in st.items()}


def _g0(st, seed):
    """What the gradient tensors hold before the call: multiples of 2^-6 in [-1, 1], so that G0 + g costs one rounding."""
    g = torch.Generator().manual_seed(seed)
    return {k: torch.randint(-64, 65, tuple(st[k].shape), generator=g).float() / 64 for k in p2v_oracle.TRAINABLE}


def _check(got, g0, g, sibling_tol, what):
    # the kernels form g~ with |g~ - g| <= sibling_tol (the bound of the non-accumulating test of the same quantity in
    # test_gpu_ops.py) and store fl(G0 + g~): one more rounding, at most half an ulp of the sum, and
    # |G0 + g~| <= |G0| + |g| + sibling_tol -- one whole fp32 ulp (2^-23) of |G0| + |g| covers it
    ref = g0.double() + g
    tol = sibling_tol + ULP * (g0.double().abs() + g.abs())
    err = (got.detach().cpu().double() - ref).abs()
    worst = float((err - tol).max())
    print(f"{what}: max err {float(err.max()):.3e}, smallest tolerance {float(tol.min()):.3e}")
    assert worst <= 0.0, f"{what}: error passes the bound by {worst:.3e} (max err {float(err.max()):.3e})"


# B = 5: the core kernels' grid is (B + 3) / 4, so the second workgroup has one live wave; N = 3 / 65: either side of the 64-slot
# register map; p > 0: the value-bias gradient comes from the column-sum rider (acc1), not from the weight-gradient product
@pytest.mark.parametrize("N,D,p", [(3, 128, 0.0), (65, 128, 0.0), (3, 256, 0.0), (65, 256, 0.0), (65, 128, 0.5)])
def test_attention_backward_accumulates(N, D, p):
    from p_companion_amd import ops
    B = 5
    st = _state(D)
    q, kv, dout = rnd(B, D, seed=50), rnd(B, N, D, seed=51), rnd(B, D, seed=52)
    names = [k for k in p2v_oracle.TRAINABLE if k.startswith("attention")]
    seed, offset = 2 ** 40 + 99, 3
    mask = None
    if p:
        mask = torch.from_numpy(philox_oracle.dropout_mask(seed, offset, philox_oracle.STREAM_ATTENTION, B * 4 * N, p)).view(B, 4, N).double()
    work = _f64(st)
    leaves = {k: work[k].clone().requires_grad_(True) for k in names}
    work.update(leaves)
    qi, ki = q.double().requires_grad_(True), kv.double().requires_grad_(True)
    (p2v_oracle.attention(qi, ki, work, mask=mask) * dout.double()).sum().backward()

    dst = {k: v.clone().cuda() for k, v in st.items()}
    if p:
        dst[ops.DROPOUT_KEY] = (p, seed, offset)
    g0 = _g0(st, 70)
    grads = {k: v.clone().cuda() for k, v in g0.items()}
    _, sv = ops.attention_forward(dst, q.cuda(), kv.cuda())
    out, dq, dk = ops.attention_backward(dst, q.cuda(), kv.cuda(), dout.cuda(), sv, grads=grads, accumulate=True)
    assert out is grads
    for k in names:
        g = leaves[k].grad
        _check(grads[k], g0[k], g, 3e-5 * max(1.0, float(g.abs().max())), k)
    # the key bias shifts every score of a head alike: its gradient is exactly 0, and under accumulate nothing clears or touches
    # the block
    assert torch.equal(grads["attention.in_proj_bias"][D:2 * D].cpu(), g0["attention.in_proj_bias"][D:2 * D])
    for k in p2v_oracle.TRAINABLE:
        if k not in names:
            assert torch.equal(grads[k].cpu(), g0[k]), k                 # the FFN's gradients are not the attention's to write
    zero = torch.zeros(())
    _check(dq, zero, qi.grad, 1e-5, "dquery")                            # (outputs, never accumulated)
    _check(dk, zero, ki.grad, 1e-5, "dkeys")


@pytest.mark.parametrize("need_dx", [False, True])
def test_ffn_backward_accumulates(need_dx):
    from p_companion_amd import ops
    rows, starts = 200, [0, 90]                     # two BatchNorm call groups, two row tiles, neither group a multiple of anything
    st = _state(128)
    x, dy = rnd(rows, 128, seed=40), rnd(rows, 128, seed=41, scale=0.1)
    names = [k for k in p2v_oracle.TRAINABLE if k.startswith("ffn")]
    work = _f64(st)
    leaves = {k: work[k].clone().requires_grad_(True) for k in names}
    work.update(leaves)
    xin = x.double().requires_grad_(True)
    bounds = starts + [rows]
    y = torch.cat([p2v_oracle.ffn(xin[bounds[i]:bounds[i + 1]], work, True, update_running=False) for i in range(len(starts))])
    (y * dy.double()).sum().backward()

    dst = {k: v.clone().cuda() for k, v in st.items()}
    g0 = _g0(st, 71)
    grads = {k: v.clone().cuda() for k, v in g0.items()}
    _, sv = ops.ffn_forward_train(dst, x.cuda(), None, rows, starts, update_running=False)
    out, dx = ops.ffn_backward(dst, x.cuda(), None, dy.cuda(), sv, need_dx=need_dx, grads=grads, accumulate=True)
    assert out is grads and (dx is not None) == need_dx
    for k in names:
        g = leaves[k].grad
        _check(grads[k], g0[k], g, 2e-5 * max(1.0, float(g.abs().max())) * max(1.0, (rows / 1000) ** 0.5), k)
    for k in p2v_oracle.TRAINABLE:
        if k not in names:
            assert torch.equal(grads[k].cpu(), g0[k]), k
    if need_dx:
        _check(dx, torch.zeros(()), xin.grad, 2e-5, "dx")
