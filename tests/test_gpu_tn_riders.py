"""Rider workgroups of the full-tile weight-gradient launches (gemm_tn.hip): with many rows (rows >= 8192) the fused Product2Vec
step's BatchNorm-backward finalize has no launch of its own -- eight workgroups of the dW3 launch run it
(PC_OPT_BN_FINALIZE_RIDES).  The riders run the finalize kernel's own function on the same inputs, so every output of the step
must keep its bits whatever the option says: in the places of slices that own no rows, appended to the grid when every slice
owns rows, with and without the optimizer riding, at PRODUCT_EMB_DIM = 256, and below the threshold where nothing rides.
Hand-built index batches: R = B (2 + K) + n_unique + 1 FFN rows exactly.  Needs an MI355X."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

P = 20_000          # products in the catalogue
K = 5


def cfg(**over):
    c = SimpleNamespace(PRODUCT_EMB_DIM=128, TYPE_EMB_DIM=64, HIDDEN_SIZE=256, NUM_ATTENTION_HEADS=4, DROPOUT=0.0,
                        MARGIN=1.0, ALPHA=0.8, NUM_COMP_TYPES=3, NUM_TYPES=40, DEVICE=torch.device("cuda"),
                        LEARNING_RATE=1e-3, BATCH_SIZE=64, PRODUCT2VEC_EPOCHS=1, NUM_EPOCHS=1)
    c.__dict__.update(over)
    return c


_tables = {}


def table(dim):
    if dim not in _tables:
        _tables[dim] = torch.randn(P, dim, generator=torch.Generator().manual_seed(11)).cuda()
    return _tables[dim]


def make_batch(B, N, n_unique, seed):
    """A batch in the unique-neighbour layout whose [B, N] neighbour matrix holds exactly n_unique distinct products (column 0
    always a real one, a fifth of the other repeated slots padding).  Returns (batch, R)."""
    from p_companion_amd import ops
    assert B - 1 <= n_unique <= B * N
    g = torch.Generator().manual_seed(seed)
    uniq = torch.randperm(P, generator=g)[:n_unique].to(torch.int32)
    rest = B * N - n_unique
    extra = uniq[torch.randint(n_unique, (rest,), generator=g)]
    col = (torch.arange(n_unique, B * N) // B)                       # slots are filled column by column
    extra[(torch.rand(rest, generator=g) < 0.2) & (col >= 1)] = -1
    nb = torch.cat([uniq, extra]).reshape(N, B).t().contiguous()
    layout = ops.unique_neighbors(nb.cuda())
    assert layout["n_unique"] == n_unique
    ri = lambda *shape: torch.randint(P, shape, generator=g, dtype=torch.int32).cuda()
    batch = {"anchor_idx": ri(B), "positive_idx": ri(B), "negative_idx": ri(B, K), "neighbor_compact": layout}
    return batch, B * (2 + K) + n_unique + 1


def set_options(rides, side=0):
    from p_companion_amd import _lib
    L = _lib.lib()
    assert L.pc_set_option(_lib.PC_OPT_BN_FINALIZE_RIDES, rides) == 0
    assert L.pc_set_option(_lib.PC_OPT_BN_FINALIZE_SIDE, side) == 0


def run_steps(batches, dim, rides, side=0, riding=True, steps=None):
    """Steps a fresh twin (same seed) over the batches under the given option settings; returns every output of the steps."""
    from p_companion_amd.product2vec import FusedAdam, Product2Vec
    torch.manual_seed(1)
    m = Product2Vec(cfg(PRODUCT_EMB_DIM=dim)).to("cuda").train()
    o = FusedAdam(m, lr=3e-3)
    out = {}
    set_options(rides, side)
    try:
        for i, b in enumerate(batches[:steps]):
            if riding:
                out[f"loss{i}"] = m.train_step_indexed(table(dim), b, optimizer=o).clone()
            else:
                out[f"loss{i}"] = m.train_step_indexed(table(dim), b).clone()
                out[f"grad{i}"] = m.flatten_parameters()[1].clone()          # every gradient, dgamma / dbeta among them
                o.step()
        torch.cuda.synchronize()
    finally:
        set_options(1, 0)
    bn = m.ffn[1]
    out.update(param=m.flatten_parameters()[0].clone(), grad=m.flatten_parameters()[1].clone(),
               running_mean=bn.running_mean.clone(), running_var=bn.running_var.clone(),
               num_batches_tracked=bn.num_batches_tracked.clone(), exp_avg=o.exp_avg.clone(), exp_avg_sq=o.exp_avg_sq.clone(),
               step_count=torch.as_tensor(int(o.step_count)))
    return out


def assert_same_bits(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), (what, k)


def test_option_defaults_and_refusals():
    from p_companion_amd import _lib
    L = _lib.lib()
    v = ctypes.c_int(-1)
    assert L.pc_get_option(_lib.PC_OPT_BN_FINALIZE_RIDES, ctypes.byref(v)) == 0 and v.value == 1
    assert L.pc_set_option(_lib.PC_OPT_BN_FINALIZE_RIDES, 2) == -1


_three = {}


def three_steps(rides, side=0):
    """The steps of tests 1 and 6, computed once per option setting: B = 1024, N = 8, D = 128, three batches, Adam riding."""
    if "batches" not in _three:
        made = [make_batch(1024, 8, 2500 + 100 * i, seed=20 + i) for i in range(3)]
        assert [r for _, r in made] == [9669, 9769, 9869] and min(r for _, r in made) >= 8192
        _three["batches"] = [b for b, _ in made]
    if (rides, side) not in _three:
        _three[(rides, side)] = run_steps(_three["batches"], 128, rides, side)
    return _three[(rides, side)]


def test_options_change_no_bit():
    """Three steps from the same state with the optimizer riding: the finalize as riders of dW3 (the default), as its own launch
    on the step's queue, and on the side queue (which overrides the riders): loss, parameters, BatchNorm buffers, both Adam
    moments and the step count, bit for bit."""
    base = three_steps(0)
    assert int(base["step_count"]) == 3 and int(base["num_batches_tracked"]) == 12
    assert_same_bits(base, three_steps(1), "rides")
    assert_same_bits(base, three_steps(1, side=1), "side overrides rides")
    assert_same_bits(base, three_steps(0, side=1), "side")


@pytest.mark.parametrize("n_unique,R,rowless", [(1023, 8192, 0), (1024, 8193, 42)])
def test_rowless_slices_present_and_absent(n_unique, R, rowless):
    """R = 8192: 64 rows per slice, all 128 slices of the dW3 launch own rows and the riders are appended to the grid.
    R = 8193: 96 rows per slice, 86 slices used, 42 own no rows and the riders take eight of their places (the slabs those would
    have zeroed are left out of the sums).  With the optimizer riding, and after a step without it the gradients themselves."""
    rps = (-(-R // 128) + 31) // 32 * 32
    assert 128 - (-(-R // rps)) == rowless
    made = [make_batch(1024, 8, n_unique, seed=40 + i) for i in range(2)]
    assert all(r == R for _, r in made)
    batches = [b for b, _ in made]
    assert_same_bits(run_steps(batches, 128, 0), run_steps(batches, 128, 1), "adam riding")
    g0, g1 = run_steps(batches, 128, 0, riding=False, steps=1), run_steps(batches, 128, 1, riding=False, steps=1)
    assert float(g0["grad0"].abs().max()) > 0
    assert_same_bits(g0, g1, "gradients only")


def test_no_optimizer_equals_the_riding_form_on_the_full_tile_path():
    """train_step_indexed without optimizer= followed by opt.step() against the step with Adam riding in its last launch, at a
    full-tile shape and with the finalize riding in dW3: the same bits (the rows < 8192 form of this is
    test_adam_riding_in_the_steps_last_launch_equals_the_separate_launch)."""
    batches = [make_batch(1024, 8, 1500 + 64 * i, seed=60 + i)[0] for i in range(2)]
    sep = run_steps(batches, 128, 1, riding=False)
    rid = run_steps(batches, 128, 1, riding=True)
    for k in rid:
        assert torch.equal(sep[k], rid[k]), k
    assert_same_bits(sep, run_steps(batches, 128, 0, riding=False), "separate launch, option off")


def test_dim_256():
    """PRODUCT_EMB_DIM = 256 (B = 1024, N = 4): dW5 takes the paired half-slice launch as well (without riders)."""
    b, R = make_batch(1024, 4, 1300, seed=70)
    assert R == 8469
    assert_same_bits(run_steps([b], 256, 0), run_steps([b], 256, 1), "dim 256")


def test_below_the_threshold_nothing_rides():
    """B = 512, R < 8192: the few-row weight-gradient kernels, the finalize keeps its launch whatever the option says."""
    b, R = make_batch(512, 8, 2000, seed=80)
    assert R == 5585 and R < 8192
    assert_same_bits(run_steps([b, b], 128, 0), run_steps([b, b], 128, 1), "below the threshold")


def test_repeatable():
    """The three steps of the first test once more with the riders on: a rider racing its host launch would show here."""
    first = three_steps(1)
    assert_same_bits(first, run_steps(_three["batches"], 128, 1), "second run")
