"""The optimizer state around the Adam kernels: the sharded optimizer's slices at every world size, its checkpoints, what happens
to the moments when the flat buffers' padding changes, and the step count after a refused step.

One process, one GPU, no real collective: ops.CallbackExchange lets a test be "rank r of world W" with Python no-ops behind the
three collective slots (fake_rank), so nothing here can wait for a peer -- the test itself plays the all-gather where a result
depends on it.  Every comparison is torch.equal, or one of the three absolute bounds tests/test_gpu_ops.py::test_adam_matches_torch
asserts for this kernel (2e-7 parameters, 1e-8 exp_avg, 1e-10 exp_avg_sq), here against torch.optim.Adam in float64 on the CPU.
Needs an MI355X."""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

LR = 1e-3
P = 2000            # rows of the Product2Vec feature table
K = 5


def fake_rank(rank, world):
    """(exchange, log): rank `rank` of a world of `world` whose all-reduce / reduce-scatter / all-gather do nothing but append
    (name, n) to `log`."""
    from p_companion_amd import ops
    log = []
    slot = lambda name: (lambda ptr, n, stream: log.append((name, n)))
    ex = ops.CallbackExchange(slot("all_reduce"), kind="no-op callbacks (one process plays every rank)",
                              reduce_scatter=slot("reduce_scatter"), all_gather=slot("all_gather"), rank=rank, world=world)
    return ex, log


def rnd(n, seed, scale):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale


# ------------------------------------------------------------------ A1: slices of every world size
_adam_cases = {}


def adam_case(n):
    """p0, four gradients and the two references for a flat buffer of n floats, computed once per n and never modified:
    the unsharded pc_adam_step_at for t = 1..4 on the device, torch.optim.Adam in float64 on the CPU.
    p0 ~ 0.1 N(0,1): an fp32 parameter carries half an ulp of rounding per step whatever the kernel does, so an ABSOLUTE bound
    of 2e-7 against a float64 reference needs |p| < 1 (4 steps x 2^-25 = 1.2e-7 in [0.5, 1); it is 4.8e-7 in [2, 4), where
    unit-variance values of a million-element buffer lie); the gradients are test_adam_matches_torch's (0.01 N(0,1))."""
    if n not in _adam_cases:
        from p_companion_amd import ops
        p0 = rnd(n, 70, 0.1)
        gs = [rnd(n, 71 + i, 0.01) for i in range(4)]
        ref = p0.double().clone().requires_grad_(True)
        opt = torch.optim.Adam([ref], lr=LR)
        for g in gs:
            ref.grad = g.double()
            opt.step()
        p, m, v = p0.cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        step = torch.zeros(1, dtype=torch.int64, device="cuda")
        for t, g in enumerate(gs, 1):
            ops.adam_step_at(p, g.cuda(), m, v, step, t, lr=LR)
        assert int(step) == 4
        _adam_cases[n] = {"p0": p0, "gs": gs, "p": p, "m": m, "v": v, "p64": ref.detach(), "m64": opt.state[ref]["exp_avg"],
                          "v64": opt.state[ref]["exp_avg_sq"]}
    return _adam_cases[n]


def close(a, b, atol, what):
    err = (a.detach().cpu().double() - b.double()).abs().max().item()
    print(f"{what}: max err {err:.3e} (bound {atol:.1e})")
    assert err <= atol, f"{what}: max err {err:.3e} > {atol:.1e}"


def run_sharded(world, length, device_counter):
    """Four sharded steps of every rank of `world` over the case's gradients; returns the ranks' state."""
    from p_companion_amd import ops
    n = world * length
    case = adam_case(n)
    # rank r's own buffers are row r (n = world * length floats with length % 4 == 0: every row starts 16-byte aligned)
    prm = case["p0"].cuda().repeat(world, 1).contiguous()
    m, v = torch.zeros(world, n, device="cuda"), torch.zeros(world, n, device="cuda")
    steps = torch.zeros(world, 1, dtype=torch.int64, device="cuda")
    scal = torch.zeros(world, 2, device="cuda")
    ranks = [fake_rank(r, world) for r in range(world)]
    for t, g in enumerate(case["gs"], 1):
        grads = g.cuda().repeat(world, 1).contiguous()            # the same gradient on every rank: its mean is itself
        for r, (ex, log) in enumerate(ranks):
            del log[:]
            ops.exchange_adam(ex, prm[r], grads[r], m[r], v[r], steps[r], 0 if device_counter else t, scal[r], lr=LR, shard=True)
            assert log == [("reduce_scatter", length), ("all_gather", length)], (t, r, log)
        # the all-gather, played by the test: slice r of rank r's parameters into every rank's buffer
        own = torch.cat([prm[r, r * length:(r + 1) * length] for r in range(world)])
        prm.copy_(own.unsqueeze(0).expand(world, n))
    return case, prm, m, v, steps


def check_sharded(world, length, device_counter):
    case, prm, m, v, steps = run_sharded(world, length, device_counter)
    n = world * length
    assert steps.flatten().tolist() == [4] * world
    for r in range(world):
        lo, hi = r * length, (r + 1) * length
        assert torch.equal(prm[r], case["p"]), ("param", r)
        for name, buf in (("exp_avg", m), ("exp_avg_sq", v)):
            ref = case["m" if name == "exp_avg" else "v"]
            assert torch.equal(buf[r, lo:hi], ref[lo:hi]), (name, r)
            assert not bool(buf[r, :lo].any()) and not bool(buf[r, hi:].any()), (name, "outside the slice of rank", r)
    # not only against the project's own unsharded kernel: the assembled state against float64 torch.optim.Adam
    m_all = torch.cat([m[r, r * length:(r + 1) * length] for r in range(world)])
    v_all = torch.cat([v[r, r * length:(r + 1) * length] for r in range(world)])
    assert m_all.numel() == n
    close(prm[0], case["p64"], 2e-7, "param vs float64 Adam")
    close(m_all, case["m64"], 1e-8, "exp_avg vs float64 Adam")
    close(v_all, case["v64"], 1e-10, "exp_avg_sq vs float64 Adam")


@pytest.mark.parametrize("length", [4, 8, 1028, 66092])
@pytest.mark.parametrize("world", [1, 2, 3, 5, 6, 7, 12, 16])
def test_slices_of_every_world_size_add_up_to_the_unsharded_update(world, length):
    """pc_exchange_adam_plan(shard) runs Adam on [rank * len, (rank + 1) * len) only: the ranks' slices, put together, are the
    unsharded update bit for bit (and float64 Adam within the kernel's bounds), moments outside a rank's slice stay exactly zero,
    every rank counts four steps, and each step issues one reduce-scatter and one all-gather of len floats."""
    check_sharded(world, length, device_counter=False)


def test_slices_with_the_device_step_counter():
    """The same at world 3 with t = 0: every rank reads its own device counter (pc_adam_step behind the reduce-scatter)."""
    check_sharded(3, 1028, device_counter=True)


# ------------------------------------------------------------------ A2: slices that cannot be 16-byte aligned
@pytest.mark.parametrize("length", [1, 2, 3, 5, 66091])
@pytest.mark.parametrize("world", [3, 5])
def test_unaligned_slices_are_refused_by_every_rank_before_any_collective(world, length):
    """len % 4 != 0: the Adam kernel moves 16-byte chunks, so rank r's slice at param + r * len cannot be served.  Every rank --
    rank 0, whose slice starts aligned, included -- must answer PC_ESHAPE before the reduce-scatter is issued: a rank that
    refuses after it leaves the others waiting in the all-gather."""
    from p_companion_amd import ops
    from p_companion_amd._lib import HipKernelError
    n = world * length
    for r in range(world):
        ex, log = fake_rank(r, world)
        bufs = [rnd(n, 10 * r + i, s).cuda() for i, s in enumerate((0.1, 0.01, 0.001, 1e-5))]
        bufs[3].abs_()
        step = torch.full((1,), 3, dtype=torch.int64, device="cuda")
        scal = torch.zeros(2, device="cuda")
        before = [b.clone() for b in bufs]
        with pytest.raises(HipKernelError, match="pc_exchange_adam_plan: PC_ESHAPE"):
            ops.exchange_adam(ex, bufs[0], bufs[1], bufs[2], bufs[3], step, 4, scal, lr=LR, shard=True)
        torch.cuda.synchronize()
        assert log == [], (r, log)
        for b, b0 in zip(bufs, before):
            assert torch.equal(b, b0), r
        assert int(step) == 3 and not bool(scal.any())


# ------------------------------------------------------------------ A3: GraphedJointStep pads for alignment
T_JOINT, B_JOINT = 601, 64
_joint = {}


def joint_setup():
    if not _joint:
        from p_companion_amd.data import generate_scaled_bpg
        # (600 product types: the batches' type ids reach the rows of the two [T, 64] tables in every rank's slice)
        bpg = generate_scaled_bpg(3000, 600, seed=3)
        _joint.update(bpg=bpg, table=bpg.cuda("cuda")["features"],
                      cfg=SimpleNamespace(PRODUCT_EMB_DIM=128, TYPE_EMB_DIM=64, DROPOUT=0.0, MARGIN=1.0, ALPHA=0.8, NUM_COMP_TYPES=3,
                                          NUM_TYPES=T_JOINT, DEVICE=torch.device("cuda")))
    return _joint


def joint_replica(rank, world, shard, pad_first=None):
    from p_companion_amd.data import ComplementaryIndexDataset, ComplementaryIndexLoader
    from p_companion_amd.p_companion import GraphedJointStep, PCompanion
    from p_companion_amd.product2vec import FusedAdam
    s = joint_setup()
    torch.manual_seed(5)
    m = PCompanion(s["cfg"], s["table"]).to("cuda").train()
    if pad_first is not None:
        m.flatten_parameters(pad_multiple=pad_first)
    o = FusedAdam(m, lr=1e-2)
    ex, log = fake_rank(rank, world)
    g = GraphedJointStep(m, o, B_JOINT, warmup=1, mode="direct", exchange=ex, shard_optimizer=shard)
    ld = ComplementaryIndexLoader(ComplementaryIndexDataset(s["bpg"], "train"), B_JOINT, shuffle=True, seed=20, device="cuda",
                                  out=g.static)
    return m, o, g, ld, log


@pytest.mark.parametrize("rank,world", [(1, 3), (4, 6)])
def test_graphed_joint_step_pads_the_flat_buffers_to_aligned_slices(rank, world):
    """n = 32 (907 + 4 T) = 105 952 floats at T = 601: padded to a multiple of the world size only, a third is 35 318 floats
    (2 mod 4) and every rank but 0 refuses its slice.  Padded to 4 * world every slice starts on a 16-byte boundary: one step by
    step() (pc_exchange_adam_plan) and two by run_epoch (pc_joint_train_epoch_plan) succeed and touch this rank's moments only."""
    m, o, g, ld, log = joint_replica(rank, world, shard=True)
    flat, gflat = m.flatten_parameters()
    n_real = sum(p.numel() for _, p in m._named_flat())
    assert n_real == 32 * (907 + 4 * T_JOINT)
    assert flat.numel() % (4 * world) == 0 and 0 <= flat.numel() - n_real < 4 * world
    assert not bool(flat[n_real:].any()) and not bool(gflat[n_real:].any())
    length = flat.numel() // world
    lo, hi = rank * length, (rank + 1) * length
    p0 = flat.clone()
    batch = next(b for b in ld if b["query_idx"].numel() == B_JOINT)
    g(batch)
    assert log == [("reduce_scatter", length), ("all_gather", length)]
    losses = g.run_epoch(ld, drop_last=True, max_steps=2)
    assert losses.shape == (2, 3) and bool(torch.isfinite(losses).all())
    assert log == [("reduce_scatter", length), ("all_gather", length)] * 3
    assert int(o.step_count) == 3 and o._host_step == 3
    for buf in (o.exp_avg, o.exp_avg_sq):
        assert bool(buf[lo:hi].any())
        assert not bool(buf[:lo].any()) and not bool(buf[hi:].any())
    # (the all-gather is a no-op here: only this rank's slice of the parameters moved)
    assert not torch.equal(flat[lo:hi], p0[lo:hi])
    assert torch.equal(flat[:lo], p0[:lo]) and torch.equal(flat[hi:], p0[hi:])
    assert not bool(flat[n_real:].any())


def test_epoch_call_refuses_unaligned_slices_before_its_first_launch():
    """pc_joint_train_epoch_plan over flat buffers padded to the world size only (105 954 floats at world 3): refused at entry --
    no collective issued, no batch built, no loss row written, no parameter moved."""
    from p_companion_amd._lib import HipKernelError
    m, o, g, ld, log = joint_replica(1, 3, shard=False, pad_first=3)      # (shard=False: the constructor leaves the padding alone)
    g.shard_optimizer = True                                               # ... and the epoch is then asked for the sharded form
    flat, _ = m.flatten_parameters()
    assert flat.numel() == 105954 and (flat.numel() // 3) % 4 == 2
    g._prepare()
    seen = []
    epoch = g.prepared._epoch

    def spy(*args):
        n, steps, losses = epoch(*args)
        losses.fill_(-7.0)
        seen.append(losses)
        return n, steps, losses
    g.prepared._epoch = spy
    p0 = flat.clone()
    static0 = {k: t.clone() for k, t in g.static.items()}
    with pytest.raises(HipKernelError, match="pc_joint_train_epoch_plan: PC_ESHAPE"):
        g.run_epoch(ld, drop_last=True, max_steps=2)
    torch.cuda.synchronize()
    assert log == []
    assert len(seen) == 1 and bool((seen[0] == -7.0).all())
    assert torch.equal(flat, p0)
    for k, t in g.static.items():
        assert torch.equal(t, static0[k]), k
    assert int(o.step_count) == 0 and o._host_step == 0


# ------------------------------------------------------------------ A4 / A5: Product2Vec + FusedAdam
def p2v_cfg():
    return SimpleNamespace(PRODUCT_EMB_DIM=128, TYPE_EMB_DIM=64, HIDDEN_SIZE=256, NUM_ATTENTION_HEADS=4, DROPOUT=0.0, MARGIN=1.0,
                           DEVICE=torch.device("cuda"))


_p2v = {}


def p2v_table():
    if "table" not in _p2v:
        _p2v["table"] = torch.randn(P, 128, generator=torch.Generator().manual_seed(11)).cuda()
    return _p2v["table"]


def make_batch(B, N, n_unique, seed, unique=True):
    """A hand-made index batch whose [B, N] neighbour matrix holds exactly n_unique distinct products (column 0 always a real
    one, a fifth of the other repeated slots padding): in the unique-neighbour layout (the one that carries the riding optimizer
    step), or as the plain matrix."""
    from p_companion_amd import ops
    assert B - 1 <= n_unique <= B * N
    g = torch.Generator().manual_seed(seed)
    uniq = torch.randperm(P, generator=g)[:n_unique].to(torch.int32)
    rest = B * N - n_unique
    extra = uniq[torch.randint(n_unique, (rest,), generator=g)]
    col = (torch.arange(n_unique, B * N) // B)                       # slots are filled column by column
    extra[(torch.rand(rest, generator=g) < 0.2) & (col >= 1)] = -1
    nb = torch.cat([uniq, extra]).reshape(N, B).t().contiguous().cuda()
    ri = lambda *shape: torch.randint(P, shape, generator=g, dtype=torch.int32).cuda()
    batch = {"anchor_idx": ri(B), "positive_idx": ri(B), "negative_idx": ri(B, K)}
    if unique:
        batch["neighbor_compact"] = ops.unique_neighbors(nb)
        assert batch["neighbor_compact"]["n_unique"] == n_unique
    else:
        batch["neighbor_idx"] = nb
    return batch


def p2v_batches(unique=True):
    key = ("batches", unique)
    if key not in _p2v:
        _p2v[key] = [make_batch(64, 4, 100 + 7 * i, seed=30 + i, unique=unique) for i in range(5)]
    return _p2v[key]


def p2v_twin(seed=1, lr=3e-3):
    from p_companion_amd.product2vec import FusedAdam, Product2Vec
    torch.manual_seed(seed)
    m = Product2Vec(p2v_cfg()).to("cuda").train()
    return m, FusedAdam(m, lr=lr)


def assert_state_dicts_equal(a, b):
    assert a["param_groups"] == b["param_groups"]
    assert sorted(a["state"]) == sorted(b["state"]) and len(a["state"]) > 0
    for i in a["state"]:
        assert a["state"][i].keys() == b["state"][i].keys()
        for k in a["state"][i]:
            assert torch.equal(a["state"][i][k], b["state"][i][k]), (i, k)


def assert_twins_equal(ma, oa, mb, ob, steps):
    n_real = sum(p.numel() for _, p in ma._named_flat())
    for (k, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        assert torch.equal(pa, pb), k
    assert torch.equal(oa.exp_avg[:n_real], ob.exp_avg[:n_real]) and torch.equal(oa.exp_avg_sq[:n_real], ob.exp_avg_sq[:n_real])
    assert bool(oa.exp_avg[:n_real].any())
    assert int(oa.step_count) == int(ob.step_count) == steps
    sa, sb = oa.state_dict(), ob.state_dict()
    assert_state_dicts_equal(sa, sb)
    for i in sb["state"]:
        assert float(sb["state"][i]["step"]) == float(steps)


def test_moments_survive_a_change_of_padding_and_nothing_is_reset_silently():
    """A resumed run re-flattens with padding behind load_state_dict() (GraphedJointStep(shard_optimizer=True) does): the loaded
    moments and step count must carry over to the longer buffers -- and where they cannot, the optimizer says so."""
    table, bs = p2v_table(), p2v_batches()
    m0, o0 = p2v_twin()
    for b in bs[:3]:
        m0.train_step_indexed(table, b, optimizer=o0)
    sd_m = {k: t.detach().clone() for k, t in m0.state_dict().items()}
    sd_o = o0.state_dict()
    assert all(float(st["step"]) == 3.0 for st in sd_o["state"].values())
    twins = []
    for pad in (None, 12):
        m, o = p2v_twin(seed=2)
        m.load_state_dict(sd_m)
        o.load_state_dict(sd_o)
        if pad is not None:
            n_before = m.flatten_parameters()[0].numel()
            flat, _ = m.flatten_parameters(pad_multiple=pad)
            assert n_before == 198272 and flat.numel() == 198276                  # (198 272 = 12 * 16 522 + 8)
        for b in bs[3:5]:
            m.train_step_indexed(table, b, optimizer=o)
        twins.append((m, o))
    (ma, oa), (mb, ob) = twins
    assert_twins_equal(ma, oa, mb, ob, steps=5)
    assert oa._host_step == ob._host_step == 5
    assert ob.exp_avg.numel() == 198276 and not bool(ob.exp_avg[198272:].any()) and not bool(ob.exp_avg_sq[198272:].any())
    # what _ensure() cannot carry over is an error once the optimizer has stepped, not a fresh start:
    # flat buffers shorter than the parameters they are said to hold ...
    flat, gflat = mb.flatten_parameters()
    mb.flatten_parameters = lambda pad_multiple=None: (flat[:1000], gflat[:1000])
    with pytest.raises(RuntimeError):
        ob.zero_grad()
    del mb.flatten_parameters
    # ... and another device
    mb.to("cpu")
    with pytest.raises(RuntimeError):
        ob.zero_grad()
    assert int(ob.step_count) == 5 and ob._host_step == 5 and torch.equal(ob.exp_avg[:198272], oa.exp_avg)


def test_a_refused_riding_step_does_not_count():
    """train_step_indexed(optimizer=) asks the optimizer for step number t (riding_state) BEFORE ops.p2v_train_step checks its
    arguments: a call refused on the host must leave the host's step number where the device counter and the moments are."""
    table, bs = p2v_table(), p2v_batches()
    ma, oa = p2v_twin()
    for b in bs[:2]:
        ma.train_step_indexed(table, b, optimizer=oa)
    mb, ob = p2v_twin()
    asked = []
    riding_state = ob.riding_state

    def spy():
        st = riding_state()
        asked.append(None if st is None else st["t"])
        return st
    ob.riding_state = spy
    mb.train_step_indexed(table, bs[0], optimizer=ob)
    flat = mb.flatten_parameters()[0]
    before = [t.clone() for t in (flat, ob.exp_avg, ob.exp_avg_sq)]
    layout = dict(bs[1]["neighbor_compact"])
    layout["n_unique"] += 1                                   # disagrees with its row list: refused by the wrapper, no launch
    with pytest.raises(ValueError, match="n_unique"):
        mb.train_step_indexed(table, dict(bs[1], neighbor_compact=layout), optimizer=ob)
    assert asked == [1, 2]                                    # the optimizer had been asked for step 2 when the call was refused
    torch.cuda.synchronize()
    for t, t0 in zip((flat, ob.exp_avg, ob.exp_avg_sq), before):
        assert torch.equal(t, t0)
    assert int(ob.step_count) == 1 and ob._host_step == 1
    mb.train_step_indexed(table, bs[1], optimizer=ob)
    assert asked == [1, 2, 2]
    assert_twins_equal(ma, oa, mb, ob, steps=2)
    assert ob._host_step == int(ob.step_count) == 2


def test_a_refused_step_before_the_optimizers_own_launch_does_not_count():
    """The same through the non-riding path (a plain neighbour matrix: the update is FusedAdam.step()'s own launch behind the
    step): both paths leave host and device at the same step after a refusal."""
    table, bs = p2v_table(), p2v_batches(unique=False)
    ma, oa = p2v_twin()
    for b in bs[:2]:
        ma.train_step_indexed(table, b, optimizer=oa)
    mb, ob = p2v_twin()
    stepped = []
    step = ob.step
    ob.step = lambda *a, **k: (stepped.append(1), step(*a, **k))[1]
    mb.train_step_indexed(table, bs[0], optimizer=ob)
    with pytest.raises(ValueError, match="negative_idx"):
        mb.train_step_indexed(table, dict(bs[1], negative_idx=bs[1]["negative_idx"][:-1].contiguous()), optimizer=ob)
    assert len(stepped) == 1 and int(ob.step_count) == 1 and ob._host_step == 1
    mb.train_step_indexed(table, bs[1], optimizer=ob)
    assert len(stepped) == 2
    assert_twins_equal(ma, oa, mb, ob, steps=2)
    assert ob._host_step == int(ob.step_count) == 2
