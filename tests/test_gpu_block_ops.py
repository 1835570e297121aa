"""The edges of csrc/block_ops.h's radix pass behind its two callers, through the public functions and bit for bit against the
numpy twins of tests/test_gpu_table_train.py and tests/test_gpu_ingest.py: the sparse Adam's sort (1024 threads, key + value)
at the wave, tile, chunk and one-workgroup / multi-workgroup edges for one, two and three digit passes, and the ingestion's row
sort (256 threads, keys only) at its tile edges on the LDS path and on the path through global memory, on rows whose waves all
hold one digit.  Needs an MI355X."""
import numpy as np
import pytest
import torch

from test_gpu_ingest import assert_equal_to_host, assert_same_bits
from test_gpu_table_train import adam_case_idx, bits, canaries_intact, guarded, sparse_adam_ref

pytestmark = pytest.mark.gpu

ADAM_R = [63, 64, 65, 1023, 1024, 1025, 4096, 4097, 8192, 8193, 12289]     # wave | tile | TT_CHUNK | TT_SMALL_R edges, three chunks
ADAM_P = [200, 255, 256, 65535, 65536]                                     # bit_length(P) = 8, 8, 9, 16, 17: 1, 1, 2, 2, 3 passes
EDGES = (64, 1024, 4096, 8192)


def adam_edge_idx(rng, R, P):
    """adam_case_idx's draw (with its -1 / P / -2 entries where it puts them), and over its valid entries: one id on the last
    two valid source positions below and the first two from every edge e in EDGES below R (its multiplicity straddles the
    wave, tile and chunk edge of the scatter), and ids that share their low bytes and differ in the top digit alone (c + 256 j;
    with P itself a multiple of 256, id 0 against the key P of the skipped sources).  Returns (idx, the ids pinned at the edges)."""
    idx = adam_case_idx(rng, R, P)
    valid = (idx >= 0) & (idx < P)
    ids = rng.choice(P, len(EDGES) + 1, replace=False).astype(np.int32)
    pinned = {}
    for e, u in zip(EDGES, ids):
        below, above = np.nonzero(valid[:e])[0][-2:], e + np.nonzero(valid[e:])[0][:2]
        if below.size and above.size:
            idx[below], idx[above] = u, u
            pinned[e] = int(u)
    free = np.nonzero(valid & ~np.isin(idx, ids[:len(EDGES)]))[0]
    free = free[rng.permutation(free.size)]
    if P > 256:
        c, tops = int(ids[-1]) % 256, min(4, (P - 1) // 256)
        for j, q in enumerate(free[:2 * (tops + 1)]):
            idx[q] = c + 256 * (j % (tops + 1))
    if P % 256 == 0:
        idx[free[-2:]] = 0                                             # (id 0 and the key P differ in the top digit alone)
    return idx, pinned


def adam_rng(R, P, D):
    return np.random.default_rng(7001 * D + 31 * R + P)


def adam_steps(R, P, D):
    from p_companion_amd import ops
    rng = adam_rng(R, P, D)
    f = np.float32
    p = rng.standard_normal((P, D)).astype(f)
    m, v = np.zeros((P, D), f), np.zeros((P, D), f)
    (pb, pd), (mb, md), (vb, vd) = guarded(p), guarded(m), guarded(v)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    lr, (b1, b2), eps = 1e-3, (0.9, 0.999), 1e-8
    nbad, straddled = 0, set()
    for t in range(1, 6):
        idx, pinned = adam_edge_idx(rng, R, P)
        straddled |= set(pinned)                                       # (an edge is left out of a step whose only source behind it is skipped)
        for e, u in pinned.items():
            at = np.nonzero(idx == u)[0]
            assert at.min() < e <= at.max()                            # the id's sources lie on both sides of the edge
        grad = (rng.standard_normal((R, D)) * 10.0 ** rng.uniform(-6, 1, (R, 1))).astype(f)
        didx, dgrad = torch.from_numpy(idx).cuda(), torch.from_numpy(grad).cuda()
        if t == 3:
            twin = [x.clone() for x in (pd, md, vd)]
            ops.sparse_adam_rows(twin[0], twin[1], twin[2], didx, dgrad, t, lr, (b1, b2), eps)
        ops.sparse_adam_rows(pd, md, vd, didx, dgrad, t, lr, (b1, b2), eps, bad=bad)
        if t == 3:
            for a, b in zip(twin, (pd, md, vd)):
                assert torch.equal(bits(a), bits(b))
        nbad += sparse_adam_ref(p, m, v, idx, grad, t, lr, b1, b2, eps)
        for name, dev, ref in (("exp_avg", md, m), ("exp_avg_sq", vd, v), ("table", pd, p)):
            got = dev.cpu().numpy()
            diff = np.nonzero((got.view(np.int32) != ref.view(np.int32)).any(axis=1))[0]
            assert diff.size == 0, (name, t, diff[:5], got[diff[:1]], ref[diff[:1]])
        assert int(bad) == nbad
    assert nbad > 0 and sorted(straddled) == [e for e in EDGES if e < R]
    assert canaries_intact(pb) and canaries_intact(mb) and canaries_intact(vb)


@pytest.mark.parametrize("P", ADAM_P)
@pytest.mark.parametrize("R", ADAM_R)
def test_sparse_adam_sort_edges(R, P):
    adam_steps(R, P, 128)


def test_sparse_adam_sort_edges_at_256_dims():
    adam_steps(8193, 65536, 256)


# ------------------------------------------------------------------ the ingestion's row sort
ROW_LENGTHS = [255, 256, 257, 511, 512, 513, 4351, 4352, 4353]             # 256-thread tile edges: LDS path, then global path


def _one_digit_lists(P, seed):
    """co_view rows of the raw lengths above on sources 0..8, and rows of the same lengths in the other two lists on sources
    10..18 and 20..28.  Every target of the row of source s is 40 + s + 256 j: the low byte is the same, so in the first pass
    every wave of a tile holds one digit.  j is drawn with replacement, skewed, so the weights differ."""
    rng = np.random.default_rng(seed)
    J = (P - 1 - 40 - 28) // 256 + 1                                       # the j with 40 + 28 + 256 j < P

    def rows(first):
        out = []
        for k, n in enumerate(ROW_LENGTHS):
            s = first + k
            j = np.minimum((rng.random(n) ** 2 * J).astype(np.int64), J - 1)
            out.append(np.stack([np.full(n, s), 40 + s + 256 * j], 1))
        return out

    cv, pv, cp = rows(0), rows(10), rows(20)
    both = np.concatenate(cv)
    pv = pv + [both[(both[:, 1] // 256) % 2 == 0]]                        # some co-view edges are purchased after view ...
    cp = cp + [both[(both[:, 1] // 256) % 3 == 1]]                        # ... and some co-purchased
    mix = lambda parts: np.concatenate(parts).astype(np.int32)[rng.permutation(sum(len(p) for p in parts))]
    return mix(cv), mix(pv), mix(cp)


@pytest.fixture(scope="module", params=[65536, 70_000], ids=["two_passes", "four_passes"])
def one_digit_lists(request):
    return request.param, _one_digit_lists(request.param, 21)


@pytest.mark.parametrize("cap", [1, 64])
def test_ingest_row_sort_tile_edges(one_digit_lists, cap):
    from p_companion_amd import ops
    from p_companion_amd.data import IntBPG, device_bpg_from_edges
    P, (cv, pv, cp) = one_digit_lists
    assert ops.INGEST_WAVE_ROW_MAX < 255 and 513 <= ops.INGEST_LDS_ROW_MAX < 4351
    types = (np.arange(P) % 7).astype(np.int32)
    for edges, first in ((cv, 0), (pv, 10), (cp, 20)):
        assert np.bincount(edges[:, 0], minlength=P)[first:first + 9].tolist() == ROW_LENGTHS
        for k in range(9):
            assert np.unique(edges[edges[:, 0] == first + k, 1] % 256).tolist() == [(40 + first + k) % 256]
    host = IntBPG.from_edges(None, types, cv, pv, cp, degree_cap=cap)
    assert host.max_degree == cap and len(host.similarity_pairs) > 0
    dev = [torch.from_numpy(a).cuda() for a in (cv, pv, cp)]
    d = device_bpg_from_edges(None, types, 7, *dev, degree_cap=cap)
    assert_equal_to_host(d, host)
    # the same lists in another order: identical bits
    gen = torch.Generator(device="cuda").manual_seed(11)
    shuffled = [a[torch.randperm(a.shape[0], device="cuda", generator=gen)].contiguous() for a in dev]
    assert not torch.equal(shuffled[0], dev[0])
    assert_same_bits(d, device_bpg_from_edges(None, types, 7, *shuffled, degree_cap=cap))
