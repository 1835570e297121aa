"""Cases behind tests/test_gpu_batch_builders.py: the Product2Vec batch builders of csrc/sampler.hip (anchors, positives, Philox
negatives; the dense, compact and unique neighbour layouts; the epoch plan) and pc_p2v_concat_step_rows, each at every size at
which its dispatch takes another path.  No GPU and no torch.cuda here: synthetic graphs as numpy arrays, the dispatch arithmetic
the sizes are chosen against (restated from sampler.hip), a traced run of the Philox oracle, the case lists, and plain numpy
references.  Everything the builders write is an integer (`weight` holds counts far below 2^24, exact in fp32): every comparison
is exact.  tests/test_batch_builder_cases_host.py checks on the CPU that the lists reach the branches they name and that every
sample of every sampler case terminates -- the rejection loop of pairs_negatives_body has no exit of its own."""
import functools

import numpy as np

from oracle import philox_oracle


# ------------------------------------------------------------------ the dispatch arithmetic of sampler.hip, restated
UQ_SMALL_MAX = 1 << 20          # products up to which the unique layout scans in 1024-product chunks (256 threads)
UQ_CHUNK = 4096                 # beyond: 4096-product chunks (1024 threads)
UQ_MAX_BLOCKS = 4096            # more chunks than this: PC_ESHAPE
NPOS = NNEG = 8                 # positives / negatives pairs_negatives_body keeps in registers
SAMPLER_THREADS = 128
SCAN_THREADS = 1024             # degree_scan_kernel: one workgroup
PLAN_THREADS = 256              # epoch_plan_kernel: one workgroup per batch


def uq_chunk(p):
    return 1024 if p <= UQ_SMALL_MAX else UQ_CHUNK


def uq_threads(p):
    return uq_chunk(p) // 4


def uq_nblk(p):
    return (p + uq_chunk(p) - 1) // uq_chunk(p)


def scan_per(b):
    """anchors per thread of degree_scan_kernel"""
    return (b + SCAN_THREADS - 1) // SCAN_THREADS


def pair_blocks(b):
    """sampler workgroups: the whole grid of build_pairs_negatives_kernel, the first workgroups of uq_pairs_count_kernel"""
    return (b + SAMPLER_THREADS - 1) // SAMPLER_THREADS


def loader_guard(max_pos, k, p):
    """data.py: k eligible products must be left for the anchor with the most positives"""
    return max_pos + k + 1 <= p


# ------------------------------------------------------------------ graphs
GRAPH_ARRAYS = ("sim_pairs", "cv_rowptr", "cv_col", "sim_rowptr", "sim_col")


def make_graph(p, rows):
    """rows: (anchor, positives, co-views) per listed anchor; every other product has empty rows.  Returns the dict the
    builders take (int32 numpy arrays and n_products; no features) plus pair_start: anchor -> id of its first pair; the
    pairs of an anchor follow each other in the order of its positives."""
    rows = sorted(rows, key=lambda r: r[0])
    anchors = [r[0] for r in rows]
    assert len(set(anchors)) == len(anchors) and 0 <= anchors[0] and anchors[-1] < p
    g = {"n_products": int(p), "pair_start": {}}
    for key, col in (("sim", 1), ("cv", 2)):
        cnt = np.zeros(p + 1, np.int64)
        for r in rows:
            cnt[r[0] + 1] = len(r[col])
        g[key + "_rowptr"] = np.cumsum(cnt).astype(np.int32)
        flat = [x for r in rows for x in r[col]]
        assert all(0 <= x < p for x in flat)
        g[key + "_col"] = np.asarray(flat, np.int32)
    pairs, n = [], 0
    for a, pos, _ in rows:
        g["pair_start"][a] = n
        pairs += [(a, q) for q in pos]
        n += len(pos)
    g["sim_pairs"] = np.asarray(pairs, np.int32).reshape(-1, 2)
    assert len(g["cv_col"]) > 0 and len(g["sim_col"]) > 0           # (the C ABI refuses NULL arrays)
    return g


def dense_neighbors(g, pair_ids, n_pad):
    """[B, n_pad]: the anchor's co-view row, cut at n_pad, -1 padded"""
    out = np.full((len(pair_ids), n_pad), -1, np.int32)
    for b, a in enumerate(g["sim_pairs"][pair_ids, 0]):
        row = g["cv_col"][g["cv_rowptr"][a]:g["cv_rowptr"][a + 1]][:n_pad]
        out[b, :len(row)] = row
    return out


def capped_degrees(g, pair_ids, n_pad):
    a = g["sim_pairs"][pair_ids, 0]
    return np.minimum(g["cv_rowptr"][a + 1] - g["cv_rowptr"][a], n_pad).astype(np.int64)


# ------------------------------------------------------------------ negatives and pairs
SAMPLER_KS = (1, 5, 8, 9, 12)                      # 8 / 9: the last K in registers, the first that re-reads negative_idx
SAMPLER_BS = (1, 127, 128, 129, 300)               # both sides of one 128-thread workgroup; three workgroups
SAMPLER_SEEDS = ((0, 0), ((7 << 33) + 9, 12345), ((1 << 40) + 5, (1 << 32) + 3))       # the last: counter words 2 AND 3
SAMPLER_POSITIVES = (20, 9, 8, 1)                  # per anchor, in batch order: sample 0 has a tail of twelve
SAMPLER_COVIEWS = (12, 7, 3, 0)
# "min": the fewest products the loader's guard allows (20 positives + K + the anchor): the anchor with 20 positives has
# exactly K eligible products.  1023 / 1024: `bits` of Philox::below changes at the power of two.
SAMPLER_PS = ("min", 1023, 1024, 1000, (1 << 20) + 1)
SAMPLER_NPADS = (0, 11, 12, 14)                    # dense layout: none, below / at / above the largest degree
MAX_DRAWS = 10_000                                 # 32-bit words per sample, asserted on the host before any launch


def sampler_products(p_class, k):
    return max(SAMPLER_POSITIVES) + k + 1 if p_class == "min" else p_class


def _sampler_cases():
    cases = []
    for i, k in enumerate(SAMPLER_KS):             # every K at every catalogue size; B and (seed, step) rotate
        for j, pc in enumerate(SAMPLER_PS):
            cases.append((pc, k, SAMPLER_BS[(i + j) % 5], (i + 2 * j) % 3))
    for b in SAMPLER_BS:                           # every B with every (seed, step), past the register window
        for s in range(3):
            cases.append((1000, 9, b, s))
    for s in range(3):                             # heavy rejection at K > 8 on both sides of a workgroup
        cases += [("min", 12, 300, s), ("min", 9, 129, s), ("min", 8, 127, s)]
    return sorted(set(cases), key=lambda c: (str(c[0]), c[1:]))


SAMPLER_CASES = _sampler_cases()                   # (p_class, K, B, index into SAMPLER_SEEDS)
# the compact and unique entries against the dense one only (the pure-Python oracle is too slow): 1025 and 4096 put 9 and
# 32 sampler workgroups in front of the unique entry's counting workgroups
SAMPLER_WIDE_CASES = [(1000, 5, 1025, 1), (1000, 9, 1025, 2), (1000, 12, 4096, 0), ("min", 9, 4096, 2), ((1 << 20) + 1, 8, 4096, 1)]


def case_id(c):
    return "-".join(str(x) for x in c)


@functools.lru_cache(maxsize=None)
def sampler_graph(p):
    """four anchors with 20, 9, 8 and 1 positives (distinct, never the anchor, in random order) and 12, 7, 3 and 0 co-views;
    the first anchor is product P - 1, the second product 0"""
    rng = np.random.default_rng(1000 + p)
    anchors = (p - 1, 0, p // 2, 1)
    rows = []
    for a, npos, ncv in zip(anchors, SAMPLER_POSITIVES, SAMPLER_COVIEWS):
        pos = rng.choice(p - 1, npos, replace=False)
        pos = np.where(pos >= a, pos + 1, pos)                      # skip the anchor itself
        rows.append((a, pos.tolist(), rng.integers(0, p, ncv).tolist()))
    g = make_graph(p, rows)
    g["anchors"] = anchors
    return g


def sampler_pair_ids(g, b):
    """sample i takes anchor i % 4 (20, 9, 8, 1 positives) and walks through its pairs"""
    ids = [g["pair_start"][g["anchors"][i % 4]] + (i // 4) % SAMPLER_POSITIVES[i % 4] for i in range(b)]
    return np.asarray(ids, np.int32)


def sampler_inputs(case):
    pc, k, b, s = case
    g = sampler_graph(sampler_products(pc, k))
    seed, step = SAMPLER_SEEDS[s]
    n_pad = SAMPLER_NPADS[(SAMPLER_KS.index(k) + SAMPLER_BS.index(b) + s) % 4] if b in SAMPLER_BS else 12
    return g, sampler_pair_ids(g, b), k, seed, step, n_pad


REASONS = ("anchor", "first8", "tail", "repeat")


def traced_oracle(g, pair_ids, n_pad, k, seed, step):
    """philox_oracle.build_batch and, per sample, what its loop did: `words` 32-bit draws, `draws` candidates, and how many
    candidates were rejected as the anchor, as one of its first eight positives, as a positive past the eighth (`tail`; `tail8`
    of them as the ninth), or as a repeat -- judged in the kernel's order.  Returns (anchor, positive, negatives,
    neighbours), [per-sample dict]."""
    b = len(pair_ids)
    tr = [dict(words=0, draws=0, anchor=0, first8=0, tail=0, tail8=0, repeat=0, got=[]) for _ in range(b)]
    anchors = g["sim_pairs"][pair_ids, 0].tolist()
    rows = {a: g["sim_col"][g["sim_rowptr"][a]:g["sim_rowptr"][a + 1]].tolist() for a in set(anchors)}

    def on_draw(i, c, stream):
        t = tr[i]
        a = anchors[i]
        pos = rows[a]
        t["draws"] += 1
        t["words"] = 4 * stream.block - len(stream.buf)
        if c == a:
            t["anchor"] += 1
        elif c in pos[:NPOS]:
            t["first8"] += 1
        elif c in pos[NPOS:]:
            t["tail"] += 1
            t["tail8"] += c == pos[NPOS]
        elif c in t["got"]:
            t["repeat"] += 1
        else:
            t["got"].append(c)

    out = philox_oracle.build_batch(pair_ids, g["sim_pairs"], g["cv_rowptr"], g["cv_col"], g["sim_rowptr"], g["sim_col"],
                                    g["n_products"], n_pad, k, seed, step, on_draw=on_draw)
    for i, t in enumerate(tr):
        assert t.pop("got") == out[2][i].tolist()                    # the trace judged as the oracle did
    return out, tr


@functools.lru_cache(maxsize=None)
def sampler_expected(case):
    """the oracle's batch of a sampler case and its trace, computed once per process"""
    g, ids, k, seed, step, n_pad = sampler_inputs(case)
    return traced_oracle(g, ids, n_pad, k, seed, step)


# ------------------------------------------------------------------ neighbour layouts
NB_NPAD = 6
NB_DEGREES = (0, 1, 2, 3, 5, 6, 7, 9)              # below, at and above n_pad
NB_GROUP = 24                                      # anchors per group
# 1024 / 1025: one and two chunks.  262 144 and 262 145 + 1024: 256 and 258 chunks -- the predecessor loop of
# uq_assign_kernel<256> strides by 256.  2^20: the last size of the 256-thread forms (1024 chunks: four strides), 2^20 + 1 the
# first of the 1024-thread forms; 4 000 000: the largest catalogue the loader keeps the unique layout for.
UNIQUE_PS = (1024, 1025, 5000, 262_144, 262_145 + 1024, 1 << 20, (1 << 20) + 1, 4_000_000)
UNIQUE_B = 50
HOT_B = 33
COMPACT_BS = (1, 1023, 1024, 1025, 4096, 8193, 9000)          # per = 1, 1, 1, 2 (threads past 512 own nothing), 4, 9, 9
DENSE_NPADS = (0, 5, 9, 12)                                    # none; below, at, above the largest degree (9)


def unique_edge_products(p):
    """first and last product of the first, second, last-but-one and last chunk, of chunk 256 (the first that a second trip
    of the predecessor loop reads) and the product P - 1"""
    c, n = uq_chunk(p), uq_nblk(p)
    e = {0, c - 1, c, 2 * c - 1, (n - 1) * c - 1, (n - 1) * c, p - 1, 256 * c, 257 * c - 1, 257 * c}
    return sorted(x for x in e if 0 <= x < p)


@functools.lru_cache(maxsize=None)
def neighbour_graph(p):
    """Two groups of 24 anchors whose co-view rows draw from two DISJOINT product pools (pool 0: the chunk-edge products and 40
    more; pool 1: their neighbours x +- 1 and 40 more), degrees 0 .. 9 around n_pad = 6 -- the edge products within the first
    six entries, so that the cap does not cut them --, three anchors without co-views and a `hot` anchor whose row is product
    P - 1 six times.  One positive per anchor: the pair id of an anchor is pair_start[anchor]."""
    rng = np.random.default_rng(7 + p)
    edge = unique_edge_products(p)
    near = sorted({x + d for x in edge for d in (-1, 1) if 0 <= x + d < p} - set(edge))
    rest = [int(x) for x in rng.choice(p, 400, replace=False) if x not in edge and x not in near]
    pools = (edge + rest[:40], near + rest[40:80])
    anchors = [int(x) for x in rng.choice(p, 2 * NB_GROUP + 4, replace=False)]
    rows, groups = [], []
    for gi, pool in enumerate(pools):
        first = list(pool[:len(pool) - 40])                          # dealt out once each, into visible slots
        group = anchors[gi * NB_GROUP:(gi + 1) * NB_GROUP]
        for i, a in enumerate(group):
            deg = NB_DEGREES[i % len(NB_DEGREES)]
            row = []
            for j in range(deg):
                row.append(first.pop(0) if first and j < NB_NPAD else int(pool[rng.integers(len(pool))]))
            rows.append((a, [(a + 7) % p], row))
        assert not first
        groups.append(group)
    bare, hot = anchors[2 * NB_GROUP:2 * NB_GROUP + 3], anchors[-1]
    rows += [(a, [(a + 7) % p], []) for a in bare] + [(hot, [(hot + 7) % p], [p - 1] * NB_NPAD)]
    g = make_graph(p, rows)
    g.update(groups=groups, bare=bare, hot=hot, edge=edge, pools=pools)
    return g


def pairs_of(g, anchors):
    return np.asarray([g["pair_start"][a] for a in anchors], np.int32)


def unique_batches(p):
    """the five batches of a unique-layout case, run in this order on one scratch: group 0; group 0 again; group 1 (products
    disjoint from group 0's: a stale count or rank would show); the hot anchor 33 times (one row of weight 33 * 6); anchors
    without co-views (padding alone: U = 0)"""
    g = neighbour_graph(p)
    rng = np.random.default_rng(11 + p)
    batch = []
    for group in g["groups"]:
        order = list(rng.permutation(NB_GROUP)) + list(rng.integers(0, NB_GROUP, UNIQUE_B - NB_GROUP))
        batch.append(pairs_of(g, [group[i] for i in order]))
    return g, [("first", batch[0]), ("again", batch[0]), ("disjoint", batch[1]), ("hot", pairs_of(g, [g["hot"]] * HOT_B)),
               ("padding", pairs_of(g, [g["bare"][i % 3] for i in range(7)]))]


def compact_batch(g, b, bare_only=False):
    rng = np.random.default_rng(13 + b)
    pool = g["bare"] if bare_only else g["groups"][0] + g["groups"][1] + g["bare"] + [g["hot"]]
    return pairs_of(g, [pool[i] for i in rng.integers(0, len(pool), b)])


def degree_scan_restated(deg, per):
    """degree_scan_kernel's ownership and scan in numpy: thread t owns anchors [t * per, min(B, t * per + per)), the exclusive
    scan of the 1024 partial sums starts each thread's run.  -> row_off [B + 1]"""
    b = len(deg)
    lo = np.minimum(np.arange(SCAN_THREADS) * per, b)
    hi = np.minimum(lo + per, b)
    part = np.asarray([deg[l:h].sum() for l, h in zip(lo, hi)], np.int64)
    start = np.cumsum(part) - part
    row_off = np.full(b + 1, -1, np.int64)
    for t in range(SCAN_THREADS):
        row_off[lo[t]:hi[t]] = start[t] + np.cumsum(deg[lo[t]:hi[t]]) - deg[lo[t]:hi[t]]
    row_off[b] = part.sum()
    return row_off


# ------------------------------------------------------------------ concat_step_rows
# (B, K, capacity of nb_rows, n_unique as the device holds it) -> rows taken from nb_rows: min(max(n_unique + 1, 1), capacity)
CONCAT_CASES = [(1, 1, 1, 0), (300, 5, 41, 0), (300, 5, 41, 40), (300, 5, 41, 17), (300, 5, 41, 41), (300, 5, 41, 1 << 30),
                (300, 5, 41, -7), (257, 12, 700, 699), (257, 12, 700, 255), (1, 12, 3, 5)]
CONCAT_SENTINEL = -77


def concat_expected(a, p, ng, nb_rows, n_unique, out_len):
    nb = min(max(n_unique + 1, 1), len(nb_rows))
    rows = np.concatenate([a, nb_rows[:nb], p, ng.reshape(-1)]).astype(np.int32)
    return np.concatenate([rows, np.full(out_len - len(rows), CONCAT_SENTINEL, np.int32)])


# ------------------------------------------------------------------ epoch_plan
PLAN_BS = (1, 255, 257, 4096)                      # one thread; one short of / one past the workgroup; sixteen trips
# (n, B, shuffled order?, degrees): n < B, n = 3 B, a last batch of one element; "big": every degree 2^20, so that a batch of
# 4096 sums to 2^32 exactly (an int accumulator would give 0)
PLAN_CASES = [(n, b, o, "small") for b in PLAN_BS for n in sorted({max(b - 1, 1), 3 * b, 2 * b + 1}) for o in (False, True)]
PLAN_CASES += [(2 * 4096 + 1, 4096, o, "big") for o in (False, True)]


def plan_inputs(case):
    n, b, shuffled, kind = case
    rng = np.random.default_rng(17 + n + b)
    deg = np.full(n, 1 << 20, np.int32) if kind == "big" else rng.integers(0, 60, n).astype(np.int32)
    order = rng.permutation(n).astype(np.int32) if shuffled else None
    return deg, order, (n + b - 1) // b


def plan_expected(deg, order, n, b):
    d = deg[order].astype(np.int64) if order is not None else deg.astype(np.int64)
    nb = (n + b - 1) // b
    return np.asarray([[d[i * b:(i + 1) * b].max(), d[i * b:(i + 1) * b].sum()] for i in range(nb)], np.int64)
