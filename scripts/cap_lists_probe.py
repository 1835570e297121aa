"""Developer tool: what the group cap costs beside the pool it caps, beside a plain-torch formulation of the same contract, and
what it does to the lists (pc_cap_lists; ops.cap_lists; PCompanionInference.recommend_capped_batch / recommend_page_batch).
On the SAME rows, proj and catalogue, alternating in one process, with group = id // 4 ("four variants each"), caps 1 and 2,
pools of 64 and 256 and n = 10 shown:

  cap_lists(pool -> n)                        the kernel alone, on retrieve_list_grouped(pool)'s output; also without groups
                                              (the sort alone)
  torch_cap_lists(pool -> n)                  the contract in plain torch: two stable sorts (id, then score), a gather of the
                                              groups, a segmented rank (a stable sort by group and a running maximum), a prefix
                                              sum and a scatter.  The probe asserts that both return the same ids and score bits.
  recommend_batch(pool) / recommend_capped_batch(n, pool)
                                              the method beside the pool call it wraps (model forward included in both)
  recommend_batch(per_type) / recommend_page_batch(n, per_type)
                                              the merged page beside the K lists it merges, per_type 4 and 16

  100 k / 100 types      generate_scaled_bpg, uploaded
  10 M / 100 types       generate_device_bpg

Rows: B queries x K = 3 predicted types from the model's forward (as long_list_probe.py).  ms from the host clock between two
device synchronisations: `--warmup` untimed rounds, then `--reps` rounds, each round one call of every leg in turn; medians
with min .. max.  What the cap does (`--effect-legs`): the share of lists it changes, the share it leaves short, and the
largest number of products of one group in a served list with and without it -- over the generator's catalogue, whose
"variants" id // 4 are unrelated products (the cap hardly ever bites: recorded, not assumed), and over a VARIANT catalogue:
the same graph with every product given the type of its group's first member and that member's features plus N(0, I) x
`--variant-noise`, so that variants score alike as they do in a shop.  Nothing here is a gate.  Writes
profiles/cap_lists_probe.json (or --out) and prints the same JSON as one line.

  python scripts/cap_lists_probe.py [--legs 100k,10M] [--effect-legs 100k] [--warmup 3] [--reps 10] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import numpy as np
import torch

from diversify_probe import served

LEGS = {"100k": (100_000, 100, 128), "10M": (10_000_000, 100, 128)}
POOLS = (64, 256)
CAPS = (1, 2)
PER_TYPE = (4, 16)
N_SHOWN = 10
VARIANTS = 4
NONE = 2 ** 31 - 1


def alternating_host(fns, warmup, reps):
    """{name: {median_ms, min_ms, max_ms, reps}}: every round runs each function once, in turn; the host clock between two
    device synchronisations."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return {k: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)), "reps": reps}
            for k, v in ms.items()}


def torch_cap_lists(idx, score, n, group, cap):
    """ops.cap_lists(idx, score, n, group, cap) in plain torch, nothing read back."""
    r, m = idx.shape
    p = group.shape[0]
    ok = (idx >= 0) & (idx < p) & torch.isfinite(score)
    ids = torch.where(ok, idx, NONE)
    sc = torch.where(ok, score, float("-inf"))
    by_id = torch.argsort(ids, dim=1, stable=True)                                # product index ascending ...
    ids, sc = ids.gather(1, by_id), sc.gather(1, by_id)
    by_sc = torch.argsort(sc, dim=1, descending=True, stable=True)                # ... under score descending
    ids, sc = ids.gather(1, by_sc), sc.gather(1, by_sc)
    real = ids != NONE
    g = torch.where(real, group[ids.clamp(max=p - 1).long()], -1)
    # the number of earlier slots of the same group: a stable sort by group keeps the serving order inside a group
    by_g = torch.argsort(g, dim=1, stable=True)
    gs = g.gather(1, by_g)
    pos = torch.arange(m, device=idx.device).expand(r, m)
    first = torch.ones_like(gs, dtype=torch.bool)
    first[:, 1:] = gs[:, 1:] != gs[:, :-1]
    start = torch.where(first, pos, 0).cummax(1).values
    before = torch.empty(r, m, dtype=torch.int64, device=idx.device).scatter_(1, by_g, pos - start)
    keep = real & ((g < 0) | (before < cap))
    place = keep.cumsum(1) - 1
    to = torch.where(keep & (place < n), place, n)                               # column n: the bin
    out_i = torch.full((r, n + 1), -1, dtype=torch.int32, device=idx.device).scatter_(1, to, ids)
    out_s = torch.full((r, n + 1), float("-inf"), device=idx.device).scatter_(1, to, sc)
    return out_i[:, :n].contiguous(), out_s[:, :n].contiguous()


def same(a, b):
    return bool(torch.equal(a[0], b[0]) and torch.equal(a[1].contiguous().view(torch.int32), b[1].contiguous().view(torch.int32)))


def most_of_a_group(idx, group):
    """the largest number of products of one group in any list of idx [..., n]"""
    idx = idx.reshape(-1, idx.shape[-1])
    g = torch.where(idx >= 0, group[idx.clamp(min=0).long()], -1)
    return int(((g[:, :, None] == g[:, None, :]) & (g[:, :, None] >= 0)).sum(2).max())


def effect(inf, q, group):
    """What the cap does to recommend_batch's lists of N_SHOWN, per pool and cap."""
    out = {}
    _, plain, _ = inf.recommend_batch(q, N_SHOWN)
    lists = plain.shape[0] * plain.shape[1]
    out["largest_group_count_uncapped"] = most_of_a_group(plain, group)
    for m in POOLS:
        for cap in CAPS:
            _, idx, _ = inf.recommend_capped_batch(q, N_SHOWN, group=group, cap=cap, pool=m)
            out[f"pool_{m}_cap_{cap}"] = {
                "share_of_lists_changed": float((idx != plain).any(2).sum()) / lists,
                "share_of_lists_short": float(((idx < 0).any(2) & ~(plain < 0).any(2)).sum()) / lists,
                "largest_group_count": most_of_a_group(idx, group)}
    for per_type in PER_TYPE:
        merged, _, _ = inf.recommend_page_batch(q, N_SHOWN, per_type=per_type)
        capped, _, _ = inf.recommend_page_batch(q, N_SHOWN, per_type=per_type, group=group, cap=1)
        out[f"page_per_type_{per_type}_cap_1"] = {
            "share_of_pages_changed": float((capped != merged).any(1).sum()) / merged.shape[0],
            "share_of_pages_short": float(((capped < 0).any(1) & ~(merged < 0).any(1)).sum()) / merged.shape[0],
            "largest_group_count": most_of_a_group(capped, group),
            "largest_group_count_uncapped": most_of_a_group(merged, group)}
    return out


def variant_arrays(bpg, g, noise, d):
    """The graph's arrays with every product a near-copy of its group's first member: that member's type, its features plus
    N(0, I) x noise."""
    from p_companion_amd.data import DeviceBPG
    if isinstance(bpg, DeviceBPG):
        arrays = dict(bpg.arrays)
    else:
        arrays = dict(g)
        arrays["max_degree"] = int(np.diff(bpg.cv_rowptr).max())
    p = g["type_idx"].shape[0]
    head = (torch.arange(p, device=g["type_idx"].device) // VARIANTS) * VARIANTS
    gen = torch.Generator(device="cpu").manual_seed(7)
    arrays["type_idx"] = g["type_idx"][head].contiguous()
    arrays["features"] = (g["features"][head] + noise * torch.randn(p, d, generator=gen).to(g["features"].device)).contiguous()
    return arrays


def leg(name, args, dev):
    from p_companion_amd import ops
    from p_companion_amd.data import DeviceBPG, generate_device_bpg, generate_scaled_bpg
    P, T, d = LEGS[name]
    t0 = time.time()
    if P <= 1_000_000:
        bpg, src = generate_scaled_bpg(P, T, seed=0, dim=d), "generate_scaled_bpg (uploaded IntBPG)"
    else:
        bpg, src = generate_device_bpg(P, T, seed=0, dim=d, world=1, with_complementary=False), "generate_device_bpg"
    g = bpg.cuda(dev)
    torch.cuda.synchronize()
    out = {"source": src, "products": P, "types": T, "dim": d, "B": args.batch, "K": 3, "n": N_SHOWN, "group": f"id // {VARIANTS}",
           "generate_s": round(time.time() - t0, 2)}
    inf = served(bpg, g["features"], T, d, dev)
    rowptr, col, table = inf.type_rowptr, inf.type_col, inf.features
    q = torch.from_numpy(np.random.default_rng(1).integers(0, P, args.batch).astype(np.int32)).to(dev)
    group = (torch.arange(P, dtype=torch.int32, device=dev) // VARIANTS).contiguous()
    with torch.no_grad():
        fwd = inf.model({"query_idx": q, "query_types": inf.type_idx[q.long()]})
    proj = fwd["projected_embeddings"].contiguous().reshape(-1, d)
    types = fwd["complementary_types"].to(torch.int32).reshape(-1).contiguous()
    out["rows"] = int(types.numel())
    fns, pools = {}, {}
    for m in POOLS:
        pools[m] = ops.retrieve_list_grouped(proj, types, rowptr, col, table, m)
        fns[f"retrieve_list_grouped_{m}"] = (lambda m=m: ops.retrieve_list_grouped(proj, types, rowptr, col, table, m))
        fns[f"cap_lists_{m}_no_group"] = (lambda m=m: ops.cap_lists(*pools[m], N_SHOWN))
        for cap in CAPS:
            fns[f"cap_lists_{m}_cap_{cap}"] = (lambda m=m, cap=cap: ops.cap_lists(*pools[m], N_SHOWN, group, cap))
            fns[f"torch_cap_lists_{m}_cap_{cap}"] = (lambda m=m, cap=cap: torch_cap_lists(*pools[m], N_SHOWN, group, cap))
        fns[f"recommend_batch_{m}"] = (lambda m=m: inf.recommend_batch(q, m))
        fns[f"recommend_capped_batch_{N_SHOWN}_of_{m}"] = (lambda m=m: inf.recommend_capped_batch(q, N_SHOWN, group=group, cap=1,
                                                                                                  pool=m))
    for per_type in PER_TYPE:
        fns[f"recommend_batch_{per_type}"] = (lambda k=per_type: inf.recommend_batch(q, k))
        fns[f"recommend_page_batch_{N_SHOWN}_of_3x{per_type}"] = (lambda k=per_type: inf.recommend_page_batch(
            q, N_SHOWN, per_type=k, group=group, cap=1))
    t = alternating_host(fns, args.warmup, args.reps)
    out.update(t)
    med = lambda k: t[k]["median_ms"]
    for m in POOLS:
        for cap in CAPS:
            out[f"torch_over_kernel_{m}_cap_{cap}"] = med(f"torch_cap_lists_{m}_cap_{cap}") / med(f"cap_lists_{m}_cap_{cap}")
        out[f"cap_lists_{m}_over_retrieve_list_{m}"] = med(f"cap_lists_{m}_cap_1") / med(f"retrieve_list_grouped_{m}")
        out[f"capped_minus_pool_call_ms_{m}"] = med(f"recommend_capped_batch_{N_SHOWN}_of_{m}") - med(f"recommend_batch_{m}")
        out[f"capped_minus_pool_call_share_{m}"] = out[f"capped_minus_pool_call_ms_{m}"] / med(f"recommend_batch_{m}")
        out[f"pool_call_spread_{m}"] = (t[f"recommend_batch_{m}"]["max_ms"] - t[f"recommend_batch_{m}"]["min_ms"]) / \
            med(f"recommend_batch_{m}")
        out[f"list_mbytes_{m}"] = out["rows"] * m * 8 / 1e6
    for per_type in PER_TYPE:
        out[f"page_minus_lists_call_ms_{per_type}"] = (med(f"recommend_page_batch_{N_SHOWN}_of_3x{per_type}") -
                                                       med(f"recommend_batch_{per_type}"))
    # the answers at the timed size: kernel and torch agree bit for bit; no group is the pool's head; two runs agree
    agree = {}
    for m in POOLS:
        for cap in CAPS:
            a, b = ops.cap_lists(*pools[m], N_SHOWN, group, cap), torch_cap_lists(*pools[m], N_SHOWN, group, cap)
            agree[f"kernel_is_torch_{m}_cap_{cap}"] = same(a, b)
            assert agree[f"kernel_is_torch_{m}_cap_{cap}"], (name, m, cap)
            agree[f"two_runs_same_bits_{m}_cap_{cap}"] = same(a, ops.cap_lists(*pools[m], N_SHOWN, group, cap))
        agree[f"no_group_is_the_pools_head_{m}"] = same(ops.cap_lists(*pools[m], N_SHOWN),
                                                        (pools[m][0][:, :N_SHOWN], pools[m][1][:, :N_SHOWN]))
    out["agreement"] = agree
    if name in args.effect_legs.split(","):
        out["effect"] = {"generator": effect(inf, q, group)}
        arrays = variant_arrays(bpg, g, args.variant_noise, d)
        alt = served(DeviceBPG(arrays, T, d), arrays["features"], T, d, dev)
        out["effect"]["variants"] = effect(alt, q, group)
        # on the variant catalogue too, kernel and torch agree where the cap bites
        with torch.no_grad():
            _, p_idx, p_sc = alt.recommend_batch(q, POOLS[0])
        flat = (p_idx.reshape(-1, POOLS[0]), p_sc.reshape(-1, POOLS[0]))
        ok = same(ops.cap_lists(*flat, N_SHOWN, group, 1), torch_cap_lists(*flat, N_SHOWN, group, 1))
        assert ok, (name, "variants")
        out["effect"]["variants"]["kernel_is_torch_64_cap_1"] = ok
        out["effect"]["note"] = (f"lists of n = {N_SHOWN}; generator: the catalogue as generated, where id // {VARIANTS} joins "
                                 f"unrelated products; variants: every product has its group's first member's type and features "
                                 f"plus N(0, I) x {args.variant_noise}")
        del alt, arrays
    else:
        out["effect"] = "not measured"
    del inf, g, bpg, proj, types, fwd, pools
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="100k,10M")
    ap.add_argument("--effect-legs", default="100k")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--variant-noise", type=float, default=0.05)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cap_lists_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("cap_lists_probe: no GPU (nothing here is measured on the CPU)")
    dev = torch.device("cuda")
    res = {"probe": "cap_lists", "device": torch.cuda.get_device_name(0), "clock": "host clock between device synchronisations",
           "legs": {}}
    for name in [s for s in args.legs.split(",") if s]:
        res["legs"][name] = leg(name, args, dev)
    for name in LEGS:
        res["legs"].setdefault(name, "not measured")
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
