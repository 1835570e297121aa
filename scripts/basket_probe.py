"""Developer tool: what the basket fusion costs beside the retrieval of the lists it fuses and beside a plain-torch formulation
of the same contract (pc_fuse_lists; ops.fuse_lists; PCompanionInference.recommend_basket_batch).  On the SAME baskets, lists
and catalogue, alternating in one process, with B baskets of I = 4 and I = 16 items, K = 3 predicted types and per_item = 16
(pools of 192 and 768 slots), n = 10 shown, the co-view exclusions installed (set_exclusions()):

  recommend_batch(items, per_item)            the B I queries' lists: the retrieval the fusion sits on (model forward included)
  fuse_lists(pool -> n)                       the kernel alone on those lists, with the baskets as sources and the exclusion
                                              CSR; also without the CSR, and combine="max"
  torch_fuse_lists(pool -> n)                 the contract (sources banned, no CSR) in plain torch: a stable sort by id, a
                                              segmented sum (scatter_add_ over the segments), a stable sort by the sums.  Its
                                              sums run in no pinned order, so the probe asserts equal results on scores rounded
                                              to odd multiples of 1/128, whose sums are exact
  recommend_basket_batch(n, per_item)         end to end, beside recommend_batch for the same rows

  100 k / 100 types      generate_scaled_bpg, uploaded
  10 M / 100 types       generate_device_bpg

ms from the host clock between two device synchronisations: `--warmup` untimed rounds, then `--reps` rounds, each round one call
of every leg in turn; medians with min .. max.  Nothing here is a gate.  Writes profiles/basket_probe.json (or --out) and prints
the same JSON as one line.

  python scripts/basket_probe.py [--legs 100k,10M] [--batch 4096] [--warmup 3] [--reps 10] [--out FILE]
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

from cap_lists_probe import alternating_host
from diversify_probe import served

LEGS = {"100k": (100_000, 100, 128), "10M": (10_000_000, 100, 128)}
ITEMS = (4, 16)
PER_ITEM = 16
N_SHOWN = 10
NONE = 2 ** 31 - 1


def torch_fuse_lists(idx, score, n, combine, source, num_products):
    """ops.fuse_lists(idx, score, n, combine, source=source, num_products=num_products) in plain torch, nothing read back (the
    sums in scatter_add_'s order: equal to the kernel's where every partial sum is exact)."""
    b, s, w = idx.shape
    m = s * w
    live = (source >= 0) & (source < num_products)
    ok = (idx >= 0) & (idx < num_products) & torch.isfinite(score) & live[:, :, None]
    member = (idx[:, :, :, None] == torch.where(live, source, -1)[:, None, None, :]).any(3)
    ok &= ~member
    ids = torch.where(ok, idx, NONE).reshape(b, m)
    sc = torch.where(ok, score, 0.0).reshape(b, m)
    by_id = torch.argsort(ids, dim=1, stable=True)
    ids, sc = ids.gather(1, by_id), sc.gather(1, by_id)
    first = torch.ones_like(ids, dtype=torch.bool)
    first[:, 1:] = ids[:, 1:] != ids[:, :-1]
    seg = first.cumsum(1) - 1                                                     # the segment of a slot: one per product id
    real = ids != NONE
    if combine == "sum":
        fused = torch.zeros(b, m, device=idx.device).scatter_add_(1, seg, sc)
    else:
        fused = torch.full((b, m), float("-inf"), device=idx.device).scatter_reduce_(1, seg, sc, "amax", include_self=True)
    support = torch.zeros(b, m, dtype=torch.int32, device=idx.device).scatter_add_(1, seg, real.int())
    seg_id = torch.full((b, m), NONE, dtype=torch.int32, device=idx.device).scatter_(1, seg, ids)      # (ascending along a row)
    fused = torch.where(seg_id != NONE, fused, float("-inf"))
    by_f = torch.argsort(fused, dim=1, descending=True, stable=True)[:, :n]      # (stable: the product index ascending)
    out_i, out_s, out_c = seg_id.gather(1, by_f), fused.gather(1, by_f), support.gather(1, by_f)
    none = out_i == NONE
    return (torch.where(none, -1, out_i).contiguous(), torch.where(none, float("-inf"), out_s).contiguous(),
            torch.where(none, 0, out_c).contiguous())


def same(a, b):
    return bool(torch.equal(a[0], b[0]) and torch.equal(a[1].contiguous().view(torch.int32), b[1].contiguous().view(torch.int32))
                and torch.equal(a[2], b[2]))


def leg(name, args, dev):
    from p_companion_amd import ops
    from p_companion_amd.data import generate_device_bpg, generate_scaled_bpg
    P, T, d = LEGS[name]
    t0 = time.time()
    if P <= 1_000_000:
        bpg, src = generate_scaled_bpg(P, T, seed=0, dim=d), "generate_scaled_bpg (uploaded IntBPG)"
    else:
        bpg, src = generate_device_bpg(P, T, seed=0, dim=d, world=1, with_complementary=False), "generate_device_bpg"
    g = bpg.cuda(dev)
    torch.cuda.synchronize()
    out = {"source": src, "products": P, "types": T, "dim": d, "B": args.batch, "K": 3, "per_item": PER_ITEM, "n": N_SHOWN,
           "exclusions": "the co-view graph and the item itself (set_exclusions())", "generate_s": round(time.time() - t0, 2)}
    inf = served(bpg, g["features"], T, d, dev)
    inf.set_exclusions()
    ex = inf.exclusions
    out["exclusion_entries"] = int(ex[1].numel())
    fns, pools, baskets = {}, {}, {}
    for items in ITEMS:
        m = items * 3 * PER_ITEM
        basket = torch.from_numpy(np.random.default_rng(items).integers(0, P, (args.batch, items)).astype(np.int32)).to(dev)
        flat = basket.reshape(-1).contiguous()
        with torch.no_grad():
            _, idx, sc = inf.recommend_batch(flat, PER_ITEM)
        pools[m] = (idx.reshape(args.batch, items, -1).contiguous(), sc.reshape(args.batch, items, -1).contiguous())
        baskets[m] = basket
        fns[f"recommend_batch_{items}_items"] = (lambda flat=flat: inf.recommend_batch(flat, PER_ITEM))
        fns[f"fuse_lists_{m}"] = (lambda m=m: ops.fuse_lists(*pools[m], N_SHOWN, "sum", baskets[m], ex))
        fns[f"fuse_lists_{m}_max"] = (lambda m=m: ops.fuse_lists(*pools[m], N_SHOWN, "max", baskets[m], ex))
        fns[f"fuse_lists_{m}_no_exclusions"] = (lambda m=m: ops.fuse_lists(*pools[m], N_SHOWN, "sum", baskets[m], num_products=P))
        fns[f"torch_fuse_lists_{m}"] = (lambda m=m: torch_fuse_lists(*pools[m], N_SHOWN, "sum", baskets[m], P))
        fns[f"recommend_basket_batch_{items}_items"] = (lambda b=basket: inf.recommend_basket_batch(b, N_SHOWN, per_item=PER_ITEM))
    t = alternating_host(fns, args.warmup, args.reps)
    out.update(t)
    med = lambda k: t[k]["median_ms"]
    agree = {}
    for items in ITEMS:
        m = items * 3 * PER_ITEM
        out[f"rows_{items}_items"] = args.batch * items * 3
        out[f"torch_over_kernel_{m}"] = med(f"torch_fuse_lists_{m}") / med(f"fuse_lists_{m}_no_exclusions")
        out[f"fuse_lists_{m}_over_recommend_batch"] = med(f"fuse_lists_{m}") / med(f"recommend_batch_{items}_items")
        out[f"basket_minus_lists_call_ms_{items}_items"] = (med(f"recommend_basket_batch_{items}_items") -
                                                            med(f"recommend_batch_{items}_items"))
        out[f"basket_minus_lists_call_share_{items}_items"] = (out[f"basket_minus_lists_call_ms_{items}_items"] /
                                                               med(f"recommend_batch_{items}_items"))
        r = t[f"recommend_batch_{items}_items"]
        out[f"lists_call_spread_{items}_items"] = (r["max_ms"] - r["min_ms"]) / r["median_ms"]
        # the answers at the timed size: kernel and torch agree bit for bit on exactly summable scores; two runs agree
        # (odd multiples of 1/128: no zero among them, whose sign torch's zero-initialised sums do not keep)
        exact = (pools[m][0], ((torch.round(pools[m][1] * 64) + 0.5) / 64).contiguous())
        for combine in ("sum", "max"):
            a = ops.fuse_lists(*exact, N_SHOWN, combine, baskets[m], num_products=P)
            agree[f"kernel_is_torch_{m}_{combine}"] = same(a, torch_fuse_lists(*exact, N_SHOWN, combine, baskets[m], P))
            assert agree[f"kernel_is_torch_{m}_{combine}"], (name, m, combine)
            a = ops.fuse_lists(*pools[m], N_SHOWN, combine, baskets[m], ex)
            agree[f"two_runs_same_bits_{m}_{combine}"] = same(a, ops.fuse_lists(*pools[m], N_SHOWN, combine, baskets[m], ex))
        full = ops.fuse_lists(*pools[m], N_SHOWN, "sum", baskets[m], ex)
        out[f"share_of_served_products_with_support_above_1_{m}"] = float((full[2] > 1).sum()) / max(int((full[2] > 0).sum()), 1)
    out["agreement"] = agree
    del inf, g, bpg, pools, baskets, fns
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="100k,10M")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "basket_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("basket_probe: no GPU (nothing here is measured on the CPU)")
    dev = torch.device("cuda")
    res = {"probe": "basket", "device": torch.cuda.get_device_name(0), "clock": "host clock between device synchronisations",
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
