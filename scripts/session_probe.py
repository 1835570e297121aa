"""Developer tool: what the session fusion (pc_fuse_sessions; ops.fuse_sessions; PCompanionInference.recommend_session_batch)
costs beside the basket fusion it is modelled on, and what ragged sessions save over baskets padded to the longest session.
One process, every leg once per round in turn, on the SAME lists and catalogue, K = 3 predicted types, per_item = 16, n = 10
shown, the co-view exclusions installed (set_exclusions()):

  rectangular pools of 192 and 768 (B baskets of I = 4 and I = 16 items: basket_probe.py's pools)
    fuse_sessions(pool -> n)                  the new kernel, the baskets as sessions of I rows: sum with the CSR, max, sum
                                              without the CSR, and sum with a weight per row
    fuse_lists(pool -> n)                     the existing kernel on the same pool, the same three forms
    torch_fuse_lists(pool -> n)               basket_probe.py's plain-torch formulation (no CSR)
    asserted: fuse_sessions == fuse_lists bit for bit in every form; == the torch formulation on exactly summable scores
  ragged sessions (B sessions, lengths drawn from 1 .. 16 at a fixed seed)
    recommend_session_batch(n, per_item)      end to end over the R real items
    recommend_basket_batch(n, per_item)       end to end over the same sessions padded with -1 to 16 items
    recommend_batch(items, per_item)          the retrieval alone, over the R real items and over the B 16 padded ones
    fuse_sessions / fuse_lists                the fusions alone on those two pools
    asserted: equal ids, score bits, types and supports

  100 k / 100 types      generate_scaled_bpg, uploaded
  10 M / 100 types       generate_device_bpg

ms from the host clock between two device synchronisations: `--warmup` untimed rounds, then `--reps` rounds; medians with
min .. max.  Nothing here is a gate.  Writes profiles/session_probe.json (or --out) and prints the same JSON as one line.

  python scripts/session_probe.py [--legs 100k,10M] [--batch 4096] [--warmup 3] [--reps 10] [--out FILE]
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

from basket_probe import same, torch_fuse_lists
from cap_lists_probe import alternating_host
from diversify_probe import served

LEGS = {"100k": (100_000, 100, 128), "10M": (10_000_000, 100, 128)}
ITEMS = (4, 16)
PER_ITEM = 16
N_SHOWN = 10
LONGEST = 16


def leg(name, args, dev):
    from p_companion_amd import ops
    from p_companion_amd.data import generate_device_bpg, generate_scaled_bpg
    P, T, d = LEGS[name]
    B = args.batch
    t0 = time.time()
    if P <= 1_000_000:
        bpg, src = generate_scaled_bpg(P, T, seed=0, dim=d), "generate_scaled_bpg (uploaded IntBPG)"
    else:
        bpg, src = generate_device_bpg(P, T, seed=0, dim=d, world=1, with_complementary=False), "generate_device_bpg"
    g = bpg.cuda(dev)
    torch.cuda.synchronize()
    out = {"source": src, "products": P, "types": T, "dim": d, "B": B, "K": 3, "per_item": PER_ITEM, "n": N_SHOWN,
           "exclusions": "the co-view graph and the item itself (set_exclusions())", "generate_s": round(time.time() - t0, 2)}
    inf = served(bpg, g["features"], T, d, dev)
    inf.set_exclusions()
    ex = inf.exclusions
    fns, pools, baskets, flats, ptrs, weights = {}, {}, {}, {}, {}, {}
    # ---- rectangular pools: the two kernels and the torch formulation on the same pool
    for items in ITEMS:
        m = items * 3 * PER_ITEM
        basket = torch.from_numpy(np.random.default_rng(items).integers(0, P, (B, items)).astype(np.int32)).to(dev)
        flat = basket.reshape(-1).contiguous()
        with torch.no_grad():
            _, idx, sc = inf.recommend_batch(flat, PER_ITEM)
        pools[m] = (idx.reshape(B, items, -1).contiguous(), sc.reshape(B, items, -1).contiguous())
        baskets[m], flats[m] = basket, flat
        ptrs[m] = torch.arange(0, B * items + 1, items, dtype=torch.int32, device=dev)
        weights[m] = torch.pow(0.5, (items - 1 - torch.arange(B * items, device=dev) % items).float()).contiguous()
        rows = lambda m: (pools[m][0].reshape(-1, 3 * PER_ITEM), pools[m][1].reshape(-1, 3 * PER_ITEM))
        fns[f"fuse_sessions_{m}"] = (lambda m=m: ops.fuse_sessions(*rows(m), ptrs[m], N_SHOWN, "sum", flats[m], None, ex))
        fns[f"fuse_lists_{m}"] = (lambda m=m: ops.fuse_lists(*pools[m], N_SHOWN, "sum", baskets[m], ex))
        fns[f"fuse_sessions_{m}_max"] = (lambda m=m: ops.fuse_sessions(*rows(m), ptrs[m], N_SHOWN, "max", flats[m], None, ex))
        fns[f"fuse_lists_{m}_max"] = (lambda m=m: ops.fuse_lists(*pools[m], N_SHOWN, "max", baskets[m], ex))
        fns[f"fuse_sessions_{m}_no_exclusions"] = (lambda m=m: ops.fuse_sessions(*rows(m), ptrs[m], N_SHOWN, "sum", flats[m],
                                                                                 num_products=P))
        fns[f"fuse_lists_{m}_no_exclusions"] = (lambda m=m: ops.fuse_lists(*pools[m], N_SHOWN, "sum", baskets[m], num_products=P))
        fns[f"fuse_sessions_{m}_weighted"] = (lambda m=m: ops.fuse_sessions(*rows(m), ptrs[m], N_SHOWN, "sum", flats[m],
                                                                            weights[m], ex))
        fns[f"torch_fuse_lists_{m}"] = (lambda m=m: torch_fuse_lists(*pools[m], N_SHOWN, "sum", baskets[m], P))
    # ---- ragged sessions: lengths 1 .. 16 at a fixed seed, beside the same sessions padded to 16
    lengths = np.random.default_rng(2024).integers(1, LONGEST + 1, B)
    ptr_h = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    R = int(ptr_h[-1])
    items_h = np.random.default_rng(2025).integers(0, P, R).astype(np.int32)
    padded_h = np.full((B, LONGEST), -1, np.int32)
    for b in range(B):
        padded_h[b, :lengths[b]] = items_h[ptr_h[b]:ptr_h[b + 1]]
    items_d, ptr_d, padded_d = (torch.from_numpy(a).to(dev) for a in (items_h, ptr_h, padded_h))
    padded_flat = padded_d.reshape(-1).clamp(0, P - 1).contiguous()
    with torch.no_grad():
        _, r_idx, r_sc = inf.recommend_batch(items_d, PER_ITEM)
        _, p_idx, p_sc = inf.recommend_batch(padded_flat, PER_ITEM)
    r_pool = (r_idx.reshape(R, -1).contiguous(), r_sc.reshape(R, -1).contiguous())
    p_pool = (p_idx.reshape(B, LONGEST, -1).contiguous(), p_sc.reshape(B, LONGEST, -1).contiguous())
    fns["recommend_session_batch_ragged"] = lambda: inf.recommend_session_batch(items_d, ptr_d, N_SHOWN, per_item=PER_ITEM)
    fns["recommend_basket_batch_padded"] = lambda: inf.recommend_basket_batch(padded_d, N_SHOWN, per_item=PER_ITEM)
    fns["recommend_batch_ragged_items"] = lambda: inf.recommend_batch(items_d, PER_ITEM)
    fns["recommend_batch_padded_items"] = lambda: inf.recommend_batch(padded_flat, PER_ITEM)
    fns["fuse_sessions_ragged"] = lambda: ops.fuse_sessions(*r_pool, ptr_d, N_SHOWN, "sum", items_d, None, ex)
    fns["fuse_lists_padded"] = lambda: ops.fuse_lists(*p_pool, N_SHOWN, "sum", padded_d, ex)
    t = alternating_host(fns, args.warmup, args.reps)
    out.update(t)
    med = lambda k: t[k]["median_ms"]
    agree = {}
    for items in ITEMS:
        m = items * 3 * PER_ITEM
        rows_m = (pools[m][0].reshape(-1, 3 * PER_ITEM), pools[m][1].reshape(-1, 3 * PER_ITEM))
        for form in ("", "_max", "_no_exclusions"):
            out[f"fuse_lists_over_fuse_sessions_{m}{form}"] = med(f"fuse_lists_{m}{form}") / med(f"fuse_sessions_{m}{form}")
        out[f"torch_over_fuse_sessions_{m}"] = med(f"torch_fuse_lists_{m}") / med(f"fuse_sessions_{m}_no_exclusions")
        for combine in ("sum", "max"):
            for label, exclude in (("", ex), ("_no_exclusions", None)):
                a = ops.fuse_sessions(*rows_m, ptrs[m], N_SHOWN, combine, flats[m], None, exclude, num_products=P)
                b = ops.fuse_lists(*pools[m], N_SHOWN, combine, baskets[m], exclude, num_products=P)
                agree[f"sessions_is_lists_{m}_{combine}{label}"] = same(a, b)
                assert agree[f"sessions_is_lists_{m}_{combine}{label}"], (name, m, combine, label)
            # (odd multiples of 1/128: exactly summable, and no zero among them -- basket_probe.py)
            exact = ((torch.round(pools[m][1] * 64) + 0.5) / 64).contiguous()
            a = ops.fuse_sessions(rows_m[0], exact.reshape(-1, 3 * PER_ITEM), ptrs[m], N_SHOWN, combine, flats[m], num_products=P)
            agree[f"sessions_is_torch_{m}_{combine}"] = same(a, torch_fuse_lists(pools[m][0], exact, N_SHOWN, combine, baskets[m], P))
            assert agree[f"sessions_is_torch_{m}_{combine}"], (name, m, combine)
        a = ops.fuse_sessions(*rows_m, ptrs[m], N_SHOWN, "sum", flats[m], weights[m], ex)
        b = ops.fuse_lists(pools[m][0], (weights[m].reshape(B, items, 1) * pools[m][1]).contiguous(), N_SHOWN, "sum", baskets[m], ex)
        agree[f"weighted_sessions_is_lists_over_scaled_scores_{m}"] = same(a, b)
        assert agree[f"weighted_sessions_is_lists_over_scaled_scores_{m}"], (name, m)
    got, want = fns["recommend_session_batch_ragged"](), fns["recommend_basket_batch_padded"]()
    agree["ragged_sessions_are_padded_baskets"] = bool(same((got[0], got[1], got[3]), (want[0], want[1], want[3])) and
                                                       torch.equal(got[2], want[2]))
    assert agree["ragged_sessions_are_padded_baskets"], name
    out["agreement"] = agree
    out["ragged"] = {"sessions": B, "lengths": f"integers 1 .. {LONGEST}, numpy default_rng(2024)", "items": R,
                     "padded_items": B * LONGEST, "items_over_padded_items": R / (B * LONGEST),
                     "retrieval_rows": R * 3, "padded_retrieval_rows": B * LONGEST * 3}
    out["ragged_over_padded_end_to_end"] = med("recommend_session_batch_ragged") / med("recommend_basket_batch_padded")
    out["ragged_over_padded_retrieval"] = med("recommend_batch_ragged_items") / med("recommend_batch_padded_items")
    out["padded_minus_ragged_end_to_end_ms"] = med("recommend_basket_batch_padded") - med("recommend_session_batch_ragged")
    del inf, g, bpg, pools, baskets, fns, r_pool, p_pool
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="100k,10M")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "session_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("session_probe: no GPU (nothing here is measured on the CPU)")
    dev = torch.device("cuda")
    res = {"probe": "session", "device": torch.cuda.get_device_name(0), "clock": "host clock between device synchronisations",
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
