"""Developer tool: what the score moments cost (pc_score_moments_grouped and its bf16 twin: the rank's plan, query tile, k-chain
and candidate stream with a subtraction, an addition and a fused multiply-add per (row, candidate) where the rank compares and
counts) and what normalise="zscore" does to a page.  On the SAME rows and catalogue, alternating in one process, on one MI355X:

  rank_grouped / rank_grouped_bf16          the rank entry, the parent's code: THE YARDSTICK of the line below
  score_moments_grouped                     the new entry, fp32 and bf16 table
  recommend_page_batch / recommend_basket_batch, with and without normalise="zscore", end to end (the model included)

  100 k / 100 types, 10 M / 100 types   12 288 rows: queries drawn from the catalogue, each against its own type, the query's
                                        table row as the projected embedding (the rank's target a random product of the type);
                                        D = 128.  The methods: 4096 queries x K = 3 slots = 12 288 rows, an untrained model
                                        whose product table is the feature tensor; page: 10 of 3 x 4; basket: 1024 x 4 items.

ms from device events (the entries) and from the host clock between two synchronisations (the methods): `--warmup` untimed
rounds, then `--reps` rounds, each round one call of every leg in turn; medians with min .. max.  Also recorded: the share of
the page's slots that each of the K type slots (the model's first, second, third predicted type) holds, with and without
normalise.  D = 256, per-kernel times and a trained model's hit@k on standardised pages are not measured here.  Writes
profiles/score_moments_probe.json (or --out) and prints the same JSON as one line.

  python scripts/score_moments_probe.py [--legs 100k,10M] [--warmup 3] [--reps 10] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from cap_lists_probe import alternating_host
from diversify_probe import served
from long_list_probe import alternating

LEGS = {"100k": (100_000, 100, 128), "10M": (10_000_000, 100, 128)}      # products, types, D
N_SHOWN, PER_TYPE, PER_ITEM, ITEMS = 10, 4, 8, 4


def slot_shares(inf, q, page):
    """the share of the page's filled slots that the query's first, second and third predicted type hold"""
    types = inf.recommend_batch(q, 1)[0]                                   # [B, K], the model's order
    held = page[2][:, :, None] == types[:, None, :]                        # [B, n, K]
    filled = float((page[0] >= 0).sum())
    return [float(held[:, :, k].sum()) / filled for k in range(types.shape[1])]


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
    out = {"source": src, "products": P, "types": T, "dim": d, "rows": args.rows, "generate_s": round(time.time() - t0, 2)}
    rowptr, col = ops.type_csr(g["type_idx"], T)
    rng = np.random.default_rng(1)
    q = torch.from_numpy(rng.integers(0, P, args.rows).astype(np.int32)).to(dev)
    proj = g["features"][q.long()].contiguous()
    types = g["type_idx"][q.long()].contiguous()
    lo_t, size = rowptr[types.long()].long(), (rowptr[types.long() + 1] - rowptr[types.long()]).long()
    pick = torch.from_numpy(rng.random(args.rows)).to(dev)
    targets = col[lo_t + (pick * size).long().clamp(max=size - 1)].contiguous()      # a random product of the row's type
    for kind, table, rank in (("fp32", g["features"], ops.rank_grouped), ("bf16", ops.catalogue_bf16(g["features"]),
                                                                          ops.rank_grouped_bf16)):
        fns = {"rank_grouped": (lambda: rank(proj, types, targets, rowptr, col, table)[0]),
               "score_moments_grouped": (lambda: ops.score_moments_grouped(proj, types, rowptr, col, table).mean)}
        t = alternating(fns, args.warmup, args.reps)
        m = ops.score_moments_grouped(proj, types, rowptr, col, table)
        ok = bool((m.count.long() == size).all() and torch.isfinite(m.mean).all() and (m.std > 0).all() and int(m.bad) == 0)
        assert ok, f"{name} {kind}: the moments are not those of the rows' types"
        out[kind] = {**t, "moments_over_rank": t["score_moments_grouped"]["median_ms"] / t["rank_grouped"]["median_ms"],
                     "counts_are_the_types_sizes": ok}
        del fns, table, m
        torch.cuda.empty_cache()
    # the methods, end to end: 4096 queries x K = 3 slots
    inf = served(bpg, g["features"], T, d, dev)
    b = args.rows // 3
    qq = q[:b].contiguous()
    basket = q[:(b // ITEMS) * ITEMS].reshape(-1, ITEMS).contiguous()
    fns = {}
    for key, kw in (("raw", {}), ("zscore", {"normalise": "zscore"})):
        fns[f"recommend_page_batch_{key}"] = (lambda kw=kw: inf.recommend_page_batch(qq, N_SHOWN, per_type=PER_TYPE, **kw))
        fns[f"recommend_basket_batch_{key}"] = (lambda kw=kw: inf.recommend_basket_batch(basket, N_SHOWN, per_item=PER_ITEM, **kw))
    t = alternating_host(fns, args.warmup, args.reps)
    med = lambda k: t[k]["median_ms"]
    out["methods"] = {**t, "queries": b, "baskets": int(basket.shape[0]), "items": ITEMS, "n": N_SHOWN, "per_type": PER_TYPE,
                      "per_item": PER_ITEM,
                      "page_zscore_over_raw": med("recommend_page_batch_zscore") / med("recommend_page_batch_raw"),
                      "basket_zscore_over_raw": med("recommend_basket_batch_zscore") / med("recommend_basket_batch_raw"),
                      "page_share_of_slots_per_type_slot": {key: slot_shares(inf, qq, fns[f"recommend_page_batch_{key}"]())
                                                            for key in ("raw", "zscore")}}
    del inf, g, bpg
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="100k,10M")
    ap.add_argument("--rows", type=int, default=12288)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_moments_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("score_moments_probe: no GPU (nothing here is measured on the CPU)")
    dev = torch.device("cuda")
    res = {"probe": "score_moments", "device": torch.cuda.get_device_name(0),
           "timing": "entries: device events; methods: host clock between two synchronisations; every round runs each leg of a "
                     "group once, in turn; median (min .. max) in ms per call",
           "yardstick": "rank_grouped (fp32) / rank_grouped_bf16 (bf16) beside score_moments_grouped: same rows, table and process",
           "not_measured": "D = 256; per-kernel times; a trained model's hit@k on standardised pages", "legs": {}}
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
