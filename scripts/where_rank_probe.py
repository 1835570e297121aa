"""Developer tool: what a per-query attribute predicate costs inside the grouped rank (pc_rank_grouped_where and its bf16 twin:
a band on a per-product value, tested per (row, candidate) inside the count) and what the work-around costs.  On the SAME rows,
targets and catalogue, alternating in one process, on one MI355X, for the fp32 and the bf16 table:

  rank_grouped / rank_grouped_bf16               the unfiltered entry, the parent's code: THE YARDSTICK of the lines below
  rank_grouped_where, 100 / 50 / 1 %             the new entry under per-row bands [u_r (1 - w), u_r (1 - w) + w] on a value uniform
                                                 in [0, 1), as scripts/where_probe.py lays them out (100 %: the band [0, 1])
  retrieve_list_grouped_where(256) + search      the only work-around: fetch the 256 filtered products of every row and look the
                                                 target up in torch; with the share of rows it cannot rank (the target passes and
                                                 stands past 256)

  100 k / 100 types, 10 M / 100 types   generate_device_bpg; 12 288 rows: queries drawn from the catalogue, each against its own
                                        type, the query's table row as the projected embedding, the target a random product of
                                        that type; D = 128

ms from device events: `--warmup` untimed rounds, then `--reps` rounds, each round one call of every leg in turn; medians with
min .. max.  The answers are asserted at the timed size: the all-pass ranks are the unfiltered ranks, and every rank below 256
is the target's position in the filtered list (and no other row's list holds its target).  D = 256 and per-kernel times are not
measured here.  Writes profiles/where_rank_probe.json (or --out) and prints the same JSON as one line.

  python scripts/where_rank_probe.py [--legs 100k,10M] [--warmup 3] [--reps 10] [--out FILE]
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

from long_list_probe import alternating

LEGS = {"100k": (100_000, 100, 128), "10M": (10_000_000, 100, 128)}      # products, types, D
WIDTHS = {"100": 1.0, "50": 0.5, "1": 0.01}                              # the share of the catalogue a row's band passes
N = 256


def leg(name, args, dev):
    from p_companion_amd import ops
    from p_companion_amd.data import generate_device_bpg
    P, T, d = LEGS[name]
    t0 = time.time()
    bpg = generate_device_bpg(P, T, seed=0, dim=d, world=1, with_complementary=False)
    g = bpg.cuda(dev)
    torch.cuda.synchronize()
    out = {"source": "generate_device_bpg", "products": P, "types": T, "dim": d, "rows": args.rows,
           "generate_s": round(time.time() - t0, 2)}
    rowptr, col = ops.type_csr(g["type_idx"], T)
    rng = np.random.default_rng(1)
    q = torch.from_numpy(rng.integers(0, P, args.rows).astype(np.int32)).to(dev)
    proj = g["features"][q.long()].contiguous()
    types = g["type_idx"][q.long()].contiguous()
    lo_t, size = rowptr[types.long()].long(), (rowptr[types.long() + 1] - rowptr[types.long()]).long()
    pick = torch.from_numpy(rng.random(args.rows)).to(dev)
    targets = col[lo_t + (pick * size).long().clamp(max=size - 1)].contiguous()      # a random product of the row's type
    gen = torch.Generator(device=dev).manual_seed(5)
    value = torch.rand(P, generator=gen, device=dev)
    u = torch.rand(args.rows, generator=gen, device=dev)
    bands = {k: ((u * (1.0 - w)).contiguous(), (u * (1.0 - w) + w).contiguous()) for k, w in WIDTHS.items()}
    wheres = {k: ops.RowWhere(value=value, lo=lo, hi=hi) for k, (lo, hi) in bands.items()}

    def search(table, k):
        idx, _ = ops.retrieve_list_grouped_where(proj, types, rowptr, col, table, N, wheres[k])
        held = idx == targets[:, None]
        return torch.where(held.any(1), held.int().argmax(1), -1).to(torch.int32)

    for kind, table, plain in (("fp32", g["features"], ops.rank_grouped),
                               ("bf16", ops.catalogue_bf16(g["features"]), ops.rank_grouped_bf16)):
        fns = {"rank_grouped": (lambda: plain(proj, types, targets, rowptr, col, table)[0])}
        for k in WIDTHS:
            fns[f"rank_where_{k}pct"] = (lambda k=k: ops.rank_grouped_where(proj, types, targets, rowptr, col, table, wheres[k])[0])
            fns[f"list_256_search_{k}pct"] = (lambda k=k: search(table, k))
        t = alternating(fns, args.warmup, args.reps)
        med = lambda key: t[key]["median_ms"]
        res = {**t, "where_over_unfiltered": {}, "search_over_where": {}, "rows_the_search_cannot_rank": {}, "agreement": {}}
        unfiltered = fns["rank_grouped"]()
        for k, (lo, hi) in bands.items():
            rank, found = fns[f"rank_where_{k}pct"](), fns[f"list_256_search_{k}pct"]()
            res["where_over_unfiltered"][f"{k}pct"] = med(f"rank_where_{k}pct") / med("rank_grouped")
            res["search_over_where"][f"{k}pct"] = med(f"list_256_search_{k}pct") / med(f"rank_where_{k}pct")
            res["rows_the_search_cannot_rank"][f"{k}pct"] = float((rank >= N).float().mean())
            vy = value[targets.long()]
            passing = (lo <= vy) & (vy <= hi)
            below = (rank >= 0) & (rank < N)
            agree = bool(torch.equal(found[below], rank[below]) and (found[~below] == -1).all() and (rank[~passing] == -1).all()
                         and (rank[passing] >= 0).all())
            assert agree, f"{name} {kind} {k} %: a rank below {N} is not the target's position in the filtered list"
            res["agreement"][f"{k}pct_every_rank_below_{N}_is_the_lists_position"] = agree
            res["agreement"][f"{k}pct_targets_that_fail_their_band"] = float((~passing).float().mean())
        same = bool(torch.equal(fns["rank_where_100pct"](), unfiltered))
        assert same, f"{name} {kind}: the all-pass ranks are not the unfiltered ranks"
        res["agreement"]["all_pass_is_unfiltered"] = same
        out[kind] = res
        del fns, table
        torch.cuda.empty_cache()
    del g, bpg
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="100k,10M")
    ap.add_argument("--rows", type=int, default=12288)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "where_rank_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("where_rank_probe: no GPU (nothing here is measured on the CPU)")
    dev = torch.device("cuda")
    res = {"probe": "where_rank", "device": torch.cuda.get_device_name(0),
           "timing": "device events; every round runs each leg of a group once, in turn; median (min .. max) in ms per call",
           "yardstick": "rank_grouped (fp32) / rank_grouped_bf16 (bf16), the unfiltered entry, beside rank_where_SHAREpct: same "
                        "rows, targets, table and process",
           "filter": "value uniform in [0, 1); row r passes [u_r (1 - w), u_r (1 - w) + w], w = 1 / 0.5 / 0.01",
           "not_measured": "D = 256; per-kernel times", "legs": {}}
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
