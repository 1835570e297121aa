"""Developer tool: what a per-query attribute filter costs inside the long-list kernel (pc_retrieve_list_grouped_where and its
bf16 twin: a band on a per-product value, tested on chip between the threshold and the append) and what the work-around costs.
On the SAME rows and catalogue, alternating in one process, on one MI355X, for n = 10 / 64 / 256 and the fp32 and bf16 tables:

  retrieve_list_grouped(n)                       the unfiltered entry, the parent's code: THE YARDSTICK of the lines below
  retrieve_list_grouped_where(n), 100 / 50 / 1 % the new entry under per-row bands [u_r, u_r + width] on a value uniform in [0, 1)
                                                 (100 %: the band [0, 1]; every row has its own u_r)
  retrieve_list_grouped(256) + post-filter(n)    what a caller had to do before: fetch the longest list, gather the values of the
                                                 served ids in torch, keep the first n that pass; with the share of rows that
                                                 come back shorter than n (and the new entry's share beside it: rows whose type
                                                 holds fewer than n passing products are short for both)

  100 k / 100 types, 10 M / 100 types   generate_device_bpg; 12 288 rows: queries drawn from the catalogue, each against its own
                                        type, the query's table row as the projected embedding; D = 128

ms from device events: `--warmup` untimed rounds, then `--reps` rounds, each round one call of every leg in turn; medians with
min .. max.  The answers are compared at the timed size: the all-pass filter is the unfiltered entry bit for bit, every served
id passes its row's band, and where the work-around's row is full it is the new entry's row.  D = 256 and per-kernel times are
not measured here.  Writes profiles/where_probe.json (or --out) and prints the same JSON as one line.

  python scripts/where_probe.py [--legs 100k,10M] [--warmup 3] [--reps 10] [--out FILE]
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
NS = (10, 64, 256)
WIDTHS = {"100": 1.0, "50": 0.5, "1": 0.01}                              # the share of the catalogue a row's band passes


def same(a, b):
    return bool(torch.equal(a[0], b[0]) and torch.equal(a[1].contiguous().view(torch.int32), b[1].contiguous().view(torch.int32)))


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
    q = torch.from_numpy(np.random.default_rng(1).integers(0, P, args.rows).astype(np.int32)).to(dev)
    proj = g["features"][q.long()].contiguous()
    types = g["type_idx"][q.long()].contiguous()
    gen = torch.Generator(device=dev).manual_seed(5)
    value = torch.rand(P, generator=gen, device=dev)
    u = torch.rand(args.rows, generator=gen, device=dev)
    bands = {k: ((u * (1.0 - w)).contiguous(), (u * (1.0 - w) + w).contiguous()) for k, w in WIDTHS.items()}
    wheres = {k: ops.RowWhere(value=value, lo=lo, hi=hi) for k, (lo, hi) in bands.items()}

    def post_filter(table, n, lo, hi):
        idx, sc = ops.retrieve_list_grouped(proj, types, rowptr, col, table, 256)
        v = value[idx.clamp(min=0).long()]
        ok = (idx >= 0) & (v >= lo[:, None]) & (v <= hi[:, None])
        order = torch.sort((~ok).to(torch.int8), dim=1, stable=True).indices[:, :n]
        kept = ok.gather(1, order)
        return (torch.where(kept, idx.gather(1, order), torch.full_like(order, -1, dtype=torch.int32)),
                torch.where(kept, sc.gather(1, order), torch.full_like(order, float("-inf"), dtype=torch.float32)))

    for kind, table in (("fp32", g["features"]), ("bf16", ops.catalogue_bf16(g["features"]))):
        fns = {}
        for n in NS:
            fns[f"retrieve_list_grouped_{n}"] = (lambda n=n: ops.retrieve_list_grouped(proj, types, rowptr, col, table, n))
            for k in WIDTHS:
                fns[f"where_{k}pct_{n}"] = (lambda n=n, k=k: ops.retrieve_list_grouped_where(proj, types, rowptr, col, table, n,
                                                                                           wheres[k]))
                fns[f"list_256_post_filter_{k}pct_{n}"] = (lambda n=n, k=k: post_filter(table, n, *bands[k]))
        t = alternating(fns, args.warmup, args.reps)
        med = lambda key: t[key]["median_ms"]
        res = {**t, "where_over_unfiltered": {}, "post_filter_over_where": {}, "rows_shorter_than_n": {}, "agreement": {}}
        for n in NS:
            for k, (lo, hi) in bands.items():
                key = f"{k}pct_{n}"
                res["where_over_unfiltered"][key] = med(f"where_{key}") / med(f"retrieve_list_grouped_{n}")
                res["post_filter_over_where"][key] = med(f"list_256_post_filter_{key}") / med(f"where_{key}")
                got, work = fns[f"where_{key}"](), fns[f"list_256_post_filter_{key}"]()
                full = (work[0] >= 0).all(1)
                v = value[got[0].clamp(min=0).long()]
                res["rows_shorter_than_n"][key] = {"where": float(((got[0] >= 0).sum(1) < n).float().mean()),
                                                   "list_256_post_filter": float((~full).float().mean())}
                res["agreement"][key] = {
                    "every_served_id_passes": bool(((got[0] < 0) | ((v >= lo[:, None]) & (v <= hi[:, None]))).all()),
                    "full_post_filter_rows_are_the_where_rows": same((got[0][full], got[1][full]), (work[0][full], work[1][full]))}
            res["agreement"][f"all_pass_{n}_is_unfiltered_{n}"] = same(fns[f"where_100pct_{n}"](), fns[f"retrieve_list_grouped_{n}"]())
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "where_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("where_probe: no GPU (nothing here is measured on the CPU)")
    dev = torch.device("cuda")
    res = {"probe": "where", "device": torch.cuda.get_device_name(0),
           "timing": "device events; every round runs each leg of a group once, in turn; median (min .. max) in ms per call",
           "yardstick": "retrieve_list_grouped_N (the unfiltered entry) beside where_SHAREpct_N, same rows, table and process",
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
