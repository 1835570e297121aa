"""Developer tool: what the per-product term on the score costs, and what SimilarProducts serves in.  On the SAME rows, in the
same process, on one MI355X:

  retrieval   ops.retrieve_topk_grouped without bias (pc_retrieve_topk_grouped, the yardstick) beside bias=half_sq_norm_bias
              (pc_retrieve_topk_grouped_biased), alternating
  rank        ops.rank_grouped without and with the bias, alternating
  bias        ops.half_sq_norm_bias, once per catalogue
  similar     SimilarProducts.similar_batch at B = 4096, scope "type" and scope "catalogue"

  100 k / 100 types      generate_device_bpg
  10 M / 100 types       generate_device_bpg

12 288 rows (queries drawn from the catalogue, each against its own type, the query's table row as the projected embedding),
top n = 10.  Host clock around a synchronised call, one untimed call first, median of `--reps` = 3; every single time is kept
("ms_all") so that the biased leg can be read against the unbiased leg's own run-to-run spread.  By bytes the bias adds 4 B to
each 512 B candidate row.  Prints ONE JSON line and, with --out, writes it.

  python scripts/similar_products_probe.py [--legs 100k,10M] [--reps 3] [--out profiles/similar_products_probe.json]
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

LEGS = {"100k": (100_000, 100, 128), "10M": (10_000_000, 100, 128)}


def timed(fns, reps):
    """{name: {median_ms, min_ms, max_ms, ms_all}}: one untimed call of each first, then `reps` rounds alternating between them,
    the host clock around each synchronised call."""
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
    return {k: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)), "ms_all": [round(x, 4) for x in v]}
            for k, v in ms.items()}


def pair(t, plain, biased):
    """The two legs and how the biased one sits against the plain one's own spread."""
    a, b = t[plain], t[biased]
    return {"unbiased": a, "biased": b, "biased_over_unbiased": b["median_ms"] / a["median_ms"],
            "unbiased_spread_ms": a["max_ms"] - a["min_ms"],
            "biased_within_unbiased_spread": bool(a["min_ms"] <= b["median_ms"] <= a["max_ms"])}


def leg(name, args, dev):
    from p_companion_amd import ops
    from p_companion_amd.data import generate_device_bpg
    from p_companion_amd.inference import SimilarProducts
    P, T, d = LEGS[name]
    t0 = time.time()
    bpg = generate_device_bpg(P, T, seed=0, dim=d, world=1, with_complementary=False)
    g = bpg.cuda(dev)
    table = g["features"]
    torch.cuda.synchronize()
    out = {"source": "generate_device_bpg", "products": P, "types": T, "dim": d, "rows": args.rows, "n": args.n,
           "generate_s": round(time.time() - t0, 2)}
    rowptr, col = ops.type_csr(g["type_idx"], T)
    out["half_sq_norm_bias"] = timed({"bias": lambda: ops.half_sq_norm_bias(table)}, args.reps)["bias"]
    out["half_sq_norm_bias"]["table_gbytes"] = table.numel() * 4 / 1e9
    bias = ops.half_sq_norm_bias(table)
    rng = np.random.default_rng(1)
    q = torch.from_numpy(rng.integers(0, P, args.rows).astype(np.int32)).to(dev)
    y = torch.from_numpy(rng.integers(0, P, args.rows).astype(np.int32)).to(dev)
    proj = table[q.long()].contiguous()
    types = g["type_idx"][q.long()].contiguous()
    t = timed({"plain": lambda: ops.retrieve_topk_grouped(proj, types, rowptr, col, table, args.n),
               "biased": lambda: ops.retrieve_topk_grouped(proj, types, rowptr, col, table, args.n, bias=bias)}, args.reps)
    out["retrieval"] = pair(t, "plain", "biased")
    t = timed({"plain": lambda: ops.rank_grouped(proj, types, y, rowptr, col, table),
               "biased": lambda: ops.rank_grouped(proj, types, y, rowptr, col, table, bias=bias)}, args.reps)
    out["rank"] = pair(t, "plain", "biased")
    del proj, types, bias
    qb = q[:args.batch].contiguous()
    out["similar_batch"] = {"B": args.batch}
    for scope in ("type", "catalogue"):
        sp = SimilarProducts(table, bpg, scope=scope)
        out["similar_batch"][scope] = timed({scope: lambda: sp.similar_batch(qb, args.n)}, args.reps)[scope]
        del sp
        torch.cuda.empty_cache()
    del g, bpg, table, rowptr, col
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="100k,10M")
    ap.add_argument("--rows", type=int, default=12288)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("similar_products_probe: no GPU (nothing here is measured on the CPU)")
    dev = torch.device("cuda")
    res = {"probe": "similar_products", "device": torch.cuda.get_device_name(0), "legs": {}}
    for name in [s for s in args.legs.split(",") if s]:
        res["legs"][name] = leg(name, args, dev)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
