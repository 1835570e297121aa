"""Developer tool: what the k-means cell index buys IndexedSimilarProducts.similar_batch over the brute-force
SimilarProducts(scope="catalogue").similar_batch, and what it costs in recall.  On the SAME queries, in the same process, on one
MI355X:

  build       ops.build_cell_index (Lloyd iterations on the device), seconds
  cells       the largest, median and empty cell counts of the index
  serve       similar_batch at B = 4096, n = 10: the brute-force leg and the indexed call at nprobe 1, 4, 8, 16, alternating
  recall      IndexedSimilarProducts.recall at each nprobe: the share of the exact lists' ids the indexed lists hold

  legs        100k: 100 000 products, 100 types, D = 128, 256 cells;   10M: 10 000 000 products, 4096 cells
  tables      "features":  generate_device_bpg's features as they are (unstructured: the worst case for any cell index)
              "clustered": made here -- one standard-normal centre per type times `--spread`, plus standard-normal noise

Host clock around a synchronised call, one untimed call of every leg first, median of `--reps`; every single time is kept
("ms_all").  Recall is reported, never gated.  Prints ONE JSON line and, with --out, writes it.

  python scripts/similar_index_probe.py [--legs 100k,10M] [--tables features,clustered] [--reps 5] [--out profiles/similar_index_probe.json]
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

LEGS = {"100k": (100_000, 100, 128, 256), "10M": (10_000_000, 100, 128, 4096)}
NPROBE = (1, 4, 8, 16)


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


def clustered_table(type_idx, n_types, dim, spread, seed):
    """One centre per type plus noise, on the device: centre_t = spread * N(0, I), row = centre_type + N(0, I)."""
    gen = torch.Generator(device=type_idx.device)
    gen.manual_seed(seed)
    centres = torch.randn(n_types, dim, device=type_idx.device, generator=gen) * spread
    table = torch.randn(type_idx.shape[0], dim, device=type_idx.device, generator=gen)
    table += centres[type_idx.long()]
    return table.contiguous()


def measure(table, bpg, cells, args, dev):
    from p_companion_amd import ops
    from p_companion_amd.inference import IndexedSimilarProducts, SimilarProducts
    P = table.shape[0]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    index = ops.build_cell_index(table, cells, iters=args.iters, seed=0)
    torch.cuda.synchronize()
    out = {"n_cells": cells, "iters": args.iters, "build_s": round(time.perf_counter() - t0, 3)}
    sizes = (index.cell_rowptr[1:] - index.cell_rowptr[:-1]).cpu().numpy()
    out["cells"] = {"largest": int(sizes.max()), "median": float(np.median(sizes)), "empty": int((sizes == 0).sum()),
                    "mean": float(sizes.mean())}
    q = torch.from_numpy(np.random.default_rng(1).integers(0, P, args.batch).astype(np.int32)).to(dev)
    exact = SimilarProducts(table, bpg, scope="catalogue")
    isp = IndexedSimilarProducts(table, bpg, index=index, nprobe=8)
    fns = {"brute_force": lambda: exact.similar_batch(q, args.n)}
    for k in NPROBE:
        fns[f"nprobe_{k}"] = (lambda k: lambda: isp.similar_batch(q, args.n, nprobe=k))(k)
    t = timed(fns, args.reps)
    out["similar_batch"] = {"B": args.batch, "n": args.n, **t}
    out["recall"] = {f"nprobe_{k}": float(isp.recall(q, args.n, k)) for k in NPROBE}
    brute = t["brute_force"]
    out["indexed_over_brute_force"] = {f"nprobe_{k}": t[f"nprobe_{k}"]["median_ms"] / brute["median_ms"] for k in NPROBE}
    out["nprobe_8_under_brute_force"] = bool(t["nprobe_8"]["max_ms"] < brute["min_ms"])
    del exact, isp, index
    torch.cuda.empty_cache()
    return out


def leg(name, args, dev):
    from p_companion_amd.data import generate_device_bpg
    P, T, d, cells = LEGS[name]
    bpg = generate_device_bpg(P, T, seed=0, dim=d, world=1, with_complementary=False)
    g = bpg.cuda(dev)
    out = {"products": P, "types": T, "dim": d, "tables": {}}
    for which in [s for s in args.tables.split(",") if s]:
        if which == "features":
            table = g["features"]
        elif which == "clustered":
            table = clustered_table(g["type_idx"], T, d, args.spread, seed=7)
        else:
            raise SystemExit(f"similar_index_probe: unknown table {which!r}")
        res = measure(table, bpg, cells, args, dev)
        res["table"] = ("generate_device_bpg features as they are" if which == "features" else
                        f"clustered: one N(0, I) centre per type x {args.spread} + N(0, I) noise")
        out["tables"][which] = res
        del table
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="100k,10M")
    ap.add_argument("--tables", default="features,clustered")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--spread", type=float, default=2.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("similar_index_probe: no GPU (nothing here is measured on the CPU)")
    dev = torch.device("cuda")
    res = {"probe": "similar_index", "device": torch.cuda.get_device_name(0), "legs": {}}
    for name in [s for s in args.legs.split(",") if s]:
        res["legs"][name] = leg(name, args, dev)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
