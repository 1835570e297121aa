"""Developer tool: what the cell index over the bf16 catalogue buys IndexedCompactSimilarProducts.similar_batch over the brute-force
CompactSimilarProducts(scope="catalogue").similar_batch, beside the fp32 index, and what it costs in recall and bytes.  On the SAME
queries, in the same process, on one MI355X (similar_index_probe.py's tables and clock):

  build       ops.build_cell_index (fp32 table) and then ops.build_cell_index_bf16 (the bf16 copy), seconds, one call each, and
              whether the two indexes have equal bits in every field
  serve       similar_batch at B = 4096, n = 10, alternating between
                brute_force            CompactSimilarProducts(scope="catalogue")            (yardstick)
                fp32_nprobe_K          IndexedSimilarProducts, K = 1, 4, 8, 16              (yardstick)
                nprobe_K               IndexedCompactSimilarProducts, K = 1, 4, 8, 16, 32, 64
                list64_nprobe_8        IndexedCompactSimilarProducts.similar_list_batch(64) at nprobe 8
  recall      recall@n at each nprobe, of both indexed classes (each relative to its own exact list)
  bytes       the tensors each serving object keeps resident (without the graph), and the bf16 build's peak above what was
              allocated on entry

  legs        100k: 100 000 products, 100 types, D = 128, 256 cells;   10M: 10 000 000 products, 4096 cells
  tables      "features":  generate_device_bpg's features as they are (unstructured: the worst case for any cell index)
              "clustered": one standard-normal centre per type times `--spread`, plus standard-normal noise

Host clock around a synchronised call, one untimed call of every leg first, median of `--reps`; every single time is kept
("ms_all").  One comparison is held: at 10M, nprobe 8, every indexed time is under every brute-force time (exit status 1
otherwise).  Everything else is reported as measured; recall is reported, never gated.  Prints ONE JSON line and, with --out,
writes it.

  python scripts/compact_index_probe.py [--legs 100k,10M] [--tables features,clustered] [--reps 5] [--out profiles/compact_index_probe.json]
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

from similar_index_probe import LEGS, clustered_table, timed

NPROBE = (1, 4, 8, 16, 32, 64)
NPROBE_FP32 = (1, 4, 8, 16)
FIELDS = ("centroids", "centroid_bias", "cell_of", "cell_rowptr", "cell_col")


def resident(obj):
    """{attribute: bytes} of the distinct device tensors a serving object keeps (its index and catalogue included, its graph not)."""
    from p_companion_amd import ops
    seen, out = set(), {}

    def walk(name, v):
        if torch.is_tensor(v):
            if v.is_cuda and v.untyped_storage().data_ptr() not in seen:
                seen.add(v.untyped_storage().data_ptr())
                out[name] = out.get(name, 0) + v.untyped_storage().nbytes()
        elif isinstance(v, (tuple, list)):
            for x in v:
                walk(name, x)
        elif isinstance(v, (ops.CellIndex, ops.CompactCatalogue)):
            for k, x in vars(v).items():
                walk(f"{name}.{k.lstrip('_')}", x)

    for k, v in vars(obj).items():
        if k not in ("bpg", "_graph"):
            walk(k.lstrip("_"), v)
    out["total"] = sum(out.values())
    return out


def build_timed(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    entry = torch.cuda.memory_allocated()
    t0 = time.perf_counter()
    index = fn()
    torch.cuda.synchronize()
    return index, round(time.perf_counter() - t0, 3), int(torch.cuda.max_memory_allocated() - entry)


def measure(table, bpg, cells, args, dev):
    from p_companion_amd import ops
    from p_companion_amd.inference import CompactSimilarProducts, IndexedCompactSimilarProducts, IndexedSimilarProducts
    P, d = table.shape
    cat = ops.CompactCatalogue(table)                                     # (rounded once here)
    cat.half_sq_norm
    index32, s32, peak32 = build_timed(lambda: ops.build_cell_index(table, cells, iters=args.iters, seed=0))
    index, s16, peak16 = build_timed(lambda: ops.build_cell_index_bf16(cat, cells, iters=args.iters, seed=0))
    wide = ops.build_cell_index(cat.table.float(), cells, iters=args.iters, seed=0) if P <= 1_000_000 else None
    out = {"n_cells": cells, "iters": args.iters,
           "build": {"fp32_s": s32, "bf16_s": s16, "fp32_peak_bytes_above_entry": peak32, "bf16_peak_bytes_above_entry": peak16,
                     "widened_table_bytes": P * d * 4, "order": "fp32 first, then bf16; one call each",
                     "bf16_equals_fp32_build_on_the_widened_table": (
                         None if wide is None else all(torch.equal(getattr(index, f), getattr(wide, f)) for f in FIELDS))}}
    del wide
    sizes = (index.cell_rowptr[1:] - index.cell_rowptr[:-1]).cpu().numpy()
    out["cells"] = {"largest": int(sizes.max()), "median": float(np.median(sizes)), "empty": int((sizes == 0).sum()),
                    "mean": float(sizes.mean())}
    q = torch.from_numpy(np.random.default_rng(1).integers(0, P, args.batch).astype(np.int32)).to(dev)
    exact = CompactSimilarProducts(cat, bpg, scope="catalogue")
    isp32 = IndexedSimilarProducts(table, bpg, index=index32, nprobe=8)
    isp = IndexedCompactSimilarProducts(cat, bpg, index=index, nprobe=8)
    probes = [k for k in NPROBE if k <= cells]
    fns = {"brute_force": lambda: exact.similar_batch(q, args.n)}
    for k in NPROBE_FP32:
        fns[f"fp32_nprobe_{k}"] = (lambda k: lambda: isp32.similar_batch(q, args.n, nprobe=k))(k)
    for k in probes:
        fns[f"nprobe_{k}"] = (lambda k: lambda: isp.similar_batch(q, args.n, nprobe=k))(k)
    fns["list64_nprobe_8"] = lambda: isp.similar_list_batch(q, 64, nprobe=8)
    t = timed(fns, args.reps)
    out["similar_batch"] = {"B": args.batch, "n": args.n, **t}
    out["recall"] = {**{f"nprobe_{k}": float(isp.recall(q, args.n, k)) for k in probes},
                     **{f"fp32_nprobe_{k}": float(isp32.recall(q, args.n, k)) for k in NPROBE_FP32}}
    brute = t["brute_force"]
    out["indexed_over_brute_force"] = {f"nprobe_{k}": t[f"nprobe_{k}"]["median_ms"] / brute["median_ms"] for k in probes}
    out["indexed_over_fp32_index"] = {f"nprobe_{k}": t[f"nprobe_{k}"]["median_ms"] / t[f"fp32_nprobe_{k}"]["median_ms"]
                                      for k in NPROBE_FP32}
    out["nprobe_8_under_brute_force"] = bool(t["nprobe_8"]["max_ms"] < brute["min_ms"])
    out["resident_bytes"] = {"IndexedCompactSimilarProducts": resident(isp), "IndexedSimilarProducts": resident(isp32),
                             "CompactSimilarProducts": resident(exact)}
    del exact, isp, isp32, index, index32, cat
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
            raise SystemExit(f"compact_index_probe: unknown table {which!r}")
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
        raise SystemExit("compact_index_probe: no GPU (nothing here is measured on the CPU)")
    dev = torch.device("cuda")
    res = {"probe": "compact_index", "device": torch.cuda.get_device_name(0), "legs": {},
           "not_measured": ["kernel times under a profiler (host clock only)", "D = 256", "batches other than --batch",
                            "set_eligible / custom exclusions on the serving legs", "the capped methods",
                            "the assignment's share of the build (DESIGN's figure is not re-measured)"]}
    for name in [s for s in args.legs.split(",") if s]:
        res["legs"][name] = leg(name, args, dev)
    held = [t["nprobe_8_under_brute_force"] for t in res["legs"].get("10M", {}).get("tables", {}).values()]
    res["held"] = {"10M_nprobe_8_every_time_under_every_brute_force_time": all(held) if held else None}
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    if held and not all(held):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
