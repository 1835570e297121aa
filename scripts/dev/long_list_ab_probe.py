#!/usr/bin/env python3
"""Developer tool: the long-list entries' time for an A/B of two library builds (PC_DEV_LIB), one process per build and turn.
The list legs of scripts/compact_catalogue_probe.py and the same with exclusion lists, nothing else:

  retrieve_list_grouped(n), n = 16 / 64 / 128 / 256     over the fp32 table and over its bf16 copy
  the same with exclude=, n = 64 / 256                   row_key = arange(rows), a row's list = the 16 products the plain call
                                                         serves it first (scripts/long_list_probe.py's triple)

  100 k / 100 types (launch-bound: recorded)   10 M / 100 types at D = 128, and with --dims 128,256 the n = 64 / 256 legs at D = 256

Rows: B = 4096 queries x K = 3 predicted types from the model's forward: 12 288.  ms from device events, `--warmup` untimed
rounds, then `--reps` rounds, each round one call of every leg in turn; medians with min .. max.  Prints one JSON line and
writes it to --out.

  PC_DEV_LIB=PARENT.so python scripts/dev/long_list_ab_probe.py --out parent_1.json       (and CHILD.so, alternating)
  python scripts/dev/long_list_ab_probe.py --summary OUT.json --parent parent_*.json --child child_*.json

--summary: per leg the processes' medians, the gate (the child's median over its processes is not above the parent's largest
process median; the 100 k legs are not gated) and exit status 1 when a gated leg fails."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

LIST_NS = (16, 64, 128, 256)
EXCL_NS = (64, 256)


def leg(P, T, d, args, dev):
    from types import SimpleNamespace

    import numpy as np
    import torch
    from p_companion_amd import ops
    from p_companion_amd.data import generate_device_bpg
    from p_companion_amd.inference import PCompanionInference
    from p_companion_amd.p_companion import PCompanion
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from long_list_probe import alternating
    bpg = generate_device_bpg(P, T, seed=0, dim=d, world=1, with_complementary=False)
    g = bpg.cuda(dev)
    cfg = SimpleNamespace(PRODUCT_EMB_DIM=d, TYPE_EMB_DIM=64, HIDDEN_SIZE=256, NUM_ATTENTION_HEADS=4, DROPOUT=0.0,
                          MARGIN=1.0, ALPHA=0.8, NUM_COMP_TYPES=3, NUM_TYPES=T, DEVICE=dev)
    torch.manual_seed(0)
    inf = PCompanionInference(PCompanion(cfg, g["features"]), cfg, bpg)
    rowptr, col = inf.type_rowptr, inf.type_col
    tables = {"fp32": inf.features, "bf16": ops.catalogue_bf16(inf.features)}
    q = torch.from_numpy(np.random.default_rng(1).integers(0, P, args.batch).astype(np.int32)).to(dev)
    with torch.no_grad():
        fwd = inf.model({"query_idx": q, "query_types": inf.type_idx[q.long()]})
    proj = fwd["projected_embeddings"].contiguous().reshape(-1, d)
    types = fwd["complementary_types"].to(torch.int32).reshape(-1).contiguous()
    rows = int(types.numel())
    served = ops.retrieve_topk_grouped(proj, types, rowptr, col, tables["fp32"], 16)[0]
    rp = (torch.arange(rows + 1, device=dev) * 16).to(torch.int32)
    ex = (torch.arange(rows, dtype=torch.int32, device=dev),) + ops.exclusion_csr(rp, served.reshape(-1).contiguous(),
                                                                                 include_self=False, num_products=P)
    fns = {}
    for n in (LIST_NS if d == 128 else EXCL_NS):
        for name, t in tables.items():
            fns[f"list_{n}_{name}"] = (lambda n=n, t=t: ops.retrieve_list_grouped(proj, types, rowptr, col, t, n))
    for n in EXCL_NS:
        for name, t in tables.items():
            fns[f"list_{n}_{name}_excluding"] = (lambda n=n, t=t: ops.retrieve_list_grouped(proj, types, rowptr, col, t, n, exclude=ex))
    out = {"products": P, "types": T, "dim": d, "rows": rows, **alternating(fns, args.warmup, args.reps)}
    a = fns["list_256_bf16_excluding"]()                   # the answers at the timed size: for comparing the builds' outputs
    out["checksum_list_256_bf16_excluding"] = [int(a[0].long().sum()), int(a[1].view(torch.int32).long().sum())]
    del inf, g, bpg, tables, proj, types, fwd
    torch.cuda.empty_cache()
    return out


def summary(args):
    import numpy as np
    runs = {side: [json.load(open(f)) for f in files] for side, files in (("parent", args.parent), ("child", args.child))}
    res = {"what": "pc_retrieve_list_grouped / _bf16, the parent's and the child's library (PC_DEV_LIB) alternating as processes on "
                   "one device; ms per call, per leg the processes' medians",
           "gate": "the child's median over its processes is not above the parent's largest process median; legs at 100 k "
                   "products are launch-bound: recorded, not gated",
           "device": runs["child"][0]["device"], "processes": {k: len(v) for k, v in runs.items()}, "legs": {}}
    failed = []
    for name, first in runs["parent"][0]["legs"].items():
        res["legs"][name] = {k: first[k] for k in ("products", "types", "dim", "rows")}
        res["legs"][name]["checksums_equal"] = len({tuple(r["legs"][name]["checksum_list_256_bf16_excluding"])
                                                    for side in runs.values() for r in side}) == 1
        for k, v in first.items():
            if not isinstance(v, dict):
                continue
            med = {side: [r["legs"][name][k]["median_ms"] for r in runs[side]] for side in runs}
            e = {"parent_median_ms": med["parent"], "child_median_ms": med["child"],
                 "parent_min_max_ms": [min(r["legs"][name][k]["min_ms"] for r in runs["parent"]),
                                       max(r["legs"][name][k]["max_ms"] for r in runs["parent"])],
                 "child_min_max_ms": [min(r["legs"][name][k]["min_ms"] for r in runs["child"]),
                                      max(r["legs"][name][k]["max_ms"] for r in runs["child"])],
                 "child_over_parent": float(np.median(med["child"]) / np.median(med["parent"]))}
            if first["products"] > 1_000_000:
                e["passes"] = bool(np.median(med["child"]) <= max(med["parent"]))
                e["slower_in_every_process"] = bool(min(med["child"]) > max(med["parent"]))
                if not e["passes"]:
                    failed.append(f"{name}/{k}")
            res["legs"][name][k] = e
    res["failed"] = failed
    with open(args.summary, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)
    return 1 if failed else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dims", default="128")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out")
    ap.add_argument("--summary")
    ap.add_argument("--parent", nargs="+")
    ap.add_argument("--child", nargs="+")
    args = ap.parse_args()
    if args.summary:
        return summary(args)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("long_list_ab_probe: no GPU (nothing here is measured on the CPU)")
    dev = torch.device("cuda")
    from p_companion_amd import _lib
    res = {"probe": "long_list_ab", "device": torch.cuda.get_device_name(0), "library": _lib.LIB_PATH, "legs": {}}
    res["legs"]["100k_d128"] = leg(100_000, 100, 128, args, dev)
    for d in [int(s) for s in args.dims.split(",") if s]:
        res["legs"][f"10M_d{d}"] = leg(10_000_000, 100, d, args, dev)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
