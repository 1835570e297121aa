"""Developer tool: what the per-row exclusion lists cost.  On the SAME rows, proj and catalogue, alternating in one process:

  retrieve_topk_grouped(n = 10)       without / with the co-view exclusion set (pc_retrieve_topk_grouped_excluding)
  rank_grouped                        without / with it (pc_rank_grouped_excluding: rk_rank_kernel + the post-pass)
  exclusion_csr                       the set itself (once per catalogue, off the serving path)

  100 k / 100 types      generate_scaled_bpg, uploaded
  10 M / 100 types       generate_device_bpg

Rows: B queries x K = 3 predicted types from the model's forward (as retrieval_probe.py); the row key is the query id, the set
ops.exclusion_csr(cv_rowptr, cv_col) with the query itself; each row's target is a product of its type drawn through the type
CSR.  ms from device events: `--warmup` untimed rounds, then `--reps` rounds, each round one call of every leg in turn; medians,
minima and the unfiltered legs' own round-to-round spread (max - min), beside which the filtered legs' excess is to be read.
The answers are compared at the timed size: no served id is in its row's list; rank < n exactly where the filtered list holds
the target.  Writes profiles/filtered_retrieval_probe.json (or --out) and prints the same JSON as one line.

  python scripts/filtered_retrieval_probe.py [--legs 100k,10M] [--warmup 3] [--reps 10] [--out FILE]
Per-kernel times: the same command under rocprofv3 --kernel-trace --stats in a run of its own (e.g. --legs 10M --reps 3).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from types import SimpleNamespace

import numpy as np
import torch

LEGS = {"100k": (100_000, 100, 128), "10M": (10_000_000, 100, 128)}
N_LIST = 10


def alternating(fns, warmup, reps):
    """{name: {median_ms, min_ms, max_ms, reps}}: every round runs each function once, in turn, between device events."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)), "reps": reps}
            for k, v in ms.items()}


def leg(name, args, dev):
    from p_companion_amd import ops
    from p_companion_amd.data import generate_device_bpg, generate_scaled_bpg
    from p_companion_amd.inference import PCompanionInference
    from p_companion_amd.p_companion import PCompanion
    P, T, d = LEGS[name]
    t0 = time.time()
    if P <= 1_000_000:
        bpg, src = generate_scaled_bpg(P, T, seed=0, dim=d), "generate_scaled_bpg (uploaded IntBPG)"
    else:
        bpg, src = generate_device_bpg(P, T, seed=0, dim=d, world=1, with_complementary=False), "generate_device_bpg"
    g = bpg.cuda(dev)
    torch.cuda.synchronize()
    out = {"source": src, "products": P, "types": T, "dim": d, "B": args.batch, "K": 3, "n": N_LIST,
           "generate_s": round(time.time() - t0, 2)}
    cfg = SimpleNamespace(PRODUCT_EMB_DIM=d, TYPE_EMB_DIM=64, HIDDEN_SIZE=256, NUM_ATTENTION_HEADS=4, DROPOUT=0.0,
                          MARGIN=1.0, ALPHA=0.8, NUM_COMP_TYPES=3, NUM_TYPES=T, DEVICE=dev)
    torch.manual_seed(0)
    model = PCompanion(cfg, g["features"])            # the product table IS the feature tensor (no second copy)
    inf = PCompanionInference(model, cfg, bpg)
    rowptr, col, table = inf.type_rowptr, inf.type_col, inf.features
    q = torch.from_numpy(np.random.default_rng(1).integers(0, P, args.batch).astype(np.int32)).to(dev)
    with torch.no_grad():
        fwd = inf.model({"query_idx": q, "query_types": inf.type_idx[q.long()]})
    proj = fwd["projected_embeddings"].contiguous().reshape(-1, d)
    types = fwd["complementary_types"].to(torch.int32).reshape(-1).contiguous()
    key = q.repeat_interleave(3).contiguous()
    cnt = (rowptr[1:] - rowptr[:-1]).long()[types.long()]
    u = torch.rand(types.numel(), generator=torch.Generator(device=dev).manual_seed(2), device=dev)
    pos = rowptr[types.long()].long() + (u * cnt).long().clamp(max=(cnt - 1).clamp(min=0))
    targets = torch.where(cnt > 0, col[pos.clamp(max=col.numel() - 1)], torch.zeros_like(types)).contiguous()
    csr_fn = lambda: ops.exclusion_csr(g["cv_rowptr"], g["cv_col"], include_self=True, num_products=P)
    ex = csr_fn()
    exclude = (key,) + ex
    out["rows"] = int(types.numel())
    out["exclusion_set"] = {"entries": int(ex[1].numel()), "mean_list": float(ex[1].numel()) / P,
                            "longest_list": int((ex[0][1:] - ex[0][:-1]).max())}
    fns = {"retrieve_topk_grouped": lambda: ops.retrieve_topk_grouped(proj, types, rowptr, col, table, N_LIST),
           "retrieve_topk_grouped_excluding": lambda: ops.retrieve_topk_grouped(proj, types, rowptr, col, table, N_LIST, exclude=exclude),
           "rank_grouped": lambda: ops.rank_grouped(proj, types, targets, rowptr, col, table),
           "rank_grouped_excluding": lambda: ops.rank_grouped(proj, types, targets, rowptr, col, table, exclude=exclude,
                                                              cand_type=inf.type_idx),
           "exclusion_csr": csr_fn}
    t = alternating(fns, args.warmup, args.reps)
    out.update(t)
    for plain in ("retrieve_topk_grouped", "rank_grouped"):
        out[plain + "_excluding"]["excess_over_unfiltered_ms"] = t[plain + "_excluding"]["median_ms"] - t[plain]["median_ms"]
        out[plain + "_excluding"]["unfiltered_spread_ms"] = t[plain]["max_ms"] - t[plain]["min_ms"]
    # the answers at the timed size
    idx, _ = fns["retrieve_topk_grouped_excluding"]()
    idx0, _ = fns["retrieve_topk_grouped"]()
    rank, bad = fns["rank_grouped_excluding"]()
    lo, hi = ex[0][key.long()].long(), ex[0][key.long() + 1].long()
    served_excluded = 0
    for j in range(N_LIST):                            # a bisection per served id, as vector operations
        y = idx[:, j].long()
        a, b = lo.clone(), hi.clone()
        for _ in range(int(ex[1].numel()).bit_length()):
            mid = (a + b) >> 1
            below = (a < b) & (ex[1][mid.clamp(max=ex[1].numel() - 1)].long() < y)
            a, b = torch.where(below, mid + 1, a), torch.where(below | (a >= b), b, mid)
        served_excluded += int(((a < hi) & (ex[1][a.clamp(max=ex[1].numel() - 1)].long() == y) & (y >= 0)).sum())
    inside = (rank >= 0) & (rank < N_LIST)
    at = idx.gather(1, rank.clamp(0, N_LIST - 1).long()[:, None]).reshape(-1)
    out["agreement"] = {"bad": int(bad), "served_ids_in_their_rows_list": served_excluded,
                        "rows_whose_list_changed": int((idx != idx0).any(1).sum()),
                        "targets_excluded": int(((rank < 0) & (cnt > 0)).sum()),
                        "targets_inside_the_list": int(inside.sum()),
                        "list_holds_target_at_rank": bool((at[inside] == targets[inside]).all()),
                        "list_holds_no_other_target": bool(not (idx[~inside] == targets[~inside][:, None]).any())}
    del inf, model, g, bpg, proj, types, fwd, ex, exclude
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="100k,10M")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "filtered_retrieval_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("filtered_retrieval_probe: no GPU (nothing here is measured on the CPU)")
    dev = torch.device("cuda")
    res = {"probe": "filtered_retrieval", "device": torch.cuda.get_device_name(0), "legs": {}}
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
