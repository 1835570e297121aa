"""Developer tool: ms per ops.rank_grouped (the rank of one known product per row among all products of its type) against
ops.retrieve_topk_grouped(n = 10) -- the kernel whose schedule it shares and whose score bits it reproduces -- on the SAME rows,
proj and catalogue, alternating in one process; and the wall time of one PCompanionInference.evaluate_catalogue over the test
split.  Writes profiles/catalogue_rank_probe.json (or --out) and prints the same JSON as one line.

  100 k / 100 types      generate_scaled_bpg, uploaded
  10 M / 100 types       generate_device_bpg; with the complementary pairs, so that evaluate_catalogue runs over its test split
  10 M / 34 800 types    about 290 candidates and one row per type
  100 M x 256 / 100      with --big only; otherwise recorded as not measured

Rows: B queries x K = 3 predicted types from the model's forward (as retrieval_probe.py); each row's target is a product of
its type drawn through the type CSR.  ms from device events: `--warmup` untimed rounds, then `--reps` rounds, each round one
call of either kernel in turn; medians and minima.  FLOPs = 2 D sum_r count(type r) (one dot product per (row, candidate); the
rank kernel's D extra per row for the target is not counted); share of peak = FLOPs / 157.3 TFLOP/s (fp32 MFMA) over the
median.  The two kernels' answers are compared at the timed size: rank < 10 exactly where the list holds the target, there.

  python scripts/catalogue_rank_probe.py [--legs 100k,10M,10M34800] [--big] [--warmup 3] [--reps 10] [--out FILE]
Per-kernel times: the same command under rocprofv3 --kernel-trace --stats in a run of its own (e.g. --legs 10M --reps 3 --no-eval).
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

PEAK_FP32 = 157.3e12
LEGS = {"100k": (100_000, 100, 128), "10M": (10_000_000, 100, 128), "10M34800": (10_000_000, 34_800, 128),
        "100M256": (100_000_000, 100, 256)}
N_LIST = 10


def alternating(fns, warmup, reps):
    """{name: {median_ms, min_ms, reps}}: every round runs each function once, in turn, between device events."""
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
    return {k: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "reps": reps} for k, v in ms.items()}


def flops(types, rowptr, d):
    cnt = (rowptr[1:] - rowptr[:-1]).long()
    return 2.0 * d * float(cnt[types.long()].sum())


def leg(name, args, dev):
    from p_companion_amd import ops
    from p_companion_amd.data import ComplementaryIndexDataset, generate_device_bpg, generate_scaled_bpg
    from p_companion_amd.inference import PCompanionInference
    from p_companion_amd.p_companion import PCompanion
    P, T, d = LEGS[name]
    with_eval = name == "10M" and not args.no_eval
    t0 = time.time()
    if P <= 1_000_000:
        bpg, src = generate_scaled_bpg(P, T, seed=0, dim=d), "generate_scaled_bpg (uploaded IntBPG)"
    else:
        bpg, src = generate_device_bpg(P, T, seed=0, dim=d, world=1, with_complementary=with_eval), "generate_device_bpg"
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
    # a target inside each row's type (a row whose type has no product keeps product 0: the count is then over nothing)
    cnt = (rowptr[1:] - rowptr[:-1]).long()[types.long()]
    u = torch.rand(types.numel(), generator=torch.Generator(device=dev).manual_seed(2), device=dev)
    pos = rowptr[types.long()].long() + (u * cnt).long().clamp(max=(cnt - 1).clamp(min=0))
    targets = torch.where(cnt > 0, col[pos.clamp(max=col.numel() - 1)], torch.zeros_like(types)).contiguous()
    out["rows"] = int(types.numel())
    rank_fn = lambda: ops.rank_grouped(proj, types, targets, rowptr, col, table)
    list_fn = lambda: ops.retrieve_topk_grouped(proj, types, rowptr, col, table, N_LIST)
    t = alternating({"rank_grouped": rank_fn, "retrieve_topk_grouped": list_fn}, args.warmup, args.reps)
    fl = flops(types, rowptr, d)
    for k in t:
        s = t[k]["median_ms"] * 1e-3
        t[k].update({"gflop": fl / 1e9, "tflops": fl / s / 1e12, "share_of_fp32_mfma_peak": fl / PEAK_FP32 / s})
    out.update(t)
    out["rank_over_retrieval"] = t["rank_grouped"]["median_ms"] / t["retrieve_topk_grouped"]["median_ms"]
    # the same answers at the timed size
    rank, bad = rank_fn()
    idx, _ = list_fn()
    inside = (rank >= 0) & (rank < N_LIST) & (cnt > 0)
    at = idx.gather(1, rank.clamp(0, N_LIST - 1).long()[:, None]).reshape(-1)
    out["agreement"] = {"bad": int(bad), "targets_inside_the_list": int(inside.sum()),
                        "list_holds_target_at_rank": bool((at[inside] == targets[inside]).all()),
                        "list_holds_no_other_target": bool(not (idx[~inside] == targets[~inside][:, None]).any())}
    if with_eval:
        ds = ComplementaryIndexDataset(bpg, "test")
        inf.evaluate_catalogue(ds, chunk=args.chunk)              # warm-up: every shape of the timed call
        torch.cuda.synchronize()
        t0 = time.time()
        metrics = inf.evaluate_catalogue(ds, chunk=args.chunk)     # (ends in its one read-back)
        out["evaluate_catalogue"] = {"wall_s": round(time.time() - t0, 3), "labelled_pairs_in_split": len(ds), "chunk": args.chunk,
                                     "model": "untrained (its initialiser): a timing, not a quality figure", "metrics": metrics}
    del inf, model, g, bpg, proj, types, fwd
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="100k,10M,10M34800")
    ap.add_argument("--big", action="store_true", help="add the 100 M x 256 / 100-type leg")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--chunk", type=int, default=65536)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-eval", action="store_true", help="skip evaluate_catalogue over the 10 M test split")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "catalogue_rank_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("catalogue_rank_probe: no GPU (nothing here is measured on the CPU)")
    dev = torch.device("cuda")
    legs = [s for s in args.legs.split(",") if s] + (["100M256"] if args.big else [])
    res = {"probe": "catalogue_rank", "device": torch.cuda.get_device_name(0), "legs": {}}
    for name in legs:
        res["legs"][name] = leg(name, args, dev)
    if "100M256" not in legs:
        res["legs"]["100M256"] = "not measured"
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
