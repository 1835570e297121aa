"""Developer tool: joint P-Companion training over a device-resident catalogue (a DeviceBPG) on one MI355X.  Writes
profiles/catalogue_joint_probe.json (and prints it as one JSON line).

  split        ops.comp_split_pairs (pc_comp_split_pairs) of the train / val modes at 10 M products
  steps        ms per joint step, B = 4096, K = 3, through GraphedJointStep.run_epoch(max_steps=S) over
                 a DeviceBPG at 100 k and 10 M products                     (legs dev100k_*, dev10M_*)
                 an IntBPG from generate_scaled_bpg at 100 k, uploaded      (legs host100k_*)
               at T = 100 and T = 34 800 types.  The product table is a Product2Vec export of the catalogue (a second
               [P,128] array beside the features: 5.1 GB each at 10 M).  The loader's per-epoch shuffle is timed on its own
               (epoch_pairs_ms); the timed runs reuse one shuffled order, so steps_ms is the steps alone.
  evaluate     Metrics.evaluate_model over the 10 M val split of every 10 M leg: the existing per-batch loop (fused=False) and the
               one-call form (pc_joint_eval_epoch) alternating in one process, a host clock around calls that end in a
               synchronise, each once untimed first; --kernel-stats CSV merges the count kernel's traced time afterwards

ms from device events around `--reps` calls after one untimed call (median and min).

  python scripts/catalogue_joint_probe.py [--legs dev100k_100,dev100k_34800,host100k_100,host100k_34800,dev10M_100,dev10M_34800]
                                          [--steps 200] [--reps 5] [--loop-reps 2] [--no-evaluate]
  python scripts/catalogue_joint_probe.py --kernel-stats profiles/eval_10M_kernel_stats.csv      (no GPU: merge a trace)
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

LEGS = {"dev100k_100": ("device", 100_000, 100), "dev100k_34800": ("device", 100_000, 34_800),
        "host100k_100": ("host", 100_000, 100), "host100k_34800": ("host", 100_000, 34_800),
        "dev10M_100": ("device", 10_000_000, 100), "dev10M_34800": ("device", 10_000_000, 34_800)}
B = 4096


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "reps": reps}


def cfg(T):
    return SimpleNamespace(PRODUCT_EMB_DIM=128, TYPE_EMB_DIM=64, HIDDEN_SIZE=256, NUM_ATTENTION_HEADS=4, DROPOUT=0.0,
                           MARGIN=1.0, ALPHA=0.8, NUM_COMP_TYPES=3, NUM_TYPES=T, DEVICE=torch.device("cuda"),
                           LEARNING_RATE=1e-3)


def leg(name, args, res):
    from p_companion_amd import ops
    from p_companion_amd.data import (ComplementaryIndexDataset, ComplementaryIndexLoader, generate_device_bpg,
                                      generate_scaled_bpg)
    from p_companion_amd.metrics import Metrics
    from p_companion_amd.p_companion import GraphedJointStep, PCompanion
    from p_companion_amd.product2vec import FusedAdam, Product2Vec
    src, P, T = LEGS[name]
    c = cfg(T)
    t0 = time.time()
    bpg = generate_device_bpg(P, T, seed=0) if src == "device" else generate_scaled_bpg(P, T, seed=0)
    torch.cuda.synchronize()
    out = {"source": "generate_device_bpg" if src == "device" else "generate_scaled_bpg (uploaded IntBPG)", "products": P,
           "types": T, "B": B, "K": 3, "generate_s": round(time.time() - t0, 2)}
    if src == "device":
        comp, sim = bpg.arrays["comp_pairs"], bpg.arrays["sim_pairs"]
        out["labelled_pairs"] = int(comp.shape[0]) + int(sim.shape[0])
        if P >= 10_000_000 and "split" not in res:
            res["split"] = {"products": P, "labelled_pairs": out["labelled_pairs"],
                            "train": timed(lambda: ops.comp_split_pairs(comp, sim, 0, "train"), 1, args.reps),
                            "val": timed(lambda: ops.comp_split_pairs(comp, sim, 0, "val"), 1, args.reps)}
    torch.manual_seed(0)
    p2v = Product2Vec(c).to("cuda").eval()
    p2v.generate_all_embeddings(bpg)
    table = p2v.last_embedding_table                                 # the exported [P,128] table on the device
    ds = ComplementaryIndexDataset(bpg, "train", seed=0)
    out["train_pairs"] = len(ds)
    torch.manual_seed(0)
    m = PCompanion(c, table).to("cuda").train()
    step = GraphedJointStep(m, FusedAdam(m), B, warmup=0, mode="direct")
    ld = ComplementaryIndexLoader(ds, B, shuffle=True, out=step.static)
    out["epoch_pairs_ms"] = timed(lambda: ld.epoch_pairs(), 1, args.reps)
    pairs = ld.epoch_pairs()
    ld.epoch_pairs = lambda: pairs                                   # the timed runs: the steps alone
    S = min(args.steps, len(ds) // B)
    t = timed(lambda: step.run_epoch(ld, max_steps=S), 1, args.reps)
    losses = step.run_epoch(ld, max_steps=S)
    out["steps"] = S
    out["step_ms"] = {"median_ms": t["median_ms"] / S, "min_ms": t["min_ms"] / S, "reps": t["reps"]}
    out["finite_losses"] = bool(torch.isfinite(losses).all())
    out["index_errors"] = m.index_errors()
    if src == "device" and P >= 10_000_000 and args.evaluate:
        va_ds = ComplementaryIndexDataset(bpg, "val", seed=0)
        if 0 < len(va_ds) % B < 10:                                   # (a rest of 1..9 rows: both paths would take the loop)
            va_ds.pairs = va_ds.pairs[:len(va_ds) - len(va_ds) % B].contiguous()
        res.setdefault("evaluate", {})[f"T{T}"] = evaluate_leg(m, va_ds, c, P, T, args)
    del step, ld, ds, m, table, p2v, bpg, pairs
    torch.cuda.empty_cache()
    return out


def evaluate_leg(m, va_ds, c, P, T, args):
    """Metrics.evaluate_model over the val split: the existing per-batch loop (fused=False) and the one-call form
    (pc_joint_eval_epoch) alternating in THIS process, a host clock around calls that end in a synchronise, each path once
    untimed first.  FLOPs of the count product from the shapes."""
    from p_companion_amd import _lib
    from p_companion_amd.data import ComplementaryIndexLoader
    from p_companion_amd.metrics import Metrics
    n, K, D = len(va_ds), int(c.NUM_COMP_TYPES), int(c.PRODUCT_EMB_DIM)
    nb = (n + B - 1) // B

    def run(fused):
        va = ComplementaryIndexLoader(va_ds, B, shuffle=False)
        torch.cuda.synchronize()
        t0 = time.time()
        met = Metrics.evaluate_model(m, va, c.DEVICE, fused=fused)
        torch.cuda.synchronize()
        return time.time() - t0, met

    loop_reps = max(0, min(args.reps, args.loop_reps))                # (0: the one-call form alone, e.g. under a kernel trace)
    run(True)                                                         # untimed
    if loop_reps:
        run(False)
    one, loop, met_one, met_loop = [], [], None, None
    for i in range(args.reps):
        s, met_one = run(True)
        one.append(s)
        if i < loop_reps:
            s, met_loop = run(False)
            loop.append(s)
    sizes = [B] * (n // B) + ([n % B] if n % B else [])
    flops = float(sum(2.0 * b * b * D for b in sizes))                # the B x B x D count product of every batch
    peak = 157.3e12                                                   # fp32 MFMA peak of one MI355X
    e = {"products": P, "types": T, "val_pairs": n, "batches": nb, "B": B, "K": K,
         "loop_s": {"median": float(np.median(loop)), "min": float(min(loop)), "reps": len(loop)} if loop else None,
         "one_call_s": {"median": float(np.median(one)), "min": float(min(one)), "reps": len(one)},
         "loop_ms_per_batch": 1e3 * float(np.median(loop)) / nb if loop else None,
         "one_call_ms_per_batch": 1e3 * float(np.median(one)) / nb,
         "speedup": float(np.median(loop)) / float(np.median(one)) if loop else None,
         "count_product_flops": flops, "fp32_mfma_peak_tflops": peak / 1e12,
         # (lower bound on the count kernel's rate: the whole call's time, not the kernel's -- its own time comes from a
         # kernel trace, profiles/eval_10M_kernel_stats.csv)
         "count_tflops_over_whole_call": flops / float(np.median(one)) / 1e12,
         "metrics_one_call": met_one, "metrics_loop": met_loop,
         "workspace_bytes": int(_lib.lib().pc_joint_eval_workspace_bytes(B, T, K, D))}
    return e


def merge_kernel_stats(path_json, path_csv, leg="T100"):
    """No GPU: adds the count kernel's own rate to an existing result file from the `rocprofv3 --kernel-trace --stats` table of a
    run of the evaluate leg (a run of its own: tracing slows the host down).  Mean ns per launch of eval_count_kernel ->
    TFLOP/s and share of the fp32 MFMA peak, FLOPs per launch from the shapes."""
    import csv
    res = json.load(open(path_json))
    rows = [r for r in csv.DictReader(open(path_csv)) if "eval_count_kernel" in r["Name"]]
    if not rows:
        raise SystemExit(f"{path_csv}: no eval_count_kernel row")
    calls = sum(int(r["Calls"]) for r in rows)
    mean_ns = sum(float(r["TotalDurationNs"]) for r in rows) / calls
    for name, e in res.get("evaluate", {}).items():
        if name != leg:                                               # (the trace is of ONE leg's evaluation)
            continue
        per_launch = e["count_product_flops"] / e["batches"]
        e["count_kernel_us_traced"] = mean_ns / 1e3
        e["count_kernel_tflops"] = per_launch / (mean_ns * 1e-9) / 1e12
        e["count_kernel_share_of_fp32_peak"] = e["count_kernel_tflops"] / e["fp32_mfma_peak_tflops"]
    line = json.dumps(res)
    with open(path_json, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-evaluate", dest="evaluate", action="store_false")
    ap.add_argument("--loop-reps", type=int, default=2, help="timed runs of the existing evaluation loop (9.6 s each at 10 M)")
    ap.add_argument("--kernel-stats", default=None, help="merge a rocprofv3 kernel-stats CSV of the evaluate leg into --out and exit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "catalogue_joint_probe.json"))
    args = ap.parse_args()
    if args.kernel_stats:
        return merge_kernel_stats(args.out, args.kernel_stats)
    if not torch.cuda.is_available():
        raise SystemExit("catalogue_joint_probe: no GPU (nothing here is measured on the CPU)")
    res = {"probe": "catalogue_joint", "device": torch.cuda.get_device_name(0), "legs": {}}
    for name in [s for s in args.legs.split(",") if s]:
        res["legs"][name] = leg(name, args, res)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
