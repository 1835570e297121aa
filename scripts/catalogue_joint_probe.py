"""Developer tool: joint P-Companion training over a device-resident catalogue (a DeviceBPG) on one MI355X.  Writes
profiles/catalogue_joint_probe.json (and prints it as one JSON line).

  split        ops.comp_split_pairs (pc_comp_split_pairs) of the train / val modes at 10 M products
  steps        ms per joint step, B = 4096, K = 3, through GraphedJointStep.run_epoch(max_steps=S) over
                 a DeviceBPG at 100 k and 10 M products                     (legs dev100k_*, dev10M_*)
                 an IntBPG from generate_scaled_bpg at 100 k, uploaded      (legs host100k_*)
               at T = 100 and T = 34 800 types.  The product table is a Product2Vec export of the catalogue (a second
               [P,128] array beside the features: 5.1 GB each at 10 M).  The loader's per-epoch shuffle is timed on its own
               (epoch_pairs_ms); the timed runs reuse one shuffled order, so steps_ms is the steps alone.
  evaluate     Metrics.evaluate_model over the 10 M val split (host clock around the call, which reads back every batch)

ms from device events around `--reps` calls after one untimed call (median and min).

  python scripts/catalogue_joint_probe.py [--legs dev100k_100,dev100k_34800,host100k_100,host100k_34800,dev10M_100,dev10M_34800]
                                          [--steps 200] [--reps 5] [--no-evaluate]
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
    if src == "device" and P >= 10_000_000 and T == 100 and args.evaluate:
        va = ComplementaryIndexLoader(ComplementaryIndexDataset(bpg, "val", seed=0), B, shuffle=False)
        torch.cuda.synchronize()
        t0 = time.time()
        met = Metrics.evaluate_model(m, va, c.DEVICE)
        torch.cuda.synchronize()
        res["evaluate"] = {"products": P, "types": T, "val_pairs": len(va.dataset), "batches": len(va),
                           "s": round(time.time() - t0, 3), "hit@10": met["hit@10"]}
    del step, ld, ds, m, table, p2v, bpg, pairs
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-evaluate", dest="evaluate", action="store_false")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "catalogue_joint_probe.json"))
    args = ap.parse_args()
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
