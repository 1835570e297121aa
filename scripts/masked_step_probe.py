"""Developer tool: what the key-padding mask (config.ATTENTION_KEY_MASK) costs a training step.

BASELINE configs[1]'s shape as bench.py runs it (100 k products, 100 types, D = 128, B = 4096; the device loader's unique
layout with loader-made rows, FusedAdam riding in the step's last launch), two models in ONE process: one steps masked
(pc_p2v_train_step_unique_masked), one unmasked (pc_p2v_train_step_unique_rows), each over its own loader with the same
seed, so both see the same batches.  The legs ALTERNATE -- `--rounds` times `--steps` steps of one, then of the other -- and
every leg is timed by the host clock between two device synchronisations, loader calls included, as bench.py times its
headline.  No target is set: the masked leg is reported beside the unmasked leg of the same process, with the spread of
each over the rounds (what a difference has to exceed to mean anything).

  python scripts/masked_step_probe.py [--products 100000] [--batch 4096] [--steps 200] [--rounds 5] [--warmup 50]
Prints ONE JSON line and writes it to profiles/masked_step_probe.json.
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


def leg(masked, bpg, table, args, dev):
    from p_companion_amd.data import SimilarityIndexLoader
    from p_companion_amd.product2vec import FusedAdam, Product2Vec
    cfg = SimpleNamespace(PRODUCT_EMB_DIM=128, TYPE_EMB_DIM=64, HIDDEN_SIZE=256, NUM_ATTENTION_HEADS=4, DROPOUT=0.0, MARGIN=1.0,
                          BATCH_SIZE=args.batch, LEARNING_RATE=1e-3, DEVICE=dev, ATTENTION_KEY_MASK=masked)
    torch.manual_seed(0)
    model = Product2Vec(cfg).to(dev).train()
    opt = FusedAdam(model, lr=cfg.LEARNING_RATE)
    model.flatten_parameters()
    loader = SimilarityIndexLoader(bpg, args.batch, shuffle=True, sampler="philox", seed=1, drop_last=True, device=dev,
                                   reuse_buffers=True)

    def batches():
        while True:
            for b in loader:
                yield b
    it = batches()
    state = {"loss": None, "slots": 0, "real": 0, "steps": 0}

    def run(steps):
        for _ in range(steps):
            b = next(it)
            nbc = b["neighbor_compact"]
            state["slots"] += b["anchor_idx"].numel() * b["n_pad"]
            state["real"] += nbc["n_real"]
            state["steps"] += 1
            state["loss"] = model.train_step_indexed(table, b, optimizer=opt)
    return run, state


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--products", type=int, default=100_000)
    ap.add_argument("--types", type=int, default=100)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=50)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("masked_step_probe: no GPU (nothing here is measured on the CPU)")
    from p_companion_amd.data import generate_scaled_bpg
    dev = torch.device("cuda")
    bpg = generate_scaled_bpg(args.products, args.types, seed=0, dim=128)
    table = bpg.cuda(dev)["features"]
    legs = {"unmasked": leg(False, bpg, table, args, dev), "masked": leg(True, bpg, table, args, dev)}
    for run, _ in legs.values():
        run(args.warmup)
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(args.rounds):
        for name, (run, _) in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(args.steps)
            torch.cuda.synchronize()
            ms[name].append(1e3 * (time.perf_counter() - t0) / args.steps)
    res = {"probe": "masked_step", "device": torch.cuda.get_device_name(0), "products": args.products, "batch": args.batch,
           "steps_per_leg": args.steps, "rounds": args.rounds, "legs": {}}
    for name, (_, st) in legs.items():
        v = ms[name]
        res["legs"][name] = {"ms_per_step_median": float(np.median(v)), "ms_per_step_min": float(min(v)), "ms_per_step_max": float(max(v)),
                             "ms_per_step_rounds": [round(x, 4) for x in v], "final_loss": float(st["loss"]),
                             "padding_share_of_slots": round(1.0 - st["real"] / max(st["slots"], 1), 4)}
    u, m = res["legs"]["unmasked"], res["legs"]["masked"]
    res["masked_over_unmasked"] = m["ms_per_step_median"] / u["ms_per_step_median"]
    res["run_to_run_spread_unmasked"] = (u["ms_per_step_max"] - u["ms_per_step_min"]) / u["ms_per_step_median"]
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "masked_step_probe.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
