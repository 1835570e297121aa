"""Developer tool: what training the product table costs a joint step.  In the same process, alternating, on one MI355X:

  frozen      PCompanion.train_step(batch, optimizer=FusedAdam)                       (the yardstick: today's step)
  trained     PCompanion.train_step(batch, optimizer=FusedAdam, table_optimizer=ProductTableAdam)
  query_grad  ops.joint_query_grad alone (pc_joint_query_grad: six launches)
  sparse_adam ops.sparse_adam_rows alone (pc_sparse_adam_rows: the sort and the update)

  100 k x 128 and 10 M x 128 products (a random table), B = 4096, K = 3, T = 100; the queries are drawn uniformly, and once more
  with a popular head (a fifth of the batch on 16 products) for the row-sparse Adam.

  adam_1M     ops.sparse_adam_rows alone at R = 2^20 uniform rows of a 10 M x 128 table: the multi-workgroup sort (R > 8192;
              the legs above run R = 4096, which one workgroup sorts) and the update over a million sources

Host clock around a synchronised call, two untimed rounds first, median of `--reps` = 20; every single time is kept
("ms_all") so that the trained leg can be read against the frozen leg's own spread.  Prints ONE JSON line and, with --out,
writes it.

  python scripts/table_train_probe.py [--legs 100k,10M,adam_1M] [--reps 20] [--out profiles/table_train_probe.json]
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

LEGS = {"100k": 100_000, "10M": 10_000_000}
B, K, T, D = 4096, 3, 100, 128


def timed(fns, reps):
    for _ in range(2):
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


def leg(P, reps, dev):
    from p_companion_amd import ops
    from p_companion_amd.p_companion import PCompanion
    from p_companion_amd.product2vec import FusedAdam
    from p_companion_amd.table_optim import ProductTableAdam
    cfg = SimpleNamespace(PRODUCT_EMB_DIM=D, TYPE_EMB_DIM=64, HIDDEN_SIZE=256, NUM_ATTENTION_HEADS=4, DROPOUT=0.0, MARGIN=1.0,
                          ALPHA=0.8, NUM_COMP_TYPES=K, NUM_TYPES=T, DEVICE=dev, LEARNING_RATE=1e-3)
    g = torch.Generator(device=dev).manual_seed(0)
    table = torch.randn(P, D, generator=g, device=dev)
    torch.manual_seed(0)
    model = PCompanion(cfg, table).to(dev).train()
    opt, topt = FusedAdam(model, lr=1e-3), ProductTableAdam(model, lr=1e-3)
    batch = {"query_idx": torch.randint(0, P, (B,), generator=g, device=dev, dtype=torch.int32),
             "query_types": torch.randint(0, T, (B,), generator=g, device=dev),
             "positive_types": torch.randint(0, T, (B, 1), generator=g, device=dev),
             "negative_types": torch.randint(0, T, (B, 1), generator=g, device=dev),
             "positive_items": torch.randn(B, D, generator=g, device=dev), "negative_items": torch.randn(B, D, generator=g, device=dev)}
    out = {"products": P, "dim": D, "B": B, "K": K, "T": T, "moment_gbytes": 2 * P * D * 4 / 1e9}
    t = timed({"frozen": lambda: model.train_step(batch, optimizer=opt),
               "trained": lambda: model.train_step(batch, optimizer=opt, table_optimizer=topt)}, reps)
    out["step"] = dict(t, trained_over_frozen=t["trained"]["median_ms"] / t["frozen"]["median_ms"],
                       added_ms=t["trained"]["median_ms"] - t["frozen"]["median_ms"])
    params = model._tensor_dict()
    params["product_embeddings.weight"] = model.product_embeddings.weight
    _, topk = model.train_step(batch)
    dq = ops.joint_query_grad(params, batch["query_idx"], topk, batch["positive_items"], batch["negative_items"], 1.0, 0.8)
    hot = batch["query_idx"].clone()
    hot[:B // 5] = hot[torch.randint(0, 16, (B // 5,), generator=g, device=dev)]
    step = [topt._step]

    def adam(idx):
        step[0] += 1
        ops.sparse_adam_rows(model.product_embeddings.weight.data, topt.exp_avg, topt.exp_avg_sq, idx, dq, step[0])

    out["entries"] = timed({"query_grad": lambda: ops.joint_query_grad(params, batch["query_idx"], topk, batch["positive_items"],
                                                                       batch["negative_items"], 1.0, 0.8),
                            "sparse_adam_uniform": lambda: adam(batch["query_idx"]),
                            "sparse_adam_popular_head": lambda: adam(hot)}, reps)
    assert model.index_errors() == 0
    return out


def adam_leg(reps, dev, P=10_000_000, R=1 << 20):
    from p_companion_amd import ops
    g = torch.Generator(device=dev).manual_seed(1)
    table = torch.randn(P, D, generator=g, device=dev)
    m, v = torch.zeros_like(table), torch.zeros_like(table)
    idx = torch.randint(0, P, (R,), generator=g, device=dev, dtype=torch.int32)
    grad = torch.randn(R, D, generator=g, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    step = [0]

    def adam():
        step[0] += 1
        ops.sparse_adam_rows(table, m, v, idx, grad, step[0], bad=bad)

    out = {"products": P, "dim": D, "rows": R, "entries": timed({"sparse_adam_uniform": adam}, reps)}
    assert int(bad) == 0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="100k,10M")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("table_train_probe: no GPU (nothing here is measured on the CPU)")
    dev = torch.device("cuda")
    res = {"probe": "table_train", "device": torch.cuda.get_device_name(0), "legs": {}}
    for name in [s for s in args.legs.split(",") if s]:
        res["legs"][name] = adam_leg(args.reps, dev) if name == "adam_1M" else leg(LEGS[name], args.reps, dev)
        torch.cuda.empty_cache()
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
