"""Developer tool: what a long list costs (pc_retrieve_list_grouped, up to 256 products per (query, type)).  On the SAME rows,
proj and catalogue, alternating in one process:

  retrieve_topk_grouped(n = 16)              the existing entry at its limit
  retrieve_list_grouped(n = 16 .. 256)       the new entry; at 16 beside the line above: what the buffer scheme costs where it
                                             is not needed
  peeled(n = 64)                             what a caller had to do before: four calls of the existing entries, each excluding
                                             what the earlier ones served (ops.exclusion_csr over a per-row CSR, row_key =
                                             arange(rows)); building the growing set is part of the leg

  100 k / 100 types      generate_scaled_bpg, uploaded
  10 M / 100 types       generate_device_bpg

Rows: B queries x K = 3 predicted types from the model's forward (as retrieval_probe.py).  ms from device events: `--warmup`
untimed rounds, then `--reps` rounds, each round one call of every leg in turn; medians with min .. max.  The answers are
compared at the timed size: the new entry at 16 is the existing entry's bit for bit, at 64 the peeled lists'.  Writes
profiles/long_list_probe.json (or --out) and prints the same JSON as one line.

  python scripts/long_list_probe.py [--legs 100k,10M] [--warmup 3] [--reps 10] [--out FILE]
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
NS = (16, 32, 64, 128, 256)
N_PEEL = 64


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
    out = {"source": src, "products": P, "types": T, "dim": d, "B": args.batch, "K": 3, "generate_s": round(time.time() - t0, 2)}
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
    rows = int(types.numel())
    out["rows"] = rows
    row_key = torch.arange(rows, dtype=torch.int32, device=dev)

    def peeled(n=N_PEEL):
        idx, sc = [], []
        for step in range((n + 15) // 16):
            if step == 0:
                i, s = ops.retrieve_topk_grouped(proj, types, rowptr, col, table, 16)
            else:
                served = torch.cat(idx, 1).contiguous()
                rp = (torch.arange(rows + 1, device=dev) * served.shape[1]).to(torch.int32)
                ex = ops.exclusion_csr(rp, served.reshape(-1), include_self=False, num_products=P)
                i, s = ops.retrieve_topk_grouped(proj, types, rowptr, col, table, 16, exclude=(row_key,) + ex)
            idx.append(i)
            sc.append(s)
        return torch.cat(idx, 1)[:, :n], torch.cat(sc, 1)[:, :n]

    fns = {"retrieve_topk_grouped_16": lambda: ops.retrieve_topk_grouped(proj, types, rowptr, col, table, 16)}
    for n in NS:
        fns[f"retrieve_list_grouped_{n}"] = (lambda n=n: ops.retrieve_list_grouped(proj, types, rowptr, col, table, n))
    fns[f"peeled_{N_PEEL}"] = peeled
    t = alternating(fns, args.warmup, args.reps)
    out.update(t)
    out["list_16_over_topk_16"] = t["retrieve_list_grouped_16"]["median_ms"] / t["retrieve_topk_grouped_16"]["median_ms"]
    out[f"peeled_{N_PEEL}_over_list_{N_PEEL}"] = t[f"peeled_{N_PEEL}"]["median_ms"] / t[f"retrieve_list_grouped_{N_PEEL}"]["median_ms"]
    # the answers at the timed size
    a_i, a_s = fns["retrieve_topk_grouped_16"]()
    b_i, b_s = fns["retrieve_list_grouped_16"]()
    c_i, c_s = fns[f"retrieve_list_grouped_{N_PEEL}"]()
    p_i, p_s = peeled()
    l_i, _ = fns["retrieve_list_grouped_256"]()
    out["agreement"] = {"list_16_is_topk_16": bool(torch.equal(a_i, b_i) and torch.equal(a_s.view(torch.int32), b_s.view(torch.int32))),
                        f"list_{N_PEEL}_is_peeled_{N_PEEL}": bool(torch.equal(c_i, p_i) and
                                                                  torch.equal(c_s.contiguous().view(torch.int32),
                                                                              p_s.contiguous().view(torch.int32))),
                        "list_256_starts_with_list_64": bool(torch.equal(l_i[:, :N_PEEL], c_i)),
                        "entries_served_at_256": int((l_i >= 0).sum())}
    del inf, model, g, bpg, proj, types, fwd
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="100k,10M")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "long_list_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("long_list_probe: no GPU (nothing here is measured on the CPU)")
    dev = torch.device("cuda")
    res = {"probe": "long_list", "device": torch.cuda.get_device_name(0), "legs": {}}
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
