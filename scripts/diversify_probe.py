"""Developer tool: what the diversity re-rank costs beside the pool it re-ranks, and what it does to the lists
(pc_diversify_lists; PCompanionInference.recommend_diverse_batch).  On the SAME rows, proj and catalogue, alternating in one
process, for a pool of 64 and of 256 and n = 10 shown:

  retrieve_list_grouped(pool)                the pool alone: the yardstick
  diversify_lists(pool -> n)                 the re-rank alone, on that call's output (cosine scale, lam = 0.7); from the pool of
                                             256 also to n = 1 and n = 32: the gather against the rounds
  recommend_batch(n) / recommend_batch(pool) / recommend_diverse_batch(n, pool)
                                             the method beside the two calls it sits between (model forward included in all)

  100 k / 100 types      generate_scaled_bpg, uploaded
  10 M / 100 types       generate_device_bpg

Rows: B queries x K = 3 predicted types from the model's forward (as long_list_probe.py).  ms from device events: `--warmup`
untimed rounds, then `--reps` rounds, each round one call of every leg in turn; medians with min .. max.  Quality
(`--quality-legs`): Metrics.intra_list_similarity (cosine) of the n served products at diversity 0, 0.3 and 0.7 with pool 64,
over the generator's features and over similar_index_probe.py's clustered table (the same graph with that table as its
features).  Nothing here is a gate.  Writes profiles/diversify_probe.json (or --out) and prints the same JSON as one line.

  python scripts/diversify_probe.py [--legs 100k,10M] [--quality-legs 100k] [--warmup 3] [--reps 10] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from types import SimpleNamespace

import numpy as np
import torch

from long_list_probe import alternating
from similar_index_probe import clustered_table

LEGS = {"100k": (100_000, 100, 128), "10M": (10_000_000, 100, 128)}
POOLS = (64, 256)
N_SHOWN = 10
DIVERSITIES = (0.0, 0.3, 0.7)
N_SWEEP = (1, 32)


def served(bpg, features, T, d, dev):
    from p_companion_amd.inference import PCompanionInference
    from p_companion_amd.p_companion import PCompanion
    cfg = SimpleNamespace(PRODUCT_EMB_DIM=d, TYPE_EMB_DIM=64, HIDDEN_SIZE=256, NUM_ATTENTION_HEADS=4, DROPOUT=0.0,
                          MARGIN=1.0, ALPHA=0.8, NUM_COMP_TYPES=3, NUM_TYPES=T, DEVICE=dev)
    torch.manual_seed(0)
    return PCompanionInference(PCompanion(cfg, features), cfg, bpg)      # the product table IS the feature tensor


def quality(inf, q):
    from p_companion_amd import ops
    from p_companion_amd.metrics import Metrics
    scale = ops.inv_norm(inf.features)
    out = {}
    for dv in DIVERSITIES:
        _, idx, _ = inf.recommend_diverse_batch(q, N_SHOWN, pool=POOLS[0], diversity=dv)
        out[f"diversity_{dv}"] = float(Metrics.intra_list_similarity(idx, inf.features, scale))
    return out


def leg(name, args, dev):
    from p_companion_amd import ops
    from p_companion_amd.data import DeviceBPG, generate_device_bpg, generate_scaled_bpg
    P, T, d = LEGS[name]
    t0 = time.time()
    if P <= 1_000_000:
        bpg, src = generate_scaled_bpg(P, T, seed=0, dim=d), "generate_scaled_bpg (uploaded IntBPG)"
    else:
        bpg, src = generate_device_bpg(P, T, seed=0, dim=d, world=1, with_complementary=False), "generate_device_bpg"
    g = bpg.cuda(dev)
    torch.cuda.synchronize()
    out = {"source": src, "products": P, "types": T, "dim": d, "B": args.batch, "K": 3, "n": N_SHOWN,
           "generate_s": round(time.time() - t0, 2)}
    inf = served(bpg, g["features"], T, d, dev)
    rowptr, col, table = inf.type_rowptr, inf.type_col, inf.features
    q = torch.from_numpy(np.random.default_rng(1).integers(0, P, args.batch).astype(np.int32)).to(dev)
    with torch.no_grad():
        fwd = inf.model({"query_idx": q, "query_types": inf.type_idx[q.long()]})
    proj = fwd["projected_embeddings"].contiguous().reshape(-1, d)
    types = fwd["complementary_types"].to(torch.int32).reshape(-1).contiguous()
    out["rows"] = int(types.numel())
    scale = ops.inv_norm(table)
    inf.recommend_diverse_batch(q, N_SHOWN)                # (forms the cached scale outside the timed rounds)
    fns = {f"recommend_batch_{N_SHOWN}": lambda: inf.recommend_batch(q, N_SHOWN)}
    pools = {}
    for m in POOLS:
        pools[m] = ops.retrieve_list_grouped(proj, types, rowptr, col, table, m)
        fns[f"retrieve_list_grouped_{m}"] = (lambda m=m: ops.retrieve_list_grouped(proj, types, rowptr, col, table, m))
        fns[f"diversify_lists_{m}_to_{N_SHOWN}"] = (lambda m=m: ops.diversify_lists(*pools[m], table, N_SHOWN, 0.7, scale=scale))
        fns[f"recommend_batch_{m}"] = (lambda m=m: inf.recommend_batch(q, m))
        fns[f"recommend_diverse_batch_{N_SHOWN}_of_{m}"] = (lambda m=m: inf.recommend_diverse_batch(q, N_SHOWN, pool=m))
    # the gather against the rounds: n = 1 is the gather and one selection, every further pick one round more
    for k in N_SWEEP:
        fns[f"diversify_lists_256_to_{k}"] = (lambda k=k: ops.diversify_lists(*pools[256], table, k, 0.7, scale=scale))
    t = alternating(fns, args.warmup, args.reps)
    out.update(t)
    one, many = (t[f"diversify_lists_256_to_{k}"]["median_ms"] for k in N_SWEEP)
    out["ms_per_round_at_256"] = (many - one) / (N_SWEEP[1] - N_SWEEP[0])
    for m in POOLS:
        out[f"diversify_{m}_over_retrieve_list_{m}"] = (t[f"diversify_lists_{m}_to_{N_SHOWN}"]["median_ms"] /
                                                        t[f"retrieve_list_grouped_{m}"]["median_ms"])
        out[f"gathered_gbytes_{m}"] = out["rows"] * m * d * 4 / 1e9
    out["inv_norm"] = alternating({"inv_norm": lambda: ops.inv_norm(table)}, 1, args.reps)["inv_norm"]
    # the answers at the timed size: no diversity is the list's own head, and two runs agree bit for bit
    a = ops.diversify_lists(*pools[64], table, N_SHOWN, 1.0, scale=scale)
    b, c = fns[f"diversify_lists_64_to_{N_SHOWN}"](), fns[f"diversify_lists_64_to_{N_SHOWN}"]()
    out["agreement"] = {"lam_1_is_the_pools_head": bool(torch.equal(a[0], pools[64][0][:, :N_SHOWN])),
                        "two_runs_same_bits": bool(torch.equal(b[0], c[0]) and torch.equal(b[1].view(torch.int32), c[1].view(torch.int32))),
                        "picks_moved_at_lam_0.7": int((b[0] != a[0]).sum())}
    if name in args.quality_legs.split(","):
        out["intra_list_similarity"] = {"features": quality(inf, q)}
        if isinstance(bpg, DeviceBPG):
            arrays = dict(bpg.arrays)
        else:
            arrays = dict(g)
            arrays["max_degree"] = int(np.diff(bpg.cv_rowptr).max())
        arrays["features"] = clustered_table(g["type_idx"], T, d, args.spread, seed=7)
        alt = served(DeviceBPG(arrays, T, d), arrays["features"], T, d, dev)
        out["intra_list_similarity"]["clustered"] = quality(alt, q)
        out["intra_list_similarity"]["note"] = (f"cosine, n = {N_SHOWN} of pool {POOLS[0]}; clustered: one N(0, I) centre per "
                                                f"type x {args.spread} + N(0, I) noise as the graph's features")
        del alt, arrays
    else:
        out["intra_list_similarity"] = "not measured"
    del inf, g, bpg, proj, types, fwd, pools
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="100k,10M")
    ap.add_argument("--quality-legs", default="100k")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--spread", type=float, default=2.0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "diversify_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("diversify_probe: no GPU (nothing here is measured on the CPU)")
    dev = torch.device("cuda")
    res = {"probe": "diversify", "device": torch.cuda.get_device_name(0), "legs": {}}
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
