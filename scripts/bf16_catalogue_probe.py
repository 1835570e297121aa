"""Developer tool: what serving from a bf16 copy of the catalogue costs and changes.  On the SAME proj / types, in the same
process, ops.retrieve_topk_grouped over the fp32 table (pc_retrieve_topk_grouped, the yardstick) and over
ops.catalogue_bf16 of it (pc_retrieve_topk_grouped_bf16), alternating; the bytes of both tables; and how far the rounded
table moves the lists.  Prints ONE JSON line.

  100 k / 100 types      generate_device_bpg
  10 M / 100 types       generate_device_bpg

B queries x K = 3 predicted types, top n.  ms from device events around `--reps` calls after `--warmup` untimed ones (median
and min).  FLOPs = 2 D sum_r count(type r) (the bf16 entry issues three times as many on the bf16 pipe: `issued_tflops`);
minimum bytes = every hit type's candidate rows once at the table's width, its CSR entries, proj, types and the outputs.
Lists: the share of (row, position) slots whose product differs from the fp32 catalogue's list, the share of rows whose
top-n SET differs, and the largest score difference on the slots that agree -- properties of the rounded table, not errors:
against a float64 computation over the rounded table the entry is held to 1e-5 by tests/test_gpu_retrieval_bf16.py.

  python scripts/bf16_catalogue_probe.py [--legs 100k,10M] [--warmup 3] [--reps 10] [--only fp32|bf16]
Per-kernel times: the same command under rocprofv3 --kernel-trace --stats (e.g. --legs 10M --reps 3).
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
PEAK_HBM = 8.0e12
LEGS = {"100k": (100_000, 100, 128), "10M": (10_000_000, 100, 128)}


def timed_pair(fns, warmup, reps):
    """{name: {median_ms, min_ms, reps}} of the calls in `fns`, alternating between them in every repetition."""
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


def roofline(types, rowptr, d, n, ms, elem):
    cnt = (rowptr[1:] - rowptr[:-1]).long()
    t = types.long()
    ok = (t >= 0) & (t < cnt.numel())
    per_row = torch.zeros_like(t)
    per_row[ok] = cnt[t[ok]]
    hit = torch.unique(t[ok])
    flops = 2.0 * d * float(per_row.sum())
    cand = float(cnt[hit].sum())
    nbytes = cand * (float(elem) * d + 4) + 4.0 * types.numel() * (d + 1 + 2 * n) + 8.0 * hit.numel()
    s = ms * 1e-3
    return {"gflop": flops / 1e9, "min_gbytes": nbytes / 1e9, "tflops": flops / s / 1e12, "tbps": nbytes / s / 1e12,
            "share_of_fp32_peak": flops / PEAK_FP32 / s, "share_of_hbm_peak": nbytes / PEAK_HBM / s}


def leg(name, args, dev):
    from p_companion_amd import ops
    from p_companion_amd.data import generate_device_bpg
    from p_companion_amd.inference import PCompanionInference
    from p_companion_amd.p_companion import PCompanion
    P, T, d = LEGS[name]
    t0 = time.time()
    bpg = generate_device_bpg(P, T, seed=0, dim=d, world=1, with_complementary=False)
    g = bpg.cuda(dev)
    torch.cuda.synchronize()
    out = {"source": "generate_device_bpg", "products": P, "types": T, "dim": d, "B": args.batch, "K": 3, "n": args.n,
           "generate_s": round(time.time() - t0, 2)}
    cfg = SimpleNamespace(PRODUCT_EMB_DIM=d, TYPE_EMB_DIM=64, HIDDEN_SIZE=256, NUM_ATTENTION_HEADS=4, DROPOUT=0.0,
                          MARGIN=1.0, ALPHA=0.8, NUM_COMP_TYPES=3, NUM_TYPES=T, DEVICE=dev)
    torch.manual_seed(0)
    model = PCompanion(cfg, g["features"])            # the product table IS the feature tensor (no second copy)
    inf = PCompanionInference(model, cfg, bpg)
    t0 = time.time()
    table16 = ops.catalogue_bf16(g["features"])
    torch.cuda.synchronize()
    out["catalogue_bf16_s"] = round(time.time() - t0, 3)
    out["table_bytes"] = {"fp32": g["features"].numel() * 4, "bf16": table16.numel() * 2}
    q = torch.from_numpy(np.random.default_rng(1).integers(0, P, args.batch).astype(np.int32)).to(dev)
    with torch.no_grad():
        fwd = inf.model({"query_idx": q, "query_types": inf.type_idx[q.long()]})
    proj = fwd["projected_embeddings"].contiguous().reshape(-1, d)
    types = fwd["complementary_types"].to(torch.int32).reshape(-1).contiguous()
    fns = {"fp32": lambda: ops.retrieve_topk_grouped(proj, types, inf.type_rowptr, inf.type_col, g["features"], args.n),
           "bf16": lambda: ops.retrieve_topk_grouped(proj, types, inf.type_rowptr, inf.type_col, table16, args.n)}
    if args.only:
        fns = {args.only: fns[args.only]}
    t = timed_pair(fns, args.warmup, args.reps)
    for k, v in t.items():
        out["retrieval_" + k] = {**v, **roofline(types, inf.type_rowptr, d, args.n, v["median_ms"], 4 if k == "fp32" else 2)}
    if len(fns) == 2:
        out["retrieval_bf16"]["issued_tflops"] = 3 * out["retrieval_bf16"]["tflops"]
        out["bf16_over_fp32_time"] = out["retrieval_bf16"]["median_ms"] / out["retrieval_fp32"]["median_ms"]
        i32, s32 = fns["fp32"]()
        i16, s16 = fns["bf16"]()
        same = i32 == i16
        a, b = torch.sort(i32, 1).values, torch.sort(i16, 1).values
        out["lists_vs_fp32_catalogue"] = {
            "slots": int(i32.numel()), "rows": int(i32.shape[0]),
            "slots_with_another_product": float((~same).float().mean()),
            "rows_with_another_top_n_set": float((a != b).any(1).float().mean()),
            "rows_with_another_first_product": float((i32[:, 0] != i16[:, 0]).float().mean()),
            "missing_slots_equal": bool(torch.equal(i32 < 0, i16 < 0)),
            "max_abs_score_diff_on_equal_slots": float((s32 - s16)[same & (i32 >= 0)].abs().max()),
            "median_abs_score": float(s32[i32 >= 0].abs().median())}
    del inf, model, g, bpg, proj, types, fwd, table16
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="100k,10M")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", choices=("fp32", "bf16"), default=None, help="time one entry alone (a profiler run)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bf16_catalogue_probe: no GPU (nothing here is measured on the CPU)")
    dev = torch.device("cuda")
    res = {"probe": "bf16_catalogue", "device": torch.cuda.get_device_name(0), "legs": {}}
    for name in [s for s in args.legs.split(",") if s]:
        res["legs"][name] = leg(name, args, dev)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
