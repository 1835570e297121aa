"""Developer tool: what serving long and diversified lists from the bf16 catalogue alone costs beside the fp32 catalogue, and
what it gives back (pc_retrieve_list_grouped_bf16, pc_diversify_lists_bf16; ops.CompactCatalogue).  On the SAME rows, proj and
catalogue, the bf16 and the fp32 leg of every pair alternating in one process:

  retrieve_list_grouped(n), n = 16 / 64 / 128 / 256        the bf16 table beside the fp32 table
  diversify_lists_bf16 beside diversify_lists               pools of 64 and 256 -> n = 10 (cosine scale, lam = 0.7); each leg
                                                            re-ranks the pool its own table served
  recommend_diverse_batch(q, 10, pool = 64 / 256)           a PCompanionInference over an ops.CompactCatalogue beside one over
                                                            the fp32 features (model forward included in both)
  differing slots                                           the share of the slots of the bf16 list that name another product
                                                            than the fp32 list's slot, n = 64 and 256 (lists of the ROUNDED table
                                                            beside lists of the fp32 table), and the share of rows with any
  memory                                                    what each serving object keeps resident for serving (the table, the
                                                            cosine factors once formed, the type arrays and CSR) and the peak of
                                                            the allocator above that during recommend_diverse_batch(10, pool 256)

  100 k / 100 types      generate_scaled_bpg, uploaded
  10 M / 100 types       generate_device_bpg

Rows: B = 4096 queries x K = 3 predicted types from the model's forward: 12 288.  ms: a host clock around a call that ends in a
device synchronise; `--warmup` untimed rounds (2), then `--reps` rounds, each round one call of every leg in turn; medians with
min .. max.  Nothing here is a gate.  Writes profiles/compact_catalogue_probe.json (or --out) and prints the same JSON as one
line.

  python scripts/compact_catalogue_probe.py [--legs 100k,10M] [--warmup 2] [--reps 9] [--out FILE]
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
LIST_NS = (16, 64, 128, 256)
POOLS = (64, 256)
DIFF_NS = (64, 256)
N_SHOWN = 10


def alternating(fns, warmup, reps):
    """{name: {median_ms, min_ms, max_ms, reps}}: every round runs each function once, in turn; a host clock around the call
    and the device synchronise that ends it."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    return {k: {"median_ms": float(np.median(v)), "min_ms": float(min(v)), "max_ms": float(max(v)), "reps": reps}
            for k, v in ms.items()}


def nbytes(*tensors):
    return int(sum(t.numel() * t.element_size() for t in tensors if t is not None))


def transient_peak(fn):
    """the allocator's peak above what is allocated when the call starts"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def leg(name, args, dev):
    from p_companion_amd import ops
    from p_companion_amd.data import DeviceBPG, generate_device_bpg, generate_scaled_bpg
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
    out = {"source": src, "products": P, "types": T, "dim": d, "B": args.batch, "K": 3, "n": N_SHOWN,
           "generate_s": round(time.time() - t0, 2)}
    cfg = SimpleNamespace(PRODUCT_EMB_DIM=d, TYPE_EMB_DIM=64, HIDDEN_SIZE=256, NUM_ATTENTION_HEADS=4, DROPOUT=0.0,
                          MARGIN=1.0, ALPHA=0.8, NUM_COMP_TYPES=3, NUM_TYPES=T, DEVICE=dev)
    torch.manual_seed(0)
    model = PCompanion(cfg, g["features"])                 # the product table IS the feature tensor
    full = PCompanionInference(model, cfg, bpg)
    cc = ops.CompactCatalogue(g["features"])
    # the compact object never sees the fp32 features: a device graph without them
    arrays = dict(bpg.arrays) if isinstance(bpg, DeviceBPG) else dict(g, max_degree=int(np.diff(bpg.cv_rowptr).max()))
    arrays.pop("features")
    compact = PCompanionInference(model, cfg, DeviceBPG(arrays, T, d), catalogue=cc)
    assert compact.features is None and "features" not in compact._graph
    rowptr, col, t32, t16 = full.type_rowptr, full.type_col, full.features, cc.table
    q = torch.from_numpy(np.random.default_rng(1).integers(0, P, args.batch).astype(np.int32)).to(dev)
    with torch.no_grad():
        fwd = full.model({"query_idx": q, "query_types": full.type_idx[q.long()]})
    proj = fwd["projected_embeddings"].contiguous().reshape(-1, d)
    types = fwd["complementary_types"].to(torch.int32).reshape(-1).contiguous()
    out["rows"] = int(types.numel())
    s32, s16 = ops.inv_norm(t32), cc.inv_norm
    full.recommend_diverse_batch(q, N_SHOWN)               # (forms the cached scale outside the timed rounds)
    fns = {}
    for n in LIST_NS:
        fns[f"retrieve_list_grouped_{n}_bf16"] = (lambda n=n: ops.retrieve_list_grouped(proj, types, rowptr, col, t16, n))
        fns[f"retrieve_list_grouped_{n}_fp32"] = (lambda n=n: ops.retrieve_list_grouped(proj, types, rowptr, col, t32, n))
    pools16 = {m: ops.retrieve_list_grouped(proj, types, rowptr, col, t16, m) for m in POOLS}
    pools32 = {m: ops.retrieve_list_grouped(proj, types, rowptr, col, t32, m) for m in POOLS}
    for m in POOLS:
        fns[f"diversify_lists_{m}_to_{N_SHOWN}_bf16"] = (lambda m=m: ops.diversify_lists_bf16(*pools16[m], t16, N_SHOWN, 0.7, scale=s16))
        fns[f"diversify_lists_{m}_to_{N_SHOWN}_fp32"] = (lambda m=m: ops.diversify_lists(*pools32[m], t32, N_SHOWN, 0.7, scale=s32))
        fns[f"recommend_diverse_batch_{N_SHOWN}_of_{m}_compact"] = (lambda m=m: compact.recommend_diverse_batch(q, N_SHOWN, pool=m))
        fns[f"recommend_diverse_batch_{N_SHOWN}_of_{m}_fp32"] = (lambda m=m: full.recommend_diverse_batch(q, N_SHOWN, pool=m))
    t = alternating(fns, args.warmup, args.reps)
    out.update(t)
    ratio = lambda a, b: t[a]["median_ms"] / t[b]["median_ms"]
    out["bf16_over_fp32"] = {
        **{f"retrieve_list_grouped_{n}": ratio(f"retrieve_list_grouped_{n}_bf16", f"retrieve_list_grouped_{n}_fp32") for n in LIST_NS},
        **{f"diversify_lists_{m}_to_{N_SHOWN}": ratio(f"diversify_lists_{m}_to_{N_SHOWN}_bf16", f"diversify_lists_{m}_to_{N_SHOWN}_fp32")
           for m in POOLS},
        **{f"recommend_diverse_batch_{N_SHOWN}_of_{m}": ratio(f"recommend_diverse_batch_{N_SHOWN}_of_{m}_compact",
                                                            f"recommend_diverse_batch_{N_SHOWN}_of_{m}_fp32") for m in POOLS}}
    # the lists of the rounded table beside the lists of the fp32 table
    out["differing_slots"] = {}
    for n in DIFF_NS:
        a, b = pools16[n][0], pools32[n][0]
        live = b >= 0
        out["differing_slots"][f"n_{n}"] = {"share_of_slots": float(((a != b) & live).sum() / live.sum().clamp(min=1)),
                                            "share_of_rows": float((a != b).any(1).float().mean()),
                                            "share_of_products_not_in_the_other_list": float(
                                                1.0 - (a[:, :, None] == b[:, None, :]).any(2)[live].float().mean()) if n <= 64
                                            else "not measured"}
    # the answers at the timed size
    w = ops.diversify_lists(*pools16[64], t16.float(), N_SHOWN, 0.7, scale=ops.inv_norm(t16.float())) if P <= 1_000_000 else None
    x, y = fns[f"diversify_lists_64_to_{N_SHOWN}_bf16"](), fns[f"diversify_lists_64_to_{N_SHOWN}_bf16"]()
    same = lambda u, v: bool(torch.equal(u[0], v[0]) and torch.equal(u[1].view(torch.int32), v[1].view(torch.int32)))
    head = ops.retrieve_topk_grouped(proj, types, rowptr, col, t16, 16)
    out["agreement"] = {"two_runs_same_bits": same(x, y),
                        "bf16_list_head_is_the_16_entry_bf16_list": same((pools16[256][0][:, :16].contiguous(),
                                                                          pools16[256][1][:, :16].contiguous()), head),
                        "diversify_bf16_is_fp32_on_the_widened_table": same(x, w) if w is not None else "not measured"}
    # memory: what serving keeps, and the transient peak of the largest call
    res16 = nbytes(t16, s16, compact.type_idx, compact.type_rowptr, compact.type_col)
    res32 = nbytes(t32, s32, full.type_idx, full.type_rowptr, full.type_col)
    p16 = transient_peak(lambda: compact.recommend_diverse_batch(q, N_SHOWN, pool=256))
    p32 = transient_peak(lambda: full.recommend_diverse_batch(q, N_SHOWN, pool=256))
    out["memory"] = {"compact": {"table_bytes": nbytes(t16), "resident_bytes": res16, "transient_peak_bytes": p16,
                                 "serving_peak_bytes": res16 + p16},
                     "fp32": {"table_bytes": nbytes(t32), "resident_bytes": res32, "transient_peak_bytes": p32,
                              "serving_peak_bytes": res32 + p32},
                     "compact_over_fp32": (res16 + p16) / (res32 + p32),
                     "note": "resident: the table, the cosine factors, type_idx and the type CSR; the model (whose product table is "
                             "the caller's) and the graph's other arrays are the same in both and not counted"}
    del full, compact, cc, g, bpg, proj, types, fwd, pools16, pools32, model
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="100k,10M")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compact_catalogue_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("compact_catalogue_probe: no GPU (nothing here is measured on the CPU)")
    dev = torch.device("cuda")
    res = {"probe": "compact_catalogue", "device": torch.cuda.get_device_name(0), "legs": {}}
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
