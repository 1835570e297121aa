"""Developer tool: what ranking targets and serving substitutes from the bf16 catalogue alone costs beside the fp32 catalogue,
and what it gives back (pc_rank_grouped_bf16, pc_retrieve_list_grouped_bf16_biased; ops.CompactCatalogue,
inference.CompactSimilarProducts).  On the SAME rows, proj, targets and catalogue, the bf16 and the fp32 leg of every pair
alternating in one process:

  rank_grouped_bf16 beside rank_grouped                     plain / excluding (the co-view lists and the query itself, keyed by
                                                            the query) / biased (the half-norm term of each table)
  retrieve_list_grouped_bf16_biased beside                  n = 16 / 64 / 256, the half-norm term of each table
    retrieve_list_grouped_biased
  CompactSimilarProducts beside SimilarProducts             similar_batch(q, 10) and similar_list_batch(q, 64), scope "type"
                                                            (the row gather and the distances included in both)
  CompactInference beside PCompanionInference               rank_targets(q, y) over B pairs, the model's forward included, the
                                                            co-view exclusions installed in both; the compact object over a graph
                                                            without features
  agreement                                                 the bf16 rank is < 256 exactly where the bf16 list holds the target
                                                            there; the same ranks for slices = 1; the share of rows whose bf16
                                                            rank (over the ROUNDED table) differs from the fp32 rank
  memory                                                    what each BUILT object keeps resident (the table, the bias, the
                                                            type arrays and CSR, the exclusion CSR): sums over the objects' own
                                                            tensors

  100 k / 100 types      generate_scaled_bpg, uploaded
  10 M / 100 types       generate_device_bpg

Rows: B = 4096 queries x K = 3 predicted types from the model's forward: 12 288; a row's target is a product of its type, drawn
uniformly.  ms: a host clock around a call that ends in a device synchronise; `--warmup` untimed rounds (2), then `--reps`
rounds, each round one call of every leg in turn; medians with min .. max.  Nothing here is a gate.  Writes
profiles/compact_rank_probe.json (or --out) and prints the same JSON as one line.

  python scripts/compact_rank_probe.py [--legs 100k,10M] [--warmup 2] [--reps 9] [--out FILE]
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
LIST_NS = (16, 64, 256)


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


def leg(name, args, dev):
    from p_companion_amd import ops
    from p_companion_amd.data import DeviceBPG, generate_device_bpg, generate_scaled_bpg
    from p_companion_amd.inference import CompactInference, CompactSimilarProducts, PCompanionInference, SimilarProducts
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
    model = PCompanion(cfg, g["features"])                 # the product table IS the feature tensor
    full = PCompanionInference(model, cfg, bpg).set_exclusions()
    cc = ops.CompactCatalogue(g["features"])
    rowptr, col, t32, t16 = full.type_rowptr, full.type_col, full.features, cc.table
    q = torch.from_numpy(np.random.default_rng(1).integers(0, P, args.batch).astype(np.int32)).to(dev)
    with torch.no_grad():
        fwd = full.model({"query_idx": q, "query_types": full.type_idx[q.long()]})
    proj = fwd["projected_embeddings"].contiguous().reshape(-1, d)
    types = fwd["complementary_types"].to(torch.int32).reshape(-1).contiguous()
    rows = int(types.numel())
    out["rows"] = rows
    # a product of the row's type, drawn uniformly
    size = (rowptr[1:] - rowptr[:-1])[types.long()].long()
    draw = torch.from_numpy(np.random.default_rng(2).integers(0, 2 ** 31, rows)).to(dev)
    targets = col[(rowptr[types.long()].long() + draw % size.clamp(min=1)).clamp(max=col.numel() - 1)].contiguous()
    exclude = (q.repeat_interleave(3).contiguous(),) + full.exclusions
    ct = full.cand_type
    b32, b16 = ops.half_sq_norm_bias(t32), cc.half_sq_norm
    rk16 = lambda **kw: ops.rank_grouped_bf16(proj, types, targets, rowptr, col, t16, **kw)
    rk32 = lambda **kw: ops.rank_grouped(proj, types, targets, rowptr, col, t32, **kw)
    fns = {"rank_grouped_plain_bf16": rk16, "rank_grouped_plain_fp32": rk32,
           "rank_grouped_excluding_bf16": lambda: rk16(exclude=exclude, cand_type=ct),
           "rank_grouped_excluding_fp32": lambda: rk32(exclude=exclude, cand_type=ct),
           "rank_grouped_biased_bf16": lambda: rk16(bias=b16), "rank_grouped_biased_fp32": lambda: rk32(bias=b32)}
    for n in LIST_NS:
        fns[f"retrieve_list_grouped_biased_{n}_bf16"] = (lambda n=n: ops.retrieve_list_grouped_bf16_biased(proj, types, rowptr, col, t16, b16, n))
        fns[f"retrieve_list_grouped_biased_{n}_fp32"] = (lambda n=n: ops.retrieve_list_grouped_biased(proj, types, rowptr, col, t32, b32, n))
    # the substitute classes; the compact one over a graph without features
    arrays = dict(bpg.arrays) if isinstance(bpg, DeviceBPG) else dict(g, max_degree=int(np.diff(bpg.cv_rowptr).max()))
    arrays.pop("features")
    bare = DeviceBPG(arrays, T, d)
    sp16 = CompactSimilarProducts(cc, bare)
    # the evaluating object over the bf16 copy, beside the fp32 one: both with the co-view exclusions installed
    compact = CompactInference(model, cfg, bare, catalogue=cc).set_exclusions()
    assert compact.features is None and "features" not in compact._graph
    qt = targets.reshape(-1, 3)[:, 0].contiguous()
    fns["rank_targets_compact"] = lambda: compact.rank_targets(q, qt)
    fns["rank_targets_fp32"] = lambda: full.rank_targets(q, qt)
    sp32 = SimilarProducts(t32, bpg)
    for what, call in (("similar_batch_10", lambda sp: sp.similar_batch(q, 10)), ("similar_list_batch_64", lambda sp: sp.similar_list_batch(q, 64))):
        fns[f"{what}_compact"] = (lambda call=call: call(sp16))
        fns[f"{what}_fp32"] = (lambda call=call: call(sp32))
    t = alternating(fns, args.warmup, args.reps)
    out.update(t)
    pairs = sorted({k.rsplit("_", 1)[0] for k in fns})
    out["bf16_over_fp32"] = {k: t[k + ("_bf16" if k + "_bf16" in t else "_compact")]["median_ms"] / t[k + "_fp32"]["median_ms"]
                             for k in pairs}
    # the answers at the timed size
    agree = {}
    for kind, kw, lst in (("plain", {}, lambda: ops.retrieve_list_grouped(proj, types, rowptr, col, t16, 256)),
                          ("biased", {"bias": b16}, lambda: ops.retrieve_list_grouped_bf16_biased(proj, types, rowptr, col, t16, b16, 256))):
        r16, _ = rk16(**kw)
        served, _ = lst()
        at = torch.gather(served, 1, r16.clamp(0, 255).long()[:, None])[:, 0]
        inside = (r16 >= 0) & (r16 < 256)
        agree[kind] = {"rank_below_256_iff_the_list_holds_the_target_there":
                       bool((at[inside] == targets[inside]).all() and not (served[~inside] == targets[~inside][:, None]).any()),
                       "same_ranks_for_one_slice": bool(torch.equal(rk16(slices=1, **kw)[0], r16)),
                       "rows_ranked_below_256": int(inside.sum()),
                       "share_of_rows_whose_rank_differs_from_fp32": float((r16 != rk32(**({"bias": b32} if kw else {}))[0]).float().mean())}
    out["agreement"] = agree
    ex = nbytes(*sp32.exclusions)
    held = lambda inf, table: nbytes(table, inf.type_idx, inf.type_rowptr, inf.type_col, *inf.exclusions)
    slot16, rank16 = compact.rank_targets(q, qt)
    direct, _ = ops.rank_grouped_bf16(proj.reshape(-1, 3, d)[torch.arange(len(q), device=dev), slot16.clamp(min=0).long()].contiguous(),
                                      torch.where(slot16 >= 0, types.reshape(-1, 3)[torch.arange(len(q), device=dev), slot16.clamp(min=0).long()],
                                                  torch.full_like(slot16, -1)).contiguous(),
                                      qt, rowptr, col, t16, exclude=(q,) + compact.exclusions, cand_type=compact.cand_type)
    agree["compact_inference"] = {"rank_targets_is_rank_grouped_bf16_on_the_matched_slot": bool(torch.equal(rank16, direct)),
                                  "pairs_with_a_slot": int((slot16 >= 0).sum())}
    out["memory"] = {"compact_similar_products_resident_bytes": nbytes(t16, b16, sp16.type_idx, *sp16._all_products) + ex,
                     "similar_products_resident_bytes": nbytes(t32, b32, sp32.type_idx, *sp32._all_products) + ex,
                     "compact_inference_resident_bytes": held(compact, compact.catalogue),
                     "fp32_inference_resident_bytes": held(full, full.features),
                     "table_bytes": {"bf16": nbytes(t16), "fp32": nbytes(t32)},
                     "note": "resident: the tensors each built object holds for serving and ranking -- the table, the bias (the "
                             "substitute classes), type_idx, the type CSR and the object's exclusion CSR (the query itself for the "
                             "substitute classes, the co-view lists and the query for the inference objects); the model and the "
                             "graph's other arrays are the same in both and not counted"}
    del full, compact, cc, g, bpg, proj, types, fwd, model, sp16, sp32
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="100k,10M")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "compact_rank_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("compact_rank_probe: no GPU (nothing here is measured on the CPU)")
    dev = torch.device("cuda")
    res = {"probe": "compact_rank", "device": torch.cuda.get_device_name(0), "legs": {}}
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
