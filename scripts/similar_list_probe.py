"""Developer tool: what a long substitute list costs (pc_retrieve_list_grouped_biased, up to 256 products per (query, type)
under the score <q, e_p> + bias[p]) and what SimilarProducts serves it in.  On the SAME rows and catalogue, alternating in one
process, on one MI355X:

  retrieve_topk_grouped(bias=, 16)                  the existing biased entry at its limit
  retrieve_list_grouped(n), n = 16 / 64 / 128 / 256 the unbiased list entry: THE YARDSTICK of the line below at the same n
  retrieve_list_grouped_biased(n), the same n       the new entry (the same kernel body; a 4-byte gather per candidate column
                                                    and one addition more)
  peeled(64)                                        what a caller had to do before: four calls of the 16-entry biased entry,
                                                    each excluding what the earlier ones served; building the growing set is
                                                    part of the leg

  100 k / 100 types, 10 M / 100 types   generate_device_bpg; 12 288 rows: queries drawn from the catalogue, each against its own
                                        type, the query's table row as the projected embedding, bias = half_sq_norm_bias(table)

  methods   SimilarProducts.similar_list_batch(64 / 256) and similar_capped_list_batch(10, pool = 64 / 256, group = id // 4) at
            B = 4096 for scope "type" and scope "catalogue", beside similar_batch(16) / similar_capped_batch(10) (pool 16)
  indexed   IndexedSimilarProducts (256 cells at 100 k, 4096 at 10 M, as similar_index_probe.py; nprobe 8):
            similar_list_batch(64 / 256) and the capped lists beside similar_batch(16), and the recall of the long lists
  short     a varianted table (--variant-products rows: centres repeated 4 times plus 1e-3 noise, group = id // 4): the share of
            the B queries whose capped list of 10 comes back short from a pool of 16 / 64 / 256

ms from device events: `--warmup` untimed rounds, then `--reps` rounds, each round one call of every leg in turn; medians with
min .. max.  The answers are compared at the timed size: the biased list at 16 is the 16-entry's bit for bit, at 64 the peeled
lists', with a zero bias the unbiased list's.  Writes profiles/similar_list_probe.json (or --out) and prints the same JSON as one
line.

  python scripts/similar_list_probe.py [--legs 100k,10M] [--warmup 3] [--reps 10] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from long_list_probe import alternating

LEGS = {"100k": (100_000, 100, 128, 256), "10M": (10_000_000, 100, 128, 4096)}      # products, types, D, cells of the index
NS = (16, 64, 128, 256)
N_PEEL = 64
POOLS = (64, 256)


def same(a, b):
    return bool(torch.equal(a[0], b[0]) and torch.equal(a[1].contiguous().view(torch.int32), b[1].contiguous().view(torch.int32)))


def entries(g, P, T, args, dev):
    """The entries alone, on 12 288 rows."""
    from p_companion_amd import ops
    table = g["features"]
    rowptr, col = ops.type_csr(g["type_idx"], T)
    bias = ops.half_sq_norm_bias(table)
    q = torch.from_numpy(np.random.default_rng(1).integers(0, P, args.rows).astype(np.int32)).to(dev)
    proj = table[q.long()].contiguous()
    types = g["type_idx"][q.long()].contiguous()
    rows = args.rows
    row_key = torch.arange(rows, dtype=torch.int32, device=dev)

    def peeled(n=N_PEEL):
        idx, sc = [], []
        for step in range((n + 15) // 16):
            exclude = None
            if step:
                served = torch.cat(idx, 1).contiguous()
                rp = (torch.arange(rows + 1, device=dev) * served.shape[1]).to(torch.int32)
                exclude = (row_key,) + ops.exclusion_csr(rp, served.reshape(-1), include_self=False, num_products=P)
            i, s = ops.retrieve_topk_grouped(proj, types, rowptr, col, table, 16, exclude=exclude, bias=bias)
            idx.append(i)
            sc.append(s)
        return torch.cat(idx, 1)[:, :n], torch.cat(sc, 1)[:, :n]

    fns = {"retrieve_topk_grouped_biased_16": lambda: ops.retrieve_topk_grouped(proj, types, rowptr, col, table, 16, bias=bias)}
    for n in NS:
        fns[f"retrieve_list_grouped_{n}"] = (lambda n=n: ops.retrieve_list_grouped(proj, types, rowptr, col, table, n))
        fns[f"retrieve_list_grouped_biased_{n}"] = (lambda n=n: ops.retrieve_list_grouped_biased(proj, types, rowptr, col, table,
                                                                                                 bias, n))
    fns[f"peeled_biased_{N_PEEL}"] = peeled
    t = alternating(fns, args.warmup, args.reps)
    out = {"rows": rows, **t}
    med = lambda k: t[k]["median_ms"]
    out["biased_over_unbiased_list"] = {str(n): med(f"retrieve_list_grouped_biased_{n}") / med(f"retrieve_list_grouped_{n}") for n in NS}
    out["biased_list_16_over_biased_topk_16"] = med("retrieve_list_grouped_biased_16") / med("retrieve_topk_grouped_biased_16")
    out[f"peeled_{N_PEEL}_over_biased_list_{N_PEEL}"] = med(f"peeled_biased_{N_PEEL}") / med(f"retrieve_list_grouped_biased_{N_PEEL}")
    zero = torch.zeros_like(bias)
    b64 = fns[f"retrieve_list_grouped_biased_{N_PEEL}"]()
    b256 = fns["retrieve_list_grouped_biased_256"]()
    out["agreement"] = {
        "biased_list_16_is_biased_topk_16": same(fns["retrieve_list_grouped_biased_16"](), fns["retrieve_topk_grouped_biased_16"]()),
        f"biased_list_{N_PEEL}_is_peeled_{N_PEEL}": same(b64, peeled()),
        "zero_bias_list_256_is_unbiased_list_256": same(ops.retrieve_list_grouped_biased(proj, types, rowptr, col, table, zero, 256),
                                                        fns["retrieve_list_grouped_256"]()),
        "biased_list_256_starts_with_biased_list_64": bool(torch.equal(b256[0][:, :N_PEEL], b64[0])),
        "entries_served_at_256": int((b256[0] >= 0).sum())}
    return out, q


def methods(g, bpg, q, cells, args, dev):
    """The serving methods at B = 4096, both scopes, and the indexed form."""
    from p_companion_amd.inference import IndexedSimilarProducts, SimilarProducts
    table = g["features"]
    P = table.shape[0]
    qb = q[:args.batch].contiguous()
    group = (torch.arange(P, dtype=torch.int32, device=dev) // 4).contiguous()
    out = {"B": args.batch, "group": "id // 4", "n_capped": 10}
    for scope in ("type", "catalogue"):
        sp = SimilarProducts(table, bpg, scope=scope)
        fns = {"similar_batch_16": lambda: sp.similar_batch(qb, 16),
               "similar_capped_batch_10_pool_16": lambda: sp.similar_capped_batch(qb, 10, group=group)}
        for m in POOLS:
            fns[f"similar_list_batch_{m}"] = (lambda m=m: sp.similar_list_batch(qb, m))
            fns[f"similar_capped_list_batch_10_pool_{m}"] = (lambda m=m: sp.similar_capped_list_batch(qb, 10, group=group, pool=m))
        out[scope] = alternating(fns, args.method_warmup, args.method_reps)
        del sp, fns
        torch.cuda.empty_cache()
    t0 = time.time()
    isp = IndexedSimilarProducts(table, bpg, n_cells=cells, nprobe=8, iters=args.iters, seed=0)
    torch.cuda.synchronize()
    fns = {"similar_batch_16": lambda: isp.similar_batch(qb, 16)}
    for m in POOLS:
        fns[f"similar_list_batch_{m}"] = (lambda m=m: isp.similar_list_batch(qb, m))
        fns[f"similar_capped_list_batch_10_pool_{m}"] = (lambda m=m: isp.similar_capped_list_batch(qb, 10, group=group, pool=m))
    out["indexed"] = {"n_cells": cells, "nprobe": 8, "kmeans_iters": args.iters, "build_s": round(time.time() - t0, 2),
                      **alternating(fns, args.method_warmup, args.method_reps)}
    for m in POOLS:
        exact = SimilarProducts.similar_list_batch(isp, qb, m)[0]
        got = isp.similar_list_batch(qb, m)[0]
        held = ((exact[:, :, None] == got[:, None, :]) & (exact[:, :, None] >= 0)).any(dim=2).sum()
        out["indexed"][f"recall_at_{m}"] = float(held) / max(int((exact >= 0).sum()), 1)
    del isp, fns
    torch.cuda.empty_cache()
    return out


def short_lists(args, dev):
    """The share of short capped lists on a varianted table: every product in four variants, group = id // 4."""
    from p_companion_amd.data import generate_device_bpg
    from p_companion_amd.inference import SimilarProducts
    P, d = args.variant_products, 128
    bpg = generate_device_bpg(P, 100, seed=3, dim=d, world=1, with_complementary=False)
    gen = torch.Generator(device=dev).manual_seed(9)
    centres = torch.randn(P // 4, d, generator=gen, device=dev)
    table = (centres.repeat_interleave(4, dim=0) + 1e-3 * torch.randn(P, d, generator=gen, device=dev)).contiguous()
    del centres
    group = (torch.arange(P, dtype=torch.int32, device=dev) // 4).contiguous()
    q = torch.from_numpy(np.random.default_rng(2).integers(0, P, args.batch).astype(np.int32)).to(dev)
    out = {"products": P, "variants_per_product": 4, "noise": 1e-3, "B": args.batch, "n": 10, "cap": 1}
    for scope in ("type", "catalogue"):
        sp = SimilarProducts(table, bpg, scope=scope)
        idx = {16: sp.similar_capped_batch(q, 10, group=group)[0]}
        for m in POOLS:
            idx[m] = sp.similar_capped_list_batch(q, 10, group=group, pool=m)[0]
        out[scope] = {f"pool_{m}": {"short_share": float(((i >= 0).sum(1) < 10).float().mean()),
                                    "mean_length": float((i >= 0).sum(1).float().mean())} for m, i in idx.items()}
        del sp
    return out


def leg(name, args, dev):
    from p_companion_amd.data import generate_device_bpg
    P, T, d, cells = LEGS[name]
    t0 = time.time()
    bpg = generate_device_bpg(P, T, seed=0, dim=d, world=1, with_complementary=False)
    g = bpg.cuda(dev)
    torch.cuda.synchronize()
    out = {"source": "generate_device_bpg", "products": P, "types": T, "dim": d, "generate_s": round(time.time() - t0, 2)}
    out["entries"], q = entries(g, P, T, args, dev)
    out["methods"] = methods(g, bpg, q, cells, args, dev)
    del g, bpg
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="100k,10M")
    ap.add_argument("--rows", type=int, default=12288)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--method-warmup", type=int, default=1)
    ap.add_argument("--method-reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--variant-products", type=int, default=100_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "similar_list_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("similar_list_probe: no GPU (nothing here is measured on the CPU)")
    dev = torch.device("cuda")
    res = {"probe": "similar_list", "device": torch.cuda.get_device_name(0),
           "timing": "device events; every round runs each leg of a group once, in turn; median (min .. max) in ms per call",
           "yardstick": "retrieve_list_grouped_N (the unbiased list entry) beside retrieve_list_grouped_biased_N, same rows and process",
           "legs": {}}
    for name in [s for s in args.legs.split(",") if s]:
        res["legs"][name] = leg(name, args, dev)
    for name in LEGS:
        res["legs"].setdefault(name, "not measured")
    res["short_lists"] = short_lists(args, dev)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
