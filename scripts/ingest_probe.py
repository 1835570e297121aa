"""Developer tool: what building a DeviceBPG from behaviour edge lists costs (ops.build_catalogue, csrc/ingest.hip), beside
the same result formed with torch's device sort -- torch.unique over (source, target) pairs as one int64 each, the technique
ops.exclusion_csr uses -- in the same process.

  100 k / 10 M products; edge lists drawn ON THE DEVICE under a fixed seed:
    co_view               16 P uniform edges + 10 % of them given twice + four hub sources with P / 50 raw edges each
    purchase_after_view   every fifth co_view edge + P uniform edges
    co_purchase           every 33rd co_view edge + 4.5 P uniform edges
  degree_cap = 32.

Per leg and per formulation: seconds from host clocks around a synchronised call (`--warmup` untimed calls, then `--reps`;
the build reads totals back, so it is not a pure device interval), and the peak of torch's allocator ABOVE the resident edge
lists during one call.  The two results are compared array for array.  A formulation that does not fit is recorded as such
instead of a time.  Writes profiles/ingest_probe.json (or --out) and prints the same JSON as one line.

  python scripts/ingest_probe.py [--legs 100k,10M] [--warmup 1] [--reps 3] [--out FILE]
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

LEGS = {"100k": 100_000, "10M": 10_000_000}
CAP = 32


def draw(P, dev):
    g = torch.Generator(device=dev).manual_seed(P)
    edges = lambda n: torch.randint(0, P, (n, 2), generator=g, device=dev, dtype=torch.int32)
    cv = edges(16 * P)
    hubs = []
    for s in torch.randint(0, P, (4,), generator=g, device=dev).tolist():
        h = edges(P // 50)
        h[:, 0] = s
        hubs.append(h)
    cv = torch.cat([cv, cv[::10]] + hubs)
    cv = cv[torch.randperm(cv.shape[0], generator=g, device=dev)].contiguous()
    pv = torch.cat([cv[::5], edges(P)]).contiguous()
    cp = torch.cat([cv[::33], edges(9 * P // 2)]).contiguous()
    return cv, pv, cp


def torch_formulation(P, cv, pv, cp, cap):
    """The dict of ops.build_catalogue through torch.unique / sort / isin over int64 keys."""
    def keys(e):
        e = e[e[:, 0] != e[:, 1]].long()
        return e[:, 0] * P + e[:, 1]
    ck, w = torch.unique(keys(cv), return_counts=True)                      # sorted by (s, t)
    pk, qk = torch.unique(keys(pv)), torch.unique(keys(cp))
    s = ck // P
    o1 = torch.sort(-w, stable=True).indices                                 # weight descending, ids ascending inside
    o2 = torch.sort(s[o1], stable=True).indices                              # ... per source
    order = o1[o2]
    start = torch.searchsorted(s, s[order])
    keep = torch.zeros_like(ck, dtype=torch.bool)
    keep[order[torch.arange(ck.numel(), device=ck.device) - start < cap]] = True
    kept = ck[keep]
    sim = kept[torch.isin(kept, pk, assume_unique=True) & ~torch.isin(kept, qk, assume_unique=True)]
    comp = qk[~torch.isin(qk, pk, assume_unique=True) & ~torch.isin(qk, ck, assume_unique=True)]

    def rowptr(k):
        r = torch.zeros(P + 1, dtype=torch.int32, device=k.device)
        r[1:] = torch.cumsum(torch.bincount(k // P, minlength=P), 0).to(torch.int32)
        return r
    pairs = lambda k: torch.stack([k // P, k % P], 1).to(torch.int32)
    cv_rowptr = rowptr(kept)
    deg = cv_rowptr[1:] - cv_rowptr[:-1]
    return dict(cv_rowptr=cv_rowptr, cv_col=(kept % P).to(torch.int32), sim_rowptr=rowptr(sim), sim_pairs=pairs(sim),
                sim_col=(sim % P).to(torch.int32), pair_deg=deg[(sim // P)], comp_pairs=pairs(comp), max_degree=int(deg.max()))


def timed(fn, warmup, reps):
    """({median_s, min_s, max_s, reps, peak_bytes_above_inputs}, last result) or ({"does_not_fit": message}, None)."""
    try:
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        s = []
        for _ in range(reps):
            del out
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            s.append(time.perf_counter() - t0)
        return {"median_s": float(np.median(s)), "min_s": float(min(s)), "max_s": float(max(s)), "reps": reps,
                "peak_bytes_above_inputs": int(peak)}, out
    except torch.OutOfMemoryError as e:
        torch.cuda.empty_cache()
        return {"does_not_fit": str(e).splitlines()[0][:200]}, None


def leg(P, args, dev):
    from p_companion_amd import ops
    cv, pv, cp = draw(P, dev)
    types = (torch.arange(P, device=dev, dtype=torch.int32) % 100).contiguous()
    torch.cuda.synchronize()
    out = {"products": P, "degree_cap": CAP, "edges": {"co_view": cv.shape[0], "purchase_after_view": pv.shape[0],
                                                       "co_purchase": cp.shape[0]},
           "input_bytes": int(8 * (cv.shape[0] + pv.shape[0] + cp.shape[0]))}
    out["build_catalogue"], a = timed(lambda: ops.build_catalogue(types, cv, pv, cp, degree_cap=CAP, n_types=100), args.warmup,
                                      args.reps)
    out["torch_unique"], b = timed(lambda: torch_formulation(P, cv, pv, cp, CAP), args.warmup, args.reps)
    if a is not None:
        out["result"] = {"co_view_edges_kept": int(a["cv_col"].numel()), "similarity_pairs": int(a["sim_pairs"].shape[0]),
                         "complementary_pairs": int(a["comp_pairs"].shape[0]), "max_degree": a["max_degree"]}
    if a is not None and b is not None:
        out["agreement"] = {k: bool(torch.equal(a[k], v) if torch.is_tensor(v) else a[k] == v) for k, v in b.items()}
        out["torch_over_build"] = out["torch_unique"]["median_s"] / out["build_catalogue"]["median_s"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="100k,10M")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ingest_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ingest_probe: no GPU (nothing here is measured on the CPU)")
    dev = torch.device("cuda")
    res = {"probe": "ingest", "device": torch.cuda.get_device_name(0), "legs": {}}
    for name in [s for s in args.legs.split(",") if s]:
        res["legs"][name] = leg(LEGS[name], args, dev)
        torch.cuda.empty_cache()
    for name in LEGS:
        res["legs"].setdefault(name, "not measured")
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
