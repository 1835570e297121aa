"""Developer tool: what deriving the behaviour edge lists from a shopper event log costs on the device (ops.event_edges,
csrc/events.hip) and what a DeviceBPG from the log costs end to end (data.device_bpg_from_events), beside a plain-torch
formulation of the same contract -- bincount, torch.unique over (session, product) as one int64 each, scatter_reduce for the
first view / last purchase, and every ordered pair of a session's items formed with repeat_interleave -- in the same process.

  100 k products / about 3 M rows and 10 M products / about 100 M rows (--rows), drawn ON THE DEVICE under a fixed seed:
    session lengths   geometric, mean 5 (sessions = rows / 5)
    products          Zipf-like: floor(P ** u) - 1, u uniform
    kind              purchase with probability 0.15
    time              uniform in [0, 3600)
  rows shuffled; max_events = 256, exclusive, degree_cap = 32.

Per leg and per formulation: seconds from a host clock around a call that ends in a synchronise (`--warmup` untimed calls,
then the median of `--reps`), and the peak of torch's allocator during one call above the resident log and above the lists
the call returns.  At the small size the two formulations' lists are asserted equal; at every size they are compared.  A
formulation that does not fit is recorded as such instead of a time.  Writes profiles/events_probe.json (or --out) and prints
the same JSON as one line.

  python scripts/events_probe.py [--legs 100k,10M] [--rows 3000000,100000000] [--warmup 1] [--reps 5] [--out FILE]
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
MAX_EVENTS, CAP, MEAN_LENGTH = 256, 32, 5


def draw(P, rows, dev):
    """(events int32 [N, 4] shuffled, n_sessions): N is about `rows`.  The columns are drawn, shuffled and stored one by one
    (1-D tensors only), and the stored log is checked against the ranges it was drawn from."""
    g = torch.Generator(device=dev).manual_seed(P)
    S = rows // MEAN_LENGTH
    length = torch.empty(S, device=dev).geometric_(1.0 / MEAN_LENGTH, generator=g).long()
    session = torch.repeat_interleave(torch.arange(S, device=dev, dtype=torch.int32), length)
    N = session.numel()
    perm = torch.randperm(N, device=dev, generator=g)
    ev = torch.empty(N, 4, dtype=torch.int32, device=dev)
    ev[:, 0] = session[perm]
    del session, length
    u = torch.rand(N, device=dev, dtype=torch.float64, generator=g)
    ev[:, 1] = (torch.pow(float(P), u).long() - 1).clamp_(0, P - 1).to(torch.int32)
    del u
    ev[:, 2] = (torch.rand(N, device=dev, generator=g) < 0.15).to(torch.int32)
    ev[:, 3] = torch.randint(0, 3600, (N,), device=dev, generator=g, dtype=torch.int32)
    del perm
    lo, hi = ev.amin(0).tolist(), ev.amax(0).tolist()
    print(f"[events_probe] drawn log: column minima {lo}, maxima {hi}", file=sys.stderr, flush=True)
    assert lo == [0, 0, 0, 0] and hi[0] == S - 1 and hi[1] < P and hi[2] == 1 and hi[3] < 3600, (lo, hi, S, P)
    return ev, S


def torch_formulation(ev, P, S, max_events=MAX_EVENTS, exclusive=True):
    """(co_view, purchase_after_view, co_purchase, skipped_sessions, n_items) of ops.event_edges through plain torch."""
    s, p, kind, t = (ev[:, k].long() for k in range(4))
    if bool(((s < 0) | (s >= S) | (p < 0) | (p >= P) | (kind < 0) | (kind > 1) | (t < 0)).any()):
        raise ValueError("a field out of range")
    rows = torch.bincount(s, minlength=S)
    keep = rows[s] <= max_events
    s, p, kind, t = s[keep], p[keep], kind[keep], t[keep]
    key, inv = torch.unique(s * P + p, return_inverse=True)               # the items, ascending by (session, product)
    I = key.numel()
    big = 2 ** 31
    fv = torch.full((I,), big, dtype=torch.int64, device=ev.device).scatter_reduce_(0, inv[kind == 0], t[kind == 0], "amin")
    fv[fv == big] = -1
    lp = torch.full((I,), -1, dtype=torch.int64, device=ev.device).scatter_reduce_(0, inv[kind == 1], t[kind == 1], "amax")
    item_s, item_p = key // P, (key % P).to(torch.int32)
    del s, p, kind, t, inv, key, keep
    m = torch.bincount(item_s, minlength=S)
    start = torch.cumsum(m, 0) - m
    per_a = m[item_s]
    a = torch.repeat_interleave(torch.arange(I, device=ev.device), per_a)
    b = start[item_s[a]] + torch.arange(a.numel(), device=ev.device) - torch.repeat_interleave(torch.cumsum(per_a, 0) - per_a, per_a)
    other = a != b
    a, b = a[other], b[other]
    va, ua, vb, ub = fv[a] >= 0, lp[a] >= 0, fv[b] >= 0, lp[b] >= 0
    both = ua & ub
    cv = va & vb & ~both if exclusive else va & vb
    pv = va & ub & (fv[a] <= lp[b])
    if exclusive:
        pv &= ~ua
    pairs = lambda mask: torch.stack([item_p[a[mask]], item_p[b[mask]]], 1)
    return pairs(cv), pairs(pv), pairs(both), int((rows > max_events).sum()), I


def timed(fn, warmup, reps, lists_of):
    """({median_s, every_s, reps, peak_bytes_above_log, peak_bytes_above_log_and_outputs}, last result) or
    ({"does_not_fit": message}, None)."""
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
        held = sum(int(x.numel() * x.element_size()) for x in lists_of(out))
        s = []
        for _ in range(reps):
            del out
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            s.append(time.perf_counter() - t0)
        return {"median_s": float(np.median(s)), "every_s": [float(x) for x in s], "reps": reps, "peak_bytes_above_log": int(peak),
                "peak_bytes_above_log_and_outputs": int(peak - held), "output_bytes": held}, out
    except torch.OutOfMemoryError as e:
        torch.cuda.empty_cache()
        return {"does_not_fit": str(e).splitlines()[0][:200]}, None


def leg(name, P, rows, args, dev):
    from p_companion_amd import ops
    from p_companion_amd.data import device_bpg_from_events
    ev, S = draw(P, rows, dev)
    types = (torch.arange(P, device=dev, dtype=torch.int32) % 100).contiguous()
    torch.cuda.synchronize()
    out = {"products": P, "rows": int(ev.shape[0]), "sessions": S, "max_events": MAX_EVENTS, "exclusive": True, "degree_cap": CAP,
           "log_bytes": int(ev.numel() * 4)}
    print(f"[events_probe] {name}: {out['rows']} rows, {S} sessions", file=sys.stderr, flush=True)
    out["event_edges"], a = timed(lambda: ops.event_edges(ev, P, S, max_events=MAX_EVENTS), args.warmup, args.reps, lambda e: e[:3])
    print(f"[events_probe] {name}: event_edges {out['event_edges']}", file=sys.stderr, flush=True)
    if a is not None:
        out["result"] = {"co_view": int(a.co_view.shape[0]), "purchase_after_view": int(a.purchase_after_view.shape[0]),
                         "co_purchase": int(a.co_purchase.shape[0]), "skipped_sessions": a.skipped_sessions, "n_items": a.n_items}
    out["torch"], b = timed(lambda: torch_formulation(ev, P, S), args.warmup, args.reps, lambda e: e[:3])
    print(f"[events_probe] {name}: torch {out['torch']}", file=sys.stderr, flush=True)
    if a is not None and b is not None:
        out["agreement"] = {n: bool(torch.equal(x, y)) for n, x, y in zip(ops.INGEST_LISTS, a[:3], b[:3])}
        out["agreement"]["stats"] = (a.skipped_sessions, a.n_items) == b[3:]
        if name == "100k":
            assert all(out["agreement"].values()), out["agreement"]
        out["torch_over_event_edges"] = out["torch"]["median_s"] / out["event_edges"]["median_s"]
    del a, b
    torch.cuda.empty_cache()
    graph_tensors = lambda g: [v for v in g.arrays.values() if torch.is_tensor(v) and v is not types]
    out["device_bpg_from_events"], g = timed(lambda: device_bpg_from_events(None, types, 100, ev, n_sessions=S, degree_cap=CAP,
                                                                            max_events=MAX_EVENTS), args.warmup, args.reps,
                                             graph_tensors)
    print(f"[events_probe] {name}: device_bpg_from_events {out['device_bpg_from_events']}", file=sys.stderr, flush=True)
    if g is not None:
        out["graph"] = {"co_view_edges_kept": int(g.arrays["cv_col"].numel()), "similarity_pairs": g.n_similarity_pairs,
                        "complementary_pairs": int(g.arrays["comp_pairs"].shape[0]), "max_degree": g.max_degree}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="100k,10M")
    ap.add_argument("--rows", default="3000000,100000000", help="rows of the 100k and of the 10M leg")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "events_probe.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("events_probe: no GPU (nothing here is measured on the CPU)")
    dev = torch.device("cuda")
    rows = dict(zip(LEGS, (int(x) for x in args.rows.split(","))))
    res = {"probe": "events", "device": torch.cuda.get_device_name(0), "legs": {}}
    for name in [s for s in args.legs.split(",") if s]:
        res["legs"][name] = leg(name, LEGS[name], rows[name], args, dev)
        torch.cuda.empty_cache()
    for name in LEGS:
        res["legs"].setdefault(name, "not measured")
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
