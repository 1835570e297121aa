"""Developer tool: time of the device-CSR embedding export (Product2Vec.generate_all_embeddings over a DeviceBPG,
pc_p2v_export_embeddings) and its roofline.  Prints ONE JSON line.

  100 k products (generate_scaled_bpg, uploaded): the device-CSR export and, for comparison, the host-CSR path
           (generate_embedding_table with numpy rowptr / col: host grouping by degree, a launch sequence per degree);
           the largest difference between the two tables and whether they are bit-equal;
  10 M products (generate_device_bpg, degree cap 32: BASELINE configs[3]): the device-CSR export.

ms per export from device events around `--reps` exports after `--warmup` untimed ones (median and min).  FLOPs and bytes
are computed from shapes: both FFN passes 2 (D H + H H + H D) per product each, the attention projections 8 D^2 per
product with neighbours (q, qt = Wk_h^T q_h, ctx, out), the core 4 HEADS D per edge (scores, weighted sums); bytes: the
feature table read, e1 written and read back, the output written, one read of every neighbour row (deg D 4 per product)
and the CSR.  Share of peak = the larger of FLOPs / 157.3 TF (fp32) and bytes / 8.0 TB/s (HBM, spec) over the measured time.

  python scripts/export_probe.py [--sizes 100000,10000000] [--warmup 2] [--reps 5] [--no-host]
Per-kernel times: the same command under rocprofv3 --kernel-trace --stats (e.g. --sizes 10000000 --reps 2 --no-host).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from types import SimpleNamespace

import numpy as np
import torch

PEAK_FP32 = 157.3e12
PEAK_HBM = 8.0e12
H, HEADS = 256, 4


def model(d, dev):
    from p_companion_amd.product2vec import Product2Vec
    cfg = SimpleNamespace(PRODUCT_EMB_DIM=d, TYPE_EMB_DIM=64, HIDDEN_SIZE=H, NUM_ATTENTION_HEADS=HEADS, DROPOUT=0.0,
                          MARGIN=1.0, LEARNING_RATE=1e-3, DEVICE=dev)
    torch.manual_seed(0)
    m = Product2Vec(cfg).to(dev).eval()
    with torch.no_grad():                         # eval-mode BatchNorm with non-trivial running statistics
        m.ffn[1].running_mean.normal_(0.0, 0.1)
        m.ffn[1].running_var.uniform_(0.5, 1.5)
    return m


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": float(np.median(ms)), "min_ms": float(min(ms)), "reps": reps}


def roofline(P, E, n_att, d, ms):
    ffn = 2.0 * (d * H + H * H + H * d)
    flops = 2 * P * ffn + n_att * 8.0 * d * d + E * 4.0 * HEADS * d
    nbytes = 4.0 * (4 * P * d + E * d + P + 1 + E)
    t_f, t_b = flops / PEAK_FP32, nbytes / PEAK_HBM
    s = ms * 1e-3
    return {"gflop": flops / 1e9, "gbytes": nbytes / 1e9, "tflops": flops / s / 1e12, "tbps": nbytes / s / 1e12,
            "bound": "compute (fp32)" if t_f >= t_b else "memory (HBM)", "share_of_peak": max(t_f, t_b) / s}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,10000000")
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip the host-CSR comparison at 100 k")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("export_probe: no GPU (nothing here is measured on the CPU)")
    from p_companion_amd.data import generate_device_bpg, generate_scaled_bpg
    dev = torch.device("cuda")
    d = args.dim
    m = model(d, dev)
    res = {"probe": "p2v_export", "dim": d, "device": torch.cuda.get_device_name(0), "sizes": {}}
    for P in (int(s) for s in args.sizes.split(",")):
        if P <= 1_000_000:
            bpg = generate_scaled_bpg(P, dim=d, seed=0)
            g = bpg.cuda(dev)
            host_csr = (bpg.cv_rowptr, bpg.cv_col)
            src = "generate_scaled_bpg"
        else:
            bpg = generate_device_bpg(P, 100, seed=0, degree_cap=32, dim=d, world=1, with_complementary=False)
            g = bpg.cuda()
            host_csr = None
            src = "generate_device_bpg(degree_cap=32)"
        feats, rowptr, col = g["features"], g["cv_rowptr"], g["cv_col"]
        E = int(col.numel())
        n_att = int((rowptr[1:] != rowptr[:-1]).sum())
        out = {"source": src, "products": P, "edges": E, "products_with_neighbours": n_att}
        t = timed(lambda: m.generate_embedding_table(feats, rowptr, col), args.warmup, args.reps)
        out["device_csr"] = {**t, **roofline(P, E, n_att, d, t["median_ms"])}
        if host_csr is not None and not args.no_host:
            t = timed(lambda: m.generate_embedding_table(feats, *host_csr), args.warmup, args.reps)
            out["host_csr"] = {**t, **roofline(P, E, n_att, d, t["median_ms"])}
            a = m.generate_embedding_table(feats, rowptr, col).clone()
            b = m.generate_embedding_table(feats, *host_csr)
            out["device_vs_host_max_abs_diff"] = float((a - b).abs().max())
            out["device_vs_host_bit_equal"] = bool(torch.equal(a, b))
        res["sizes"][str(P)] = out
        del bpg, g, feats, rowptr, col
        m.last_embedding_table = None
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
