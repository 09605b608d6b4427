"""Gram / history-fold kernel rates on the GPU.

Times dls_rows_gram_f32, dls_history_gram_f32 and, for comparison,
dls_pairwise_sqdist_f32 from the same build on K = 10 and K = 64 rows of the
ResNet-18 flat size (11,173,962 parameters, rounded up to the store's pitch): HIP event
timing per launch pair (the kernel and its finish launch) over --repeats calls after 3
warm-up calls, the median and the best.  Bytes are what the algorithm needs: K * P * 4
read (plus P * 4 of base), and for the fold another K * P * 4 read and K * P * 4
written; the rate is those bytes over the median time, against 8 TB/s HBM peak
(about 6.3 TB/s achievable).

Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RESNET18_P = 11_173_962
HBM_PEAK = 8.0e12


def timed(fn, repeats):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, nargs="+", default=[10, 64])
    ap.add_argument("--params", type=int, default=RESNET18_P)
    ap.add_argument("--repeats", type=int, default=20)
    args = ap.parse_args()
    from distributed_learning_simulator_amd import _native
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    P = (args.params + 63) // 64 * 64
    out = {"probe": "gram", "P": P, "repeats": args.repeats, "cases": []}
    for K in args.rows:
        g = torch.Generator(device=dev).manual_seed(K)
        base = torch.randn(P, device=dev, generator=g)
        U = base[None, :] + 0.01 * torch.randn(K, P, device=dev, generator=g)
        H = torch.zeros(K, P, device=dev)
        rows = torch.arange(K, dtype=torch.int32, device=dev)
        G = torch.empty((K, K), dtype=torch.float64, device=dev)
        row_bytes = K * P * 4
        calls = {
            "pairwise_sqdist": (lambda: _native.pairwise_sqdist(U, rows, P, out=G), row_bytes),
            "rows_gram": (lambda: _native.rows_gram(U, rows, P, out=G), row_bytes),
            "rows_gram_base": (lambda: _native.rows_gram(U, rows, P, base=base, out=G),
                               row_bytes + 4 * P),
            "history_gram_base": (lambda: _native.history_gram(U, rows, H, rows, P, base=base,
                                                               out=G), 3 * row_bytes + 4 * P),
        }
        for name, (fn, nbytes) in calls.items():
            ms = timed(fn, args.repeats)
            med = statistics.median(ms)
            out["cases"].append({"call": name, "K": K, "bytes": nbytes, "ms_median": med,
                                 "ms_best": min(ms), "tb_per_s_median": nbytes / (med * 1e-3) / 1e12,
                                 "fraction_of_hbm_peak_median": nbytes / (med * 1e-3) / HBM_PEAK})
        del U, H
    print(json.dumps(out))


if __name__ == "__main__":
    main()
