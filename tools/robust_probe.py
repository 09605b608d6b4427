"""dls_trimmed_mean_f32 against the FedAvg stream over the same rows.

Synthetic ResNet-18-sized client rows (the flat layout's P = 11.2 M fp32, random
normal values).  For K = 4, 16, 50, 64 and trim = 0, about K/10 and the median it
times dls_trimmed_mean_f32 and, in the same process on the same rows,
dls_fedavg_f32 EXACT, alternating the two launch by launch, with HIP events,
after at least 100 ms of warm-up launches of both.  The algorithmic traffic of
either call is (K + 1) * P * 4 bytes.

Prints one JSON line per (K, trim): median and best ms of both kernels, their
bytes/s and the ratio of the medians.  --P shrinks the rows (a multiple of 4).
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

# the tree this file lies in, unless PYTHONPATH names another one first
sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--P", type=int, default=None, help="row length (default: ResNet-18's)")
    ap.add_argument("--K", type=int, nargs="+", default=[4, 16, 50, 64])
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup-ms", type=float, default=100.0)
    args = ap.parse_args()
    from distributed_learning_simulator_amd import _native
    from distributed_learning_simulator_amd.layout import ParameterLayout
    from distributed_learning_simulator_amd.model_shapes import resnet18_cifar
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    P = args.P if args.P is not None else ParameterLayout(resnet18_cifar()).P
    kmax = max(args.K)
    g = torch.Generator(device=dev).manual_seed(0)
    U = torch.randn((kmax, P), generator=g, device=dev, dtype=torch.float32)
    out = torch.empty(P, dtype=torch.float32, device=dev)
    for K in args.K:
        rows = torch.randperm(kmax, generator=torch.Generator().manual_seed(K))[:K].to(
            dev, dtype=torch.int32)
        w = torch.full((K,), 100.0, dtype=torch.float32, device=dev)
        for trim in sorted({0, max(1, round(K / 10)) if K > 2 else 0, (K - 1) // 2}):
            def robust():
                _native.trimmed_mean(U, rows, trim, P, out)

            def fedavg():
                _native.fedavg(U, rows, w, 100.0 * K, P, out, mode=_native.FEDAVG_EXACT)

            t0 = time.perf_counter()
            while True:  # warm-up: both kernels, until the wall clock says enough
                robust()
                fedavg()
                torch.cuda.synchronize(dev)
                if (time.perf_counter() - t0) * 1e3 >= args.warmup_ms:
                    break
            ms = {"robust": [], "fedavg": []}
            for _ in range(args.repeats):
                for name, fn in (("robust", robust), ("fedavg", fedavg)):
                    e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    ms[name].append(e0.elapsed_time(e1))
            nbytes = (K + 1) * P * 4
            r, f = statistics.median(ms["robust"]), statistics.median(ms["fedavg"])
            print(json.dumps({"probe": "robust", "K": K, "trim": trim, "P": P, "bytes": nbytes,
                              "robust_ms_median": r, "robust_ms_best": min(ms["robust"]),
                              "robust_TBps_median": nbytes / (r * 1e-3) / 1e12,
                              "fedavg_ms_median": f, "fedavg_ms_best": min(ms["fedavg"]),
                              "fedavg_TBps_median": nbytes / (f * 1e-3) / 1e12,
                              "ratio_robust_over_fedavg": r / f}), flush=True)


if __name__ == "__main__":
    main()
