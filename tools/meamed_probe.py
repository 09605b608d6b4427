"""dls_mean_around_median_f32 against dls_trimmed_mean_f32 over the same rows.

Synthetic ResNet-18-sized client rows (the flat layout's P = 11.2 M fp32, random
normal values).  For K = 8, 16, 32, 64 it times dls_mean_around_median_f32 with
keep = K - 2 * (K // 4) (Bulyan's stage 2 at the largest f the rule allows, seen
from its theta selected rows) and, in the same process on the same rows,
dls_trimmed_mean_f32 (trim 0) and dls_pairwise_sqdist_f32 (both of its launches: the
other launch of a Bulyan round), alternating the three launch by launch, with HIP
events, after at least 100 ms of warm-up launches of all of them.  The rows'
traffic is K * P * 4 bytes for each.

Prints one JSON line per K: median and best ms of the kernels, the bytes/s of the
window kernel and the ratios of the medians.  --P shrinks the rows (a multiple of
4), --keep overrides the window.
"""
import argparse
import ctypes
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
    ap.add_argument("--K", type=int, nargs="+", default=[8, 16, 32, 64])
    ap.add_argument("--keep", type=int, default=None, help="default: K - 2 * (K // 4)")
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--warmup-ms", type=float, default=100.0)
    args = ap.parse_args()
    from distributed_learning_simulator_amd import _native
    from distributed_learning_simulator_amd.layout import ParameterLayout
    from distributed_learning_simulator_amd.model_shapes import resnet18_cifar
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lib = _native.lib()
    P = args.P if args.P is not None else ParameterLayout(resnet18_cifar()).P
    kmax = max(args.K)
    g = torch.Generator(device=dev).manual_seed(0)
    U = torch.randn((kmax, P), generator=g, device=dev, dtype=torch.float32)
    out = torch.empty(P, dtype=torch.float32, device=dev)
    for K in args.K:
        keep = args.keep if args.keep is not None else K - 2 * (K // 4)
        rows = torch.randperm(kmax, generator=torch.Generator().manual_seed(K))[:K].to(
            dev, dtype=torch.int32)
        D = torch.empty((K, K), dtype=torch.float64, device=dev)
        work = torch.empty(int(lib.dls_pairwise_sqdist_workspace(K, P)), dtype=torch.uint8,
                           device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def window():
            _native.mean_around_median(U, rows, keep, P, out)

        def trimmed():
            _native.trimmed_mean(U, rows, 0, P, out)

        def pairdist():
            rc = lib.dls_pairwise_sqdist_f32(U.data_ptr(), U.stride(0), rows.data_ptr(), K, P,
                                             D.data_ptr(), work.data_ptr(), stream)
            assert rc == 0, lib.dls_last_error()

        kernels = (("window", window), ("trimmed_mean", trimmed), ("pairdist", pairdist))
        t0 = time.perf_counter()
        while True:  # warm-up: every kernel, until the wall clock says enough
            for _, fn in kernels:
                fn()
            torch.cuda.synchronize(dev)
            if (time.perf_counter() - t0) * 1e3 >= args.warmup_ms:
                break
        ms = {name: [] for name, _ in kernels}
        for _ in range(args.repeats):
            for name, fn in kernels:
                e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1))
        med = {name: statistics.median(v) for name, v in ms.items()}
        nbytes = (K + 1) * P * 4
        print(json.dumps({"probe": "meamed", "K": K, "keep": keep, "P": P, "bytes": nbytes,
                          "window_ms_median": med["window"], "window_ms_best": min(ms["window"]),
                          "window_TBps_median": nbytes / (med["window"] * 1e-3) / 1e12,
                          "trimmed_mean_ms_median": med["trimmed_mean"],
                          "trimmed_mean_ms_best": min(ms["trimmed_mean"]),
                          "pairdist_ms_median": med["pairdist"],
                          "ratio_window_over_trimmed_mean": med["window"] / med["trimmed_mean"],
                          "bulyan_round_ms": med["pairdist"] + med["window"]}), flush=True)


if __name__ == "__main__":
    main()
