"""dls_weiszfeld_step_f32 against its unfused parts over the same rows.

Synthetic ResNet-18-sized client rows (the flat layout's P = 11.2 M fp32, random
normal values).  For K = 8, 16, 32, 64 it times, in one process on the same rows,
launch by launch in turn, with HIP events, after at least 100 ms of warm-up
launches of all of them:
  - dls_weiszfeld_step_f32 (both launches; preallocated workspace and outputs),
  - dls_rows_sqdist_to_f32 (both launches),
  - dls_fedavg_f32 EXACT,
  - dls_trimmed_mean_f32 at trim (K-1)/2: the median start of the rule.
The rows' traffic is K * P * 4 bytes for each.

Prints one JSON line per K: median and best ms of each, the step's row bytes/s,
the ratios of the medians (step / FedAvg, step / (distances + FedAvg): the fused
step against the unfused pair) and the whole rule's kernel time, median start +
one distance pass + --iters steps.  --P shrinks the rows (a multiple of 4).
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
    ap.add_argument("--iters", type=int, default=3, help="steps of the whole-rule figure")
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
    z = torch.empty(P, dtype=torch.float32, device=dev)
    for K in args.K:
        rows = torch.randperm(kmax, generator=torch.Generator().manual_seed(K))[:K].to(
            dev, dtype=torch.int32)
        n = torch.full((K,), 100.0, dtype=torch.float32, device=dev)
        w = torch.full((K,), 1.0 / K, dtype=torch.float32, device=dev)
        d2 = torch.empty((K,), dtype=torch.float64, device=dev)
        nbytes_work = int(lib.dls_weiszfeld_workspace(K, P))
        work = torch.empty(nbytes_work, dtype=torch.uint8, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def step():
            rc = lib.dls_weiszfeld_step_f32(U.data_ptr(), U.stride(0), rows.data_ptr(), K,
                                            w.data_ptr(), P, z.data_ptr(), d2.data_ptr(),
                                            work.data_ptr(), stream)
            assert rc == 0, lib.dls_last_error()

        def sqdist():
            rc = lib.dls_rows_sqdist_to_f32(U.data_ptr(), U.stride(0), rows.data_ptr(), K, P,
                                            out.data_ptr(), d2.data_ptr(), work.data_ptr(), stream)
            assert rc == 0, lib.dls_last_error()

        def fedavg():
            _native.fedavg(U, rows, n, 100.0 * K, P, out, mode=_native.FEDAVG_EXACT)

        def median():
            _native.trimmed_mean(U, rows, (K - 1) // 2, P, out)

        kernels = (("step", step), ("sqdist", sqdist), ("fedavg", fedavg), ("median", median))
        fedavg()  # `out` is the point of the distance pass: finite from the start
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
        row_bytes = K * P * 4
        print(json.dumps({"probe": "geomedian", "K": K, "P": P, "row_bytes": row_bytes,
                          "workspace_bytes": nbytes_work,
                          "step_ms_median": med["step"], "step_ms_best": min(ms["step"]),
                          "step_TBps_median": row_bytes / (med["step"] * 1e-3) / 1e12,
                          "sqdist_ms_median": med["sqdist"], "sqdist_ms_best": min(ms["sqdist"]),
                          "fedavg_ms_median": med["fedavg"], "fedavg_ms_best": min(ms["fedavg"]),
                          "median_ms_median": med["median"], "median_ms_best": min(ms["median"]),
                          "ratio_step_over_fedavg": med["step"] / med["fedavg"],
                          "ratio_step_over_unfused_pair":
                              med["step"] / (med["sqdist"] + med["fedavg"]),
                          "rule_iters": args.iters,
                          "rule_ms": med["median"] + med["sqdist"] + args.iters * med["step"]}),
              flush=True)


if __name__ == "__main__":
    main()
