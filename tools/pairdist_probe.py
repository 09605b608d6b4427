"""dls_pairwise_sqdist_f32 against the FedAvg stream over the same rows.

Synthetic ResNet-18-sized client rows (the flat layout's P = 11.2 M fp32, random
normal values).  For K = 8, 16, 32, 64 it times dls_pairwise_sqdist_f32 (both of
its launches, with a preallocated workspace and output) and, in the same process
on the same rows, dls_fedavg_f32 EXACT and dls_trimmed_mean_f32 (trim 0),
alternating the three launch by launch, with HIP events, after at least 100 ms of
warm-up launches of all of them.  The rows' traffic is K * P * 4 bytes for each.

Prints one JSON line per K: median and best ms of the kernels, the row bytes/s and
pair-terms/s of the distance kernel, and the ratios of the medians.  --P shrinks
the rows (a multiple of 4).
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
        rows = torch.randperm(kmax, generator=torch.Generator().manual_seed(K))[:K].to(
            dev, dtype=torch.int32)
        w = torch.full((K,), 100.0, dtype=torch.float32, device=dev)
        D = torch.empty((K, K), dtype=torch.float64, device=dev)
        nbytes_work = int(lib.dls_pairwise_sqdist_workspace(K, P))
        work = torch.empty(nbytes_work, dtype=torch.uint8, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def pairdist():
            rc = lib.dls_pairwise_sqdist_f32(U.data_ptr(), U.stride(0), rows.data_ptr(), K, P,
                                             D.data_ptr(), work.data_ptr(), stream)
            assert rc == 0, lib.dls_last_error()

        def fedavg():
            _native.fedavg(U, rows, w, 100.0 * K, P, out, mode=_native.FEDAVG_EXACT)

        def trimmed():
            _native.trimmed_mean(U, rows, 0, P, out)

        kernels = (("pairdist", pairdist), ("fedavg", fedavg), ("trimmed_mean", trimmed))
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
        terms = K * (K - 1) // 2 * P
        print(json.dumps({"probe": "pairdist", "K": K, "P": P, "row_bytes": row_bytes,
                          "workspace_bytes": nbytes_work, "pair_terms": terms,
                          "pairdist_ms_median": med["pairdist"],
                          "pairdist_ms_best": min(ms["pairdist"]),
                          "pairdist_TBps_median": row_bytes / (med["pairdist"] * 1e-3) / 1e12,
                          "pairdist_Gterms_per_s": terms / (med["pairdist"] * 1e-3) / 1e9,
                          "fedavg_ms_median": med["fedavg"], "fedavg_ms_best": min(ms["fedavg"]),
                          "trimmed_mean_ms_median": med["trimmed_mean"],
                          "ratio_pairdist_over_fedavg": med["pairdist"] / med["fedavg"],
                          "ratio_pairdist_over_trimmed_mean":
                              med["pairdist"] / med["trimmed_mean"]}), flush=True)


if __name__ == "__main__":
    main()
