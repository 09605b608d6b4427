"""dls_centered_clip_step_f32 against dls_weiszfeld_step_f32 over the same rows.

Synthetic ResNet-18-sized client rows (the flat layout's P = 11.2 M fp32, random
normal values).  For K = 10 and 64 it times, in one process on the same rows, launch
by launch in turn, with HIP events, after at least 100 ms of warm-up launches of both
(preallocated workspace and outputs, both launches of each):
  - dls_weiszfeld_step_f32: reads K * P * 4 bytes, writes P * 4;
  - dls_centered_clip_step_f32: the same plus P * 4 bytes of z read, in place from a
    point that starts at the rows' mean (the coefficients are 1 / K, so it stays there).

Prints one JSON line per K: median and best ms of each, the rows' bytes/s and the ratio
of the medians (clip step / Weiszfeld step).  --P shrinks the rows (a multiple of 4).
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
    ap.add_argument("--K", type=int, nargs="+", default=[10, 64])
    ap.add_argument("--repeats", type=int, default=30)
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
    zw = torch.empty(P, dtype=torch.float32, device=dev)
    zc = torch.empty(P, dtype=torch.float32, device=dev)
    for K in args.K:
        rows = torch.randperm(kmax, generator=torch.Generator().manual_seed(K))[:K].to(
            dev, dtype=torch.int32)
        w = torch.full((K,), 1.0 / K, dtype=torch.float32, device=dev)
        d2 = torch.empty((K,), dtype=torch.float64, device=dev)
        nbytes_work = int(lib.dls_weiszfeld_workspace(K, P))
        work = torch.empty(nbytes_work, dtype=torch.uint8, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def weiszfeld():
            rc = lib.dls_weiszfeld_step_f32(U.data_ptr(), U.stride(0), rows.data_ptr(), K,
                                            w.data_ptr(), P, zw.data_ptr(), d2.data_ptr(),
                                            work.data_ptr(), stream)
            assert rc == 0, lib.dls_last_error()

        def clip():
            rc = lib.dls_centered_clip_step_f32(U.data_ptr(), U.stride(0), rows.data_ptr(), K,
                                                w.data_ptr(), P, zc.data_ptr(), d2.data_ptr(),
                                                work.data_ptr(), stream)
            assert rc == 0, lib.dls_last_error()

        kernels = (("weiszfeld", weiszfeld), ("clip", clip))
        weiszfeld()
        zc.copy_(zw)  # the clip step's point: the rows' mean
        t0 = time.perf_counter()
        while True:  # warm-up: both kernels, until the wall clock says enough
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
        assert torch.isfinite(zc).all()
        med = {name: statistics.median(v) for name, v in ms.items()}
        row_bytes = K * P * 4
        print(json.dumps({"probe": "centered_clip", "K": K, "P": P, "row_bytes": row_bytes,
                          "weiszfeld_ms_median": med["weiszfeld"],
                          "weiszfeld_ms_best": min(ms["weiszfeld"]),
                          "clip_ms_median": med["clip"], "clip_ms_best": min(ms["clip"]),
                          "weiszfeld_TBps_median": row_bytes / (med["weiszfeld"] * 1e-3) / 1e12,
                          "clip_TBps_median": row_bytes / (med["clip"] * 1e-3) / 1e12,
                          "ratio_clip_over_weiszfeld": med["clip"] / med["weiszfeld"]}),
              flush=True)


if __name__ == "__main__":
    main()
