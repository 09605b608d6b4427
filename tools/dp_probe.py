"""dls_dp_clip_noise_step_f32 against the pieces it fuses (DESIGN "Differentially private
FedAvg").

Synthetic rows (random normal) at the ResNet-18 row length (the flat layout's P = 11.2 M
fp32) for K = 10 and K = 64 clients.  In one process, with HIP events after at least 100 ms
of warm-up launches, on preallocated operands, it times:
  - the fused step with sigma > 0:   (K + 2) * 4 * P bytes;
  - the same step with sigma = 0:    the same bytes, no generator;
  - dls_centered_clip_step_f32 on the same rows: the same bytes (plus its distances);
  - dls_philox_normal_f32 alone:     4 * P bytes written.
A timed interval holds --batch launches back to back (the device never waits for the host).
K rows of ResNet-18 are 447 MB (K = 10) and 2.9 GB (K = 64), more than the 256 MiB die-level
cache, so every launch streams from HBM.  z is restored outside the timed region.

Prints one JSON line: per K the median and best ms and the GB/s of each, and the two ratios
that decide whether fusing was worth a kernel: fused / clip step, and fused / (clip step +
generator).  --P replaces the row length.
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


def timed(fn, restore, repeats, batch, warmup_ms, dev):
    """(median, best) ms per launch: ``batch`` launches back to back between two events."""
    t0 = time.perf_counter()
    while True:
        restore()
        for _ in range(batch):
            fn()
        torch.cuda.synchronize(dev)
        if (time.perf_counter() - t0) * 1e3 >= warmup_ms:
            break
    ms = []
    for _ in range(repeats):
        restore()
        e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        e0.record()
        for _ in range(batch):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / batch)
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--P", type=int, default=None)
    ap.add_argument("--K", type=int, nargs="+", default=[10, 64])
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--batch", type=int, default=4, help="launches per timed interval")
    ap.add_argument("--warmup-ms", type=float, default=100.0)
    args = ap.parse_args()
    from distributed_learning_simulator_amd import _native
    from distributed_learning_simulator_amd.layout import ParameterLayout
    from distributed_learning_simulator_amd.model_shapes import resnet18_cifar
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lib = _native.lib()
    P = args.P if args.P else ParameterLayout(resnet18_cifar()).P
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    seed, sid, sigma = 0x9E3779B97F4A7C15, 1, 0.01
    results = []
    for K in args.K:
        g = torch.Generator(device=dev).manual_seed(K)
        U = torch.randn((K, P), generator=g, device=dev)
        z0 = torch.randn(P, generator=g, device=dev)
        z = torch.empty_like(z0)
        out = torch.empty_like(z0)
        rows = torch.arange(K, dtype=torch.int32, device=dev)
        c = torch.full((K,), 1.0 / K, device=dev)
        dist2 = torch.empty(K, dtype=torch.float64, device=dev)
        work = torch.empty(max(int(lib.dls_weiszfeld_workspace(K, P)), 16), dtype=torch.uint8,
                           device=dev)

        def restore():
            z.copy_(z0)

        def fused(s):
            def run():
                rc = lib.dls_dp_clip_noise_step_f32(U.data_ptr(), P, rows.data_ptr(), K,
                                                    c.data_ptr(), P, z.data_ptr(), s, seed, sid,
                                                    stream)
                assert rc == 0, lib.dls_last_error()
            return run

        def clip():
            rc = lib.dls_centered_clip_step_f32(U.data_ptr(), P, rows.data_ptr(), K, c.data_ptr(),
                                                P, z.data_ptr(), dist2.data_ptr(),
                                                work.data_ptr(), stream)
            assert rc == 0, lib.dls_last_error()

        def normal():
            rc = lib.dls_philox_normal_f32(out.data_ptr(), P, seed, sid, 0, stream)
            assert rc == 0, lib.dls_last_error()

        t = {name: timed(fn, restore, args.repeats, args.batch, args.warmup_ms, dev)
             for name, fn in (("fused_noise", fused(sigma)), ("fused_sigma0", fused(0.0)),
                              ("clip_step", clip), ("philox_normal", normal))}
        assert bool(torch.isfinite(z).all()) and bool(torch.isfinite(out).all())
        step_bytes, gen_bytes = (K + 2) * 4 * P, 4 * P
        row = {"K": K, "P": P, "step_bytes": step_bytes, "normal_bytes": gen_bytes}
        for name, (med, best) in t.items():
            nbytes = gen_bytes if name == "philox_normal" else step_bytes
            row[name] = {"ms_median": med, "ms_best": best, "GBps_median": nbytes / med / 1e6}
        row["fused_over_clip_step"] = t["fused_noise"][0] / t["clip_step"][0]
        row["fused_over_clip_step_plus_normal"] = \
            t["fused_noise"][0] / (t["clip_step"][0] + t["philox_normal"][0])
        results.append(row)
        del U
    print(json.dumps({"probe": "dp", "sigma": sigma, "batch": args.batch, "results": results}),
          flush=True)


if __name__ == "__main__":
    main()
