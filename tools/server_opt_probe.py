"""dls_server_opt_step_f32 against the same step written as torch ops.

Synthetic operands (random normal agg, x, m; v = a square plus tau^2) at the ResNet-18
row length (the flat layout's P = 11.2 M fp32) and at P = 64 * 2^14, which stays in the
caches.  For every kind - sgd without and with momentum, adagrad, adam, yogi - it times,
with HIP events after at least 100 ms of warm-up launches, on preallocated operands:
  - the fused step: 7 * 4 * P bytes (5 * 4 * P for sgd with momentum, 3 * 4 * P without);
  - the same arithmetic as elementwise torch ops (in place where torch allows it).
A timed interval holds --batch launches back to back (the device never waits for the
host) that rotate over --sets operand sets: two ResNet-18 sets are 447 MB, more than the
256 MiB die-level cache, so every launch streams from HBM, as a step that follows a
round's K x P aggregation does.  The moments are restored outside the timed region, so
the values stay finite.

Prints one JSON line: per P and kind the median and best ms of both, the fused step's
achieved bytes/s and the ratio torch / fused.  --P replaces the two row lengths.
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

CASES = (("sgd", 0.0, 3), ("sgd_momentum", 0.9, 5), ("adagrad", 0.9, 7), ("adam", 0.9, 7),
         ("yogi", 0.9, 7))


def torch_step(kind, agg, x, m, v, c):
    """The contract's arithmetic in torch ops; returns the new model."""
    lr, beta1, omb1, beta2, omb2, tau = c
    d = agg - x
    if kind == "sgd":
        if m is None:
            return x + lr * d
        m.mul_(beta1).add_(d)
        return x + lr * m
    m.mul_(beta1).add_(omb1 * d)
    d2 = d * d
    if kind == "adagrad":
        v.add_(d2)
    elif kind == "adam":
        v.mul_(beta2).add_(omb2 * d2)
    else:
        v.sub_((omb2 * d2) * torch.sign(v - d2))
    return x + (lr * m) / (torch.sqrt(v) + tau)


def timed(fn, restore, repeats, batch, warmup_ms, dev):
    """(median, best) ms per launch: ``batch`` launches back to back between two events,
    so the device never waits for the host."""
    t0 = time.perf_counter()
    while True:
        restore()
        for i in range(batch):
            fn(i)
        torch.cuda.synchronize(dev)
        if (time.perf_counter() - t0) * 1e3 >= warmup_ms:
            break
    ms = []
    for _ in range(repeats):
        restore()
        e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
        e0.record()
        for i in range(batch):
            fn(i)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / batch)
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--P", type=int, nargs="+", default=None)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8, help="launches per timed interval")
    ap.add_argument("--sets", type=int, default=2, help="operand sets the launches rotate over")
    ap.add_argument("--warmup-ms", type=float, default=100.0)
    args = ap.parse_args()
    from distributed_learning_simulator_amd import _native
    from distributed_learning_simulator_amd.layout import ParameterLayout
    from distributed_learning_simulator_amd.model_shapes import resnet18_cifar
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lib = _native.lib()
    sizes = args.P if args.P else [ParameterLayout(resnet18_cifar()).P, 64 * 2 ** 14]
    lr, beta2, tau = 0.01, 0.99, 1e-3
    results = []
    for P in sizes:
        g = torch.Generator(device=dev).manual_seed(0)
        sets = []
        for _ in range(args.sets):
            x = torch.randn(P, generator=g, device=dev)
            agg = x + 0.01 * torch.randn(P, generator=g, device=dev)
            m0 = 0.01 * torch.randn(P, generator=g, device=dev)
            v0 = (0.01 * torch.randn(P, generator=g, device=dev)) ** 2 + tau * tau
            sets.append(dict(x=x, agg=agg, m0=m0, v0=v0, m=torch.empty_like(m0),
                             v=torch.empty_like(v0), out=torch.empty_like(x)))

        def restore():
            for s in sets:
                s["m"].copy_(s["m0"])
                s["v"].copy_(s["v0"])

        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        for name, beta1, vectors in CASES:
            kind = name.split("_")[0]
            code = _native.SERVER_OPT_KINDS[kind]
            c = _native.server_opt_coeffs(lr, beta1, beta2, tau)
            use_m, use_v = name != "sgd", kind != "sgd"

            def fused(i):
                s = sets[i % len(sets)]
                rc = lib.dls_server_opt_step_f32(
                    code, s["agg"].data_ptr(), s["x"].data_ptr(),
                    s["m"].data_ptr() if use_m else None, s["v"].data_ptr() if use_v else None,
                    s["out"].data_ptr(), P, *c, stream)
                assert rc == 0, lib.dls_last_error()

            def eager(i):
                s = sets[i % len(sets)]
                torch_step(kind, s["agg"], s["x"], s["m"] if use_m else None,
                           s["v"] if use_v else None, c)

            tf = timed(fused, restore, args.repeats, args.batch, args.warmup_ms, dev)
            te = timed(eager, restore, args.repeats, args.batch, args.warmup_ms, dev)
            assert all(torch.isfinite(s["out"]).all() for s in sets)
            nbytes = vectors * 4 * P
            results.append({"P": P, "kind": name, "bytes": nbytes,
                            "fused_ms_median": tf[0], "fused_ms_best": tf[1],
                            "fused_TBps_median": nbytes / (tf[0] * 1e-3) / 1e12,
                            "torch_ms_median": te[0], "torch_ms_best": te[1],
                            "ratio_torch_over_fused": te[0] / tf[0]})
    print(json.dumps({"probe": "server_opt", "lr": lr, "beta2": beta2, "tau": tau,
                      "batch": args.batch, "sets": args.sets, "results": results}), flush=True)


if __name__ == "__main__":
    main()
