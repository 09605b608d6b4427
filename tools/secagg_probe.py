"""dls_secagg_mask_f32 and dls_secagg_unmask_f32 against dls_fedavg_f32 (DESIGN "Secure
aggregation").

Synthetic rows at the ResNet-18 row length (the flat layout's P = 11.2 M) for K = 10 and
K = 64 clients.  In one process, with HIP events after at least 100 ms of warm-up launches, on
preallocated operands, it times:
  - the client's mask of one row among K participants: 3 * 4 * P bytes, K Philox blocks
    per four coordinates (its self mask and K - 1 pair masks);
  - the server's unmask of K rows, nobody dropped: (K + 2) * 4 * P bytes, K blocks (the
    self masks);
  - the unmask with K // 4 dropped: S = K - K // 4 rows, (S + 2) * 4 * P bytes,
    S * (1 + K // 4) blocks;
  - dls_fedavg_f32 over the same K fp32 rows: (K + 1) * 4 * P bytes, the traffic floor of a
    K-row stream.
A timed interval holds --batch launches back to back (the device never waits for the host).
K rows of ResNet-18 are 447 MB (K = 10) and 2.9 GB (K = 64), more than the 256 MiB die-level
cache, so every launch streams from HBM.

Prints one JSON line: per K the median and best ms and the GB/s of each, the Philox blocks per
coordinate, and the unmask / FedAvg ratios.  --P replaces the row length.
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


def timed(fn, repeats, batch, warmup_ms, dev):
    """(median, best) ms per launch: ``batch`` launches back to back between two events."""
    t0 = time.perf_counter()
    while True:
        for _ in range(batch):
            fn()
        torch.cuda.synchronize(dev)
        if (time.perf_counter() - t0) * 1e3 >= warmup_ms:
            break
    ms = []
    for _ in range(repeats):
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
    from distributed_learning_simulator_amd.aggregation import (secagg_client_streams,
                                                                secagg_server_streams)
    from distributed_learning_simulator_amd.layout import ParameterLayout
    from distributed_learning_simulator_amd.model_shapes import resnet18_cifar
    from distributed_learning_simulator_amd.workers.fed_secagg_worker import to_stream_table
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lib = _native.lib()
    P = args.P if args.P else ParameterLayout(resnet18_cifar()).P
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    seed, f, bits = 0x9E3779B97F4A7C15, 16, 20
    results = []
    for K in args.K:
        g = torch.Generator(device=dev).manual_seed(K)
        U = torch.randn((K, P), generator=g, device=dev)
        Y = U.view(torch.int32)  # the same K rows, read as masked payloads: any bits will do
        base = torch.randn(P, generator=g, device=dev)
        w = base + 0.01 * torch.randn(P, generator=g, device=dev)
        y = torch.empty(P, dtype=torch.int32, device=dev)
        out = torch.empty(P, device=dev)
        stats = torch.zeros(2, dtype=torch.int32, device=dev)
        rows = torch.arange(K, dtype=torch.int32, device=dev)
        weight = torch.ones(K, device=dev)
        ids = list(range(K))
        gone = ids[:K // 4]
        alive = ids[K // 4:]
        tables = {"mask": secagg_client_streams(K // 2, ids, 1),
                  "unmask": secagg_server_streams(ids, [], 1),
                  "unmask_dropped": secagg_server_streams(alive, gone, 1)}
        dev_tables = {name: tuple(to_stream_table(t, dev) for t in pair)
                      for name, pair in tables.items()}

        def ptr(t):
            return None if t is None else t.data_ptr()

        def mask():
            add, sub = dev_tables["mask"]
            rc = lib.dls_secagg_mask_f32(w.data_ptr(), base.data_ptr(), P, f, bits, 1, ptr(add),
                                         len(tables["mask"][0]), ptr(sub), len(tables["mask"][1]),
                                         seed, y.data_ptr(), stats.data_ptr(), stream)
            assert rc == 0, lib.dls_last_error()

        def unmask(name, first, count):
            def run():
                add, sub = dev_tables[name]
                rc = lib.dls_secagg_unmask_f32(Y.data_ptr(), P, rows[first:].data_ptr(), count,
                                               ptr(add), len(tables[name][0]), ptr(sub),
                                               len(tables[name][1]), seed, base.data_ptr(), f,
                                               float(count), P, out.data_ptr(), None, stream)
                assert rc == 0, lib.dls_last_error()
            return run

        def fedavg():
            rc = lib.dls_fedavg_f32(U.data_ptr(), P, rows.data_ptr(), weight.data_ptr(), K,
                                    float(K), P, _native.FEDAVG_EXACT, out.data_ptr(), stream)
            assert rc == 0, lib.dls_last_error()

        runs = (("mask", mask, 3 * 4 * P, sum(map(len, tables["mask"]))),
                ("unmask", unmask("unmask", 0, K), (K + 2) * 4 * P, sum(map(len, tables["unmask"]))),
                ("unmask_dropped", unmask("unmask_dropped", K // 4, len(alive)),
                 (len(alive) + 2) * 4 * P, sum(map(len, tables["unmask_dropped"]))),
                ("fedavg", fedavg, (K + 1) * 4 * P, 0))
        row = {"K": K, "P": P, "dropped": len(gone)}
        for name, fn, nbytes, nstreams in runs:
            med, best = timed(fn, args.repeats, args.batch, args.warmup_ms, dev)
            row[name] = {"ms_median": med, "ms_best": best, "bytes": nbytes,
                         "GBps_median": nbytes / med / 1e6, "streams": nstreams,
                         "philox_blocks_per_coordinate": nstreams / 4.0}
        row["unmask_over_fedavg"] = row["unmask"]["ms_median"] / row["fedavg"]["ms_median"]
        row["unmask_dropped_over_fedavg"] = \
            row["unmask_dropped"]["ms_median"] / row["fedavg"]["ms_median"]
        results.append(row)
        del U, Y
    print(json.dumps({"probe": "secagg", "frac_bits": f, "bits": bits, "batch": args.batch,
                      "results": results}), flush=True)


if __name__ == "__main__":
    main()
