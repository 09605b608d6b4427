"""dls_hetero_fedavg_f32 at the ResNet-18 row length (DESIGN "Width-heterogeneous FedAvg").

With HIP events after at least 100 ms of warm-up, --batch launches back to back per timed
interval, on preallocated operands, in one run, at K = 10 and K = 64 clients of a plan with the
levels {1, 0.5, 0.25}:
  - every client at width 1, and the three widths dealt round-robin;
  - both with prefix windows (shift 0: the vector path wherever the row lengths allow) and with
    every window rolled on by one (the element path);
  - dls_fedavg_f32 over the same K full-width rows, the yardstick.
Per case: the time, the traffic model sum_k 4 P_k + 8 P bytes ((K + 1) 4 P for dls_fedavg_f32)
and the bytes/s it amounts to.  Two ragged buffers are alternated so that no launch finds its
rows in the 256 MiB die-level cache.

Prints one JSON line.
"""
import argparse
import json
import os
import sys

import torch

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.scaffold_probe import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8, help="launches per timed interval")
    ap.add_argument("--warmup-ms", type=float, default=100.0)
    args = ap.parse_args()
    from distributed_learning_simulator_amd import _native
    from distributed_learning_simulator_amd.hetero import HeteroPlan
    from distributed_learning_simulator_amd.models import ResNet18
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    plan = HeteroPlan(ResNet18().hetero_views(), (1.0, 0.5, 0.25))
    P = plan.P
    go = lambda fn: timed(fn, args.repeats, args.batch, args.warmup_ms, dev)
    g = torch.Generator(device=dev).manual_seed(0)
    out = {"probe": "hetero", "P": P, "level_P": plan.level_P, "tensors": len(plan.views),
           "batch": args.batch, "cases": []}
    for K in (10, 64):
        sets = [0.01 * torch.randn(K, P, generator=g, device=dev) for _ in range(2)]
        flat_sets = [s.view(-1) for s in sets]
        weights = [float(w) for w in torch.randint(100, 1000, (K,), generator=g, device=dev).tolist()]
        prev, res = torch.randn(P, generator=g, device=dev), torch.empty(P, device=dev)
        rows = torch.arange(K, dtype=torch.int32, device=dev)
        weight = torch.tensor(weights, device=dev)
        tf = go(lambda i: _native.fedavg(sets[i % 2], rows, weight, sum(weights), P, res))
        fed_bytes = (K + 1) * 4 * P
        fed = {"ms_median": tf[0], "ms_best": tf[1], "model_bytes": fed_bytes,
               "TBps_median": fed_bytes / (tf[0] * 1e-3) / 1e12}
        for widths in ("all_1", "1_0.5_0.25"):
            levels = [0 if widths == "all_1" else k % 3 for k in range(K)]
            starts, at = [], 0
            for lvl in levels:  # the narrow rows packed one after the other
                starts.append(at)
                at += plan.level_P[lvl]
            nbytes = 4 * at + 8 * P
            for window in ("prefix", "rolled"):
                plan.set_shifts({name: 1 for name in plan.groups} if window == "rolled" else {})
                th = go(lambda i: _native.hetero_fedavg(plan, levels, starts, weights,
                                                        flat_sets[i % 2], prev, res))
                out["cases"].append({"K": K, "widths": widths, "window": window,
                                     "ms_median": th[0], "ms_best": th[1], "model_bytes": nbytes,
                                     "TBps_median": nbytes / (th[0] * 1e-3) / 1e12,
                                     "fedavg": fed, "time_over_fedavg": th[0] / tf[0],
                                     "bytes_over_fedavg": nbytes / fed_bytes})
        del sets, flat_sets
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
