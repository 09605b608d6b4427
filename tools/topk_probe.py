"""dls_topk_compress_f32 and dls_sparse_fedavg_f32 against the same work in torch ops
(DESIGN, "Top-k sparsification").

Synthetic operands at the ResNet-18 row length (the flat layout's P = 11.2 M fp32), ratio
0.01, K = 100 clients for the server's side.  With HIP events after at least 100 ms of
warm-up launches, on preallocated operands, it times
  - one topk_compress (a memset and nine kernels, five passes over P-sized arrays; the
    unavoidable traffic is reading w, base, e and writing e: 16 * P bytes) against
    u = (w - base) + e; torch.topk of |u|; gather; e = u with the sent entries zeroed;
  - one sparse_fedavg of K payloads of k pairs against index_add_ of the K * k weighted
    values into a clone of the base (not the same bits: index_add_ uses float atomics).
A timed interval holds --batch launches back to back that rotate over --sets operand sets
(two ResNet-18 sets of w, base, e are 268 MB, more than the 256 MiB die-level cache).  The
residual is restored outside the timed region.

Prints one JSON line: median and best ms of each, the compressor's achieved fraction of
16 * P bytes at the 8 TB/s HBM peak, and the ratios torch / fused.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

# the tree this file lies in, unless PYTHONPATH names another one first
sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK = 8.0e12


def timed(fn, restore, repeats, batch, warmup_ms, dev):
    """(median, best) ms per launch: ``batch`` launches back to back between two events."""
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
    ap.add_argument("--P", type=int, default=None)
    ap.add_argument("--ratio", type=float, default=0.01)
    ap.add_argument("--K", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4, help="launches per timed interval")
    ap.add_argument("--sets", type=int, default=2, help="operand sets the launches rotate over")
    ap.add_argument("--warmup-ms", type=float, default=100.0)
    args = ap.parse_args()
    from distributed_learning_simulator_amd import _native
    from distributed_learning_simulator_amd.layout import ParameterLayout
    from distributed_learning_simulator_amd.model_shapes import resnet18_cifar
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    layout = ParameterLayout(resnet18_cifar())
    P = args.P if args.P else layout.P
    k = max(1, math.ceil(args.ratio * (layout.numel if not args.P else P)))
    K = args.K
    g = torch.Generator(device=dev).manual_seed(0)

    # ---- the client's side
    sets = []
    for _ in range(args.sets):
        base = torch.randn(P, generator=g, device=dev)
        w = base + 0.01 * torch.randn(P, generator=g, device=dev)
        e0 = 0.003 * torch.randn(P, generator=g, device=dev)
        sets.append(dict(w=w, base=base, e0=e0, e=torch.empty_like(e0),
                         idx=torch.empty(k, dtype=torch.int32, device=dev),
                         val=torch.empty(k, dtype=torch.float32, device=dev),
                         stats=torch.empty(2, dtype=torch.int32, device=dev),
                         ws=_native.topk_workspace(P, dev)))

    def restore():
        for s in sets:
            s["e"].copy_(s["e0"])

    def fused(i):
        s = sets[i % len(sets)]
        _native.topk_compress(s["w"], s["base"], s["e"], k, P, s["idx"], s["val"], s["stats"], s["ws"])

    def eager(i):
        s = sets[i % len(sets)]
        u = (s["w"] - s["base"]) + s["e"]
        idx = torch.topk(u.abs(), k, sorted=False).indices
        val = u[idx]
        u[idx] = 0.0
        s["e"].copy_(u)
        return idx, val

    tf = timed(fused, restore, args.repeats, args.batch, args.warmup_ms, dev)
    te = timed(eager, restore, args.repeats, args.batch, args.warmup_ms, dev)
    restore()
    fused(0)
    assert sets[0]["stats"].tolist() == [k, 0]
    floor = 16 * P
    compress = {"k": k, "floor_bytes": floor, "passes_over_P": 5,
                "fused_ms_median": tf[0], "fused_ms_best": tf[1],
                "fused_fraction_of_floor_at_hbm_peak": floor / HBM_PEAK / (tf[0] * 1e-3),
                "torch_ms_median": te[0], "torch_ms_best": te[1],
                "ratio_torch_over_fused": te[0] / tf[0]}
    del sets

    # ---- the server's side: K clients, k pairs each
    base = torch.randn(P, generator=g, device=dev)
    idx = torch.cat([torch.randperm(P, generator=g, device=dev)[:k].sort().values
                     for _ in range(K)]).to(torch.int32)
    val = 0.01 * torch.randn(K * k, generator=g, device=dev)
    ns = torch.randint(100, 1001, (K,), generator=g, device=dev).to(torch.float32)
    total = float(ns.sum())
    off = torch.arange(K + 1, dtype=torch.int64, device=dev) * k
    outs = [torch.empty(P, device=dev) for _ in range(args.sets)]
    idx64 = idx.to(torch.int64)
    scale = (ns / total).repeat_interleave(k)

    def fused_server(i):
        _native.sparse_fedavg(base, idx, val, off, ns, total, P, outs[i % len(outs)])

    def eager_server(i):
        out = outs[i % len(outs)]
        out.copy_(base)
        out.index_add_(0, idx64, val * scale)

    sf = timed(fused_server, lambda: None, args.repeats, args.batch, args.warmup_ms, dev)
    se = timed(eager_server, lambda: None, args.repeats, args.batch, args.warmup_ms, dev)
    server = {"K": K, "pairs": K * k, "bytes": 8 * P + 8 * K * k,
              "fused_ms_median": sf[0], "fused_ms_best": sf[1],
              "torch_ms_median": se[0], "torch_ms_best": se[1],
              "ratio_torch_over_fused": se[0] / sf[0]}
    print(json.dumps({"probe": "topk", "P": P, "ratio": args.ratio, "batch": args.batch,
                      "sets": args.sets, "compress": compress, "sparse_fedavg": server}),
          flush=True)


if __name__ == "__main__":
    main()
