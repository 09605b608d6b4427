"""The three fed_scaffold kernels at the ResNet-18 row length (DESIGN "SCAFFOLD").

With HIP events after at least 100 ms of warm-up, --batch launches back to back per timed
interval, on preallocated operands, in one run:
  - dls_scaffold_server_step_f32 at K = 10 and K = 64 beside dls_fedavg_f32 over the same
    rows; the traffic model puts their ratio near (K + 4) / (K + 1).  Two sets of rows are
    alternated so that no launch finds its rows in the 256 MiB die-level cache;
  - dls_scaffold_local_step_f32 over ResNet-18's 62 tensors (wd and control on) beside
    torch.optim.SGD.step() plus the torch ops the correction costs per tensor (g += corr
    slice), with the launches per step of the fused path and the ops torch issues (a lower
    bound of its launches: one correction per tensor and the two multi-tensor passes of
    SGD's step, each of which is several launches);
  - dls_scaffold_finish_f32 beside the same arithmetic as three torch ops.

Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, repeats, batch, warmup_ms, dev):
    """(median, best) ms per call of fn(i)."""
    t0 = time.perf_counter()
    while True:
        for i in range(batch):
            fn(i)
        torch.cuda.synchronize(dev)
        if (time.perf_counter() - t0) * 1e3 >= warmup_ms:
            break
    ms = []
    for _ in range(repeats):
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
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--batch", type=int, default=8, help="launches per timed interval")
    ap.add_argument("--warmup-ms", type=float, default=100.0)
    args = ap.parse_args()
    from distributed_learning_simulator_amd import _native
    from distributed_learning_simulator_amd.layout import ParameterLayout
    from distributed_learning_simulator_amd.model_shapes import resnet18_cifar
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    layout = ParameterLayout(resnet18_cifar())
    P, N = layout.P, 100
    go = lambda fn: timed(fn, args.repeats, args.batch, args.warmup_ms, dev)
    g = torch.Generator(device=dev).manual_seed(0)
    out = {"probe": "scaffold", "P": P, "tensors": len(layout), "batch": args.batch, "server": []}

    for K in (10, 64):
        sets = [0.01 * torch.randn(K, P, generator=g, device=dev) for _ in range(2)]
        rows = torch.arange(K, dtype=torch.int32, device=dev)
        weight = torch.randint(100, 1000, (K,), generator=g, device=dev).float()
        total = float(weight.sum())
        b = torch.full((K,), _native.scaffold_coeff(5, 0.1, N), device=dev)
        x, c = torch.randn(P, generator=g, device=dev), torch.randn(P, generator=g, device=dev)
        xo, co, avg = torch.empty_like(x), torch.empty_like(c), torch.empty_like(x)
        ts = go(lambda i: _native.scaffold_server_step(sets[i % 2], rows, weight, b, total, P, 1.0,
                                                       K / N, x, c, xo, co))
        tf = go(lambda i: _native.fedavg(sets[i % 2], rows, weight, total, P, avg))
        nbytes = (K + 4) * 4 * P
        out["server"].append({"K": K, "step_ms_median": ts[0], "step_ms_best": ts[1],
                              "fedavg_ms_median": tf[0], "fedavg_ms_best": tf[1],
                              "ratio_step_over_fedavg": ts[0] / tf[0],
                              "traffic_model_ratio": (K + 4) / (K + 1),
                              "step_TBps_median": nbytes / (ts[0] * 1e-3) / 1e12})
        del sets

    params = [torch.nn.Parameter(torch.randn(s, generator=g, device=dev) * 0.05) for s in layout.shapes]
    for p in params:
        p.grad = torch.randn(p.shape, generator=g, device=dev) * 0.01
    base, corr = (torch.randn(P, generator=g, device=dev) * 0.01 for _ in range(2))
    datas, grads = [p.data for p in params], [p.grad for p in params]
    tl = go(lambda i: _native.scaffold_local_step(datas, grads, layout.offsets, base, corr, 1e-3, 5e-4))
    opt = torch.optim.SGD(params, lr=1e-3, weight_decay=5e-4)
    views = [corr[o:o + n].view(s) for o, n, s in zip(layout.offsets, layout.numels, layout.shapes)]

    def eager(i):
        for gr, v in zip(grads, views):  # g += c - c_i, then the optimizer's own step
            gr.add_(v)
        opt.step()

    te = go(eager)
    T = len(params)
    out["local_step"] = {"fused_ms_median": tl[0], "fused_ms_best": tl[1],
                         "fused_launches": -(-T // _native.SCAFFOLD_MAX_SEGS),
                         "torch_ms_median": te[0], "torch_ms_best": te[1],
                         "torch_ops": T + 2,  # T corrections, SGD's weight-decay and update passes
                         "ratio_torch_over_fused": te[0] / tl[0],
                         "fused_TBps_median": 4 * 4 * layout.numel / (tl[0] * 1e-3) / 1e12}

    y, x, c, ci = (torch.randn(P, generator=g, device=dev) for _ in range(4))
    delta, stats = torch.empty_like(y), torch.zeros(4, dtype=torch.int32, device=dev)
    a = _native.scaffold_coeff(5, 0.1)
    tk = go(lambda i: _native.scaffold_finish(y, x, c, ci, delta, P, a, stats))
    ci.normal_(generator=g)

    def eager_finish(i):
        torch.sub(y, x, out=delta)
        ci.sub_(c)
        ci.sub_(delta, alpha=a)

    tt = go(eager_finish)
    out["finish"] = {"fused_ms_median": tk[0], "fused_ms_best": tk[1], "torch_ms_median": tt[0],
                     "torch_ms_best": tt[1], "ratio_torch_over_fused": tt[0] / tk[0],
                     "fused_TBps_median": 6 * 4 * P / (tk[0] * 1e-3) / 1e12}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
