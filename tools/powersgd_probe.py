"""dls_powersgd_compress_f32 and dls_powersgd_fedavg_f32 beside the same steps in torch ops,
dls_topk_compress_f32 and dense dls_fedavg_f32 in one run (DESIGN, "Low-rank compression").

Synthetic operands at the ResNet-18 row (the flat layout's P = 11.2 M fp32).  Timing is
tools/topk_probe.py's: HIP events around --batch launches back to back after at least 100 ms
of warm-up launches, rotating over --sets operand sets; median, best and worst are reported.
  - compress: r = 1, 4, 16; the traffic counted is 24 bytes per coordinate (12 read and 4
    written in the first pass, 4 + 4 in the last).
  - torch_compress: per compressed tensor matmul, torch.linalg.qr, matmul and addmm on views of
    the same flat rows, u = (w - base) + e formed once for the row.
  - topk_compress: dls_topk_compress_f32 at k = 0.01 P.
  - fedavg: K = 10 and 64 at r = 4 and 16; 8 bytes per coordinate plus the factors.  The regime
    named is the one the arithmetic says: 2 K r flops per coordinate against 8 bytes.
  - torch_fedavg: per compressed tensor one baddbmm of the stacked fl(c_i P^_i) and Q_i onto base.
  - dense_fedavg: dls_fedavg_f32 over K dense rows.

Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

# the tree this file lies in, unless PYTHONPATH names another one first
sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.topk_probe import HBM_PEAK  # noqa: E402

MFMA_F32_PEAK = 157.3e12  # MI355X dense fp32 matrix flop/s


def timed(fn, repeats, batch, warmup_ms, dev):
    """ms per launch, median / best / worst of ``repeats`` intervals of ``batch`` launches."""
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
    return {"ms_median": statistics.median(ms), "ms_best": min(ms), "ms_worst": max(ms)}


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--ranks", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--server-ranks", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--K", type=int, nargs="+", default=[10, 64])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4, help="launches per timed interval")
    ap.add_argument("--sets", type=int, default=2, help="operand sets the launches rotate over")
    ap.add_argument("--warmup-ms", type=float, default=100.0)
    args = ap.parse_args()
    from distributed_learning_simulator_amd import _native
    from distributed_learning_simulator_amd.layout import ParameterLayout
    from distributed_learning_simulator_amd.model_shapes import resnet18_cifar
    from distributed_learning_simulator_amd.workers.fed_powersgd_worker import sent_floats
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lay = ParameterLayout(list(resnet18_cifar()))
    P = lay.P
    g = torch.Generator(device=dev).manual_seed(0)

    def run(fn):
        return timed(fn, args.repeats, args.batch, args.warmup_ms, dev)

    sets = []
    for _ in range(args.sets):
        base = torch.randn(P, generator=g, device=dev)
        sets.append(dict(w=base + 0.01 * torch.randn(P, generator=g, device=dev), base=base,
                         e=torch.zeros(P, device=dev), stats=torch.empty(4, dtype=torch.int32, device=dev)))
    client = []
    for r in args.ranks:
        plan = _native.powersgd_layout_plan(lay, r, dev)
        ws = _native.powersgd_workspace(plan, dev)
        q0 = torch.randn(plan.L, generator=g, device=dev)
        payload = torch.empty(plan.L, device=dev)
        views = [(o, n, m, po, qo) for o, n, m, kind, po, qo, *_ in plan.rows[:plan.T] if kind]

        def compress(i):
            s = sets[i % len(sets)]
            _native.powersgd_compress(s["w"], s["base"], s["e"], plan, q0, payload, s["stats"], ws)

        def torch_compress(i):
            s = sets[i % len(sets)]
            u = (s["w"] - s["base"]) + s["e"]
            for o, n, m, po, qo in views:
                U = u[o:o + n * m].view(n, m)
                Ph = torch.linalg.qr(U @ q0[qo:qo + m * r].view(m, r)).Q
                Q = U.t() @ Ph
                payload[po:po + n * r].view(n, r).copy_(Ph)
                payload[qo:qo + m * r].view(m, r).copy_(Q)
                torch.addmm(U, Ph, Q.t(), alpha=-1.0, out=s["e"][o:o + n * m].view(n, m))

        t = run(compress)
        assert sets[0]["stats"][0].item() == 0
        for s in sets:
            s["e"].zero_()
        client.append({"r": r, "compressed_tensors": len(views), "payload_floats": sent_floats(plan),
                       "workspace_bytes": ws.numel(), "compress": t,
                       "bytes": 24 * P, "hbm_fraction_of_peak": 24 * P / HBM_PEAK / (t["ms_median"] * 1e-3),
                       "torch_compress": run(torch_compress)})
        client[-1]["ratio_torch_over_compress"] = \
            client[-1]["torch_compress"]["ms_median"] / t["ms_median"]
        for s in sets:
            s["e"].zero_()
        compress(0)  # agreement of the two paths: the residual norms of one step from e = 0
        mine = float(sets[0]["e"].norm())
        sets[0]["e"].zero_()
        torch_compress(0)
        client[-1]["residual_norm"] = {"compress": mine, "torch": float(sets[0]["e"].norm())}
        for s in sets:
            s["e"].zero_()
    k = P // 100
    idx, val = torch.empty(k, dtype=torch.int32, device=dev), torch.empty(k, device=dev)
    tws = _native.topk_workspace(P, dev)
    t_topk = run(lambda i: _native.topk_compress(sets[i % len(sets)]["w"], sets[i % len(sets)]["base"],
                                                  sets[i % len(sets)]["e"], k, P, idx, val,
                                                  sets[i % len(sets)]["stats"], tws))
    base = sets[0]["base"]
    del sets
    server, out = [], torch.empty(P, device=dev)
    for K in args.K:
        weight = torch.arange(100, 100 + K, device=dev, dtype=torch.float32)
        total = float(weight.sum())
        rows = torch.arange(K, dtype=torch.int32, device=dev)
        dense = base[None] + 0.01 * torch.randn(K, P, generator=g, device=dev)
        t_dense = run(lambda i: _native.fedavg(dense, rows, weight, total, P, out))
        del dense
        for r in args.server_ranks:
            plan = _native.powersgd_layout_plan(lay, r, dev)
            pay = 0.1 * torch.randn(K, plan.L, generator=g, device=dev)
            views = [(o, n, m, po, qo) for o, n, m, kind, po, qo, *_ in plan.rows[:plan.T] if kind]
            c = (weight / total).view(K, 1, 1)

            def torch_fedavg(i):
                for o, n, m, po, qo in views:
                    A = (c * pay[:, po:po + n * r].view(K, n, r)).permute(1, 0, 2).reshape(1, n, K * r)
                    B = pay[:, qo:qo + m * r].view(K, m, r).permute(0, 2, 1).reshape(1, K * r, m)
                    torch.baddbmm(base[o:o + n * m].view(1, n, m), A, B,
                                  out=out[o:o + n * m].view(1, n, m))

            t = run(lambda i: _native.powersgd_fedavg(base, pay, plan, weight, total, out))
            flops, nbytes = 2.0 * K * r * P, 8 * P + 4 * K * plan.L
            server.append({"K": K, "r": r, "fedavg": t, "bytes": nbytes, "flops": flops,
                           "hbm_fraction_of_peak": nbytes / HBM_PEAK / (t["ms_median"] * 1e-3),
                           "mfma_fraction_of_peak": flops / MFMA_F32_PEAK / (t["ms_median"] * 1e-3),
                           "regime": "memory" if nbytes / HBM_PEAK > flops / MFMA_F32_PEAK else "mfma",
                           "torch_fedavg": run(torch_fedavg), "dense_fedavg": t_dense})
            server[-1]["ratio_torch_over_fedavg"] = \
                server[-1]["torch_fedavg"]["ms_median"] / t["ms_median"]
            del pay
    print(json.dumps({"probe": "powersgd", "lib": os.path.basename(_native.LIB_PATH), "P": P,
                      "batch": args.batch, "sets": args.sets, "repeats": args.repeats,
                      "client": client, "topk_compress": {"k": k, **t_topk}, "server": server}),
          flush=True)


if __name__ == "__main__":
    main()
