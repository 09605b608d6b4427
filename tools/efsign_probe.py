"""dls_efsign_compress_f32 and dls_efsign_fedavg_f32 against the same steps in torch ops and
against dls_fedavg_f32 over the corresponding dense rows (DESIGN, "Scaled-sign compression").

Synthetic operands at the ResNet-18 row length (the flat layout's P = 11.2 M fp32 in 62
tensors), K = 10 and 64 clients for the server's side.  Timing is tools/topk_probe.py's:
HIP events around --batch launches back to back after at least 100 ms of warm-up launches,
rotating over --sets operand sets, the residual restored outside the timed region.
  - compress: the least traffic is reading w, base, e and writing e and the bits, 16 P + P /
    8 bytes; the kernels move 24 P + P / 8 (u is stored and read back once the scales are
    known).  Against u = (w - base) + e; an fp64 index_add_ of |u| per tensor; where();
    a shift-and-sum pack.
  - fedavg: (K / 8 + 8) P bytes.  Against a loop over the clients that unpacks a row to +-1
    and adds c[i][tensor] * sign, and against one exact dls_fedavg_f32 over K dense rows
    ((4 K + 4) P bytes).

Prints one JSON line; ``lib`` names the library file, so a build with the other kernel forms
(-DDLS_EFSIGN_PACK_VEC=1, -DDLS_EFSIGN_DECODE_LDS=1) loaded through DLS_HIP_LIB is told apart.
"""
import argparse
import json
import os
import sys

import torch

# the tree this file lies in, unless PYTHONPATH names another one first
sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.topk_probe import HBM_PEAK, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--K", type=int, nargs="+", default=[10, 64])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4, help="launches per timed interval")
    ap.add_argument("--sets", type=int, default=2, help="operand sets the launches rotate over")
    ap.add_argument("--warmup-ms", type=float, default=100.0)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch-op baselines")
    args = ap.parse_args()
    from distributed_learning_simulator_amd import _native
    from distributed_learning_simulator_amd.layout import ParameterLayout
    from distributed_learning_simulator_amd.model_shapes import resnet18_cifar
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    layout = ParameterLayout(resnet18_cifar())
    P, T = layout.P, len(layout)
    seg = _native.efsign_layout_segments(layout, dev)
    g = torch.Generator(device=dev).manual_seed(0)
    seg_id = torch.repeat_interleave(torch.arange(T, device=dev), seg.bounds.diff())
    real = torch.arange(P, device=dev) < (seg.bounds[:-1] + seg.count)[seg_id]
    shifts = torch.arange(64, device=dev)

    def run(fn, restore=lambda: None, repeats=args.repeats):
        return timed(fn, restore, repeats, args.batch, args.warmup_ms, dev)

    few = max(3, args.repeats // 4)  # the torch-op baselines take many launches each

    # ---- the client's side
    sets = []
    for _ in range(args.sets):
        base = torch.randn(P, generator=g, device=dev)
        e0 = 0.003 * torch.randn(P, generator=g, device=dev)
        sets.append(dict(w=base + 0.01 * torch.randn(P, generator=g, device=dev), base=base, e0=e0,
                         e=torch.empty_like(e0),
                         bits=torch.empty(P // 64, dtype=torch.int64, device=dev),
                         scales=torch.empty(T, device=dev),
                         stats=torch.empty(1, dtype=torch.int32, device=dev),
                         ws=_native.efsign_workspace(P, T, dev)))

    def restore():
        for s in sets:
            s["e"].copy_(s["e0"])

    def fused(i):
        s = sets[i % len(sets)]
        _native.efsign_compress(s["w"], s["base"], s["e"], seg, s["bits"], s["scales"], s["stats"],
                                s["ws"])

    def eager(i):
        s = sets[i % len(sets)]
        u = ((s["w"] - s["base"]) + s["e"]) * real
        l1 = torch.zeros(T, dtype=torch.float64, device=dev).index_add_(0, seg_id, u.abs().double())
        sc = (l1 / seg.count).float()[seg_id]
        neg = u < 0
        s["e"].copy_(torch.where(neg, u + sc, u - sc) * real)
        return (neg.view(-1, 64).to(torch.int64) << shifts).sum(1)

    tf = run(fused, restore)
    floor, moved = 16 * P + P // 8, 24 * P + P // 8
    compress = {"floor_bytes": floor, "moved_bytes": moved, "fused_ms_median": tf[0],
                "fused_ms_best": tf[1], "fused_floor_bytes_per_s": floor / (tf[0] * 1e-3),
                "fused_moved_bytes_per_s": moved / (tf[0] * 1e-3),
                "fused_fraction_of_floor_at_hbm_peak": floor / HBM_PEAK / (tf[0] * 1e-3)}
    if not args.no_torch:
        te = run(eager, restore, few)
        compress.update(torch_ms_median=te[0], torch_ms_best=te[1],
                        ratio_torch_over_fused=te[0] / tf[0])
    restore()
    fused(0)
    assert sets[0]["stats"].tolist() == [0]
    del sets

    # ---- the server's side
    base = torch.randn(P, generator=g, device=dev)
    outs = [torch.empty(P, device=dev) for _ in range(args.sets)]
    servers = []
    for K in args.K:
        bits = torch.randint(-2 ** 63, 2 ** 63 - 1, (K, P // 64), generator=g, device=dev)
        scales = 0.01 * torch.rand(K, T, generator=g, device=dev)
        ns = torch.randint(100, 1001, (K,), generator=g, device=dev).to(torch.float32)
        total = float(ns.sum())
        c = (scales * ns[:, None]) / total

        def fused_server(i):
            _native.efsign_fedavg(base, bits, scales, seg, ns, total, outs[i % len(outs)])

        def eager_server(i):
            out = outs[i % len(outs)]
            out.copy_(base)
            for k in range(K):
                sign = 1.0 - 2.0 * ((bits[k][:, None] >> shifts) & 1).view(-1).float()
                out.add_(sign * c[k][seg_id] * real)

        sf = run(fused_server)
        nbytes = (K / 8 + 8) * P
        rec = {"K": K, "bytes": nbytes, "bytes_per_coordinate": K / 8 + 8,
               "fused_ms_median": sf[0], "fused_ms_best": sf[1],
               "fused_bytes_per_s": nbytes / (sf[0] * 1e-3),
               "fused_fraction_at_hbm_peak": nbytes / HBM_PEAK / (sf[0] * 1e-3)}
        if not args.no_torch:
            se = run(eager_server, repeats=few)
            rec.update(torch_ms_median=se[0], torch_ms_best=se[1],
                       ratio_torch_over_fused=se[0] / sf[0])
        del bits, scales
        U = 0.01 * torch.randn(K, P, generator=g, device=dev)
        rows = torch.arange(K, dtype=torch.int32, device=dev)
        sd = run(lambda i: _native.fedavg(U, rows, ns, total, P, outs[i % len(outs)]))
        rec.update(dense_fedavg_ms_median=sd[0], dense_fedavg_ms_best=sd[1],
                   dense_fedavg_bytes=(4 * K + 4) * P, ratio_dense_over_fused=sd[0] / sf[0])
        del U
        servers.append(rec)
    print(json.dumps({"probe": "efsign", "lib": os.path.basename(_native.LIB_PATH), "P": P, "T": T,
                      "batch": args.batch, "sets": args.sets, "compress": compress,
                      "fedavg": servers}), flush=True)


if __name__ == "__main__":
    main()
