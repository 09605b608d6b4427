"""dls_drive_compress_f32, dls_drive_fedavg_f32 and dls_hadamard_rotate_f32 beside the
scaled-sign pair and dense FedAvg in one run (DESIGN, "Rotated one-bit compression").

Synthetic operands at the ResNet-18 row length (the flat layout's P = 11.2 M fp32), K = 10
and 64 clients for the server's side.  Timing is tools/topk_probe.py's: HIP events around
--batch launches back to back after at least 100 ms of warm-up launches, rotating over --sets
operand sets.
  - compress: w and base read, the bits and scales written, 8 P + P / 8 bytes, against
    dls_efsign_compress_f32's 24 P + P / 8 on the same w and base.
  - fedavg: (K / 8 + 8) P bytes, against dls_efsign_fedavg_f32 (the same bytes, no rotation)
    and one exact dls_fedavg_f32 over K dense rows ((4 K + 4) P bytes).
  - the bare rotation, forward and inverse: 8 P bytes.

Prints one JSON line; ``lib`` names the library file, so a build with the other cross-lane
form (-DDLS_DRIVE_XLANE=0) loaded through DLS_HIP_LIB is told apart.
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
    args = ap.parse_args()
    from distributed_learning_simulator_amd import _native
    from distributed_learning_simulator_amd.layout import ParameterLayout
    from distributed_learning_simulator_amd.model_shapes import resnet18_cifar
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    layout = ParameterLayout(resnet18_cifar())
    P, T = layout.P, len(layout)
    NB = _native.drive_blocks(P)
    Pd = NB * _native.DRIVE_BLOCK
    seg = _native.efsign_layout_segments(layout, dev)
    g = torch.Generator(device=dev).manual_seed(0)

    def run(fn, restore=lambda: None):
        return timed(fn, restore, args.repeats, args.batch, args.warmup_ms, dev)

    def rate(nbytes, t):
        return {"bytes": nbytes, "ms_median": t[0], "ms_best": t[1],
                "bytes_per_s": nbytes / (t[0] * 1e-3),
                "fraction_at_hbm_peak": nbytes / HBM_PEAK / (t[0] * 1e-3)}

    # ---- the client's side
    sets = []
    for _ in range(args.sets):
        base = torch.randn(P, generator=g, device=dev)
        sets.append(dict(w=base + 0.01 * torch.randn(P, generator=g, device=dev), base=base,
                         e=torch.zeros(P, device=dev), y=torch.empty(Pd, device=dev),
                         bits=torch.empty(Pd // 64, dtype=torch.int64, device=dev),
                         scales=torch.empty(NB, device=dev), tscales=torch.empty(T, device=dev),
                         stats=torch.empty(4, dtype=torch.int32, device=dev),
                         ws=_native.efsign_workspace(P, T, dev)))

    def drive(i, scale="unbiased"):
        s = sets[i % len(sets)]
        _native.drive_compress(s["w"], s["base"], P, 7, 1, scale, s["bits"], s["scales"], s["stats"])

    def efsign(i):
        s = sets[i % len(sets)]
        _native.efsign_compress(s["w"], s["base"], s["e"], seg, s["bits"], s["tscales"], s["stats"],
                                s["ws"])

    def rotate(i, inverse=False):
        s = sets[i % len(sets)]
        if inverse:
            _native.hadamard_rotate(s["y"], P, 7, 1, inverse=True, out=s["e"])
        else:
            _native.hadamard_rotate(s["w"], P, 7, 1, out=s["y"])

    compress = {"drive": rate(8 * P + P // 8, run(drive)),
                "drive_mse": rate(8 * P + P // 8, run(lambda i: drive(i, "mse"))),
                "efsign": rate(24 * P + P // 8, run(efsign))}
    compress["ratio_efsign_over_drive"] = (compress["efsign"]["ms_median"] /
                                           compress["drive"]["ms_median"])
    rotation = {"forward": rate(8 * P, run(rotate)),
                "inverse": rate(8 * P, run(lambda i: rotate(i, True)))}
    drive(0)
    assert sets[0]["stats"][0].item() == 0
    del sets

    # ---- the server's side
    base = torch.randn(P, generator=g, device=dev)
    outs = [torch.empty(P, device=dev) for _ in range(args.sets)]
    servers = []
    for K in args.K:
        bits = torch.randint(-2 ** 63, 2 ** 63 - 1, (K, Pd // 64), generator=g, device=dev)
        scales = 0.01 * torch.rand(K, max(NB, T), generator=g, device=dev)
        ns = torch.randint(100, 1001, (K,), generator=g, device=dev).to(torch.float32)
        total = float(ns.sum())
        nbytes = (K / 8 + 8) * P
        rec = {"K": K, "bytes_per_coordinate": K / 8 + 8,
               "drive": rate(nbytes, run(lambda i: _native.drive_fedavg(
                   base, bits, scales, ns, total, P, 7, 1, outs[i % len(outs)]))),
               "efsign": rate(nbytes, run(lambda i: _native.efsign_fedavg(
                   base, bits, scales, seg, ns, total, outs[i % len(outs)])))}
        del bits, scales
        U = 0.01 * torch.randn(K, P, generator=g, device=dev)
        rows = torch.arange(K, dtype=torch.int32, device=dev)
        rec["dense_fedavg"] = rate((4 * K + 4) * P, run(
            lambda i: _native.fedavg(U, rows, ns, total, P, outs[i % len(outs)])))
        rec["ratio_dense_over_drive"] = (rec["dense_fedavg"]["ms_median"] /
                                         rec["drive"]["ms_median"])
        del U
        servers.append(rec)
    print(json.dumps({"probe": "drive", "lib": os.path.basename(_native.LIB_PATH), "P": P, "NB": NB,
                      "batch": args.batch, "sets": args.sets, "compress": compress,
                      "rotation": rotation, "fedavg": servers}), flush=True)


if __name__ == "__main__":
    main()
