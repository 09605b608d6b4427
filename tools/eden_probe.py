"""dls_eden_compress_f32 and dls_eden_fedavg_f32 at 2 and 4 bits beside the one-bit rotated
server, the QSGD server at the same bits and dense FedAvg, in one run (DESIGN, "Multi-bit
rotated compression").

Synthetic operands at the ResNet-18 row length (the flat layout's P = 11.2 M fp32), K = 10 and
64 clients for the server's side.  Timing is tools/topk_probe.py's: HIP events around --batch
launches back to back after at least 100 ms of warm-up launches, rotating over --sets operand
sets.
  - compress: w and base read, the codes and scales written, 8 P + b P / 8 bytes, both scales,
    beside dls_drive_compress_f32 (8 P + P / 8) on the same w and base.
  - fedavg: (K b / 8 + 8) P bytes, against dls_qsgd_fedavg_f32 at the same bits (the same bytes,
    no rotation, no table), dls_drive_fedavg_f32 ((K / 8 + 8) P) and one exact dls_fedavg_f32
    over K dense rows ((4 K + 4) P bytes).

Prints one JSON line; ``lib`` names the library file, so a build with another lookup form
loaded through DLS_HIP_LIB is told apart.
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
    ap.add_argument("--bits", type=int, nargs="+", default=[2, 4])
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
    P = ParameterLayout(resnet18_cifar()).P
    NB = _native.drive_blocks(P)
    g = torch.Generator(device=dev).manual_seed(0)

    def run(fn):
        return timed(fn, lambda: None, args.repeats, args.batch, args.warmup_ms, dev)

    def rate(nbytes, t):
        return {"bytes": nbytes, "ms_median": t[0], "ms_best": t[1],
                "bytes_per_s": nbytes / (t[0] * 1e-3),
                "fraction_at_hbm_peak": nbytes / HBM_PEAK / (t[0] * 1e-3)}

    # ---- the client's side
    compress = []
    sets = []
    for _ in range(args.sets):
        base = torch.randn(P, generator=g, device=dev)
        sets.append(dict(w=base + 0.01 * torch.randn(P, generator=g, device=dev), base=base,
                         codes=torch.empty(_native.eden_code_words(P, 4), dtype=torch.int32, device=dev),
                         bits=torch.empty(NB * _native.DRIVE_BLOCK // 64, dtype=torch.int64, device=dev),
                         scales=torch.empty(NB, device=dev),
                         stats=torch.empty(4, dtype=torch.int32, device=dev)))

    def eden(i, bits, scale):
        s = sets[i % len(sets)]
        _native.eden_compress(s["w"], s["base"], P, bits, 7, 1, scale, s["codes"], s["scales"], s["stats"])

    def drive(i):
        s = sets[i % len(sets)]
        _native.drive_compress(s["w"], s["base"], P, 7, 1, "unbiased", s["bits"], s["scales"], s["stats"])

    for bits in args.bits:
        compress.append({"bits": bits, **{scale: rate(8 * P + bits * P // 8, run(
            lambda i: eden(i, bits, scale))) for scale in ("unbiased", "mse")}})
    compress.append({"bits": 1, "drive": rate(8 * P + P // 8, run(drive))})
    eden(0, 4, "unbiased")
    assert sets[0]["stats"][0].item() == 0
    del sets

    # ---- the server's side
    base = torch.randn(P, generator=g, device=dev)
    outs = [torch.empty(P, device=dev) for _ in range(args.sets)]
    servers = []
    for K in args.K:
        ns = torch.randint(100, 1001, (K,), generator=g, device=dev).to(torch.float32)
        total = float(ns.sum())
        scales = 0.01 * torch.rand(K, max(NB, _native.qsgd_buckets(P)), generator=g, device=dev)
        rec = {"K": K}
        for bits in args.bits:  # every field is a level: random words time the same
            codes = torch.randint(-2 ** 31, 2 ** 31 - 1, (K, max(_native.eden_code_words(P, bits),
                                                                 _native.qsgd_code_words(P, bits))),
                                  generator=g, device=dev, dtype=torch.int32)
            rec[f"eden_b{bits}"] = rate((K * bits / 8 + 8) * P, run(lambda i: _native.eden_fedavg(
                base, codes, scales, ns, total, P, bits, 7, 1, outs[i % len(outs)])))
            rec[f"qsgd_b{bits}"] = rate((K * bits / 8 + 8) * P, run(lambda i: _native.qsgd_fedavg(
                base, codes, scales, ns, total, P, bits, outs[i % len(outs)])))
            rec[f"ratio_eden_over_qsgd_b{bits}"] = (rec[f"eden_b{bits}"]["ms_median"] /
                                                    rec[f"qsgd_b{bits}"]["ms_median"])
            del codes
        words = torch.randint(-2 ** 63, 2 ** 63 - 1, (K, NB * _native.DRIVE_BLOCK // 64),
                              generator=g, device=dev)
        rec["drive"] = rate((K / 8 + 8) * P, run(lambda i: _native.drive_fedavg(
            base, words, scales, ns, total, P, 7, 1, outs[i % len(outs)])))
        del words
        U = 0.01 * torch.randn(K, P, generator=g, device=dev)
        rows = torch.arange(K, dtype=torch.int32, device=dev)
        rec["dense_fedavg"] = rate((4 * K + 4) * P, run(
            lambda i: _native.fedavg(U, rows, ns, total, P, outs[i % len(outs)])))
        del U
        servers.append(rec)
    print(json.dumps({"probe": "eden", "lib": os.path.basename(_native.LIB_PATH), "P": P, "NB": NB,
                      "batch": args.batch, "sets": args.sets, "compress": compress,
                      "fedavg": servers}), flush=True)


if __name__ == "__main__":
    main()
