"""dls_qsgd_compress_f32 and dls_qsgd_fedavg_f32 at 2, 4 and 8 bits beside the one-bit servers,
dense FedAvg and the same quantizer in torch ops, in one run (DESIGN, "Stochastic quantization").

Synthetic operands at the ResNet-18 row length (the flat layout's P = 11.2 M fp32), K = 10 and
64 clients for the server's side.  Timing is tools/topk_probe.py's: HIP events around --batch
launches back to back after at least 100 ms of warm-up launches, rotating over --sets operand
sets.
  - compress: w and base read, the codes and scales written, 8 P + b P / 8 bytes, both norms;
    beside it the same quantizer as torch ops on the same w and base (unpacked int8 levels).
  - fedavg: (K b / 8 + 8) P bytes, against dls_efsign_fedavg_f32 and dls_drive_fedavg_f32 ((K /
    8 + 8) P) and one exact dls_fedavg_f32 over K dense rows ((4 K + 4) P bytes).

Prints one JSON line.
"""
import argparse
import json
import os
import sys

import torch

# the tree this file lies in, unless PYTHONPATH names another one first
sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.topk_probe import HBM_PEAK, timed  # noqa: E402


def torch_quantize(w, base, NB, s, norm, g):
    """The contract's quantizer in torch ops: u, the bucket norms, t, the random rounding and
    the signed levels as int8 (one byte per coordinate, not packed)."""
    u = (w - base).view(NB, -1)
    n = u.abs().amax(dim=1, keepdim=True) if norm == "max" else u.double().square().sum(
        dim=1, keepdim=True).sqrt().float()
    t = u.abs() * (s / n)
    l0 = t.floor()
    lev = torch.minimum(l0 + (torch.rand(u.shape, generator=g, device=u.device) < t - l0), n.new_tensor(s))
    return torch.where(u < 0, -lev, lev).to(torch.int8), n / s


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--K", type=int, nargs="+", default=[10, 64])
    ap.add_argument("--bits", type=int, nargs="+", default=[2, 4, 8])
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
    NB = _native.qsgd_buckets(P)
    Pb = NB * _native.QSGD_BUCKET  # the row with its last bucket whole, for the torch view
    seg = _native.efsign_layout_segments(layout, dev)
    g = torch.Generator(device=dev).manual_seed(0)

    def run(fn):
        return timed(fn, lambda: None, args.repeats, args.batch, args.warmup_ms, dev)

    def rate(nbytes, t):
        return {"bytes": nbytes, "ms_median": t[0], "ms_best": t[1],
                "bytes_per_s": nbytes / (t[0] * 1e-3),
                "fraction_at_hbm_peak": nbytes / HBM_PEAK / (t[0] * 1e-3)}

    # ---- the client's side
    sets = []
    for _ in range(args.sets):
        base = torch.zeros(Pb, device=dev)
        base[:P] = torch.randn(P, generator=g, device=dev)
        w = base.clone()
        w[:P] += 0.01 * torch.randn(P, generator=g, device=dev)
        sets.append(dict(w=w, base=base, scales=torch.empty(NB, device=dev),
                         codes=torch.empty(_native.qsgd_code_words(P, 8), dtype=torch.int32, device=dev),
                         stats=torch.empty(4, dtype=torch.int32, device=dev)))

    def qsgd(i, bits, norm):
        s = sets[i % len(sets)]
        _native.qsgd_compress(s["w"], s["base"], P, bits, norm, 7, 1, s["codes"], s["scales"], s["stats"])

    compress = []
    for bits in args.bits:
        rec = {"bits": bits}
        for norm in ("l2", "max"):
            rec[norm] = rate(8 * P + bits * P // 8, run(lambda i: qsgd(i, bits, norm)))
            rec["torch_" + norm] = rate(8 * P + P, run(lambda i: torch_quantize(
                sets[i % len(sets)]["w"], sets[i % len(sets)]["base"], NB, float((1 << (bits - 1)) - 1), norm, g)))
            rec["ratio_torch_over_" + norm] = rec["torch_" + norm]["ms_median"] / rec[norm]["ms_median"]
        compress.append(rec)
    qsgd(0, 4, "l2")
    assert sets[0]["stats"][0].item() == 0
    del sets

    # ---- the server's side
    base = torch.randn(P, generator=g, device=dev)
    outs = [torch.empty(P, device=dev) for _ in range(args.sets)]
    servers = []
    for K in args.K:
        ns = torch.randint(100, 1001, (K,), generator=g, device=dev).to(torch.float32)
        total = float(ns.sum())
        scales = 0.01 * torch.rand(K, max(NB, T, _native.drive_blocks(P)), generator=g, device=dev)
        rec = {"K": K}
        for bits in args.bits:  # any field but -2^(b-1) is a level; random words time the same
            codes = torch.randint(-2 ** 31, 2 ** 31 - 1, (K, _native.qsgd_code_words(P, bits)),
                                  generator=g, device=dev, dtype=torch.int32)
            rec[f"qsgd_b{bits}"] = rate((K * bits / 8 + 8) * P, run(lambda i: _native.qsgd_fedavg(
                base, codes, scales, ns, total, P, bits, outs[i % len(outs)])))
            del codes
        Pd = _native.drive_blocks(P) * _native.DRIVE_BLOCK
        words = torch.randint(-2 ** 63, 2 ** 63 - 1, (K, Pd // 64), generator=g, device=dev)
        rec["drive"] = rate((K / 8 + 8) * P, run(lambda i: _native.drive_fedavg(
            base, words, scales, ns, total, P, 7, 1, outs[i % len(outs)])))
        rec["efsign"] = rate((K / 8 + 8) * P, run(lambda i: _native.efsign_fedavg(
            base, words, scales, seg, ns, total, outs[i % len(outs)])))
        del words
        U = 0.01 * torch.randn(K, P, generator=g, device=dev)
        rows = torch.arange(K, dtype=torch.int32, device=dev)
        rec["dense_fedavg"] = rate((4 * K + 4) * P, run(
            lambda i: _native.fedavg(U, rows, ns, total, P, outs[i % len(outs)])))
        for bits in args.bits:
            rec[f"ratio_dense_over_qsgd_b{bits}"] = (rec["dense_fedavg"]["ms_median"] /
                                                     rec[f"qsgd_b{bits}"]["ms_median"])
        del U
        servers.append(rec)
    print(json.dumps({"probe": "qsgd", "lib": os.path.basename(_native.LIB_PATH), "P": P, "NB": NB,
                      "batch": args.batch, "sets": args.sets, "compress": compress,
                      "fedavg": servers}), flush=True)


if __name__ == "__main__":
    main()
