"""dls_mx_compress_f32 and dls_mx_fedavg_f32 (E4M3, E5M2, E2M1) beside the QSGD pair, dense FedAvg
and the same quantizer in torch ops, in one run (DESIGN, "Microscaling FP8 / FP4").

Synthetic operands at the ResNet-18 row length (the flat layout's P = 11.2 M fp32), K = 10 and
64 clients for the server's side.  Timing is tools/topk_probe.py's: HIP events around --batch
launches back to back after at least 100 ms of warm-up launches, rotating over --sets operand
sets.
  - compress: w and base read, the codes and scale bytes written, 8 P + b P / 8 + P / 32 bytes
    (8 P more with the residual), every format and rounding; beside it the same quantizer as
    torch ops on the same w and base (values on the element grid, not packed).
  - fedavg: (K (b / 8 + 1 / 32) + 8) P bytes, against dls_qsgd_fedavg_f32 at 4 bits (beside
    E2M1) and 8 bits (beside the FP8 formats), (K b / 8 + 8) P, and one exact dls_fedavg_f32
    over K dense rows ((4 K + 4) P bytes).

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

# format -> (mantissa bits, emax, emin, fmax)
GRID = {"e4m3": (3, 8, -6, 448.0), "e5m2": (2, 15, -14, 57344.0), "e2m1": (1, 2, 0, 6.0)}


def torch_quantize(w, base, fmt, rounding, g):
    """The contract's quantizer in torch ops: u, the blocks' power-of-two scales, t, the grid
    step at t and the rounding; returns the decoded values and the scale exponents."""
    M, _, emin, fmax = GRID[fmt]
    u = (w - base).view(-1, 32)
    e = torch.ceil(torch.log2(u.abs().amax(dim=1, keepdim=True) / fmax)).clamp(-127, 127)
    t = torch.ldexp(u.abs(), -e)
    q = torch.exp2(torch.floor(torch.log2(t)).clamp(min=emin) - M)
    l0 = torch.floor(t / q)
    f = t / q - l0
    if rounding == "nearest":
        up = (f > 0.5) | ((f == 0.5) & (l0 % 2 == 1))
    else:
        up = torch.rand(u.shape, generator=g, device=u.device) < f
    return torch.copysign(torch.ldexp((l0 + up) * q, e), u), e.to(torch.int16)


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
    P = ParameterLayout(resnet18_cifar()).P
    NG = -(-P // _native.MX_GROUP)
    Pb = NG * _native.MX_GROUP  # the row with its last group whole, for the torch view
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
        sets.append(dict(w=w, base=base, residual=torch.zeros(P, device=dev),
                         scales=torch.empty(_native.mx_scale_bytes(P), dtype=torch.uint8, device=dev),
                         codes=torch.empty(_native.mx_code_words(P, "e4m3"), dtype=torch.int32, device=dev),
                         stats=torch.empty(4, dtype=torch.int32, device=dev)))

    def mx(i, fmt, rounding, feedback=False):
        s = sets[i % len(sets)]
        _native.mx_compress(s["w"], s["base"], s["residual"] if feedback else None, P, fmt, rounding,
                            7, 1, s["codes"], s["scales"], s["stats"])

    compress = []
    for fmt in _native.MX_FORMATS:
        b = _native.mx_code_bits(fmt)
        rec = {"format": fmt}
        for rounding in _native.MX_ROUNDINGS:
            rec[rounding] = rate(8 * P + b * P // 8 + P // 32, run(lambda i: mx(i, fmt, rounding)))
            rec["torch_" + rounding] = rate(8 * P + 4 * P, run(lambda i: torch_quantize(
                sets[i % len(sets)]["w"], sets[i % len(sets)]["base"], fmt, rounding, g)))
            rec["ratio_torch_over_" + rounding] = (rec["torch_" + rounding]["ms_median"] /
                                                   rec[rounding]["ms_median"])
        rec["nearest_with_residual"] = rate(16 * P + b * P // 8 + P // 32,
                                            run(lambda i: mx(i, fmt, "nearest", True)))
        compress.append(rec)
    mx(0, "e4m3", "nearest")
    assert sets[0]["stats"][0].item() == 0
    del sets

    # ---- the server's side
    base = torch.randn(P, generator=g, device=dev)
    outs = [torch.empty(P, device=dev) for _ in range(args.sets)]
    servers = []
    for K in args.K:
        ns = torch.randint(100, 1001, (K,), generator=g, device=dev).to(torch.float32)
        total = float(ns.sum())
        sbytes = torch.randint(100, 140, (K, _native.mx_scale_bytes(P)), generator=g, device=dev,
                               dtype=torch.uint8)
        qscales = 0.01 * torch.rand(K, _native.qsgd_buckets(P), generator=g, device=dev)
        rec = {"K": K}
        for fmt in _native.MX_FORMATS:
            b = _native.mx_code_bits(fmt)
            # random words with bit 3 of every nibble clear: no NaN or infinity encoding
            codes = torch.randint(-2 ** 31, 2 ** 31 - 1, (K, _native.mx_code_words(P, fmt)),
                                  generator=g, device=dev, dtype=torch.int32) & 0x77777777
            rec["mx_" + fmt] = rate((K * (b / 8 + 1 / 32) + 8) * P, run(lambda i: _native.mx_fedavg(
                base, codes, sbytes, ns, total, P, fmt, outs[i % len(outs)])))
            del codes
        for bits in (4, 8):
            codes = torch.randint(-2 ** 31, 2 ** 31 - 1, (K, _native.qsgd_code_words(P, bits)),
                                  generator=g, device=dev, dtype=torch.int32)
            rec[f"qsgd_b{bits}"] = rate((K * bits / 8 + 8) * P, run(lambda i: _native.qsgd_fedavg(
                base, codes, qscales, ns, total, P, bits, outs[i % len(outs)])))
            del codes
        U = 0.01 * torch.randn(K, P, generator=g, device=dev)
        rows = torch.arange(K, dtype=torch.int32, device=dev)
        rec["dense_fedavg"] = rate((4 * K + 4) * P, run(
            lambda i: _native.fedavg(U, rows, ns, total, P, outs[i % len(outs)])))
        del U
        for fmt, bits in (("e2m1", 4), ("e4m3", 8), ("e5m2", 8)):
            rec[f"ratio_mx_{fmt}_over_qsgd_b{bits}"] = (rec["mx_" + fmt]["ms_median"] /
                                                        rec[f"qsgd_b{bits}"]["ms_median"])
            rec[f"ratio_dense_over_mx_{fmt}"] = (rec["dense_fedavg"]["ms_median"] /
                                                 rec["mx_" + fmt]["ms_median"])
        servers.append(rec)
    print(json.dumps({"probe": "mx", "lib": os.path.basename(_native.LIB_PATH), "P": P, "NG": NG,
                      "batch": args.batch, "sets": args.sets, "compress": compress,
                      "fedavg": servers}), flush=True)


if __name__ == "__main__":
    main()
