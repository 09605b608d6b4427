"""dls_sketch_f32, dls_unsketch_f32 and one FedSketchServer round beside the same sketch in
torch ops and dls_topk_compress_f32 in one run (DESIGN, "FetchSGD's Count Sketch").

Synthetic operands at the ResNet-18 row length (the flat layout's P = 11.2 M fp32), R = 5 rows
and C = 2^18 columns (--cols: further table widths for the two kernels alone).  Timing is
tools/topk_probe.py's: HIP events around --batch launches back to back after at least 100 ms
of warm-up launches, rotating over --sets operand sets.
  - sketch: every row of the table reads the update again, so the logical traffic is R * 4 P
    bytes without base and R * 8 P with it; the bytes HBM must deliver are 4 P (8 P) if the
    re-reads hit the caches.  Both rates are reported.
  - unsketch: 4 P bytes written and the table read.
  - server_round: FedSketchServer's steps 1-8 over K = 10 tables, end to end with its torch
    glue (a host clock around a synchronise).
  - torch_index_add: u = w - base, then per row table[r].index_add_(0, bucket[r], sign[r] * u)
    with the bucket and sign tensors built beforehand from the same Philox words (not timed);
    floating-point atomics, so its bits vary.  Its table is compared with the kernel's.
  - topk_compress: dls_topk_compress_f32 at k = 0.01 P, the compressor of the client that
    can keep a residual.

Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import torch

# the tree this file lies in, unless PYTHONPATH names another one first
sys.path.append(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.topk_probe import HBM_PEAK, timed  # noqa: E402

SEED, STREAM = 7, 3


def torch_hash(P, R, C, dev):
    """(bucket int64 [R, P], sign fp32 [R, P]) of the contract, from dls_philox_u32's words."""
    from distributed_learning_simulator_amd import _native
    NQ = -(-P // C)
    j = torch.arange(P, device=dev)
    m = _native.philox_u32(8 * NQ, SEED, STREAM, device=dev).view(NQ, 8).to(torch.int64) & (C - 1)
    bucket = torch.stack([(j % C) ^ m[j // C, r] for r in range(R)])
    sign = torch.empty((R, P), device=dev)
    for r in range(R):
        w = _native.philox_u32(-(-P // 32), SEED, STREAM, first=2 ** 32 + r * 2 ** 26, device=dev)
        sign[r] = 1.0 - 2.0 * ((w.to(torch.int64)[j // 32] >> (j % 32)) & 1)
    return bucket, sign


def main():
    ap = argparse.ArgumentParser(description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=5)
    ap.add_argument("--cols", type=int, nargs="+", default=[1 << 18])
    ap.add_argument("--K", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4, help="launches per timed interval")
    ap.add_argument("--sets", type=int, default=2, help="operand sets the launches rotate over")
    ap.add_argument("--warmup-ms", type=float, default=100.0)
    args = ap.parse_args()
    from distributed_learning_simulator_amd import _native
    from distributed_learning_simulator_amd.layout import ParameterLayout
    from distributed_learning_simulator_amd.model_shapes import resnet18_cifar
    from distributed_learning_simulator_amd.servers.fed_sketch_server import FedSketchServer
    from distributed_learning_simulator_amd.workers.fed_sketch_worker import SketchUpdate
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    shapes = list(resnet18_cifar())
    P, R = ParameterLayout(shapes).P, args.rows
    g = torch.Generator(device=dev).manual_seed(0)

    def run(fn):
        return timed(fn, lambda: None, args.repeats, args.batch, args.warmup_ms, dev)

    def rate(logical, hbm, t):
        return {"logical_bytes": logical, "hbm_bytes": hbm, "ms_median": t[0], "ms_best": t[1],
                "logical_bytes_per_s": logical / (t[0] * 1e-3),
                "hbm_fraction_of_peak": hbm / HBM_PEAK / (t[0] * 1e-3)}

    sets = []
    for _ in range(args.sets):
        base = torch.randn(P, generator=g, device=dev)
        sets.append(dict(w=base + 0.01 * torch.randn(P, generator=g, device=dev), base=base,
                         est=torch.empty(P, device=dev), e=torch.zeros(P, device=dev),
                         stats=torch.empty(4, dtype=torch.int32, device=dev)))
    kernels = []
    for C in args.cols:
        tables = [torch.empty((R, C), device=dev) for _ in sets]
        ws = _native.sketch_workspace(P, R, C, dev)

        def sketch(i, with_base=True):
            s = sets[i % len(sets)]
            _native.sketch(s["w"], s["base"] if with_base else None, P, R, C, SEED, STREAM,
                           tables[i % len(sets)], s["stats"], ws)

        kernels.append({
            "C": C, "workspace_bytes": ws.numel(),
            "sketch": rate(R * 8 * P, 8 * P + 4 * R * C, run(sketch)),
            "sketch_no_base": rate(R * 4 * P, 4 * P + 4 * R * C, run(lambda i: sketch(i, False))),
            "unsketch": rate(4 * P + 4 * R * C, 4 * P + 4 * R * C, run(lambda i: _native.unsketch(
                tables[i % len(sets)], P, R, C, SEED, STREAM, sets[i % len(sets)]["est"])))})
        assert sets[0]["stats"][0].item() == 0

    # ---- the baselines, at the first width
    C = args.cols[0]
    table = torch.empty((R, C), device=dev)
    _native.sketch(sets[0]["w"], sets[0]["base"], P, R, C, SEED, STREAM, table, sets[0]["stats"],
                   _native.sketch_workspace(P, R, C, dev))
    bucket, sign = torch_hash(P, R, C, dev)
    ttab = torch.empty((R, C), device=dev)

    def index_add(i):
        s = sets[i % len(sets)]
        u = s["w"] - s["base"]
        ttab.zero_()
        for r in range(R):
            ttab[r].index_add_(0, bucket[r], sign[r] * u)

    t_index_add = run(index_add)
    index_add(0)
    worst = float((ttab - table).abs().max())  # about 43 terms of 0.01: fp32 reordering only
    assert worst < 1e-5, worst
    del bucket, sign
    k = P // 100
    idx, val = torch.empty(k, dtype=torch.int32, device=dev), torch.empty(k, device=dev)
    tws = _native.topk_workspace(P, dev)

    def topk(i):
        s = sets[i % len(sets)]
        _native.topk_compress(s["w"], s["base"], s["e"], k, P, idx, val, s["stats"], tws)

    t_topk = run(topk)
    del sets

    # ---- the server's round: K tables in, the new model out
    server = FedSketchServer(rows=R, cols=C, ratio=0.01, momentum=0.9, seed=SEED, stream_id=STREAM,
                             initial_model={n: torch.zeros(s, device=dev) for n, s in shapes},
                             tester=None, worker_number=args.K, synchronous=True, device=dev)
    ids = list(range(args.K))
    server._payloads = {i: (100 + i, SketchUpdate(0.01 * torch.randn(R, C, generator=g, device=dev), P))
                        for i in ids}
    ms = []
    for n in range(3 + args.repeats):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        server._sketch_flat(ids)
        torch.cuda.synchronize(dev)
        ms.append((time.perf_counter() - t0) * 1e3)
    ms = sorted(ms[3:])
    sk = kernels[0]["sketch"]["ms_median"]
    print(json.dumps({
        "probe": "sketch", "lib": os.path.basename(_native.LIB_PATH), "P": P, "R": R,
        "batch": args.batch, "sets": args.sets, "kernels": kernels,
        "torch_index_add": {"C": C, "ms_median": t_index_add[0], "ms_best": t_index_add[1],
                            "max_abs_difference_to_kernel": worst},
        "ratio_index_add_over_sketch": t_index_add[0] / sk,
        "topk_compress": {"k": k, "ms_median": t_topk[0], "ms_best": t_topk[1]},
        "ratio_topk_over_sketch": t_topk[0] / sk,
        "server_round": {"K": args.K, "C": C, "k": server.k, "ms_median": ms[len(ms) // 2],
                         "ms_best": ms[0]}}), flush=True)


if __name__ == "__main__":
    main()
