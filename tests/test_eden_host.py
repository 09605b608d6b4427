"""fed_eden without a GPU: the committed codebooks, the reference's error against the
codebook's own and against QSGD's, the library's argument checks and their order, factory
dispatch and the simulator's flags."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import cpu_doubles, eden_ref as ref, qsgd_ref
from tests.test_topk_host import CPU, FakeTrainer, initial_model, make_model

F32 = np.float32


def cells(b):
    """(p_m, conditional mean) of |N(0, 1)| over the cells of the committed boundaries, fp64."""
    from tools.eden_tables import Phi, cell_mean
    edges = [0.0] + [float(t) for t in ref.EDEN_BOUNDS[b]] + [math.inf]
    return [(2.0 * (Phi(hi) - Phi(lo)), cell_mean(lo, hi)) for lo, hi in zip(edges, edges[1:])]


@pytest.mark.parametrize("b", [2, 4])
def test_tables_are_lloyd_max(b):
    """Centroid = conditional mean of its cell, boundary = midpoint, to 1e-6 relative; the
    header carries the binding's values."""
    cent, bound = ref.EDEN_CENTROIDS[b], ref.EDEN_BOUNDS[b]
    assert len(cent) == 1 << (b - 1) and len(bound) == len(cent) - 1
    for c, (_, mean) in zip(cent, cells(b)):
        assert abs(c - mean) <= 1e-6 * mean
    for m, t in enumerate(bound):
        assert abs(t - 0.5 * (cent[m] + cent[m + 1])) <= 1e-6 * t
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "dls_hip.h")).read()
    for name, table in (("CENT", cent), ("BOUND", bound)):
        body = re.search(rf"#define DLS_EDEN_{name}{b} \{{(.*?)\}}", header).group(1)
        assert tuple(float.fromhex(x.strip().rstrip("f")) for x in body.split(",")) == table
        assert all(F32(x) == x for x in table)


@pytest.mark.parametrize("b", [2, 4])
def test_reference_error(b):
    """8 blocks of N(0, 1): the min-MSE decode's NMSE is the codebook's distortion 1 - sum p_m
    cent_m^2 within 5 % (the sampling error of 32,768 coordinates is about 1 %), and the
    unbiased decode's NMSE lies below QSGD's at the same bits under either norm."""
    rng = np.random.default_rng(2022)
    P = 8 * ref.D
    u, base = rng.standard_normal(P).astype(F32), np.zeros(P, F32)
    words = rng.integers(0, 2 ** 32, P, dtype=np.uint64).astype(np.uint32)
    y = ref.rotate(u, P, words[:P // 32]).astype(np.float64)

    def nmse(mode):
        codes, scales, bad = ref.compress(u, base, P, b, words[:P // 32], mode)
        assert bad == 0
        return ((ref.decode(codes, scales, b) - y) ** 2).sum() / (y ** 2).sum()

    distortion = 1.0 - sum(p * float(c) ** 2 for (p, _), c in zip(cells(b), ref.EDEN_CENTROIDS[b]))
    assert abs(nmse(1) - distortion) <= 0.05 * distortion
    for norm in (0, 1):
        codes, scales, _ = qsgd_ref.compress(u, base, P, b, norm, words)
        q = ((qsgd_ref.decode(codes, scales, P, b) - u) ** 2).sum() / (u.astype(np.float64) ** 2).sum()
        assert nmse(0) < q


def test_library_checks_and_their_order():
    """Fake 16-byte aligned addresses: every call is refused before anything is launched or
    written.  DLS_EINVAL (-1) for the values, then DLS_ELAYOUT (-2), then the overlaps (-1)."""
    from distributed_learning_simulator_amd import _native
    L, u64 = _native.lib(), ctypes.c_uint64
    a, b, c, d, e = (ctypes.c_void_p(k << 24) for k in (1, 2, 3, 4, 5))
    off = ctypes.c_void_p((1 << 24) + 4)

    def compress(w=a, base=b, P=4096, bits=4, mode=0, codes=c, scales=d, stats=e):
        return L.dls_eden_compress_f32(w, base, P, bits, u64(0), u64(1), mode, codes, scales, stats, None)

    def fedavg(base=a, codes=b, ldc=512, scales=c, lds=1, K=1, P=4096, bits=4, out=d):
        return L.dls_eden_fedavg_f32(base, codes, ldc, scales, lds, e, 4.0, K, P, bits, u64(0), u64(1),
                                     out, None)

    got = [compress(stats=None), compress(bits=3), compress(bits=8), compress(mode=2), compress(P=0),
           compress(P=1 << 31), compress(P=96, bits=1), compress(w=off, mode=-1),
           compress(P=96), compress(w=off), compress(codes=off), compress(scales=off),
           compress(P=96, codes=a), compress(codes=a), compress(scales=b), compress(stats=b)]
    assert got == [-1] * 8 + [-2] * 5 + [-1] * 3
    assert b"alias w or base" in L.dls_last_error()
    got = [fedavg(out=None), fedavg(bits=3), fedavg(K=0), fedavg(P=32), fedavg(P=96, K=0),
           fedavg(P=96), fedavg(ldc=511), fedavg(lds=0), fedavg(codes=off), fedavg(ldc=511, out=a),
           fedavg(out=a)]
    assert got == [-1] * 5 + [-2] * 5 + [-1]
    assert fedavg(bits=2, ldc=255) == -2 and fedavg(bits=2, ldc=256, out=a) == -1  # 128 * 2 words


def test_binding_messages():
    from distributed_learning_simulator_amd import _native
    assert [_native.eden_code_words(P, b) for P, b in ((64, 2), (4096, 4), (4160, 4))] == [256, 512, 1024]
    w, codes, scales = torch.zeros(4096), torch.zeros(512, dtype=torch.int32), torch.zeros(1)
    good = dict(w=w, base=torch.zeros(4096), P=4096, bits=4, seed=0, stream_id=1, scale="mse",
                codes=codes, scales=scales, stats=torch.zeros(4, dtype=torch.int32))
    for match, change in (("not on the GPU", {}), ("bits=3", {"bits": 3}), ("bits=True", {"bits": True}),
                          ("scale='l2'", {"scale": "l2"}), ("multiple of 64", {"P": 1000}),
                          ("codes must be an int32", {"codes": codes[:256]}), ("seed=-1", {"seed": -1}),
                          ("w and codes overlap", {"codes": w.view(torch.int32)}),
                          ("16-byte aligned", {"w": torch.zeros(4100)[1:]})):
        with pytest.raises(RuntimeError, match=match):
            _native.eden_compress(**{**good, **change})
    good = dict(base=w, codes=codes[None], scales=scales[None], weight=torch.ones(1), total=1.0,
                P=4096, bits=4, seed=0, stream_id=1, out=torch.zeros(4096))
    for match, change in (("not on the GPU", {}), (r"codes must be an int32 \[K=1, >= 512\]",
                                                    {"codes": codes[None, :256]}),
                          ("bits=8", {"bits": 8}), ("total=0.0", {"total": 0.0}),
                          ("out and base overlap", {"out": w})):
        with pytest.raises(RuntimeError, match=match):
            _native.eden_fedavg(**{**good, **change})


def test_factory_sharding_and_refusals(monkeypatch):
    from distributed_learning_simulator_amd import factory
    from distributed_learning_simulator_amd.servers.fed_eden_server import FedEDENServer
    from distributed_learning_simulator_amd.workers.fed_eden_worker import EDENUpdate, FedEDENWorker
    cpu_doubles.install(monkeypatch)
    make = lambda **kw: factory.get_server("fed_eden", sharded=False, initial_model=initial_model(),
                                           tester=None, worker_number=3, synchronous=True,
                                           device=CPU, **kw)
    server = make(bits=2, seed=7)
    assert type(server) is FedEDENServer and (server.bits, server.seed) == (2, 7)
    kwargs = dict(worker_id=0, trainer=FakeTrainer(make_model(), 10), worker_data_queue=None, round=1)
    worker = factory.get_worker("fed_eden", bits=2, scale="mse", seed=7, **kwargs)
    assert type(worker) is FedEDENWorker and (worker.bits, worker.scale, worker.seed) == (2, "mse", 7)
    for bad in ({"bits": 3}, {"scale": "l2"}, {"seed": -1}):
        with pytest.raises(ValueError, match="FedEDENWorker: "):
            factory.get_worker("fed_eden", **{**kwargs, **bad})
    with pytest.raises(RuntimeError, match="one-process server only"):
        factory.get_server("fed_eden", sharded=True, tester=None, worker_number=2)
    for extra in ({"aggregation_rule": "median"}, {"server_optimizer": "adam"}, {"dp_clip": 1.0},
                  {"attack": "sign_flip", "attackers": (1,)}, {"aggregation_mode": "fma"}, {"bits": 8},
                  {"seed": -1}):
        with pytest.raises(ValueError, match="rotated codes and scales|one arithmetic|bits=8|seed="):
            make(**extra)
    good = (torch.zeros(256, dtype=torch.int32), torch.ones(1), 128, 2)  # P = 128: one block
    assert EDENUpdate(*good).nbytes == 256 * 4 + 4
    for match, change in (("must be an EDENUpdate", None), ("P=64", {2: 64}), ("bits=4", {3: 4}),
                          ("int32 vector of NB \\* 128 \\* bits = 256", {0: torch.zeros(512, dtype=torch.int32)}),
                          ("fp32 vector of NB = 1", {1: torch.ones(2)}),
                          ("finite and non-negative", {1: torch.tensor([-1.0])})):
        args = [change.get(i, x) for i, x in enumerate(good)] if change else None
        with pytest.raises(ValueError, match=match):
            server.worker_data_queue.add_task((0, 10, EDENUpdate(*args) if args else {"w": 1}))
    assert not server._payloads


def test_simulator_flags():
    from distributed_learning_simulator_amd import simulator
    head = ["--worker_number", "2", "--round", "1", "--distributed_algorithm"]
    cfg = simulator.get_config(head + ["fed_eden"])
    assert simulator.worker_kwargs(cfg) == {"bits": 4, "scale": "unbiased", "seed": 0}
    cfg = simulator.get_config(head + ["fed_eden", "--eden_bits", "2", "--eden_scale", "mse", "--eden_seed", "7"])
    assert simulator.worker_kwargs(cfg) == {"bits": 2, "scale": "mse", "seed": 7}
    assert simulator.server_kwargs(cfg) == {"aggregation_mode": "exact", "seed": 7, "bits": 2}
    for bad in (["fed", "--eden_bits", "4"], ["fed_drive", "--eden_scale", "mse"], ["fed_qsgd", "--eden_seed", "1"],
                ["fed_eden", "--drive_seed", "1"], ["fed_eden", "--qsgd_bits", "4"], ["fed_eden", "--eden_bits", "8"],
                ["fed_eden", "--eden_scale", "l2"], ["fed_eden", "--eden_seed", "-1"]):
        with pytest.raises(SystemExit):
            simulator.get_config(head + bad)
