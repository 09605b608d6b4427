"""fed_qsgd without a GPU: the library's argument checks and their order, the binding's
messages, factory dispatch, the server's refusals and payload validation, the simulator's
flags."""
import ctypes

import pytest
import torch

from tests import cpu_doubles, qsgd_ref as ref
from tests.test_topk_host import CPU, FakeTrainer, initial_model, make_model


def test_library_checks_and_their_order():
    """Fake 16-byte aligned addresses: every call is refused before anything is launched or
    written.  DLS_EINVAL (-1) for the values, then DLS_ELAYOUT (-2), then the overlaps (-1)."""
    from distributed_learning_simulator_amd import _native
    L, u64 = _native.lib(), ctypes.c_uint64
    a, b, c, d, e = (ctypes.c_void_p(k << 24) for k in (1, 2, 3, 4, 5))
    off = ctypes.c_void_p((1 << 24) + 4)

    def compress(w=a, base=b, P=1024, bits=4, norm=1, codes=c, scales=d, stats=e):
        return L.dls_qsgd_compress_f32(w, base, P, bits, norm, u64(0), u64(1), codes, scales, stats, None)

    def fedavg(base=a, codes=b, ldc=128, scales=c, lds=2, K=1, P=1024, bits=4, out=d):
        return L.dls_qsgd_fedavg_f32(base, codes, ldc, scales, lds, e, 4.0, K, P, bits, out, None)

    got = [compress(stats=None), compress(bits=3), compress(bits=16), compress(norm=2),
           compress(P=0), compress(P=1 << 31), compress(P=96, bits=1), compress(w=off, norm=-1),
           compress(P=96), compress(w=off), compress(codes=off), compress(scales=off),
           compress(P=96, codes=a), compress(codes=a), compress(scales=b), compress(stats=b)]
    assert got == [-1] * 8 + [-2] * 5 + [-1] * 3
    assert b"alias w or base" in L.dls_last_error()
    got = [fedavg(out=None), fedavg(bits=6), fedavg(K=0), fedavg(P=32), fedavg(P=96, K=0),
           fedavg(P=96), fedavg(ldc=124), fedavg(ldc=130), fedavg(lds=1), fedavg(codes=off),
           fedavg(ldc=124, out=a), fedavg(out=a)]
    assert got == [-1] * 5 + [-2] * 6 + [-1]
    assert fedavg(bits=8) == -2  # ldc below 16 bits NB = 256 words


def test_binding_messages():
    from distributed_learning_simulator_amd import _native
    assert [_native.qsgd_code_words(P, b) for P, b in ((64, 2), (512, 4), (576, 8), (1472, 2))] == [32, 64, 256, 96]
    assert _native.qsgd_buckets(1472) == 3 == ref.buckets(1472)
    w, codes, scales = torch.zeros(1024), torch.zeros(128, dtype=torch.int32), torch.zeros(2)
    good = dict(w=w, base=torch.zeros(1024), P=1024, bits=4, norm="l2", seed=0, stream_id=1,
                codes=codes, scales=scales, stats=torch.zeros(4, dtype=torch.int32))
    for match, change in (("not on the GPU", {}), ("bits=3", {"bits": 3}), ("norm='l1'", {"norm": "l1"}),
                          ("multiple of 64", {"P": 1000}), ("codes must be an int32", {"codes": codes[:64]}),
                          ("scales must be an fp32", {"scales": scales[:1]}), ("seed=-1", {"seed": -1}),
                          ("w and codes overlap", {"codes": w.view(torch.int32)}),
                          ("16-byte aligned", {"w": torch.zeros(1028)[1:]})):
        with pytest.raises(RuntimeError, match=match):
            _native.qsgd_compress(**{**good, **change})
    good = dict(base=w, codes=codes[None], scales=scales[None], weight=torch.ones(1), total=1.0,
                P=1024, bits=4, out=torch.zeros(1024))
    for match, change in (("not on the GPU", {}), (r"codes must be an int32 \[K=1, >= 256\]", {"bits": 8}),
                          ("multiple of 4", {"codes": torch.zeros(1, 130, dtype=torch.int32)}),
                          ("total=0.0", {"total": 0.0}), ("out and base overlap", {"out": w})):
        with pytest.raises(RuntimeError, match=match):
            _native.qsgd_fedavg(**{**good, **change})


def make_server(monkeypatch, **kwargs):
    from distributed_learning_simulator_amd import factory
    cpu_doubles.install(monkeypatch)
    return factory.get_server("fed_qsgd", sharded=False, initial_model=initial_model(), tester=None,
                              worker_number=3, synchronous=True, device=CPU, **kwargs)


def test_factory_sharding_and_refusals(monkeypatch):
    from distributed_learning_simulator_amd import factory
    from distributed_learning_simulator_amd.servers.fed_qsgd_server import FedQSGDServer
    from distributed_learning_simulator_amd.workers.fed_qsgd_worker import FedQSGDWorker
    server = make_server(monkeypatch, bits=2)
    assert type(server) is FedQSGDServer and server.bits == 2
    kwargs = dict(worker_id=0, trainer=FakeTrainer(make_model(), 10), worker_data_queue=None, round=1)
    worker = factory.get_worker("fed_qsgd", bits=8, norm="max", seed=7, **kwargs)
    assert type(worker) is FedQSGDWorker and (worker.bits, worker.norm, worker.seed) == (8, "max", 7)
    for bad in ({"bits": 3}, {"norm": "l1"}, {"seed": -1}, {"worker_id": 1 << 32}):
        with pytest.raises(ValueError, match="FedQSGDWorker: "):
            factory.get_worker("fed_qsgd", **{**kwargs, **bad})
    with pytest.raises(RuntimeError, match="one-process server only"):
        factory.get_server("fed_qsgd", sharded=True, tester=None, worker_number=2)
    with pytest.raises(ValueError, match="needs a model to start from"):
        factory.get_server("fed_qsgd", sharded=False, tester=None, worker_number=2)
    for extra in ({"aggregation_rule": "median"}, {"server_optimizer": "adam"}, {"dp_clip": 1.0},
                  {"attack": "sign_flip", "attackers": (1,)}, {"aggregation_mode": "fma"}, {"bits": 3}):
        with pytest.raises(ValueError, match="quantized levels and scales|one arithmetic|bits=3"):
            make_server(monkeypatch, **extra)


def test_server_rejects_payloads(monkeypatch):
    """P = 128: one bucket, 64 words at 4 bits.  A bad payload leaves nothing behind."""
    from distributed_learning_simulator_amd.workers.fed_qsgd_worker import QSGDUpdate
    server = make_server(monkeypatch)
    good = (torch.zeros(64, dtype=torch.int32), torch.ones(1), 128, 4)
    assert QSGDUpdate(*good).nbytes == 64 * 4 + 4
    for match, change in (("must be a QSGDUpdate", None), ("P=64", {2: 64}), ("bits=8", {3: 8}),
                          ("int32 vector of NB \\* 16 \\* bits = 64", {0: torch.zeros(32, dtype=torch.int32)}),
                          ("int32 vector", {0: torch.zeros(64, dtype=torch.int64)}),
                          ("fp32 vector of NB = 1", {1: torch.ones(2)}),
                          ("finite and non-negative", {1: torch.tensor([float("inf")])}),
                          ("finite and non-negative", {1: torch.tensor([-1.0])})):
        args = [change.get(i, a) for i, a in enumerate(good)] if change else None
        with pytest.raises(ValueError, match=match):
            server.worker_data_queue.add_task((0, 10, QSGDUpdate(*args) if args else {"w": 1}))
    assert not server._payloads


def test_simulator_flags():
    from distributed_learning_simulator_amd import simulator
    head = ["--worker_number", "2", "--round", "1", "--distributed_algorithm"]
    cfg = simulator.get_config(head + ["fed_qsgd"])
    assert simulator.worker_kwargs(cfg) == {"bits": 4, "norm": "l2", "seed": 0}
    cfg = simulator.get_config(head + ["fed_qsgd", "--qsgd_bits", "2", "--qsgd_norm", "max", "--qsgd_seed", "7"])
    assert simulator.worker_kwargs(cfg) == {"bits": 2, "norm": "max", "seed": 7}
    assert simulator.server_kwargs(cfg) == {"aggregation_mode": "exact", "bits": 2}
    for bad in (["fed", "--qsgd_bits", "4"], ["fed_drive", "--qsgd_norm", "max"], ["fed_qsgd", "--drive_seed", "1"],
                ["fed_qsgd", "--qsgd_bits", "3"], ["fed_qsgd", "--qsgd_norm", "l1"], ["fed_qsgd", "--qsgd_seed", "-1"]):
        with pytest.raises(SystemExit):
            simulator.get_config(head + bad)
