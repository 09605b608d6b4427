"""fed_mx without a GPU: tests/mx_ref.py against torch's float8 casts and the E2M1 table, the
library's argument checks and their order, the binding's messages, factory dispatch, the
server's refusals and payload validation, the simulator's flags."""
import ctypes

import numpy as np
import pytest
import torch

from tests import cpu_doubles, mx_ref as ref
from tests.test_topk_host import CPU, FakeTrainer, initial_model, make_model

F32 = np.float32


@pytest.mark.parametrize("fmt,dtype", [("e4m3", torch.float8_e4m3fn), ("e5m2", torch.float8_e5m2)])
def test_reference_against_torch_casts(fmt, dtype):
    """Nearest codes are the bits of torch's CPU cast of the exactly scaled values t = u 2^-e:
    a few decades with a fixed block maximum in 1..fmax (so t is an fp32 value), the ties
    between neighbouring codes, both zeros."""
    rng, fmax = np.random.default_rng(3), ref.FORMATS[fmt][4]
    grid = ref.value(np.arange(0, 0x7F if fmt == "e4m3" else 0x7C), fmt)
    ties = ((grid[:-1] + grid[1:]) / 2).astype(F32)
    u = np.concatenate([ties, -ties, [0.0, -0.0], rng.standard_normal(3 * 512 - 2 * ties.size - 2)
                        * 10.0 ** rng.uniform(-4, 2, 3 * 512 - 2 * ties.size - 2)]).astype(F32)
    u[::32] = fmax * rng.choice([1.0, 0.5, 2.0 ** -7, 1.0 / fmax], u.size // 32)
    codes, sb, _, bad = ref.compress(u, np.zeros_like(u), None, u.size, fmt, 0, None)
    t = np.ldexp(u, -(np.repeat(sb.astype(np.int64), 32) - 127)).astype(F32)
    want = torch.from_numpy(t).to(dtype).view(torch.uint8).numpy()
    assert bad == 0 and np.array_equal(ref.unpack(codes, fmt), want)


def test_reference_e2m1_table():
    """Every grid point, every tie (to the even code) and points either side of them."""
    table = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
    assert np.array_equal(ref.value(np.arange(8), "e2m1"), table)
    mid = (table[:-1] + table[1:]) / 2
    t = np.concatenate([table, mid, mid * (1 - 2.0 ** -20), mid * (1 + 2.0 ** -20), [0.2, 5.9]])
    want = np.concatenate([np.arange(8), [0, 2, 2, 4, 4, 6, 6], np.arange(7), np.arange(1, 8), [0, 7]])
    u = np.zeros(64, F32)
    u[:t.size], u[32:32 + t.size], u[31], u[63] = t, -t, 6.0, 6.0
    codes, sb, _, _ = ref.compress(u, np.zeros(64, F32), None, 64, "e2m1", 0, None)
    got = ref.unpack(codes, "e2m1")
    assert np.array_equal(got[:t.size], want) and np.array_equal(got[32:32 + t.size], want | 8)
    assert sb[:2].tolist() == [127, 127] and not sb[2:].any()


def test_library_checks_and_their_order():
    """Fake 16-byte aligned addresses: every call is refused before anything is launched or
    written.  DLS_EINVAL (-1) for the values, then DLS_ELAYOUT (-2), then the overlaps (-1)."""
    from distributed_learning_simulator_amd import _native
    L, u64 = _native.lib(), ctypes.c_uint64
    a, b, c, d, e, r = (ctypes.c_void_p(k << 24) for k in (1, 2, 3, 4, 5, 6))
    off = ctypes.c_void_p((1 << 24) + 4)

    def compress(w=a, base=b, res=None, P=1024, fmt=0, rnd=0, codes=c, scales=d, stats=e):
        return L.dls_mx_compress_f32(w, base, res, P, fmt, rnd, u64(0), u64(1), codes, scales, stats, None)

    def fedavg(base=a, codes=b, ldc=256, scales=c, lds=32, K=1, P=1024, fmt=0, out=d):
        return L.dls_mx_fedavg_f32(base, codes, ldc, scales, lds, e, 4.0, K, P, fmt, out, None)

    got = [compress(stats=None), compress(fmt=3), compress(rnd=2), compress(P=0), compress(P=1 << 31),
           compress(w=off, fmt=-1), compress(P=96), compress(w=off), compress(res=off),
           compress(scales=off), compress(codes=a), compress(scales=b), compress(res=r, stats=r),
           compress(res=a)]
    assert got == [-1] * 6 + [-2] * 4 + [-1] * 4
    assert b"residual must not alias" in L.dls_last_error()
    got = [fedavg(out=None), fedavg(fmt=3), fedavg(K=0), fedavg(P=32), fedavg(P=96), fedavg(ldc=252),
           fedavg(ldc=258), fedavg(lds=16), fedavg(lds=40), fedavg(codes=off), fedavg(out=a)]
    assert got == [-1] * 4 + [-2] * 6 + [-1]
    assert fedavg(fmt=2, ldc=124) == -2 and fedavg(fmt=1, ldc=128) == -2  # 128 and 256 words


def test_binding_messages():
    from distributed_learning_simulator_amd import _native
    assert [_native.mx_code_words(P, f) for P, f in ((64, "e2m1"), (512, "e4m3"), (576, "e5m2"))] == [64, 128, 256]
    assert _native.mx_scale_bytes(1472) == 48 == 16 * ref.groups(1472) and _native.MX_BLOCK == ref.BLOCK
    assert list(_native.MX_FORMATS) == list(ref.FORMATS) and list(_native.MX_ROUNDINGS) == ["nearest", "stochastic"]
    w, codes, scales = torch.zeros(1024), torch.zeros(256, dtype=torch.int32), torch.zeros(32, dtype=torch.uint8)
    good = dict(w=w, base=torch.zeros(1024), residual=None, P=1024, format="e4m3", rounding="nearest",
                seed=0, stream_id=1, codes=codes, scales=scales, stats=torch.zeros(4, dtype=torch.int32))
    for match, change in (("not on the GPU", {}), ("format='e3m2'", {"format": "e3m2"}),
                          ("rounding='up'", {"rounding": "up"}), ("multiple of 64", {"P": 1000}),
                          ("codes must be an int32", {"codes": codes[:128]}),
                          ("scales must be an uint8", {"scales": scales[:16]}), ("seed=-1", {"seed": -1}),
                          ("residual must be an fp32", {"residual": torch.zeros(512)}),
                          ("w and residual overlap", {"residual": w}),
                          ("16-byte aligned", {"w": torch.zeros(1028)[1:]})):
        with pytest.raises(RuntimeError, match=match):
            _native.mx_compress(**{**good, **change})
    good = dict(base=w, codes=codes[None], scales=scales[None], weight=torch.ones(1), total=1.0,
                P=1024, format="e4m3", out=torch.zeros(1024))
    for match, change in (("not on the GPU", {}), (r"codes must be an int32 \[K=1, >= 256\]", {"codes": codes[None, :128]}),
                          ("multiple of 16", {"scales": torch.zeros(1, 40, dtype=torch.uint8)}),
                          ("total=0.0", {"total": 0.0}), ("out and base overlap", {"out": w})):
        with pytest.raises(RuntimeError, match=match):
            _native.mx_fedavg(**{**good, **change})


def make_server(monkeypatch, **kwargs):
    from distributed_learning_simulator_amd import factory
    cpu_doubles.install(monkeypatch)
    return factory.get_server("fed_mx", sharded=False, initial_model=initial_model(), tester=None,
                              worker_number=3, synchronous=True, device=CPU, **kwargs)


def test_factory_sharding_and_refusals(monkeypatch):
    from distributed_learning_simulator_amd import factory
    from distributed_learning_simulator_amd.servers.fed_mx_server import FedMXServer
    from distributed_learning_simulator_amd.workers.fed_mx_worker import FedMXWorker
    server = make_server(monkeypatch, format="e2m1")
    assert type(server) is FedMXServer and server.format == "e2m1"
    kwargs = dict(worker_id=0, trainer=FakeTrainer(make_model(), 10), worker_data_queue=None, round=1)
    worker = factory.get_worker("fed_mx", format="e5m2", rounding="stochastic", seed=7, **kwargs)
    assert type(worker) is FedMXWorker and not worker.error_feedback
    assert (worker.format, worker.rounding, worker.seed) == ("e5m2", "stochastic", 7)
    assert factory.get_worker("fed_mx", **kwargs).error_feedback
    assert factory.get_worker("fed_mx", rounding="stochastic", error_feedback=1, **kwargs).error_feedback
    for bad in ({"format": "e3m2"}, {"rounding": "up"}, {"seed": -1}, {"worker_id": 1 << 32}):
        with pytest.raises(ValueError, match="FedMXWorker: "):
            factory.get_worker("fed_mx", **{**kwargs, **bad})
    with pytest.raises(RuntimeError, match="one-process server only"):
        factory.get_server("fed_mx", sharded=True, tester=None, worker_number=2)
    with pytest.raises(ValueError, match="needs a model to start from"):
        factory.get_server("fed_mx", sharded=False, tester=None, worker_number=2)
    for extra in ({"aggregation_rule": "median"}, {"server_optimizer": "adam"}, {"dp_clip": 1.0},
                  {"attack": "sign_flip", "attackers": (1,)}, {"aggregation_mode": "fma"}, {"format": "e3m2"}):
        with pytest.raises(ValueError, match="microscaling codes and scales|one arithmetic|format='e3m2'"):
            make_server(monkeypatch, **extra)


def test_server_rejects_payloads(monkeypatch):
    """P = 128: one group, 128 words at 8 bits and 16 scale bytes.  A bad payload leaves nothing
    behind."""
    from distributed_learning_simulator_amd.workers.fed_mx_worker import MXUpdate
    server = make_server(monkeypatch)
    good = (torch.zeros(128, dtype=torch.int32), torch.zeros(16, dtype=torch.uint8), 128, "e4m3")
    assert MXUpdate(*good).nbytes == 512 + 16
    bad_scale = torch.zeros(16, dtype=torch.uint8)
    bad_scale[3] = 255
    for match, change in (("must be an MXUpdate", None), ("P=64", {2: 64}), ("format='e2m1'", {3: "e2m1"}),
                          ("int32 vector of 128", {0: torch.zeros(64, dtype=torch.int32)}),
                          ("int32 vector", {0: torch.zeros(128, dtype=torch.int64)}),
                          ("uint8 vector of 16", {1: torch.zeros(4, dtype=torch.uint8)}),
                          ("uint8 vector", {1: torch.zeros(16)}), ("scale byte is 255", {1: bad_scale})):
        args = [change.get(i, a) for i, a in enumerate(good)] if change else None
        with pytest.raises(ValueError, match=match):
            server.worker_data_queue.add_task((0, 10, MXUpdate(*args) if args else {"w": 1}))
    assert not server._payloads


def test_simulator_flags():
    from distributed_learning_simulator_amd import simulator
    head = ["--worker_number", "2", "--round", "1", "--distributed_algorithm"]
    cfg = simulator.get_config(head + ["fed_mx"])
    assert simulator.worker_kwargs(cfg) == {"format": "e4m3", "rounding": "nearest", "seed": 0, "error_feedback": None}
    cfg = simulator.get_config(head + ["fed_mx", "--mx_format", "e2m1", "--mx_rounding", "stochastic",
                                       "--mx_error_feedback", "1", "--mx_seed", "7"])
    assert simulator.worker_kwargs(cfg) == {"format": "e2m1", "rounding": "stochastic", "seed": 7, "error_feedback": True}
    assert simulator.server_kwargs(cfg) == {"aggregation_mode": "exact", "format": "e2m1"}
    for bad in (["fed", "--mx_format", "e4m3"], ["fed_qsgd", "--mx_seed", "1"], ["fed_mx", "--qsgd_bits", "4"],
                ["fed_mx", "--mx_format", "e3m2"], ["fed_mx", "--mx_rounding", "up"], ["fed_mx", "--mx_seed", "-1"]):
        with pytest.raises(SystemExit):
            simulator.get_config(head + bad)
