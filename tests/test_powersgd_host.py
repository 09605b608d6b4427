"""fed_powersgd without a GPU: the compressed / dense rule and the payload offsets, the
library's argument checks and their order, factory dispatch, the simulator's flags, the sharded
refusal, and the worker's warm-start and no-state modes on a fake ``_native``."""
import ctypes

import pytest
import torch

from tests import cpu_doubles, powersgd_ref as ref
from tests.test_topk_host import CPU, FakeTrainer, initial_model, make_model


@pytest.mark.parametrize("model,r,compressed,floats", [
    ("LeNet5", 4, [(6, 25), (16, 150), (120, 400), (84, 120), (10, 84)], 4296), ("LeNet5", 16, [(120, 400), (84, 120)], 15210),
    ("ResNet18", 4, None, 154910), ("ResNet18", 16, None, 587578)])
def test_rule_and_offsets(model, r, compressed, floats):
    """The plan of a model's layout against the reference's restatement; the uplink at
    ResNet-18, rank 4, is 154910 floats of 11173962 (1/72)."""
    from distributed_learning_simulator_amd import _native
    from distributed_learning_simulator_amd.layout import ParameterLayout
    from distributed_learning_simulator_amd.models import MODELS
    from distributed_learning_simulator_amd.workers.fed_powersgd_worker import sent_floats
    lay = ParameterLayout.from_dict(dict(MODELS[model]().named_parameters()))
    plan = _native.powersgd_layout_plan(lay, r, CPU)
    bounds, dims, kinds, blocks, L = ref.plan(lay.shapes, r)
    assert bounds == list(lay.offsets) + [lay.P] and (plan.T, plan.P, plan.L) == (len(lay), lay.P, L)
    assert [plan.kind(t) for t in range(plan.T)] == kinds
    assert [plan.blocks(t) for t in range(plan.T)] == blocks and sent_floats(plan) == floats
    assert all(p % 64 == 0 and q % 64 == 0 for p, q in blocks)
    assert all(kind == (len(s) >= 2 and r <= min(n, m) and (n + m) * r < n * m)
               for s, (n, m), kind in zip(lay.shapes, dims, kinds))
    if compressed is not None:
        assert [d for d, k in zip(dims, kinds) if k] == compressed
    assert tuple(plan.table.shape) == (plan.T + 1, _native.POWERSGD_PLAN_WORDS)
    for bad in (dict(r=0), dict(r=17), dict(bounds=bounds[:-1]), dict(bounds=[b + 32 for b in bounds]),
                dict(dims=[(n + 64, m) for n, m in dims])):
        with pytest.raises(RuntimeError, match="DLS_EINVAL"):
            _native.powersgd_plan(**{**dict(bounds=bounds, dims=dims, r=r, device=CPU), **bad})


def test_library_checks_and_their_order():
    """Fake 16-byte aligned addresses: every call is refused before anything is launched.
    DLS_EINVAL (-1) comes before DLS_ELAYOUT (-2) when both apply."""
    from distributed_learning_simulator_amd import _native
    L_, a, off = _native.lib(), ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 4)
    b, c, d = (ctypes.c_void_p(k << 24) for k in (2, 3, 4))

    def compress(w=a, base=b, e=c, P=128, T=2, r=4, q0=d, payload=ctypes.c_void_p(5 << 24), L=128,
                 wsb=1 << 20):
        return L_.dls_powersgd_compress_f32(w, base, e, P, a, T, r, q0, payload, L, a, a, wsb, None)

    def fedavg(base=a, pay=b, ldp=128, L=128, T=2, r=4, total=4.0, K=1, P=128, out=c):
        return L_.dls_powersgd_fedavg_f32(base, pay, ldp, L, a, T, r, a, total, K, P, out, None)

    got = [compress(w=None), compress(P=0), compress(P=1 << 31), compress(T=0), compress(T=3),
           compress(r=0), compress(r=17), compress(L=0), compress(wsb=16), compress(e=a),
           compress(payload=d), compress(P=96, r=0), compress(P=160), compress(L=96),
           compress(w=off), compress(e=ctypes.c_void_p((3 << 24) + 4))]
    assert got == [-1] * 12 + [-2] * 4
    got = [fedavg(base=None), fedavg(K=0), fedavg(P=32), fedavg(r=17), fedavg(L=1 << 31),
           fedavg(total=0.0), fedavg(total=float("inf")), fedavg(out=a), fedavg(P=160, K=0),
           fedavg(P=160, T=1), fedavg(ldp=64), fedavg(ldp=130), fedavg(pay=off)]
    assert got == [-1] * 9 + [-2] * 4
    dims = (ctypes.c_int64 * 4)(6, 25, 10, 1)
    assert L_.dls_powersgd_payload_len(dims, 2, 4) == 64 + 128 + 64
    assert L_.dls_powersgd_payload_len(dims, 2, 17) == -1 and L_.dls_powersgd_payload_len(None, 2, 4) == -1
    assert L_.dls_powersgd_workspace(dims, 2, 4, 160) == -2 and L_.dls_powersgd_workspace(dims, 2, 4, 0) == -1
    assert L_.dls_powersgd_workspace(dims, 2, 4, 256) == 80 + 6 * 128 + 6 * 64


def test_factory_sharding_and_refusals(monkeypatch):
    from distributed_learning_simulator_amd import factory
    from distributed_learning_simulator_amd.servers.fed_powersgd_server import FedPowerSGDServer
    from distributed_learning_simulator_amd.workers.fed_powersgd_worker import FedPowerSGDWorker
    cpu_doubles.install(monkeypatch)
    kwargs = dict(sharded=False, initial_model=initial_model(), tester=None, worker_number=3,
                  synchronous=True, device=CPU)
    server = factory.get_server("fed_powersgd", rank=2, **kwargs)
    assert type(server) is FedPowerSGDServer and server.rank == 2
    worker = factory.get_worker("fed_powersgd", worker_id=0, trainer=FakeTrainer(make_model(), 10),
                                worker_data_queue=None, round=1, rank=2, seed=7, warm_start=False)
    assert type(worker) is FedPowerSGDWorker and (worker.rank, worker.seed, worker.warm_start) == (2, 7, False)
    with pytest.raises(RuntimeError, match="one-process server only"):
        factory.get_server("fed_powersgd", sharded=True, tester=None, worker_number=2)
    with pytest.raises(ValueError, match="needs a model to start from"):
        factory.get_server("fed_powersgd", sharded=False, tester=None, worker_number=2)
    with pytest.raises(ValueError, match="must be a LowRankUpdate"):
        server.worker_data_queue.add_task((0, 10, {"w": 1}))
    for extra in ({"aggregation_rule": "median"}, {"server_optimizer": "adam"}, {"dp_clip": 1.0},
                  {"attack": "sign_flip", "attackers": (1,)}, {"aggregation_mode": "fma"},
                  {"rank": 0}, {"rank": 17}, {"rank": True}):
        with pytest.raises(ValueError, match="low-rank factors|one arithmetic|FedPowerSGDServer: "):
            factory.get_server("fed_powersgd", **{**kwargs, **extra})


def test_simulator_flags():
    from distributed_learning_simulator_amd import simulator
    head = ["--worker_number", "2", "--round", "1", "--distributed_algorithm"]
    cfg = simulator.get_config(head + ["fed_powersgd"])
    assert simulator.worker_kwargs(cfg) == {"rank": 4, "seed": 0, "warm_start": True,
                                            "error_feedback": True}
    assert simulator.server_kwargs(cfg) == {"aggregation_mode": "exact", "rank": 4}
    cfg = simulator.get_config(head + ["fed_powersgd", "--powersgd_rank", "16", "--powersgd_seed", "7",
                                       "--powersgd_warm_start", "0", "--powersgd_error_feedback", "0"])
    assert simulator.worker_kwargs(cfg) == {"rank": 16, "seed": 7, "warm_start": False,
                                            "error_feedback": False}
    for bad in (["fed", "--powersgd_rank", "4"], ["fed_sketch", "--powersgd_seed", "1"],
                ["fed_topk", "--powersgd_warm_start", "1"], ["fed_powersgd", "--sketch_rows", "3"],
                ["fed_powersgd", "--powersgd_rank", "0"], ["fed_powersgd", "--powersgd_rank", "17"],
                ["fed_powersgd", "--powersgd_seed", "-1"], ["fed_powersgd", "--powersgd_warm_start", "2"]):
        with pytest.raises(SystemExit):
            simulator.get_config(head + bad)


@pytest.mark.parametrize("warm_start,error_feedback", [(True, True), (False, True), (True, False)])
def test_worker_modes_on_a_fake_native(monkeypatch, warm_start, error_feedback):
    """Round 1 draws Q0 from Philox, one stream id per compressed tensor; afterwards the worker
    reads its own last payload (warm start) or draws again with the round in the counter;
    without error feedback no residual exists and e == None reaches the library."""
    from distributed_learning_simulator_amd import _native
    from distributed_learning_simulator_amd.workers.fed_powersgd_worker import FedPowerSGDWorker
    draws, calls = [], []

    def philox_normal(n, seed, stream_id, first=0, out=None, **_):
        draws.append((n, seed, stream_id, first))
        return out.fill_(1.0)

    def compress(w, base, e, plan, q0, payload, stats, workspace, stream=None):
        calls.append((e, q0))
        stats.zero_()
        return payload.fill_(float(len(calls)))

    monkeypatch.setattr(_native, "philox_normal", philox_normal)
    monkeypatch.setattr(_native, "powersgd_compress", compress)
    torch.manual_seed(0)
    model = torch.nn.Linear(40, 12)  # weight [12, 40] is compressed at rank 2, the bias dense
    worker = FedPowerSGDWorker(worker_id=0, trainer=FakeTrainer(model, 10), worker_data_queue=None,
                               round=2, rank=2, seed=5, warm_start=warm_start,
                               error_feedback=error_feedback)
    worker.load_model({k: v.detach().clone() for k, v in model.named_parameters()})
    ups = [worker.lowrank_update() for _ in range(3)]
    assert [worker.plan.kind(t) for t in range(2)] == [1, 0] and ups[0].floats == (12 + 40) * 2 + 12
    assert (worker.residual is None) == (not error_feedback)
    assert all((e is None) == (not error_feedback) for e, _ in calls)
    if warm_start:
        assert draws == [(128, 5, 0, 0)]
        assert calls[1][1] is ups[0].payload and calls[2][1] is ups[1].payload
    else:
        assert draws == [(128, 5, 0, 0), (128, 5, 0, 128), (128, 5, 0, 256)]
        assert all(q0 is not up.payload for (_, q0), up in zip(calls, ups))
