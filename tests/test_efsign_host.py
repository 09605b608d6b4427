"""fed_efsign without a GPU: factory dispatch, the server's refusals and payload validation,
the simulator's flag, and the reference against a hand-written case."""
import numpy as np
import pytest
import torch

from tests import cpu_doubles
from tests import efsign_ref as ref
from tests.test_topk_host import CPU, FakeTrainer, initial_model, make_model

F32 = np.float32


def test_reference_hand_written():
    bounds, count = ref.segments([3, 64])
    assert bounds == [0, 64, 128]
    w = np.zeros(128, F32)
    w[:3] = [1.0, -2.0, -0.0]
    w[64:128] = 0.5
    w[100] = -1.5
    words, s, e, bad = ref.compress(w, np.zeros(128, F32), np.zeros(128, F32), bounds, count)
    assert words.tolist() == [2, 1 << 36] and s.tolist() == [1.0, F32(33.0 / 64)] and bad == 0
    assert e[:4].tolist() == [0.0, -1.0, -1.0, 0.0] and e[100] == F32(-1.5) + s[1]
    out = ref.fedavg(np.full(128, -0.0, F32), [(words, s), (words, s)], bounds, count, [1, 3])
    assert out[:3].tolist() == [1.0, -1.0, 1.0] and np.signbit(out[3:64]).all()


def make_server(monkeypatch, **kwargs):
    from distributed_learning_simulator_amd import factory
    cpu_doubles.install(monkeypatch)
    return factory.get_server("fed_efsign", sharded=False, initial_model=initial_model(),
                              tester=None, worker_number=3, synchronous=True, device=CPU, **kwargs)


def test_factory_and_sharding(monkeypatch):
    from distributed_learning_simulator_amd import factory
    from distributed_learning_simulator_amd.servers.fed_efsign_server import FedEFSignServer
    from distributed_learning_simulator_amd.workers.fed_efsign_worker import FedEFSignWorker
    assert type(make_server(monkeypatch)) is FedEFSignServer
    worker = factory.get_worker("fed_efsign", worker_id=0, trainer=FakeTrainer(make_model(), 10),
                                worker_data_queue=None, round=1, error_feedback=False)
    assert type(worker) is FedEFSignWorker and worker.error_feedback is False
    with pytest.raises(RuntimeError, match="one-process server only"):
        factory.get_server("fed_efsign", sharded=True, tester=None, worker_number=2)
    with pytest.raises(ValueError, match="needs a model to start from"):
        factory.get_server("fed_efsign", sharded=False, tester=None, worker_number=2)


@pytest.mark.parametrize("kwargs", [{"aggregation_rule": "median"}, {"server_optimizer": "adam"},
                                    {"attack": "sign_flip", "attackers": (1,)}, {"dp_clip": 1.0},
                                    {"aggregation_mode": "fma"}])
def test_server_refuses(monkeypatch, kwargs):
    with pytest.raises(ValueError, match="sign bits and scales|one arithmetic"):
        make_server(monkeypatch, **kwargs)


def test_server_rejects_payloads(monkeypatch):
    from distributed_learning_simulator_amd.workers.fed_efsign_worker import SignUpdate
    server = make_server(monkeypatch)
    good = (torch.zeros(2, dtype=torch.int64), torch.ones(2), 128)
    assert SignUpdate(*good).nbytes == 128 // 8 + 4 * 2
    for match, change in (("must be a SignUpdate", None), ("P=64", {2: 64}),
                          ("int64 vector of P / 64 = 2", {0: torch.zeros(3, dtype=torch.int64)}),
                          ("int64 vector", {0: torch.zeros(2, dtype=torch.int32)}),
                          ("fp32 vector of T = 2", {1: torch.ones(3)}),
                          ("finite and non-negative", {1: torch.tensor([1.0, float("nan")])}),
                          ("finite and non-negative", {1: torch.tensor([-1.0, 1.0])})):
        args = [change.get(i, a) for i, a in enumerate(good)] if change else None
        with pytest.raises(ValueError, match=match):
            server.worker_data_queue.add_task((0, 10, SignUpdate(*args) if args else {"w": 1}))
    assert not server._payloads


def test_simulator_flag():
    from distributed_learning_simulator_amd import simulator
    head = ["--worker_number", "2", "--round", "1", "--distributed_algorithm"]
    cfg = simulator.get_config(head + ["fed_efsign"])
    assert simulator.worker_kwargs(cfg) == {"error_feedback": True}
    cfg = simulator.get_config(head + ["fed_efsign", "--efsign_error_feedback", "0"])
    assert simulator.worker_kwargs(cfg) == {"error_feedback": False}
    assert simulator.server_kwargs(cfg) == {"aggregation_mode": "exact"}
    assert "fed_efsign" in simulator.__doc__
    for bad in (["fed", "--efsign_error_feedback", "1"], ["fed_efsign", "--topk_ratio", "0.1"],
                ["fed_efsign", "--efsign_error_feedback", "2"]):
        with pytest.raises(SystemExit):
            simulator.get_config(head + bad)
