"""fed_drive without a GPU: factory dispatch, the server's refusals and payload validation,
the simulator's flags."""
import pytest
import torch

from tests import cpu_doubles
from tests.test_topk_host import CPU, FakeTrainer, initial_model, make_model


def make_server(monkeypatch, **kwargs):
    from distributed_learning_simulator_amd import factory
    cpu_doubles.install(monkeypatch)
    return factory.get_server("fed_drive", sharded=False, initial_model=initial_model(),
                              tester=None, worker_number=3, synchronous=True, device=CPU, **kwargs)


def test_factory_and_sharding(monkeypatch):
    from distributed_learning_simulator_amd import factory
    from distributed_learning_simulator_amd.servers.fed_drive_server import FedDriveServer
    from distributed_learning_simulator_amd.workers.fed_drive_worker import FedDriveWorker
    assert type(make_server(monkeypatch, seed=7)) is FedDriveServer
    worker = factory.get_worker("fed_drive", worker_id=0, trainer=FakeTrainer(make_model(), 10),
                                worker_data_queue=None, round=1, seed=7, scale="mse")
    assert type(worker) is FedDriveWorker and (worker.seed, worker.scale) == (7, "mse")
    with pytest.raises(RuntimeError, match="one-process server only"):
        factory.get_server("fed_drive", sharded=True, tester=None, worker_number=2)
    with pytest.raises(ValueError, match="needs a model to start from"):
        factory.get_server("fed_drive", sharded=False, tester=None, worker_number=2)


@pytest.mark.parametrize("kwargs", [{"aggregation_rule": "median"}, {"server_optimizer": "adam"},
                                    {"attack": "sign_flip", "attackers": (1,)}, {"dp_clip": 1.0},
                                    {"aggregation_mode": "fma"}, {"seed": -1}])
def test_server_refuses(monkeypatch, kwargs):
    with pytest.raises(ValueError, match="sign bits and scales|one arithmetic|seed="):
        make_server(monkeypatch, **kwargs)


def test_server_rejects_payloads(monkeypatch):
    from distributed_learning_simulator_amd.workers.fed_drive_worker import DriveUpdate
    server = make_server(monkeypatch)  # P = 128: one block, 64 words
    good = (torch.zeros(64, dtype=torch.int64), torch.ones(1), 128, 1)
    assert DriveUpdate(*good).nbytes == 4096 // 8 + 4
    for match, change in (("must be a DriveUpdate", None), ("P=64", {2: 64}),
                          ("rotation of round 2", {3: 2}),
                          ("int64 vector of Pd / 64 = 64", {0: torch.zeros(2, dtype=torch.int64)}),
                          ("int64 vector", {0: torch.zeros(64, dtype=torch.int32)}),
                          ("fp32 vector of NB = 1", {1: torch.ones(2)}),
                          ("finite and non-negative", {1: torch.tensor([float("nan")])}),
                          ("finite and non-negative", {1: torch.tensor([-1.0])})):
        args = [change.get(i, a) for i, a in enumerate(good)] if change else None
        with pytest.raises(ValueError, match=match):
            server.worker_data_queue.add_task((0, 10, DriveUpdate(*args) if args else {"w": 1}))
    assert not server._payloads


def test_simulator_flags():
    from distributed_learning_simulator_amd import simulator
    head = ["--worker_number", "2", "--round", "1", "--distributed_algorithm"]
    cfg = simulator.get_config(head + ["fed_drive"])
    assert simulator.worker_kwargs(cfg) == {"seed": 0, "scale": "unbiased"}
    cfg = simulator.get_config(head + ["fed_drive", "--drive_seed", "7", "--drive_scale", "mse"])
    assert simulator.worker_kwargs(cfg) == {"seed": 7, "scale": "mse"}
    assert simulator.server_kwargs(cfg) == {"aggregation_mode": "exact", "seed": 7}
    for bad in (["fed", "--drive_seed", "1"], ["fed_efsign", "--drive_scale", "mse"],
                ["fed_drive", "--efsign_error_feedback", "1"], ["fed_drive", "--drive_scale", "l2"],
                ["fed_drive", "--drive_seed", "-1"]):
        with pytest.raises(SystemExit):
            simulator.get_config(head + bad)
