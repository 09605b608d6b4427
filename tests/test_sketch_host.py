"""fed_sketch without a GPU: factory dispatch, the server's refusals, the simulator's flags and
the binding's host-side checks."""
import pytest
import torch

from tests import cpu_doubles
from tests.test_topk_host import CPU, FakeTrainer, initial_model, make_model


def make_server(monkeypatch, **kwargs):
    from distributed_learning_simulator_amd import factory
    cpu_doubles.install(monkeypatch)
    return factory.get_server("fed_sketch", sharded=False, initial_model=initial_model(),
                              tester=None, worker_number=3, synchronous=True, device=CPU, **kwargs)


def test_factory_and_sharding(monkeypatch):
    from distributed_learning_simulator_amd import factory
    from distributed_learning_simulator_amd.servers.fed_sketch_server import FedSketchServer
    from distributed_learning_simulator_amd.workers.fed_sketch_worker import FedSketchWorker
    server = make_server(monkeypatch, rows=3, seed=7)  # P = 128: cols clamps to 1024, k to 1
    assert type(server) is FedSketchServer and (server.cols, server.k) == (1024, 1)
    assert tuple(server.u.shape) == (3, 1024) and not server.u.any() and not server.v.any()
    worker = factory.get_worker("fed_sketch", worker_id=0, trainer=FakeTrainer(make_model(), 10),
                                worker_data_queue=None, round=1, rows=3, cols=2048, seed=7)
    assert type(worker) is FedSketchWorker and (worker.rows, worker.cols, worker.seed) == (3, 2048, 7)
    with pytest.raises(RuntimeError, match="one-process server only"):
        factory.get_server("fed_sketch", sharded=True, tester=None, worker_number=2)
    with pytest.raises(ValueError, match="needs a model to start from"):
        factory.get_server("fed_sketch", sharded=False, tester=None, worker_number=2)
    with pytest.raises(ValueError, match="must be a SketchUpdate"):
        server.worker_data_queue.add_task((0, 10, {"w": 1}))


@pytest.mark.parametrize("kwargs", [{"aggregation_rule": "median"}, {"server_optimizer": "adam"},
                                    {"attack": "sign_flip", "attackers": (1,)}, {"dp_clip": 1.0},
                                    {"aggregation_mode": "fma"}, {"seed": -1}, {"rows": 4},
                                    {"cols": 3000}, {"k": 0}, {"k": 129}, {"ratio": 0.0},
                                    {"momentum": 1.0}])
def test_server_refuses(monkeypatch, kwargs):
    with pytest.raises(ValueError, match="Count Sketch tables|one arithmetic|FedSketchServer: "):
        make_server(monkeypatch, **kwargs)


def test_simulator_flags():
    from distributed_learning_simulator_amd import simulator
    head = ["--worker_number", "2", "--round", "1", "--distributed_algorithm"]
    cfg = simulator.get_config(head + ["fed_sketch"])
    assert simulator.worker_kwargs(cfg) == {"rows": 5, "cols": None, "seed": 0}
    cfg = simulator.get_config(head + ["fed_sketch", "--sketch_rows", "3", "--sketch_cols", "4096",
                                       "--sketch_ratio", "0.5", "--sketch_momentum", "0", "--sketch_seed", "7"])
    assert simulator.worker_kwargs(cfg) == {"rows": 3, "cols": 4096, "seed": 7}
    assert simulator.server_kwargs(cfg) == {"aggregation_mode": "exact", "rows": 3, "cols": 4096,
                                            "seed": 7, "ratio": 0.5, "momentum": 0.0}
    for bad in (["fed", "--sketch_rows", "3"], ["fed_drive", "--sketch_seed", "1"],
                ["fed_sketch", "--drive_seed", "1"], ["fed_sketch", "--sketch_rows", "2"],
                ["fed_sketch", "--sketch_cols", "1000"], ["fed_sketch", "--sketch_ratio", "0"],
                ["fed_sketch", "--sketch_momentum", "1"], ["fed_sketch", "--sketch_seed", "-1"]):
        with pytest.raises(SystemExit):
            simulator.get_config(head + bad)


def test_binding_checks_on_the_host():
    """Each refused before the library is asked for anything."""
    from distributed_learning_simulator_amd import _native
    assert [_native.sketch_default_cols(P) for P in (128, 1 << 16, 11_173_964, 1 << 30)] == \
        [1024, 2048, 1 << 18, 1 << 24]
    w, table, stats = torch.zeros(64), torch.zeros(3, 1024), torch.zeros(1, dtype=torch.int32)
    good = dict(w=w, base=None, P=64, R=3, C=1024, seed=0, stream_id=0, table=table, stats=stats,
                workspace=None)
    for match, change in (("R=2", {"R": 2}), ("C=512", {"C": 512}), ("C=1536", {"C": 1536}),
                          ("P=66", {"P": 66}), ("P=0", {"P": 0}), ("w must be", {"P": 68}),
                          ("base must be", {"base": torch.zeros(64, dtype=torch.float64)}),
                          ("table must be", {"table": torch.zeros(1024, 3).t()}),
                          ("stats must be", {"stats": torch.zeros(1)}), ("seed", {"seed": -1})):
        with pytest.raises(RuntimeError, match=match):
            _native.sketch(**{**good, **change})
    for match, change in (("R=4", {"R": 4}), ("table must be", {"table": torch.zeros(3, 2048)}),
                          ("est must be", {"est": torch.zeros(60)}), ("stream_id", {"stream_id": 1 << 64})):
        with pytest.raises(RuntimeError, match=match):
            _native.unsketch(**{**dict(table=table, P=64, R=3, C=1024, seed=0, stream_id=0, est=w),
                                **change})
