"""fed_hetero without a GPU: the slice views of both models against their torch forward, the
width-1 shapes, and what the wrappers, the server, the factory and the simulator refuse."""
import numpy as np
import pytest
import torch

from tests import hetero_ref as ref

CPU = torch.device("cpu")


def plan_of(model, widths):
    from distributed_learning_simulator_amd.hetero import HeteroPlan
    return HeteroPlan(model.hetero_views(), widths)


@pytest.mark.parametrize("width", [0.5, 0.25])
@pytest.mark.parametrize("name,shape", [("LeNet5", (1, 32, 32)), ("ResNet18", (3, 32, 32))])
def test_sub_model_is_the_global_model_with_the_rest_zeroed(name, shape, width):
    """Pins the [O, I, R] view of every tensor, fc1's flatten order included: the sub-model cut
    out by the reference slicing computes what the global model computes once every weight
    outside the slices is zero (eval mode; the two differ in the order of exact-zero terms)."""
    from distributed_learning_simulator_amd.models import MODELS
    torch.manual_seed(0)
    full = MODELS[name]().eval()
    with torch.no_grad():
        for p in full.parameters():  # biases and batch-norm vectors away from their 0 / 1 start
            p.copy_(torch.randn_like(p) * (0.3 if p.dim() == 1 else p.std()))
    plan = plan_of(full, (1.0, width))
    flat = plan.layout.flatten(dict(full.named_parameters()), device=CPU).numpy()
    row = ref.extract(flat, plan.tensors(), plan.slices[1], plan.level_P[1])
    sub = MODELS[name](width=width).eval()
    assert plan.level_layouts[1].matches(dict(sub.named_parameters()))
    with torch.no_grad():
        for n, v in plan.level_layouts[1].views(torch.from_numpy(row)).items():
            dict(sub.named_parameters())[n].copy_(v)
        zeroed, _ = ref.scatter(row, plan.tensors(), plan.slices[1], plan.P)
        for n, v in plan.layout.views(torch.from_numpy(zeroed)).items():
            dict(full.named_parameters())[n].copy_(v)
        x = torch.randn((2,) + shape)
        assert torch.allclose(sub(x), full(x), rtol=1e-4, atol=1e-5)


def test_width_one_is_todays_model():
    from distributed_learning_simulator_amd import model_shapes
    from distributed_learning_simulator_amd.models import LeNet5, ResNet18
    for cls, shapes in ((LeNet5, model_shapes.lenet5()), (ResNet18, model_shapes.resnet18_cifar())):
        assert [(n, tuple(p.shape)) for n, p in cls(width=1).named_parameters()] == shapes
        assert [(v.name, v.shape) for v in cls().hetero_views()] == shapes
    with pytest.raises(ValueError, match="width ratio"):
        LeNet5(width=0)


def test_wrappers_refuse():
    from distributed_learning_simulator_amd import _native
    from distributed_learning_simulator_amd.hetero import HeteroPlan, vector_view
    from distributed_learning_simulator_amd.models import LeNet5
    with pytest.raises(ValueError, match="1..MAX_LEVELS=8 width levels, not 9"):
        plan_of(LeNet5(), [1 - 0.1 * i for i in range(9)])
    plan = HeteroPlan([vector_view("b", 8, "c")], (1.0, 0.5))
    assert plan.level_P == [64, 64]
    ragged, prev = torch.zeros(128), torch.zeros(64)
    call = lambda levels, starts, weights: _native.hetero_fedavg(plan, levels, starts, weights,
                                                                 ragged, prev)
    with pytest.raises(RuntimeError, match=r"K=1025 clients \(1\.\.HETERO_MAX_K=1024\)"):
        call([0] * 1025, [0] * 1025, [1.0] * 1025)
    for w in (0.0, -1.0, float("inf"), float("nan"), 1e39):
        with pytest.raises(RuntimeError, match=r"weights\[1\]"):
            call([0, 1], [0, 64], [1.0, w])
    with pytest.raises(RuntimeError, match="not a level of the plan"):
        call([0, 2], [0, 64], [1.0, 1.0])
    for start in (68, 66, -4):  # past the end of ragged, off a 16-byte boundary, before it
        with pytest.raises(RuntimeError, match="the row of client 1"):
            call([0, 1], [0, start], [1.0, 1.0])
    with pytest.raises(RuntimeError, match="not on the GPU"):  # every check passes
        call([0, 1], [0, 64], [1.0, 2.0])
    with pytest.raises(RuntimeError, match="rows must be"):
        _native.hetero_extract(plan, prev, torch.zeros(64))


def test_server_factory_and_simulator_refuse(monkeypatch):
    from distributed_learning_simulator_amd import _native, distributed, factory, simulator
    from distributed_learning_simulator_amd.models import LeNet5
    from distributed_learning_simulator_amd.servers.fed_hetero_server import (FedHeteroServer,
                                                                             HeteroUpdate)
    from distributed_learning_simulator_amd.workers.fed_hetero_worker import FedHeteroWorker
    from tests.test_topk_host import FakeTrainer

    def extract(plan, flat, rows=None, stream=None):  # the downlink from the numpy restatement
        return [torch.from_numpy(ref.extract(flat.numpy(), plan.tensors(), plan.slices[l], n))
                for l, n in enumerate(plan.level_P)]

    monkeypatch.setattr(_native, "hetero_extract", extract)
    model = LeNet5()
    make = lambda **kw: factory.get_server("fed_hetero", sharded=False, synchronous=True, device=CPU,
                                           **{"tester": None, "worker_number": 3, "widths": (1.0, 0.5),
                                              "views": model.hetero_views(),
                                              "initial_model": dict(model.named_parameters()), **kw})
    server = make()
    assert type(server) is FedHeteroServer and server._levels == [0, 1, 0]
    for kwargs, match in (({"widths": [1 - 0.1 * i for i in range(9)]}, "MAX_LEVELS=8"),
                          ({"worker_number": 1025}, "MAX_K=1024"),
                          ({"aggregation_rule": "median"}, "does not support aggregation_rule"),
                          ({"aggregation_mode": "fma"}, "one arithmetic"),
                          ({"initial_model": None}, "full-width model to start from"),
                          ({"views": None}, "slice views")):
        with pytest.raises(ValueError, match=match):
            make(**kwargs)
    half = server.plan.level_P[1]
    for match, task in (("must be a HeteroUpdate", (1, 10, {"w": 1})),
                        (f"has {half + 64} elements, level 1", (1, 10, HeteroUpdate(0.5, torch.zeros(half + 64)))),
                        ("dealt it 1.0", (0, 10, HeteroUpdate(0.5, torch.zeros(half)))),
                        ("sample count 0", (1, 0, HeteroUpdate(0.5, torch.zeros(half)))),
                        ("sample count nan", (1, float("nan"), HeteroUpdate(0.5, torch.zeros(half))))):
        with pytest.raises(ValueError, match=match):
            server.worker_data_queue.add_task(task)
    assert not server._counts
    with pytest.raises(RuntimeError, match="fed_hetero runs on the one-process server only"):
        distributed.get_sharded_server("fed_hetero", tester=None, worker_number=2)
    worker = factory.get_worker("fed_hetero", trainer=FakeTrainer(LeNet5(width=0.5), 10), width=0.5,
                                worker_id=1, worker_data_queue=server.worker_data_queue, round=1)
    assert type(worker) is FedHeteroWorker
    worker.load_model(server.worker_data_queue.get_result(consumer=1))
    assert worker.hetero_update().row.numel() == half
    wide = FedHeteroWorker(trainer=FakeTrainer(LeNet5(), 10), width=0.5, worker_id=1,
                           worker_data_queue=server.worker_data_queue, round=1)
    with pytest.raises(ValueError, match="build the trainer's model with width="):
        wide.load_model(server._broadcast())
    head = ["--worker_number", "4", "--round", "1", "--distributed_algorithm"]
    cfg = simulator.get_config(head + ["fed_hetero", "--hetero_widths", "1,0.5,0.25",
                                       "--hetero_rolling", "1"])
    assert [simulator.hetero_width(cfg, i) for i in range(4)] == [1.0, 0.5, 0.25, 1.0]
    assert simulator.server_kwargs(cfg) == {"aggregation_mode": "exact", "rolling": True,
                                            "widths": (1.0, 0.5, 0.25)}
    cfg = simulator.get_config(head + ["fed_hetero"])
    assert simulator.server_kwargs(cfg)["widths"] == (1.0,) and simulator.hetero_width(cfg, 3) == 1.0
    for bad in (["fed", "--hetero_widths", "1,0.5"], ["fed_hetero", "--hetero_widths", "1,0"],
                ["fed_hetero", "--hetero_rolling", "2"]):
        with pytest.raises(SystemExit):
            simulator.get_config(head + bad)
