"""fed_scaffold without a GPU: the float32 restatement against the fp64 formulas, the option-II
identity, the worker's and server's refusals, the factory and the simulator's flags."""
import numpy as np
import pytest
import torch

from tests import cpu_doubles, scaffold_ref as ref
from tests.test_topk_host import CPU, FakeTrainer, initial_model, make_model

U24 = 2.0 ** -24


def gamma(n):
    """An expression whose every term passes through at most n fp32 roundings (round to nearest,
    unit roundoff u = 2^-24, no underflow) is off by at most ((1 + u)^n - 1) * sum |terms|, to
    first order n * u * sum |terms|; no output of the three contracts is deeper than 7 at the
    K = 4 used here, so |err| <= 7 * 2^-24 * sum |terms| throughout.  n is counted per
    contract below."""
    assert n <= 7
    return n * U24


def test_float32_restatement_against_fp64():
    rng = np.random.default_rng(1)
    K, P = 4, 512
    v = lambda *shape: rng.normal(0, 1, shape).astype(np.float32)
    # fp64 runs on the fp32-rounded coefficients: the coefficients' own rounding is the caller's
    lr, wd, mu = (float(np.float32(t)) for t in (0.1, 5e-4, 0.01))
    p, g, x, corr = v(P), v(P), v(P), v(P)
    got = ref.local_step(p, g, x, corr, lr, wd, mu, True)
    want = ref.local_step(p, g, x, corr, lr, wd, mu, True, np.float64)
    terms = abs(p) + lr * (abs(g) + wd * abs(p) + mu * (abs(p) + abs(x)) + abs(corr))
    # deepest terms, wd * p and mu * (p - x): the product (and the subtraction before it), the
    # additions into d that follow (with corr the last), lr * d, p - : at most 6 roundings
    assert (abs(got - want) <= gamma(6) * terms.astype(np.float64)).all()
    y, c, ci = v(P), v(P), v(P)
    a = float(ref.coeff(5, 0.1))
    d32, n32, bad = ref.finish(y, x, c, ci, a, True)
    d64, n64, _ = ref.finish(y, x, c, ci, a, True, np.float64)
    assert bad == 0 and (abs(d32 - d64) <= gamma(1) * (abs(y) + abs(x)).astype(np.float64)).all()
    # y - x, a *, the outer subtraction: 3 roundings on the deepest term
    terms = abs(ci) + abs(c) + a * (abs(y) + abs(x))
    assert (abs(n32 - n64) <= gamma(3) * terms.astype(np.float64)).all()
    U, n = v(K, P), [300, 120, 777, 64]
    b = [float(ref.coeff(5, 0.1, 10)) for _ in range(K)]
    eta, f = 1.0, float(np.float32(K / 10))
    x32, c32 = ref.server_step(U, n, b, eta, f, x, c, True)
    x64, c64 = ref.server_step(U, n, b, eta, f, x, c, True, np.float64)
    w = np.asarray(n, np.float64) / sum(n)
    # row 0's term: product, quotient, K - 1 additions, eta *, x + : K + 3 = 7 roundings
    terms = abs(x) + eta * (abs(U.astype(np.float64)) * w[:, None]).sum(0)
    assert (abs(x32 - x64) <= gamma(K + 3) * terms).all()
    # row 0 of s: product, K - 1 additions, the last subtraction: K + 1; f * c: 3
    terms = abs(c) * (1 + f) + (abs(U.astype(np.float64)) * np.asarray(b)[:, None]).sum(0)
    assert (abs(c32 - c64) <= gamma(K + 1) * terms).all()


def test_option_two_identity():
    """c_i' - c_i = -c - a * delta: what lets the server derive the control delta from the row."""
    rng = np.random.default_rng(2)
    y, x, c, ci = rng.normal(0, 1, (4, 64))
    a = 1.0 / (5 * 0.1)
    delta, new, _ = ref.finish(y, x, c, ci, a, True, np.float64)
    assert np.allclose(new - ci, -c - a * delta, rtol=0, atol=1e-14)


class MomentumTrainer(FakeTrainer):
    def get_optimizer(self):
        return torch.optim.SGD(self.model.parameters(), lr=0.1, momentum=0.9)


def test_factory_and_refusals(monkeypatch):
    from distributed_learning_simulator_amd import factory
    from distributed_learning_simulator_amd.servers.fed_scaffold_server import FedScaffoldServer
    from distributed_learning_simulator_amd.workers.fed_scaffold_worker import (FedScaffoldWorker,
                                                                                ScaffoldUpdate)
    cpu_doubles.install(monkeypatch)
    make = lambda **kw: factory.get_server("fed_scaffold", sharded=False, tester=None, worker_number=3,
                                           synchronous=True, device=CPU,
                                           **{"initial_model": initial_model(), **kw})
    server = make(global_lr=0.5)
    assert type(server) is FedScaffoldServer and server.control.numel() == server.layout.P == 128
    assert make(control=False).control is None
    wk = dict(worker_id=0, worker_data_queue=None, round=1)
    worker = factory.get_worker("fed_scaffold", trainer=FakeTrainer(make_model(), 10), mu=0.01,
                                control=False, **wk)
    assert type(worker) is FedScaffoldWorker and (worker.mu, worker.use_control) == (0.01, False)
    assert {"scaffold", "send_parameter"} <= set(worker.trainer.callbacks)
    with pytest.raises(ValueError, match="momentum=0.9 must be 0"):
        factory.get_worker("fed_scaffold", trainer=MomentumTrainer(make_model(), 10), **wk)
    for mu in (-0.1, float("nan"), "0.1"):
        with pytest.raises(ValueError, match="mu="):
            factory.get_worker("fed_scaffold", trainer=FakeTrainer(make_model(), 10), mu=mu, **wk)
    for kwargs in ({"aggregation_rule": "median"}, {"server_optimizer": "adam"}, {"dp_clip": 1.0},
                   {"attack": "sign_flip", "attackers": (1,)}, {"aggregation_mode": "fma"},
                   {"global_lr": 0.0}, {"initial_model": None}):
        with pytest.raises(ValueError, match="one fused step|one arithmetic|global_lr=|needs a model"):
            make(**kwargs)
    for match, payload in (("must be a ScaffoldUpdate", {"w": 1}),
                           ("P=64", ScaffoldUpdate(torch.zeros(64), 5, 0.1)),
                           ("steps=0", ScaffoldUpdate(torch.zeros(128), 0, 0.1))):
        with pytest.raises(ValueError, match=match):
            server.worker_data_queue.add_task((0, 10, payload))
    assert not server._payloads


def test_simulator_flags():
    from distributed_learning_simulator_amd import simulator
    head = ["--worker_number", "2", "--round", "1", "--distributed_algorithm"]
    cfg = simulator.get_config(head + ["fed_scaffold"])
    assert simulator.worker_kwargs(cfg) == {"mu": 0.0, "control": True}
    assert simulator.server_kwargs(cfg) == {"aggregation_mode": "exact", "global_lr": 1.0,
                                            "control": True}
    cfg = simulator.get_config(head + ["fed_scaffold", "--scaffold_control", "0", "--scaffold_mu",
                                       "0.01", "--scaffold_global_lr", "0.5"])
    assert simulator.worker_kwargs(cfg) == {"mu": 0.01, "control": False}
    assert simulator.server_kwargs(cfg)["global_lr"] == 0.5
    for bad in (["fed", "--scaffold_mu", "0.1"], ["fed_scaffold", "--scaffold_mu", "-1"],
                ["fed_scaffold", "--scaffold_control", "2"]):
        with pytest.raises(SystemExit):
            simulator.get_config(head + bad)
