"""fed_topk without a GPU: the numpy reference against closed forms, FedTopKWorker /
FedTopKServer on CPU doubles built on that reference, validation, the simulator's flags,
and the library's and the wrappers' argument checks."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import topk_ref
from tests.topk_ref import bits

F32 = np.float32
NEG0 = np.uint32(0x80000000)


# ------------------------------------------------------------------ the reference
def test_reference_compress_hand_written():
    #               0    1     2     3    4     5    6    7     8    9    10   11
    w = np.array([0.5, -3.0, 0.25, 2.0, -0.0, 1.0, -2.0, 0.0, 4.0, 2.0, -1.0, 0.125], F32)
    base, e = np.zeros(12, F32), np.zeros(12, F32)
    e[4] = F32(-0.0)                    # u[4] = -0.0 + -0.0 = -0.0
    e[5] = F32(1.0)                     # u[5] = 2.0: the residual lifts it into the tie
    u = topk_ref.update(w, base, e)
    assert bits(u)[4] == NEG0 and u[5] == 2.0
    # keys: 4.0 > 3.0 > {2.0 at 3, 5, 6 (-2.0), 9} > ...; k = 4 takes two of the tie: 3 and 5
    idx, val, e_new, bad = topk_ref.compress(w, base, e, 4)
    assert idx.tolist() == [1, 3, 5, 8] and idx.dtype == np.int32
    assert val.tolist() == [-3.0, 2.0, 2.0, 4.0] and bad == 0
    expect = u.copy()
    expect[[1, 3, 5, 8]] = 0.0
    assert np.array_equal(bits(e_new), bits(expect))
    assert bits(e_new)[4] == NEG0 and e_new[6] == -2.0 and e_new[9] == 2.0
    # k = 5: the tie's next member is the -2.0 at 6 (+x and -x tie, the lowest index wins)
    assert topk_ref.compress(w, base, e, 5)[0].tolist() == [1, 3, 5, 6, 8]
    # k = 1 and k = P
    idx, val, e_new, _ = topk_ref.compress(w, base, e, 1)
    assert idx.tolist() == [8] and val.tolist() == [4.0] and e_new[8] == 0.0 and e_new[1] == -3.0
    idx, val, e_new, _ = topk_ref.compress(w, base, e, 12)
    assert idx.tolist() == list(range(12)) and np.array_equal(bits(val), bits(u))
    assert np.array_equal(bits(e_new), np.zeros(12, np.uint32))  # all +0.0, the -0.0 was sent
    assert bits(val)[4] == NEG0


def test_reference_nonfinite_keys_are_largest():
    w = np.array([1.0, np.inf, 3e38, np.nan, -np.inf, 0.0, 2.0, -np.nan], F32)
    z = np.zeros(8, F32)
    idx, _, _, bad = topk_ref.compress(w, z, z, 2)
    assert idx.tolist() == [3, 7] and bad == 4
    assert topk_ref.compress(w, z, z, 3)[0].tolist() == [1, 3, 7]


def test_reference_exact_split_invariant():
    rng = np.random.default_rng(0)
    for P, k in ((64, 1), (64, 64), (1000, 10), (4100, 2050)):
        w, base = rng.standard_normal(P).astype(F32), rng.standard_normal(P).astype(F32)
        e = (rng.standard_normal(P) * 0.1).astype(F32)
        w[rng.random(P) < 0.1] = 0.5   # ties
        base[rng.random(P) < 0.5] = 0.0
        u = topk_ref.update(w, base, e)
        idx, val, e_new, _ = topk_ref.compress(w, base, e, k)
        assert idx.size == k and np.all(np.diff(idx) > 0)
        sent = np.zeros(P, bool)
        sent[idx] = True
        assert np.array_equal(bits(val), bits(u[idx]))
        assert np.all(bits(e_new[sent]) == 0) and np.array_equal(bits(e_new[~sent]), bits(u[~sent]))
        cut = topk_ref.keys(u)[idx].min()
        assert np.all(topk_ref.keys(u)[~sent] <= cut)


def test_reference_sparse_fedavg_closed_forms():
    P = 8
    base = np.array([1.0, -0.0, 0.5, 2.0, -0.0, 3.0, 0.25, -1.0], F32)
    v = np.array([0.1, 0.2, -0.3, 0.4, 0.5, -0.6, 0.7, 0.8], F32)
    n = 300
    out = topk_ref.sparse_fedavg(base, [(np.arange(P, dtype=np.int32), v)], [n])
    assert np.array_equal(bits(out), bits(base + ((v * F32(n)).astype(F32) / F32(n)).astype(F32)))
    # an untouched -0.0 stays -0.0 (copied, not added to zero); a touched one is base + acc
    out = topk_ref.sparse_fedavg(base, [(np.array([0, 4], np.int32), np.array([0.5, -0.0], F32))], [n])
    assert bits(out)[1] == NEG0 and bits(out)[4] == NEG0 and out[0] == 1.5
    assert np.array_equal(bits(out[[2, 3, 5, 6, 7]]), bits(base[[2, 3, 5, 6, 7]]))
    # two clients that overlap on coordinates 2 and 5: the hand-computed chain in both orders
    a = (np.array([1, 2, 5], np.int32), np.array([0.1, 0.3, 1e-3], F32))
    b = (np.array([2, 5, 7], np.int32), np.array([1e-8, 0.7, 0.2], F32))
    na, nb = 100, 999
    N = F32(na + nb)

    def term(x, n_):
        return (F32(x) * F32(n_)) / N

    ab = topk_ref.sparse_fedavg(base, [a, b], [na, nb])
    ba = topk_ref.sparse_fedavg(base, [b, a], [nb, na])
    for c, (x, y) in ((2, (0.3, 1e-8)), (5, (1e-3, 0.7))):
        assert bits(ab[c:c + 1])[0] == bits(np.array([base[c] + (term(x, na) + term(y, nb))], F32))[0]
        assert bits(ba[c:c + 1])[0] == bits(np.array([base[c] + (term(y, nb) + term(x, na))], F32))[0]
    assert ab[1] == base[1] + term(0.1, na) and ab[7] == base[7] + term(0.2, nb)
    rest = [0, 1, 3, 4, 6, 7]
    assert np.array_equal(bits(ab[rest]), bits(ba[rest]))
    # where both sent, the order can show in the bits: many coordinates, some must differ
    rng = np.random.default_rng(1)
    big = rng.standard_normal(4096).astype(F32)
    every = np.arange(4096, dtype=np.int32)
    pa, pb, pc = ((every, rng.standard_normal(4096).astype(F32)) for _ in range(3))
    x = topk_ref.sparse_fedavg(big, [pa, pb, pc], [100, 999, 517])
    y = topk_ref.sparse_fedavg(big, [pc, pb, pa], [517, 999, 100])
    assert (bits(x) != bits(y)).any() and np.allclose(x, y, rtol=1e-5, atol=1e-6)


# ------------------------------------------------------- worker and server, CPU doubles
class FakeTrainer:
    """What FedTopKWorker touches of a trainer; the test plays the training."""

    def __init__(self, model, samples):
        self.model = model
        self.dataset = (torch.zeros(samples, 1), torch.zeros(samples))
        self.callbacks = {}

    def add_named_callback(self, point, name, fn):
        self.callbacks[name] = fn

    def set_device(self, device):
        pass

    def get_optimizer(self):  # the sign_SGD worker looks at it
        return torch.optim.SGD(self.model.parameters(), lr=0.1)


CPU = torch.device("cpu")


def make_model(seed=0):
    torch.manual_seed(seed)
    return torch.nn.Linear(5, 3)  # weight [3, 5], bias [3]: 18 real parameters, P = 128


def initial_model():
    return {k: v.detach().clone() for k, v in make_model().named_parameters()}


def flat_of(layout, d):
    return layout.flatten(d, device=CPU).numpy()


def make_run(monkeypatch, error_feedback=True, server_cls=None, ratio=0.1):
    from distributed_learning_simulator_amd.servers.fed_topk_server import FedTopKServer
    from distributed_learning_simulator_amd.workers.fed_topk_worker import FedTopKWorker
    topk_ref.install(monkeypatch)
    server = (server_cls or FedTopKServer)(initial_model=initial_model(), tester=None,
                                           worker_number=3, synchronous=True, device=CPU)
    ns = {0: 300, 1: 120, 2: 777}
    workers = {i: FedTopKWorker(worker_id=i, trainer=FakeTrainer(make_model(10 + i), ns[i]),
                                worker_data_queue=server.worker_data_queue, round=2,
                                topk_ratio=ratio, error_feedback=error_feedback)
               for i in range(3)}
    for i, w in workers.items():
        assert "send_parameter" in w.trainer.callbacks
        w.load_model(server.worker_data_queue.get_result(consumer=i))
        assert w.k == math.ceil(ratio * 18) and w.layout.P == 128
    return server, workers, ns


def train(worker, deltas):
    """The model moves by ``deltas``: {flat real-parameter position in the weight: step}."""
    with torch.no_grad():
        weight = dict(worker.trainer.model.named_parameters())["weight"].view(-1)
        for pos, d in deltas.items():
            weight[pos] += d


def play_round(server, workers, ns, order, deltas):
    layout = server.layout
    prev = flat_of(layout, server.prev_model)
    captured = {}
    for wid in order:
        train(workers[wid], deltas[wid])
        p = workers[wid].sparse_update()
        captured[wid] = (p.idx.numpy().copy(), p.val.numpy().copy())
        server.worker_data_queue.add_task((wid, ns[wid], p))
    models = {wid: server.worker_data_queue.get_result(consumer=wid) for wid in order}
    ref = topk_ref.sparse_fedavg(prev, [captured[i] for i in order], [ns[i] for i in order])
    for wid in order:
        assert np.array_equal(bits(flat_of(layout, models[wid])), bits(ref))
        workers[wid].load_model(models[wid])
    assert np.array_equal(bits(flat_of(layout, server.prev_model)), bits(ref))
    return captured


ROUND1 = {0: {0: 1.0, 1: -0.9, 2: 0.8}, 1: {0: 0.5, 7: 0.25}, 2: {3: -0.125, 14: 2.0}}
ROUND2 = {0: {0: 0.5, 4: 0.45}, 1: {1: 0.5, 2: -0.75}, 2: {3: 1.0, 5: 0.5}}


@pytest.mark.parametrize("error_feedback", [True, False])
def test_two_rounds_on_cpu_doubles(monkeypatch, error_feedback):
    server, workers, ns = make_run(monkeypatch, error_feedback)
    first = play_round(server, workers, ns, [2, 0, 1], ROUND1)
    assert first[0][0].tolist() == [0, 1]          # 0.8 at position 2 just missed the cut
    assert server.round == 1
    residual = workers[0].residual.numpy()
    assert abs(residual[2] - 0.8) < 1e-6 and residual[0] == 0.0 and residual[1] == 0.0
    second = play_round(server, workers, ns, [1, 2, 0], ROUND2)
    assert server.round == 2 and [sorted(c) for c in server.payload_counts] == [[0, 1, 2]] * 2
    assert all(n == 2 for c in server.payload_counts for n in c.values())
    if error_feedback:   # ... and is sent in round 2 from the residual, ahead of the 0.45
        assert second[0][0].tolist() == [0, 2] and abs(second[0][1][1] - 0.8) < 1e-6
    else:                # plain top-k forgets it
        assert second[0][0].tolist() == [0, 4]


def test_get_subset_model(monkeypatch):
    from distributed_learning_simulator_amd.servers.fed_topk_server import FedTopKServer
    seen = {}

    class Recording(FedTopKServer):
        def _process_aggregated_parameter(self, aggregated):
            for key, subset in (("pair", [0, 2]), ("swapped", [2, 0]), ("one", [1]), ("empty", [])):
                seen[key] = {k: v.clone() for k, v in self.get_subset_model(subset).items()}
            with pytest.raises(ValueError, match="sent no update"):
                self.get_subset_model([0, 9])
            return aggregated

    server, workers, ns = make_run(monkeypatch, server_cls=Recording)
    prev = flat_of(server.layout, server.prev_model)
    # all three move position 0, so the subset's order is in the chain
    deltas = {0: {0: 1.0, 1: 0.3}, 1: {0: 0.7, 2: 0.1}, 2: {0: -0.9, 1: 0.2}}
    cap = play_round(server, workers, ns, [1, 2, 0], deltas)
    lay = server.layout
    for key, subset in (("pair", [0, 2]), ("swapped", [2, 0]), ("one", [1])):
        ref = topk_ref.sparse_fedavg(prev, [cap[i] for i in subset], [ns[i] for i in subset])
        assert np.array_equal(bits(flat_of(lay, seen[key])), bits(ref)), key
    assert np.array_equal(bits(flat_of(lay, seen["empty"])), bits(prev))


# ------------------------------------------------------------------ validation
@pytest.mark.parametrize("ratio", [0.0, -0.1, 1.5, float("nan"), "0.1", True, None])
def test_worker_rejects_ratio(ratio):
    from distributed_learning_simulator_amd.workers.fed_topk_worker import FedTopKWorker
    with pytest.raises(ValueError, match="topk_ratio"):
        FedTopKWorker(worker_id=0, trainer=FakeTrainer(make_model(), 10), worker_data_queue=None,
                      round=1, topk_ratio=ratio)


def test_topk_count():
    from distributed_learning_simulator_amd.workers.fed_topk_worker import topk_count
    assert topk_count(0.01, 11173962) == 111740 and topk_count(0.05, 61706) == 3086
    assert topk_count(1e-9, 18) == 1 and topk_count(1.0, 18) == 18 and topk_count(0.1, 18) == 2


def test_server_rejects_payloads(monkeypatch):
    from distributed_learning_simulator_amd.workers.fed_topk_worker import SparseUpdate
    server, _, _ = make_run(monkeypatch)
    P = server.layout.P

    def send(idx, val, rows=P):
        server.worker_data_queue.add_task((0, 10, SparseUpdate(
            torch.tensor(idx, dtype=torch.int32), torch.tensor(val, dtype=torch.float32), rows)))

    with pytest.raises(ValueError, match="strictly ascending"):
        send([3, 1], [0.1, 0.2])
    with pytest.raises(ValueError, match="strictly ascending"):
        send([1, 1], [0.1, 0.2])
    with pytest.raises(ValueError, match=r"0\.\.P-1"):
        send([1, P], [0.1, 0.2])
    with pytest.raises(ValueError, match=r"0\.\.P-1"):
        send([-1, 2], [0.1, 0.2])
    with pytest.raises(ValueError, match="P=64"):
        send([1, 2], [0.1, 0.2], rows=64)
    with pytest.raises(ValueError, match="val"):
        send([1, 2], [0.1])
    with pytest.raises(ValueError, match="int32"):
        server.worker_data_queue.add_task((0, 10, SparseUpdate(torch.tensor([1]), torch.tensor([0.1]), P)))
    with pytest.raises(ValueError, match="SparseUpdate"):
        server.worker_data_queue.add_task((0, 10, {"weight": torch.zeros(3, 5)}))
    assert not server._payloads and server.round == 0


def test_server_needs_a_model_and_refuses_dense_features(monkeypatch):
    from distributed_learning_simulator_amd.servers.fed_topk_server import FedTopKServer
    topk_ref.install(monkeypatch)
    with pytest.raises(ValueError, match="tester or initial_model"):
        FedTopKServer(tester=None, worker_number=3, synchronous=True, device=CPU)
    reason = "it holds the clients' sparse updates, not fp32 rows"
    for extra in ({"aggregation_rule": "median"}, {"attack": "alie", "attackers": (0,)},
                  {"server_optimizer": "adam"}):
        with pytest.raises(ValueError) as err:
            FedTopKServer(initial_model=initial_model(), tester=None, worker_number=3,
                          synchronous=True, device=CPU, **extra)
        assert "FedTopKServer does not support" in str(err.value) and reason in str(err.value)
    with pytest.raises(ValueError, match="aggregation_mode"):
        FedTopKServer(initial_model=initial_model(), tester=None, worker_number=3,
                      synchronous=True, device=CPU, aggregation_mode="fma")


def test_worker_raises_on_nonfinite_update(monkeypatch):
    _, workers, _ = make_run(monkeypatch)
    train(workers[1], {3: float("inf"), 4: float("nan")})
    with pytest.raises(ValueError, match=r"worker 1: 2 coordinates"):
        workers[1].sparse_update()


def test_factory_names(monkeypatch):
    from distributed_learning_simulator_amd import distributed, factory
    from distributed_learning_simulator_amd.servers.fed_topk_server import FedTopKServer
    from distributed_learning_simulator_amd.workers.fed_topk_worker import FedTopKWorker
    topk_ref.install(monkeypatch)
    server = factory.get_server("fed_topk", sharded=False, initial_model=initial_model(),
                                tester=None, worker_number=2, synchronous=True, device=CPU)
    assert type(server) is FedTopKServer
    worker = factory.get_worker("fed_topk", worker_id=0, trainer=FakeTrainer(make_model(), 4),
                                worker_data_queue=server.worker_data_queue, round=1,
                                topk_ratio=0.5, error_feedback=False)
    assert type(worker) is FedTopKWorker and worker.topk_ratio == 0.5 and not worker.error_feedback
    servers = {"fed": "FedServer", "fed_quant": "FedQuantServer", "sign_SGD": "SignSGDServer",
               "multiround_shapley_value": "MultiRoundShapleyValueServer",
               "GTG_shapley_value": "GTGShapleyValueServer"}
    for name, cls in servers.items():
        made = factory.get_server(name, sharded=False, tester=None, worker_number=2,
                                  synchronous=True, device=CPU)
        assert type(made).__name__ == cls, name
    workers = {"fed": "FedWorker", "fed_quant": "FedQuantWorker", "sign_SGD": "SignSGDWorker",
               "multiround_shapley_value": "FedWorker", "GTG_shapley_value": "FedWorker"}
    for name, cls in workers.items():
        extra = {"qat": False} if name == "fed_quant" else {}
        made = factory.get_worker(name, worker_id=0, trainer=FakeTrainer(make_model(), 4),
                                  worker_data_queue=server.worker_data_queue, round=1, **extra)
        assert type(made).__name__ == cls, name
    with pytest.raises(RuntimeError, match="unknown algorithm"):
        factory.get_server("fed_topq", sharded=False)
    with pytest.raises(RuntimeError, match="one-process server only"):
        distributed.get_sharded_server("fed_topk", tester=None, worker_number=2)
    with pytest.raises(RuntimeError, match="one-process server only"):
        factory.get_server("fed_topk", sharded=True, tester=None, worker_number=2)


# ------------------------------------------------------------------ simulator flags
BASE = ["--worker_number", "4", "--round", "2"]


def test_simulator_flags():
    from distributed_learning_simulator_amd import simulator
    cfg = simulator.get_config(["--distributed_algorithm", "fed_topk"] + BASE)
    assert cfg.topk_ratio == 0.01 and cfg.topk_error_feedback == 1
    assert simulator.worker_kwargs(cfg) == {"topk_ratio": 0.01, "error_feedback": True}
    assert simulator.server_kwargs(cfg) == {"aggregation_mode": "exact"}
    cfg = simulator.get_config(["--distributed_algorithm", "fed_topk", "--topk_ratio", "0.05",
                                "--topk_error_feedback", "0"] + BASE)
    assert simulator.worker_kwargs(cfg) == {"topk_ratio": 0.05, "error_feedback": False}
    for flag in (["--topk_ratio", "0.05"], ["--topk_error_feedback", "1"]):
        for algo in ("fed", "fed_quant", "sign_SGD", "GTG_shapley_value"):
            with pytest.raises(SystemExit):
                simulator.get_config(["--distributed_algorithm", algo] + flag + BASE)
    with pytest.raises(SystemExit):
        simulator.get_config(["--distributed_algorithm", "fed_topk", "--topk_error_feedback", "2"] + BASE)


def test_simulator_kwargs_unchanged_for_existing_algorithms():
    from distributed_learning_simulator_amd import simulator
    expect = {"fed": {"aggregation_mode": "exact"}, "fed_quant": {"aggregation_mode": "exact"},
              "sign_SGD": {},
              "GTG_shapley_value": {"aggregation_mode": "exact", "utility_metric": "acc"},
              "multiround_shapley_value": {"aggregation_mode": "exact", "utility_metric": "acc"}}
    for algo, kwargs in expect.items():
        cfg = simulator.get_config(["--distributed_algorithm", algo] + BASE)
        assert simulator.server_kwargs(cfg) == kwargs, algo
        assert simulator.worker_kwargs(cfg) == {}, algo
    cfg = simulator.get_config(["--distributed_algorithm", "fed", "--aggregation_rule",
                                "trimmed_mean", "--trim", "1", "--server_optimizer", "adam"] + BASE)
    assert simulator.server_kwargs(cfg) == {"aggregation_mode": "exact",
                                            "aggregation_rule": "trimmed_mean", "trim": 1,
                                            "server_optimizer": "adam"}


# ------------------------------------------------------- the library without a GPU
def _ptrs(n, start=1 << 20, step=1 << 16):
    """Never-dereferenced, 16-byte aligned, far apart: validation comes before any access."""
    return [ctypes.c_void_p(start + i * step) for i in range(n)]


def test_entry_points_reject_bad_arguments_without_gpu():
    from distributed_learning_simulator_amd import _native
    L = _native.lib()
    w, base, e, idx, val, stats, ws, out, off, weight = _ptrs(10)
    P, k = 64, 8

    def compress(**kw):
        a = dict(w=w, base=base, e=e, P=P, k=k, idx=idx, val=val, stats=stats, ws=ws)
        a.update(kw)
        rc = L.dls_topk_compress_f32(a["w"], a["base"], a["e"], a["P"], a["k"], a["idx"], a["val"],
                                     a["stats"], a["ws"], None)
        return rc, L.dls_last_error()

    for name in ("w", "base", "e", "idx", "val", "stats", "ws"):
        rc, msg = compress(**{name: None})
        assert rc == -1 and b"null pointer" in msg, name
    for bad_k in (0, -1, P + 1):
        rc, msg = compress(k=bad_k)
        assert rc == -1 and b"k=" in msg
    rc, msg = compress(P=62, k=1)
    assert rc == -2 and b"multiple of 4" in msg
    for bad_p in (0, 1 << 31, 1 << 40):
        rc, msg = compress(P=bad_p, k=1)
        assert rc == -1 and b"P=" in msg
    for name in ("w", "base", "e", "idx", "val", "ws"):
        rc, msg = compress(**{name: ctypes.c_void_p((1 << 24) + 4)})
        assert rc == -2 and b"alignment" in msg, name
    for other in (w, base):  # e on, and half a row into, w / base
        for shift in (0, 2 * P):
            rc, msg = compress(e=ctypes.c_void_p(other.value + shift))
            assert rc == -1 and b"alias" in msg

    assert L.dls_topk_workspace(0) == -1 and b"P=" in L.dls_last_error()
    assert L.dls_topk_workspace(1 << 31) == -1
    small, large = L.dls_topk_workspace(64), L.dls_topk_workspace(11174464)
    assert 0 < small < large and small % 16 == 0 and large < 1 << 20

    def sparse(**kw):
        a = dict(base=base, idx=idx, val=val, off=off, weight=weight, K=3, total=10.0, P=P, out=out)
        a.update(kw)
        rc = L.dls_sparse_fedavg_f32(a["base"], a["idx"], a["val"], a["off"], a["weight"], a["K"],
                                     a["total"], a["P"], a["out"], None)
        return rc, L.dls_last_error()

    for name in ("base", "idx", "val", "off", "weight", "out"):
        rc, msg = sparse(**{name: None})
        assert rc == -1 and b"null pointer" in msg, name
    for bad_k in (0, -2):
        rc, msg = sparse(K=bad_k)
        assert rc == -1 and b"K=" in msg
    rc, msg = sparse(P=62)
    assert rc == -2 and b"multiple of 4" in msg
    rc, msg = sparse(P=1 << 31)
    assert rc == -1 and b"P=" in msg
    for name in ("base", "out"):
        rc, msg = sparse(**{name: ctypes.c_void_p((1 << 24) + 8)})
        assert rc == -2 and b"alignment" in msg
    for shift in (0, 16):
        rc, msg = sparse(out=ctypes.c_void_p(base.value + shift))
        assert rc == -1 and b"alias" in msg


def test_wrappers_validate_operands_without_gpu():
    from distributed_learning_simulator_amd import _native
    P, k = 64, 8

    def ops():
        return dict(w=torch.zeros(P), base=torch.zeros(P), e=torch.zeros(P), k=k, P=P,
                    idx=torch.zeros(k, dtype=torch.int32), val=torch.zeros(k),
                    stats=torch.zeros(2, dtype=torch.int32),
                    workspace=_native.topk_workspace(P, CPU))

    def compress(match, **kw):
        a = ops()
        a.update(kw)
        with pytest.raises(RuntimeError, match=match):
            _native.topk_compress(a["w"], a["base"], a["e"], a["k"], a["P"], a["idx"], a["val"],
                                  a["stats"], a["workspace"])

    compress("not on the GPU")  # every check passes
    for name in ("w", "base", "e"):
        for bad in (torch.zeros(P, dtype=torch.float64), torch.zeros(P - 4), torch.zeros(2 * P)[::2],
                    torch.zeros(2, P)):
            compress(name + " must be", **{name: bad})
        compress(" on meta", **{name: torch.zeros(P, device="meta")})
        compress(name + " must be 16-byte aligned", **{name: torch.zeros(P + 4)[1:P + 1]})
    compress("idx must be", idx=torch.zeros(k, dtype=torch.int64))
    compress("idx must be", idx=torch.zeros(k - 1, dtype=torch.int32))
    compress("val must be", val=torch.zeros(k, dtype=torch.float16))
    compress("val must be", val=torch.zeros(2 * k)[::2])
    compress("stats must be", stats=torch.zeros(1, dtype=torch.int32))
    compress("workspace must be", workspace=torch.zeros(64, dtype=torch.uint8))
    compress("workspace must be", workspace=torch.zeros(1 << 16, dtype=torch.float32))
    for bad_k in (0, P + 1, 2.0, True):
        compress("k=", k=bad_k)
    for bad_p in (62, 0, -4, 1 << 31):
        compress("P=", P=bad_p)
    a = ops()
    compress("e and w overlap", e=a["w"], w=a["w"])
    both = torch.zeros(2 * P)
    compress("e and base overlap", e=both[:P], base=both[4:P + 4])
    compress("e and val overlap", e=both[:P], val=both[P - 4:P + 4])

    K, nnz = 3, 10

    def sops():
        return dict(base=torch.zeros(P), idx=torch.zeros(nnz, dtype=torch.int32), val=torch.zeros(nnz),
                    off=torch.tensor([0, 4, 4, nnz]), weight=torch.ones(K), total=3.0, P=P,
                    out=torch.zeros(P))

    def sparse(match, **kw):
        a = sops()
        a.update(kw)
        with pytest.raises(RuntimeError, match=match):
            _native.sparse_fedavg(a["base"], a["idx"], a["val"], a["off"], a["weight"], a["total"],
                                  a["P"], a["out"])

    sparse("not on the GPU")
    sparse("not on the GPU", idx=torch.zeros(0, dtype=torch.int32), val=torch.zeros(0),
           off=torch.zeros(K + 1, dtype=torch.int64))
    for name in ("base", "out"):
        for bad in (torch.zeros(P, dtype=torch.float64), torch.zeros(P - 4), torch.zeros(2 * P)[::2]):
            sparse(name + " must be", **{name: bad})
        sparse(" on meta", **{name: torch.zeros(P, device="meta")})
    sparse("16-byte aligned", out=torch.zeros(P + 4)[1:P + 1])
    sparse("weight must be", weight=torch.ones(K, dtype=torch.float64))
    sparse("weight must be", weight=torch.ones(0))
    sparse("off must be", off=torch.tensor([0, 4, nnz]))
    sparse("off must be", off=torch.tensor([0, 4, 4, nnz], dtype=torch.int32))
    sparse("idx must be", idx=torch.zeros(nnz, dtype=torch.int64))
    sparse("val must be", val=torch.zeros(nnz + 1))
    sparse("val must be", val=torch.zeros(nnz, dtype=torch.float64))
    for bad_total in (0.0, -1.0, float("inf"), float("nan")):
        sparse("total=", total=bad_total)
    for bad_p in (62, 0, 1 << 31):
        sparse("P=", P=bad_p)
    a = sops()
    sparse("out and base overlap", out=a["base"], base=a["base"])
    both = torch.zeros(2 * P)
    sparse("out and base overlap", base=both[:P], out=both[P - 4:2 * P - 4])
    sparse("out and val overlap", out=both[:P], val=both[P - 4:P - 4 + nnz])


def test_padding_slots_are_only_ever_sent_as_zeros(monkeypatch):
    """k counts the real parameters; with ratio 1 every real coordinate is sent and the
    layout's padding never is (18 real parameters in rows of P = 128)."""
    server, workers, ns = make_run(monkeypatch, ratio=1.0)
    assert math.ceil(1.0 * 18) == 18
    w = workers[0]
    assert w.k == 18
    train(w, {i: 0.1 * (i + 1) for i in range(15)})
    with torch.no_grad():
        dict(w.trainer.model.named_parameters())["bias"] += 1.0
    p = w.sparse_update()
    real = list(range(15)) + [64, 65, 66]
    assert p.idx.tolist() == real and len(p) == 18 and p.nbytes == 144
    assert float(w.residual.abs().max()) == 0.0


# ------------------------------------------------------------------ the launch plan
def test_launch_shape_constants_match_the_header():
    import os
    import re
    from distributed_learning_simulator_amd import _native
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                             "include", "dls_hip.h")).read()
    macros = dict(re.findall(r"#define DLS_TOPK_(\w+) (\d+)", text))
    assert {k: int(v) for k, v in macros.items()} == {
        "CHUNK": _native.TOPK_CHUNK, "HIST_BLOCKS": _native.TOPK_HIST_BLOCKS,
        "SCAN_BLOCK": _native.TOPK_SCAN_BLOCK}


def test_plan_model_matches_the_workspace_query():
    """topk_ref's chunk count against dls_topk_workspace (a host function) on both sides
    of every chunk edge near each launch cap, and at the ends of the range."""
    from distributed_learning_simulator_amd import _native
    L = _native.lib()
    C, H, S = _native.TOPK_CHUNK, _native.TOPK_HIST_BLOCKS, _native.TOPK_SCAN_BLOCK
    sizes = {4, 64, C - 4, C, C + 4, 65540, topk_ref.P_SCAN2, topk_ref.P_STRIDE, topk_ref.P_RESNET,
             _native.TOPK_MAX_P - 3}
    for cap in (S, 2 * S, H, 2 * H):
        for n in (cap - 1, cap, cap + 1):
            sizes |= {n * C - 4, n * C, n * C + 4}
    for P in sorted(sizes):
        assert L.dls_topk_workspace(P) == topk_ref.workspace_bytes(P), P
        assert topk_ref.nchunks(P) == (P + C - 1) // C
    # the trips and the chunks per scan thread step exactly past a full grid / block
    assert [topk_ref.hist_trips(n * C) for n in (1, H, H + 1, 2 * H, 2 * H + 1)] == [1, 1, 2, 2, 3]
    assert [topk_ref.hist_trips(H * C + d) for d in (0, 4)] == [1, 2]
    assert [topk_ref.scan_per(n * C) for n in (1, S, S + 1, 2 * S, 2 * S + 1)] == [1, 1, 2, 2, 3]
    assert [topk_ref.scan_per(S * C + d) for d in (0, 4)] == [1, 2]


def test_scale_shapes_reach_the_paths_they_are_named_for():
    """A change to a launch cap fails here, not by silently un-testing the GPU path."""
    from distributed_learning_simulator_amd import _native
    C, H, S = _native.TOPK_CHUNK, _native.TOPK_HIST_BLOCKS, _native.TOPK_SCAN_BLOCK
    R = topk_ref
    # P_SCAN2: two chunks per scan thread, the upper threads own nothing, one ragged vector
    assert R.scan_per(R.P_SCAN2) == 2 and R.scan_per(R.P_SCAN2 - 2 * C) == 1
    assert R.nchunks(R.P_SCAN2) < 2 * (S - 1) and R.P_SCAN2 % C == 4
    # P_STRIDE: a second histogram trip that holds the ragged chunk; three chunks per scan thread
    assert R.hist_trips(R.P_STRIDE) == 2 and R.hist_trips(R.P_STRIDE - 2 * C) == 1
    assert R.nchunks(R.P_STRIDE) == H + 2 and 0 < R.P_STRIDE % C < C
    assert R.scan_per(R.P_STRIDE) >= 3
    assert R.hist_trips(R.P_RESNET) >= 2 and R.scan_per(R.P_RESNET) >= 3
    assert R.nchunks(R.P_RESNET) == 2729 and R.nchunks(R.P_RESNET) - H == 681
    for P in (R.P_SCAN2, R.P_STRIDE, R.P_RESNET):
        assert P % 4 == 0 and P <= _native.TOPK_MAX_P
