"""fed_secagg without a GPU: the stream-id algebra, the numpy reference against closed forms,
FedSecAggWorker / FedSecAggServer on CPU stand-ins built on that reference, validation, the
simulator's flags, and the library's and the wrappers' argument checks."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import dp_ref, secagg_ref

F32, U32 = np.float32, np.uint32
CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ stream ids
def test_stream_id_packing_and_ranges():
    from distributed_learning_simulator_amd.aggregation import secagg_stream_id as sid
    assert sid(0, 0, 0) == 0 and sid(1, 2, 3) == (1 << 32) | (2 << 16) | 3
    assert sid((1 << 32) - 1, 65535, 65535) == (1 << 64) - 1
    assert sid(7, 5, 5) != sid(7, 5, 6) != sid(8, 5, 6)
    for bad in ((-1, 0, 0), (1 << 32, 0, 0), (0, -1, 0), (0, 0, 65536), (0, 70000, 70001),
                (0, 1.0, 2), (True, 0, 0), (0, None, 1)):
        with pytest.raises(ValueError, match="must be an integer in"):
            sid(*bad)
    with pytest.raises(ValueError, match="must not exceed"):
        sid(0, 3, 2)


def _signed(add, sub):
    """stream id -> its net count over (add, sub) lists."""
    net = {}
    for t in add:
        net[t] = net.get(t, 0) + 1
    for t in sub:
        net[t] = net.get(t, 0) - 1
    return {t: c for t, c in net.items() if c}


def test_stream_lists_cancel_for_every_split_of_five_workers():
    from distributed_learning_simulator_amd.aggregation import (secagg_client_streams,
                                                                secagg_server_streams)
    ids = [0, 3, 4, 9, 65535]
    for r in (1, 2):
        for mask in range(1, 1 << 5):  # every non-empty survivor set
            alive = [w for i, w in enumerate(ids) if mask >> i & 1]
            gone = [w for w in ids if w not in alive]
            for order in (alive, alive[::-1], alive[1:] + alive[:1]):  # arrival orders
                add, sub = [], []
                for w in order:
                    a, s = secagg_client_streams(w, ids[::-1], r)
                    add, sub = add + a, sub + s
                sa, ss = secagg_server_streams(order, gone, r)
                assert _signed(add + sa, sub + ss) == {}, (alive, gone)
                assert len(sa) + len(ss) == len(alive) + len(alive) * len(gone)
    a, s = secagg_client_streams(3, ids, 1)
    assert len(a) == 1 + 3 and len(s) == 1 and len(set(a + s)) == 5
    assert secagg_server_streams([2, 1], [], 4) == ([], [(4 << 32) | (1 << 16) | 1,
                                                         (4 << 32) | (2 << 16) | 2])
    with pytest.raises(ValueError, match="not among the participants"):
        secagg_client_streams(5, ids, 1)
    with pytest.raises(ValueError, match="distinct"):
        secagg_client_streams(3, [3, 3, 4], 1)
    with pytest.raises(ValueError, match="both survive and drop"):
        secagg_server_streams([1, 2], [2], 1)
    with pytest.raises(ValueError, match="worker ids in"):
        secagg_server_streams([1, 70000], [], 1)


def test_capacity():
    from distributed_learning_simulator_amd.aggregation import secagg_check_capacity as cap
    assert cap(20, [1] * 64) == 64 and cap(31, [1]) == 1 and cap(2, [1 << 30]) == 1 << 30
    assert cap(20, [1] * 4096) == 4096  # (2^19 - 1) * 2^12 < 2^31
    with pytest.raises(ValueError, match="largest secagg_bits that fits is 19"):
        cap(20, [1] * 4097)
    with pytest.raises(ValueError, match="largest secagg_bits that fits is 18"):
        cap(20, [1000] * 10)  # (2^17 - 1) * 10^4 < 2^31 <= (2^18 - 1) * 10^4
    with pytest.raises(ValueError, match="largest secagg_bits that fits is 30"):
        cap(31, [1, 1, 1])
    assert cap(31, [1, 1]) == 2  # 2 * (2^30 - 1) < 2^31
    with pytest.raises(ValueError, match="no secagg_bits fits"):
        cap(2, [1 << 31])
    for bad in (1, 32, 20.0, True):
        with pytest.raises(ValueError, match="secagg_bits must be"):
            cap(bad, [1])
    for bad in ([], [0], [1.0], [True], [1 << 32]):
        with pytest.raises(ValueError, match="weights must be"):
            cap(20, bad)


# ------------------------------------------------------------------ the reference
def test_reference_words_are_dp_refs():
    for P, seed, sid in ((4, 0, 0), (13, 7, (3 << 32) | (1 << 16) | 2), (260, (1 << 64) - 1, (1 << 64) - 1)):
        assert np.array_equal(secagg_ref.words(P, seed, sid), dp_ref.words(P, seed, sid))


def test_reference_encode_hand_written():
    f, b = 4, 6  # steps of 1/16, L = 31
    L = 31
    d = np.array([0.0, -0.0, 0.5 / 16, 1.5 / 16, 2.5 / 16, -0.5 / 16, -1.5 / 16, L / 16,
                  -L / 16, (L + 1) / 16, -(L + 1) / 16, (L + 0.5) / 16, (L + 0.49) / 16, 1e30,
                  np.inf, -np.inf, np.nan, 1e-45, 0.3], F32)
    q, sat, bad = secagg_ref.quantise(d, np.zeros_like(d), f, b)
    assert q.tolist() == [0, 0, 0, 2, 2, 0, -2, L, -L, L, -L, L, L, L, 0, 0, 0, 0, 5]
    assert sat.tolist() == [False] * 9 + [True, True, True, False, True] + [False] * 5
    assert bad.tolist() == [False] * 14 + [True] * 3 + [False] * 2
    e, n_sat, n_bad = secagg_ref.encode(d, np.zeros_like(d), f, b, 3)
    assert (n_sat, n_bad) == (4, 3) and e[3] == 6 and e[6] == U32((1 << 32) - 6)
    # a weight that wraps the sign bit: 31 * 2^27 = 0xF8000000, -31 * 2^27 = 0x08000000
    e, _, _ = secagg_ref.encode(d, np.zeros_like(d), f, b, 1 << 27)
    assert e[7] == 0xF8000000 and e[8] == 0x08000000
    # the product overflows fp32: saturated, not non-finite
    q, sat, bad = secagg_ref.quantise(np.array([3e38, -3e38], F32), np.zeros(2, F32), 126, 31)
    assert q.tolist() == [(1 << 30) - 1, -(1 << 30) + 1] and sat.all() and not bad.any()


def test_reference_decode_hand_written():
    base = np.array([1.0, -0.0, 0.0, 2.0], F32)
    S = np.array([3, 0, 0xFFFFFFFF, 0x80000000], U32)
    out = secagg_ref.decode(S, base, 1, 3.0).view(F32)
    assert out[0] == F32(1.5) and out[1] == 0.0 and out[3] == F32(2.0 - 2.0 ** 30 / 3.0)
    assert out[2] == F32(np.float64(-0.5) / 3.0) and np.signbit(out[1]) == np.signbit(F32(0.0))
    # a tie after the cast: (2^24 + 1) is halfway between two floats and rounds to even
    S = np.array([3 * ((1 << 24) + 1), 3 * ((1 << 24) + 3)], U32)
    out = secagg_ref.decode(S, np.zeros(2, F32), 0, 3.0).view(F32)
    assert out.tolist() == [float(1 << 24), float((1 << 24) + 4)]


def test_reference_mask_and_unmask_cancel():
    from distributed_learning_simulator_amd.aggregation import (secagg_client_streams,
                                                                secagg_server_streams)
    rng = np.random.default_rng(0)
    P, ids, seed, f, b = 24, [0, 1, 2, 5], 99, 10, 16
    base = rng.standard_normal(P).astype(F32)
    W = base + (rng.standard_normal((4, P)) * 0.1).astype(F32)
    ws = [3, 1, 2, 5]
    Y = np.stack([secagg_ref.mask(W[i], base, f, b, ws[i], *secagg_client_streams(w, ids, 7), seed)[0]
                  for i, w in enumerate(ids)])
    E = np.stack([secagg_ref.encode(W[i], base, f, b, ws[i])[0] for i in range(4)])
    assert not np.array_equal(Y, E)
    for rows in ([0, 1, 2, 3], [3, 1, 0], [2]):
        alive = [ids[r] for r in rows]
        gone = [w for w in ids if w not in alive]
        total = sum(ws[r] for r in rows)
        out, S = secagg_ref.unmask(Y, rows, *secagg_server_streams(alive, gone, 7), seed, base, f,
                                   total, P)
        assert np.array_equal(S, secagg_ref.ring_sum(E[rows]))
        assert np.array_equal(out, secagg_ref.decode(S, base, f, total))
        if gone:  # without the recovery streams the sum is still masked
            _, S2 = secagg_ref.unmask(Y, rows, *secagg_server_streams(alive, [], 7), seed, base, f,
                                      total, P)
            assert not np.array_equal(S2, S)


# ------------------------------------------------------- worker and server, CPU stand-ins
class FakeTrainer:
    """What FedSecAggWorker touches of a trainer; the test plays the training."""

    def __init__(self, model, samples):
        self.model = model
        self.dataset = (torch.zeros(samples, 1), torch.zeros(samples))
        self.callbacks = {}

    def add_named_callback(self, point, name, fn):
        self.callbacks[name] = fn

    def set_device(self, device):
        pass


def make_model(seed=0):
    torch.manual_seed(seed)
    return torch.nn.Linear(5, 3)  # weight [3, 5], bias [3]: 18 real parameters, P = 128


def initial_model():
    return {k: v.detach().clone() for k, v in make_model().named_parameters()}


def flat_of(layout, d):
    return layout.flatten(d, device=CPU).numpy()


NS = {0: 300, 1: 120, 2: 777, 3: 64}


def make_server(monkeypatch, server_cls=None, **kwargs):
    from distributed_learning_simulator_amd.servers.fed_secagg_server import FedSecAggServer
    secagg_ref.install(monkeypatch)
    kwargs.setdefault("worker_number", 4)
    return (server_cls or FedSecAggServer)(initial_model=initial_model(), tester=None,
                                           synchronous=True, device=CPU, **kwargs)


def make_run(monkeypatch, weighted=False, server_cls=None, **kwargs):
    from distributed_learning_simulator_amd.workers.fed_secagg_worker import FedSecAggWorker
    server = make_server(monkeypatch, server_cls, **kwargs)
    fmt = {k: kwargs[k] for k in ("secagg_bits", "secagg_frac_bits", "secagg_seed") if k in kwargs}
    workers = {i: FedSecAggWorker(worker_id=i, trainer=FakeTrainer(make_model(10 + i), NS[i]),
                                  worker_data_queue=server.worker_data_queue, round=3,
                                  participants=range(4), secagg_weighted=weighted, **fmt)
               for i in range(4)}
    for i, w in workers.items():
        assert "send_parameter" in w.trainer.callbacks
        w.load_model(server.worker_data_queue.get_result(consumer=i))
        assert w.layout.P == 128
    return server, workers


def train(worker, rng, scale=0.05):
    with torch.no_grad():
        for p in worker.trainer.model.parameters():
            p += torch.from_numpy((rng.standard_normal(tuple(p.shape)) * scale).astype(F32))


def play_round(server, workers, order, rng, weighted):
    """One round: returns (the fp64 weighted mean of the survivors' d, delta, saturated)."""
    lay = server.layout
    prev = flat_of(lay, server.prev_model)
    f, b = server.secagg_frac_bits, server.secagg_bits
    alive = [w for w in order if w not in server.secagg_dropouts]
    E, D, wts, sat = {}, {}, {}, 0
    for wid in order:
        train(workers[wid], rng)
        w = flat_of(lay, dict(workers[wid].trainer.model.named_parameters()))
        wts[wid] = NS[wid] if weighted else 1
        E[wid], n_sat, _ = secagg_ref.encode(w, prev, f, b, wts[wid])
        D[wid] = (w - prev).astype(np.float64)
        p = workers[wid].masked_update(NS[wid])
        assert p.saturated == n_sat and p.weight == wts[wid] and p.round == server.round + 1
        assert not np.array_equal(p.y.numpy().view(U32), E[wid])  # it is masked
        sat += n_sat if wid in alive else 0
        server.worker_data_queue.add_task((wid, NS[wid], p))
    models = {wid: server.worker_data_queue.get_result(consumer=wid) for wid in order}
    total = sum(wts[w] for w in alive)
    ref = secagg_ref.decode(secagg_ref.ring_sum(np.stack([E[w] for w in alive])), prev, f, total)
    for wid in order:
        assert np.array_equal(flat_of(lay, models[wid]).view(U32), ref)
        workers[wid].load_model(models[wid])
    assert np.array_equal(flat_of(lay, server.prev_model).view(U32), ref)
    assert server.last_secagg == {"round": server.round, "survivors": tuple(sorted(alive)),
                                  "dropped": server.secagg_dropouts, "total": total,
                                  "saturated": sat, "streams_removed":
                                  len(alive) * (1 + len(server.secagg_dropouts))}
    mean = sum(wts[w] * D[w] for w in alive) / total
    # what the server added to prev, recovered exactly: the decode of the same integer sum on a zero base
    delta = secagg_ref.decode(secagg_ref.ring_sum(np.stack([E[w] for w in alive])),
                              np.zeros_like(prev), f, total).view(F32).astype(np.float64)
    return mean, delta, sat


@pytest.mark.parametrize("weighted", [False, True])
def test_three_rounds_four_workers_one_dropout(monkeypatch, weighted):
    """The server's model equals the reference from the quantised updates bit for bit, and its
    step lies within the derived bound of the fp64 mean of the clients' d_i.

    The bound.  With nothing saturated, q_k = rint(d_k 2^f) where d_k 2^f is exact in fp32 (a
    power-of-two scaling in the normal range), so |q_k 2^-f - d_k| <= 2^-(f+1).  The integer
    sum is exact, so x = sum w_k q_k 2^-f / total is a convex combination of the q_k 2^-f and
    |x - mean| <= 2^-(f+1).  delta = fl32(fl64(x)): the cast moves it by at most half an ulp
    of the result, 2^-24 |delta|; the fp64 quotient's 2^-53 |x| is 2^29 times smaller than
    that and is covered by the slack of the first term away from exact ties (the data here
    is random: no d_k 2^f sits at a tie).  Hence |delta - mean| <= 2^-(f+1) + 2^-24 |delta|."""
    bits = 12 if weighted else 20  # (2^11 - 1) * (300 + 120 + 777) < 2^31
    f = 8 if weighted else 16
    server, workers = make_run(monkeypatch, weighted, secagg_dropouts=(3,), secagg_seed=1234,
                               secagg_bits=bits, secagg_frac_bits=f)
    rng = np.random.default_rng(5)
    for order in ([2, 0, 3, 1], [3, 1, 0, 2], [0, 1, 2, 3]):
        mean, delta, sat = play_round(server, workers, order, rng, weighted)
        assert sat == 0
        assert np.all(np.abs(delta - mean) <= 2.0 ** -(f + 1) + 2.0 ** -24 * np.abs(delta))
        assert np.abs(delta).max() > 2.0 ** -f  # the step is not all zeros
    assert server.round == 3 and all(w.sent_rounds == 3 for w in workers.values())


def test_arrival_order_changes_no_bit(monkeypatch):
    """Weighted, with a dropout: the same trained models, sent in three orders."""
    finals = []
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [2, 0, 3, 1]):
        server, workers = make_run(monkeypatch, True, secagg_bits=12, secagg_frac_bits=8,
                                   secagg_dropouts=(1,))
        start = flat_of(server.layout, server.prev_model).copy()
        rng = np.random.default_rng(3)
        payloads = {}
        for wid in range(4):  # the same draws per worker in every run
            train(workers[wid], rng)
            payloads[wid] = workers[wid].masked_update(NS[wid])
        for wid in order:
            server.worker_data_queue.add_task((wid, NS[wid], payloads[wid]))
        assert server.round == 1
        finals.append(flat_of(server.layout, server.prev_model).copy())
    assert np.array_equal(finals[0].view(U32), finals[1].view(U32))
    assert np.array_equal(finals[0].view(U32), finals[2].view(U32))
    assert not np.array_equal(finals[0], start)  # the round did move the model


def test_get_subset_model(monkeypatch):
    from distributed_learning_simulator_amd.servers.fed_secagg_server import FedSecAggServer
    seen = {}

    class Recording(FedSecAggServer):
        def _process_aggregated_parameter(self, aggregated):
            seen["all"] = self.get_subset_model([2, 0, 1])
            seen["empty"] = self.get_subset_model([])
            for subset in ([0, 1], [0, 1, 2, 3], [0], [0, 1, 2, 2], [0, 1, 9]):
                with pytest.raises(ValueError, match="exists to prevent"):
                    self.get_subset_model(subset)
            return aggregated

    server, workers = make_run(monkeypatch, server_cls=Recording, secagg_dropouts=(3,))
    prev = flat_of(server.layout, server.prev_model).copy()
    with pytest.raises(ValueError, match="exists to prevent"):
        server.get_subset_model([0, 1, 2])  # no round yet
    assert server.get_subset_model([]) is server.prev_model
    play_round(server, workers, [1, 3, 0, 2], np.random.default_rng(1), False)
    assert np.array_equal(flat_of(server.layout, seen["empty"]).view(U32), prev.view(U32))
    assert np.array_equal(flat_of(server.layout, seen["all"]).view(U32),
                          flat_of(server.layout, server.prev_model).view(U32))


# ------------------------------------------------------------------ validation
def test_threshold_and_dropouts(monkeypatch):
    server = make_server(monkeypatch, worker_number=5)
    assert server.secagg_threshold == 3 and server.secagg_dropouts == ()
    assert make_server(monkeypatch, worker_number=5, secagg_dropouts=[4, 1]).secagg_dropouts == (1, 4)
    with pytest.raises(ValueError, match="fewer than secagg_threshold=3"):
        make_server(monkeypatch, worker_number=5, secagg_dropouts=(0, 1, 2))
    make_server(monkeypatch, worker_number=5, secagg_dropouts=(0, 1, 2), secagg_threshold=2)
    with pytest.raises(ValueError, match="fewer than secagg_threshold=5"):
        make_server(monkeypatch, worker_number=5, secagg_dropouts=(0,), secagg_threshold=5)
    for bad in (0, 6, 2.0, True):
        with pytest.raises(ValueError, match="secagg_threshold must be"):
            make_server(monkeypatch, worker_number=5, secagg_threshold=bad)
    for bad, match in (((5,), "worker ids in 0..worker_number - 1"), ((1, 1), "distinct"),
                       ((-1,), "non-negative"), ((1.0,), "non-negative"), (3, "collection")):
        with pytest.raises(ValueError, match=match):
            make_server(monkeypatch, worker_number=5, secagg_dropouts=bad)
    with pytest.raises(ValueError, match="ROBUST_MAX_K=64"):
        make_server(monkeypatch, worker_number=65)
    for kw in ({"secagg_bits": 1}, {"secagg_bits": 32}, {"secagg_frac_bits": 127},
               {"secagg_frac_bits": -1}, {"secagg_seed": 1 << 64}, {"secagg_seed": -1}):
        with pytest.raises(ValueError, match=next(iter(kw))):
            make_server(monkeypatch, **kw)


def test_the_four_refusals_and_the_model_it_needs(monkeypatch):
    from distributed_learning_simulator_amd.servers.fed_secagg_server import FedSecAggServer
    secagg_ref.install(monkeypatch)
    with pytest.raises(ValueError, match="tester or initial_model"):
        FedSecAggServer(tester=None, worker_number=3, synchronous=True, device=CPU)
    reason = "it never holds an individual update"
    for extra in ({"aggregation_rule": "median"}, {"attack": "alie", "attackers": (0,)},
                  {"server_optimizer": "adam"}, {"dp_clip": 1.0}):
        with pytest.raises(ValueError) as err:
            make_server(monkeypatch, **extra)
        assert "FedSecAggServer does not support" in str(err.value) and reason in str(err.value)
    with pytest.raises(ValueError, match="aggregation_mode") as err:
        make_server(monkeypatch, aggregation_mode="fma")
    assert reason in str(err.value)


def test_server_rejects_payloads(monkeypatch):
    from distributed_learning_simulator_amd.workers.fed_secagg_worker import MaskedUpdate
    server, workers = make_run(monkeypatch)
    P = server.layout.P

    def send(wid=0, n=10, **kw):
        a = dict(y=torch.zeros(P, dtype=torch.int32), P=P, round=1, frac_bits=16, bits=20, weight=1,
                 saturated=0)
        a.update(kw)
        server.worker_data_queue.add_task((wid, n, MaskedUpdate(**a)))

    with pytest.raises(ValueError, match="must be a MaskedUpdate"):
        server.worker_data_queue.add_task((0, 10, {"weight": torch.zeros(3, 5)}))
    with pytest.raises(ValueError, match="P=64"):
        send(P=64)
    with pytest.raises(ValueError, match="masked for round 2"):
        send(round=2)
    with pytest.raises(ValueError, match="format"):
        send(bits=19)
    with pytest.raises(ValueError, match="format"):
        send(frac_bits=15)
    with pytest.raises(ValueError, match="neither 1 nor the reported sample count 10"):
        send(weight=11)
    with pytest.raises(ValueError, match="y must be an int32 vector"):
        send(y=torch.zeros(P))
    with pytest.raises(ValueError, match="y must be an int32 vector"):
        send(y=torch.zeros(P - 4, dtype=torch.int32))
    with pytest.raises(ValueError, match="not a worker id"):
        send(wid=4)
    assert not server._arrived and server.round == 0
    send(wid=0)
    with pytest.raises(ValueError, match="a second payload"):
        send(wid=0)
    # weights that are neither all 1 nor all the sample counts
    send(wid=1, n=10, weight=10)
    send(wid=2, n=10, weight=1)
    with pytest.raises(ValueError, match="neither all 1 nor all the reported sample counts"):
        send(wid=3, n=10, weight=10)
    assert not server._arrived
    # capacity: four workers of weight 2^11 at 20 bits
    for wid in range(3):
        send(wid=wid, n=1 << 11, weight=1 << 11, round=2)
    with pytest.raises(ValueError, match="largest secagg_bits that fits is 19"):
        send(wid=3, n=1 << 11, weight=1 << 11, round=2)


def test_worker_validation_and_nonfinite_update(monkeypatch):
    from distributed_learning_simulator_amd.workers.fed_secagg_worker import FedSecAggWorker

    def worker(**kw):
        a = dict(worker_id=0, trainer=FakeTrainer(make_model(), 10), worker_data_queue=None, round=1,
                 participants=(0, 1))
        a.update(kw)
        return FedSecAggWorker(**a)

    for kw, match in (({"secagg_bits": 32}, "secagg_bits"), ({"secagg_frac_bits": 127}, "secagg_frac_bits"),
                      ({"secagg_seed": -1}, "secagg_seed"), ({"participants": (1, 2)}, "not among"),
                      ({"participants": (0, 0, 1)}, "distinct"),
                      ({"participants": range(65)}, "ROBUST_MAX_K=64")):
        with pytest.raises(ValueError, match=match):
            worker(**kw)
    with pytest.raises(RuntimeError, match="no model loaded"):
        worker().masked_update(10)
    _, workers = make_run(monkeypatch)
    with torch.no_grad():
        w = dict(workers[1].trainer.model.named_parameters())["weight"].view(-1)
        w[3], w[4] = float("inf"), float("nan")
    with pytest.raises(ValueError, match=r"worker 1: 2 coordinates"):
        workers[1].masked_update(10)
    assert workers[1].sent_rounds == 0
    # a saturated update is sent, and counted
    with torch.no_grad():
        w[3], w[4] = 100.0, 0.0
    assert workers[1].masked_update(10).saturated == 1


def test_factory_names(monkeypatch):
    from distributed_learning_simulator_amd import distributed, factory
    from distributed_learning_simulator_amd.servers.fed_secagg_server import FedSecAggServer
    from distributed_learning_simulator_amd.workers.fed_secagg_worker import FedSecAggWorker
    secagg_ref.install(monkeypatch)
    server = factory.get_server("fed_secagg", sharded=False, initial_model=initial_model(),
                                tester=None, worker_number=2, synchronous=True, device=CPU,
                                secagg_dropouts=(), secagg_threshold=None)
    assert type(server) is FedSecAggServer and server.secagg_threshold == 2
    worker = factory.get_worker("fed_secagg", worker_id=1, trainer=FakeTrainer(make_model(), 4),
                                worker_data_queue=server.worker_data_queue, round=1,
                                participants=(0, 1), secagg_bits=10, secagg_weighted=True)
    assert type(worker) is FedSecAggWorker and worker.secagg_bits == 10 and worker.secagg_weighted
    with pytest.raises(RuntimeError, match="one-process server only"):
        distributed.get_sharded_server("fed_secagg", tester=None, worker_number=2)
    with pytest.raises(RuntimeError, match="one-process server only"):
        factory.get_server("fed_secagg", sharded=True, tester=None, worker_number=2)


# ------------------------------------------------------------------ simulator flags
BASE = ["--worker_number", "4", "--round", "2"]


def test_simulator_flags():
    from distributed_learning_simulator_amd import simulator
    cfg = simulator.get_config(["--distributed_algorithm", "fed_secagg"] + BASE)
    assert simulator.worker_kwargs(cfg) == {"secagg_bits": 20, "secagg_frac_bits": 16,
                                            "secagg_seed": 0, "secagg_weighted": False,
                                            "participants": (0, 1, 2, 3)}
    assert simulator.server_kwargs(cfg) == {"aggregation_mode": "exact", "secagg_bits": 20,
                                            "secagg_frac_bits": 16, "secagg_seed": 0,
                                            "secagg_threshold": None, "secagg_dropouts": ()}
    cfg = simulator.get_config(["--distributed_algorithm", "fed_secagg", "--secagg_bits", "12",
                                "--secagg_frac_bits", "8", "--secagg_seed", "77",
                                "--secagg_weighted", "1", "--secagg_dropouts", "3,1",
                                "--secagg_threshold", "2"] + BASE)
    assert simulator.worker_kwargs(cfg) == {"secagg_bits": 12, "secagg_frac_bits": 8,
                                            "secagg_seed": 77, "secagg_weighted": True,
                                            "participants": (0, 1, 2, 3)}
    assert simulator.server_kwargs(cfg) == {"aggregation_mode": "exact", "secagg_bits": 12,
                                            "secagg_frac_bits": 8, "secagg_seed": 77,
                                            "secagg_threshold": 2, "secagg_dropouts": (3, 1)}
    for flag in (["--secagg_bits", "12"], ["--secagg_frac_bits", "8"], ["--secagg_seed", "0"],
                 ["--secagg_weighted", "0"], ["--secagg_dropouts", "1"], ["--secagg_threshold", "2"]):
        for algo in ("fed", "fed_topk", "fed_quant", "sign_SGD", "GTG_shapley_value"):
            with pytest.raises(SystemExit):
                simulator.get_config(["--distributed_algorithm", algo] + flag + BASE)
    for flag in (["--secagg_weighted", "2"], ["--secagg_dropouts", "a"], ["--dp_clip", "1.0"],
                 ["--topk_ratio", "0.1"]):
        with pytest.raises(SystemExit):
            simulator.get_config(["--distributed_algorithm", "fed_secagg"] + flag + BASE)
    assert "--distributed_algorithm fed_secagg" in simulator.__doc__
    with open(os.path.join(ROOT, "README.md")) as fh:
        assert "--secagg_dropouts" in fh.read()
    # the other algorithms' keyword arguments did not move
    for algo in ("fed", "fed_topk", "fed_quant"):
        cfg = simulator.get_config(["--distributed_algorithm", algo] + BASE)
        assert simulator.server_kwargs(cfg) == {"aggregation_mode": "exact"}, algo


# ------------------------------------------------------- the library without a GPU
def _ptrs(n, start=1 << 20, step=1 << 16):
    """Never-dereferenced, 16-byte aligned, far apart: validation comes before any access."""
    return [ctypes.c_void_p(start + i * step) for i in range(n)]


def mask_call(L, **kw):
    w, base, add, sub, y, stats = _ptrs(6)
    a = dict(w=w, base=base, P=64, frac_bits=16, bits=20, weight=1, add=add, n_add=2, sub=sub,
             n_sub=1, seed=0, y=y, stats=stats)
    a.update(kw)
    rc = L.dls_secagg_mask_f32(a["w"], a["base"], a["P"], a["frac_bits"], a["bits"], a["weight"],
                               a["add"], a["n_add"], a["sub"], a["n_sub"], a["seed"], a["y"],
                               a["stats"], None)
    return rc, L.dls_last_error()


def unmask_call(L, **kw):
    Y, rows, add, sub, base, out, sum_out = _ptrs(7)
    a = dict(Y=Y, ldy=64, rows=rows, K=3, add=add, n_add=0, sub=sub, n_sub=3, seed=0, base=base,
             frac_bits=16, total=3.0, P=64, out=out, sum_out=sum_out)
    a.update(kw)
    rc = L.dls_secagg_unmask_f32(a["Y"], a["ldy"], a["rows"], a["K"], a["add"], a["n_add"], a["sub"],
                                 a["n_sub"], a["seed"], a["base"], a["frac_bits"], a["total"],
                                 a["P"], a["out"], a["sum_out"], None)
    return rc, L.dls_last_error()


# (keyword arguments, status, what the message holds): every bound of the two entry points
MASK_ERRORS = [(dict(w=None), -1, b"null pointer"), (dict(base=None), -1, b"null pointer"),
               (dict(y=None), -1, b"null pointer"), (dict(stats=None), -1, b"null pointer"),
               (dict(add=None), -1, b"null stream table"), (dict(sub=None), -1, b"null stream table"),
               (dict(bits=1), -1, b"bits=1 (2..31)"), (dict(bits=32), -1, b"bits=32 (2..31)"),
               (dict(weight=0), -1, b"weight=0"), (dict(frac_bits=-1), -1, b"frac_bits=-1 (0..126)"),
               (dict(frac_bits=127), -1, b"frac_bits=127"), (dict(n_add=-1), -1, b"n_add=-1"),
               (dict(n_sub=-1), -1, b"n_sub=-1"),
               (dict(n_add=1088, n_sub=1), -1, b"DLS_SECAGG_MAX_STREAMS=1088"),
               (dict(P=-4), -1, b"P=-4"), (dict(P=62), -2, b"multiples of 4"),
               (dict(w=ctypes.c_void_p((1 << 24) + 4)), -2, b"alignment"),
               (dict(base=ctypes.c_void_p((1 << 24) + 8)), -2, b"alignment"),
               (dict(y=ctypes.c_void_p((1 << 24) + 4)), -2, b"alignment"),
               (dict(stats=ctypes.c_void_p((1 << 24) + 2)), -2, b"alignment"),
               (dict(add=ctypes.c_void_p((1 << 24) + 4)), -2, b"8-byte (stream tables)"),
               (dict(sub=ctypes.c_void_p((1 << 24) + 4)), -2, b"8-byte (stream tables)")]
UNMASK_ERRORS = [(dict(Y=None), -1, b"null pointer"), (dict(rows=None), -1, b"null pointer"),
                 (dict(base=None), -1, b"null pointer"), (dict(out=None), -1, b"null pointer"),
                 (dict(sub=None), -1, b"null stream table"),
                 (dict(add=None, n_add=1), -1, b"null stream table"),
                 (dict(K=0), -1, b"K=0 (1..DLS_ROBUST_MAX_K=64)"), (dict(K=65), -1, b"K=65"),
                 (dict(frac_bits=-1), -1, b"frac_bits=-1"), (dict(frac_bits=127), -1, b"frac_bits=127"),
                 (dict(n_add=-1), -1, b"n_add=-1"), (dict(n_add=1086), -1, b"DLS_SECAGG_MAX_STREAMS"),
                 (dict(total=0.5), -1, b"total=0.5"), (dict(total=float("inf")), -1, b"total=inf"),
                 (dict(total=float("nan")), -1, b"total="), (dict(P=-4), -1, b"P=-4"),
                 (dict(P=62), -2, b"multiples of 4"), (dict(ldy=62), -2, b"multiples of 4"),
                 (dict(ldy=60, P=64), -2, b"ldu >= P"),
                 (dict(Y=ctypes.c_void_p((1 << 24) + 4)), -2, b"alignment"),
                 (dict(base=ctypes.c_void_p((1 << 24) + 4)), -2, b"alignment"),
                 (dict(out=ctypes.c_void_p((1 << 24) + 8)), -2, b"alignment"),
                 (dict(sum_out=ctypes.c_void_p((1 << 24) + 4)), -2, b"alignment"),
                 (dict(rows=ctypes.c_void_p((1 << 24) + 2)), -2, b"alignment"),
                 (dict(sub=ctypes.c_void_p((1 << 24) + 4)), -2, b"8-byte (stream tables)")]


def test_entry_points_reject_bad_arguments_without_gpu():
    from distributed_learning_simulator_amd import _native
    L = _native.lib()
    for kw, status, text in MASK_ERRORS:
        rc, msg = mask_call(L, **kw)
        assert rc == status and text in msg and b"dls_secagg_mask_f32" in msg, (kw, rc, msg)
    for kw, status, text in UNMASK_ERRORS:
        rc, msg = unmask_call(L, **kw)
        assert rc == status and text in msg and b"dls_secagg_unmask_f32" in msg, (kw, rc, msg)
    # P == 0 launches nothing; an empty table may be null; sum_out may be null
    assert mask_call(L, P=0)[0] == 0 and mask_call(L, P=0, add=None, n_add=0)[0] == 0
    assert unmask_call(L, P=0, sum_out=None, add=None)[0] == 0
    assert unmask_call(L, P=0, n_add=64, n_sub=1024)[0] == 0  # DLS_SECAGG_MAX_STREAMS itself


def test_wrappers_validate_operands_without_gpu():
    from distributed_learning_simulator_amd import _native
    assert _native.SECAGG_MAX_STREAMS == 1088
    P = 64

    def mops():
        return dict(w=torch.zeros(P), base=torch.zeros(P), P=P, frac_bits=16, bits=20, weight=1,
                    add_streams=torch.zeros(2, dtype=torch.int64), sub_streams=None, seed=0,
                    y=torch.zeros(P, dtype=torch.int32), stats=torch.zeros(2, dtype=torch.int32))

    def mask(match, **kw):
        a = mops()
        a.update(kw)
        with pytest.raises(RuntimeError, match=match):
            _native.secagg_mask(**a)

    mask("not on the GPU")  # every check passes
    mask("not on the GPU", add_streams=None, sub_streams=torch.zeros(0, dtype=torch.int64))
    for name in ("w", "base"):
        for bad in (torch.zeros(P, dtype=torch.float64), torch.zeros(P - 4), torch.zeros(2 * P)[::2]):
            mask(name + " must be", **{name: bad})
        mask(" on meta", **{name: torch.zeros(P, device="meta")} if name != "w"
             else {"base": torch.zeros(P, device="meta")})
    mask("must be 16-byte aligned", w=torch.zeros(P + 4)[1:P + 1])
    mask("y must be", y=torch.zeros(P))
    mask("y must be", y=torch.zeros(P - 4, dtype=torch.int32))
    mask("stats must be", stats=torch.zeros(3, dtype=torch.int32))
    mask("add_streams must be", add_streams=torch.zeros(2, dtype=torch.int32))
    mask("sub_streams must be", sub_streams=torch.zeros(2, 2, dtype=torch.int64))
    mask("SECAGG_MAX_STREAMS", add_streams=torch.zeros(1088, dtype=torch.int64),
         sub_streams=torch.zeros(1, dtype=torch.int64))
    for name, bads in (("bits", (1, 32, 20.0, True)), ("frac_bits", (-1, 127, 1.0)),
                       ("weight", (0, 1 << 32, 1.0)), ("seed", (-1, 1 << 64, 0.5))):
        for bad in bads:
            mask(name + "=", **{name: bad})
    for bad_p in (62, -4):
        mask("P=", P=bad_p)
    both = torch.zeros(2 * P)
    mask("y and w overlap", w=both[:P], y=both.view(torch.int32)[P - 4:2 * P - 4])

    K = 3

    def uops():
        return dict(Y=torch.zeros(K, P, dtype=torch.int32), rows=torch.arange(K, dtype=torch.int32),
                    add_streams=None, sub_streams=torch.zeros(K, dtype=torch.int64), seed=0,
                    base=torch.zeros(P), frac_bits=16, total=3.0, P=P, out=torch.zeros(P),
                    sum_out=torch.zeros(P, dtype=torch.int32))

    def unmask(match, **kw):
        a = uops()
        a.update(kw)
        with pytest.raises(RuntimeError, match=match):
            _native.secagg_unmask(**a)

    unmask("not on the GPU")
    unmask("not on the GPU", sum_out=None)
    unmask("Y must be an int32", Y=torch.zeros(K, P))
    unmask("Y must be an int32", Y=torch.zeros(P, dtype=torch.int32))
    unmask("rows must be", rows=torch.arange(K))
    unmask("K=0 rows", rows=torch.zeros(0, dtype=torch.int32))
    unmask("K=65 rows", rows=torch.zeros(65, dtype=torch.int32))
    unmask("P=", P=P + 4)
    unmask("P=", P=62)
    unmask("row pitch", Y=torch.zeros(K, P + 2, dtype=torch.int32), P=P)
    unmask("base must be", base=torch.zeros(P - 4))
    unmask("out must be", out=torch.zeros(P, dtype=torch.float64))
    unmask("sum_out must be", sum_out=torch.zeros(P))
    unmask("frac_bits=", frac_bits=127)
    for bad in (0.5, float("inf"), float("nan"), "3", True):
        unmask("total=", total=bad)
    unmask("SECAGG_MAX_STREAMS", add_streams=torch.zeros(1000, dtype=torch.int64),
           sub_streams=torch.zeros(89, dtype=torch.int64))
    unmask("seed=", seed=-1)
    unmask("16-byte aligned", out=torch.zeros(P + 4)[1:P + 1])
    Yb = torch.zeros(K + 1, P, dtype=torch.int32)
    unmask("Y and sum_out overlap", Y=Yb[:K], sum_out=Yb[K - 1])
    unmask("out and sum_out overlap", out=Yb[K].view(torch.float32), sum_out=Yb[K])


# ------------------------------------------------------------ source plumbing
def test_source_plumbing():
    from distributed_learning_simulator_amd import _native
    csrc = os.path.join(ROOT, "distributed_learning_simulator_amd", "csrc")
    with open(os.path.join(csrc, "Makefile")) as fh:
        text = fh.read()
    srcs = next(line for line in text.splitlines() if line.startswith("SRCS :=")).split()[2:]
    assert "secagg.hip" in srcs and _native.CSRC_HASHED[:len(srcs)] == srcs
    hashed = next(line for line in text.splitlines() if line.startswith("HASHED :="))
    rule = next(line for line in text.splitlines() if line.startswith("_build/%.o:"))
    assert "philox_common.h" in hashed and "philox_common.h" in rule
    assert "philox_common.h" in _native.CSRC_HASHED
    for f in ("dpnoise.hip", "secagg.hip"):
        with open(os.path.join(csrc, f)) as fh:
            src = fh.read()
        assert '#include "philox_common.h"' in src and "struct PhiloxKey" not in src
        assert "getenv" not in src and "asm" not in src  # plain C++ only
    with open(os.path.join(ROOT, "include", "dls_hip.h")) as fh:
        header = fh.read()
    assert "#define DLS_SECAGG_MAX_STREAMS 1088" in header and "#define DLS_ABI_VERSION 2" in header
    L = _native.lib()
    for name in ("dls_secagg_mask_f32", "dls_secagg_unmask_f32"):
        assert "int " + name + "(" in header and name in _native.SIGNATURES and hasattr(L, name)
    assert L.dls_source_hash().decode() == _native.source_hash()
