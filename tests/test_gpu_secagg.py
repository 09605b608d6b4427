"""GPU checks of the two secure-aggregation kernels (csrc/secagg.hip) against
tests/secagg_ref.py, every comparison on bits: the mask kernel at every stream count and
launch-plan edge with the encode's edge values, the unmask kernel at every chunking of the
row table, the cancellation of the client and server stream lists through both kernels,
every refusal of the two entry points, and FedSecAggServer / FedSecAggWorker on the device."""
import numpy as np
import pytest
import torch

from tests import secagg_ref as R
from tests.test_secagg_host import (MASK_ERRORS, NS, UNMASK_ERRORS, FakeTrainer, initial_model,
                                    make_model, mask_call, unmask_call)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
F32, U32 = np.float32, np.uint32
SEED = 0x9E3779B97F4A7C15
TILE = 256  # coordinates per wave and visit
# 2048 waves of one tile each, and one vector more: the first P at which a wave (wave 0)
# visits a second tile; the plan is tiles = ceil(P / 256), tpw = ceil(tiles / 2048)
BIG_P = 2048 * TILE + 4
# stream ids with both halves in use: rounds 1 and 2^32 - 1, worker ids up to 65535
STREAMS = [((1 + (i % 2) * ((1 << 32) - 2)) << 32) | ((i * 37 % 65536) << 16) | (65535 - i)
           for i in range(1088)]
STREAM_COUNTS = ((0, 0), (1, 0), (0, 1), (3, 2), (64, 0), (31, 32))


def _native():
    from distributed_learning_simulator_amd import _native
    return _native


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == U32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).to(DEV)


def _table(ids):
    t = R.stream_table(ids)
    return None if t is None else t.to(DEV)


def _bits(t):
    a = t.cpu().numpy()
    return a.view(U32)


# ------------------------------------------------------------------ the mask kernel
F_EDGE, B_EDGE, W_EDGE = 4, 6, 1 << 27  # steps of 1/16, L = 31; 31 * 2^27 wraps the sign bit
L_EDGE = 31


def edge_inputs(P, rng):
    """(w, base): random, with the encode's edge values in the first slots.  The edge slots
    have base 0 but for the subnormal difference, which is between two normal numbers."""
    w = (rng.standard_normal(P) * 0.7).astype(F32)
    base = (rng.standard_normal(P) * 0.7).astype(F32)
    s = F32(1.0 / 16.0)
    edge = [0.5 * s, 1.5 * s, 2.5 * s, -0.5 * s, -1.5 * s, -2.5 * s,   # ties, both sides of even
            L_EDGE * s, -L_EDGE * s, (L_EDGE + 1) * s, -(L_EDGE + 1) * s,
            (L_EDGE + 0.5) * s, np.inf, -np.inf, np.nan, -0.0, 3e38, 1e-45]
    n = min(P, len(edge))
    w[:n], base[:n] = np.array(edge[:n], F32), 0.0
    if P > len(edge) + 1:  # 1.5 * 2^-126 - 2^-126 = 2^-127
        w[len(edge)], base[len(edge)] = F32(1.5 * 2.0 ** -126), F32(2.0 ** -126)
    return w, base


def run_mask(w, base, P, f, b, weight, add, sub, stats0=(5, 7), stream=None):
    y = torch.full((P + 8,), -1, dtype=torch.int32, device=DEV)
    stats = torch.tensor(stats0, dtype=torch.int32, device=DEV)
    _native().secagg_mask(_dev(w), _dev(base), P, f, b, weight, _table(add), _table(sub), SEED, y,
                          stats, stream=stream)
    torch.cuda.synchronize()
    got = y.cpu().numpy()
    assert (got[P:] == -1).all()
    return got[:P].view(U32), stats.tolist()


@pytest.mark.parametrize("P", [4, TILE - 4, TILE, TILE + 4, BIG_P])
def test_mask_bits(P):
    rng = np.random.default_rng(P)
    w, base = edge_inputs(P, rng)
    for n_add, n_sub in STREAM_COUNTS:
        add, sub = STREAMS[:n_add], STREAMS[64:64 + n_sub]
        want, n_sat, n_bad = R.mask(w, base, F_EDGE, B_EDGE, W_EDGE, add, sub, SEED)
        got, stats = run_mask(w, base, P, F_EDGE, B_EDGE, W_EDGE, add, sub)
        assert np.array_equal(got, want), (n_add, n_sub)
        assert stats == [5 + n_sat, 7 + n_bad], (n_add, n_sub)  # added to, not overwritten
    if P >= 20:
        assert n_bad == 3 and n_sat >= 4
    # the default format on the same data, and a wide one whose product overflows fp32
    for f, b, weight in ((16, 20, 3), (126, 31, 1), (0, 2, (1 << 32) - 1)):
        want, n_sat, n_bad = R.mask(w, base, f, b, weight, STREAMS[:3], STREAMS[64:66], SEED)
        got, stats = run_mask(w, base, P, f, b, weight, STREAMS[:3], STREAMS[64:66], stats0=(0, 0))
        assert np.array_equal(got, want) and stats == [n_sat, n_bad], (f, b)


def test_mask_does_not_depend_on_the_call():
    """Pieces of a row masked separately are NOT the row's mask (a piece restarts at
    coordinate 0), but another HIP stream and another position in memory give the same bits."""
    P = TILE + 4
    w, base = edge_inputs(P, np.random.default_rng(1))
    want, _ = run_mask(w, base, P, 16, 20, 1, STREAMS[:3], STREAMS[64:66])
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        got, _ = run_mask(w, base, P, 16, 20, 1, STREAMS[:3], STREAMS[64:66], stream=side)
    assert np.array_equal(got, want)
    big = torch.zeros(3 * P + 12, device=DEV)
    big[4:4 + P].copy_(_dev(w))
    big[P + 8:2 * P + 8].copy_(_dev(base))
    y = torch.zeros(P, dtype=torch.int32, device=DEV)
    _native().secagg_mask(big[4:4 + P], big[P + 8:2 * P + 8], P, 16, 20, 1, _table(STREAMS[:3]),
                          _table(STREAMS[64:66]), SEED, y,
                          torch.zeros(2, dtype=torch.int32, device=DEV))
    assert np.array_equal(_bits(y), want)


# ---------------------------------------------------------------- the unmask kernel
def run_unmask(Y, rows, add, sub, base, f, total, P, stream=None, with_sum=True):
    out = torch.full((P + 8,), -7.0, device=DEV)
    S = torch.full((P + 8,), -1, dtype=torch.int32, device=DEV) if with_sum else None
    _native().secagg_unmask(Y, _dev(np.asarray(rows, np.int32)), _table(add), _table(sub), SEED,
                            _dev(base), f, total, P, out, S, stream=stream)
    torch.cuda.synchronize()
    assert (out[P:] == -7.0).all() and (S is None or (S[P:] == -1).all())
    return _bits(out[:P]), (None if S is None else _bits(S[:P]))


@pytest.mark.parametrize("K", [1, 2, 31, 32, 33, 64])
def test_unmask_bits(K):
    rng = np.random.default_rng(K)
    P, ldy = TILE + 4, TILE + 12  # two tiles, the second ragged; ldy > P
    Yh = rng.integers(0, 1 << 32, size=(K + 3, ldy), dtype=np.uint64).astype(U32)
    Y = _dev(Yh)
    rows = (rng.permutation(K) + 2).tolist()  # permuted, offset inside the larger Y
    base = rng.standard_normal(P).astype(F32)
    side = torch.cuda.Stream(DEV)
    for (n_add, n_sub), total in (((0, 0), float(K)), ((1, 0), 7.0), ((0, 1), 1.0),
                                  ((3, 2), 1e6 + 1.0)):
        add, sub = STREAMS[:n_add], STREAMS[64:64 + n_sub]
        want, S = R.unmask(Yh, rows, add, sub, SEED, base, 16, total, P)
        out, got_S = run_unmask(Y, rows, add, sub, base, 16, total, P)
        assert np.array_equal(got_S, S) and np.array_equal(out, want), (n_add, n_sub)
        with torch.cuda.stream(side):  # the same on a second HIP stream, without sum_out
            out2, _ = run_unmask(Y, rows, add, sub, base, 16, total, P, stream=side,
                                 with_sum=False)
        assert np.array_equal(out2, want), (n_add, n_sub)


def test_unmask_the_most_streams_and_the_second_visit():
    rng = np.random.default_rng(9)
    for P, K, n_add, n_sub in ((1024, 33, 64, 1024), (BIG_P, 2, 1, 2)):
        Yh = rng.integers(0, 1 << 32, size=(K, P), dtype=np.uint64).astype(U32)
        base = rng.standard_normal(P).astype(F32)
        add, sub = STREAMS[:n_add], STREAMS[64:64 + n_sub]
        rows = list(range(K))[::-1]
        want, S = R.unmask(Yh, rows, add, sub, SEED, base, 12, 33.0, P)
        out, got_S = run_unmask(_dev(Yh), rows, add, sub, base, 12, 33.0, P)
        assert np.array_equal(got_S, S) and np.array_equal(out, want), P


def test_unmask_decode_edges():
    """Two rows whose sum wraps: v = INT32_MIN, v = -1, and quotients that are rounding ties
    after the cast to fp32, or that the fp64 division rounds onto one."""
    tie = (1 << 24) + 1  # halfway between two floats: to even
    vs = [0x80000000, 0xFFFFFFFF, 0, 1, 3 * tie, 3 * (tie + 2), (-3 * tie) & 0xFFFFFFFF,
          7 * tie, 10 * ((1 << 25) + 2), 0x7FFFFFFF, 0x80000001, 12345677]
    S = np.array(vs + [0] * (16 - len(vs)), U32)
    a = np.array([0x40000000, 0x7FFFFFFF] + [5] * 14, U32)
    Yh = np.stack([a, S - a])  # wraps
    assert np.array_equal(R.ring_sum(Yh), S)
    Y = _dev(Yh)
    P = 16
    for base in (np.zeros(P, F32), np.full(P, -0.0, F32),
                 np.random.default_rng(0).standard_normal(P).astype(F32)):
        for f in (0, 1, 16, 126):
            # 3, 7 and 10 divide the ties above exactly; 2^31 - 1 + 0.5 is an fp64 that is no
            # integer; 1e15 + 1: a quotient far below one ulp of the base
            for total in (1.0, 3.0, 7.0, 10.0, 49.0, 2.0 ** 31 - 0.5, 1e15 + 1.0):
                want, _ = R.unmask(Yh, [0, 1], [], [], SEED, base, f, total, P)
                out, got_S = run_unmask(Y, [0, 1], [], [], base, f, total, P)
                assert np.array_equal(got_S, S)
                assert np.array_equal(out, want), (f, total)
    # the ties are ties: with f = 0 and total = 3 the two neighbours round to even
    out, _ = run_unmask(Y, [0, 1], [], [], np.zeros(P, F32), 0, 3.0, P)
    assert out.view(F32)[[4, 5]].tolist() == [float(1 << 24), float((1 << 24) + 4)]
    assert out.view(F32)[0] == F32(-2.0 ** 31 / 3.0) and out.view(F32)[1] == F32(-1.0 / 3.0)


# ------------------------------------------------------------------ cancellation
@pytest.mark.parametrize("K", [2, 5, 64])
def test_masks_cancel_through_both_kernels(K):
    from distributed_learning_simulator_amd.aggregation import (secagg_client_streams,
                                                                secagg_server_streams)
    rng = np.random.default_rng(100 + K)
    P, f, b, rnd = 2 * TILE + 4, 10, 16, 3
    ids = [3 * k + 1 for k in range(K)]
    base = rng.standard_normal(P).astype(F32)
    W = (base + rng.standard_normal((K, P)).astype(F32) * 0.2).astype(F32)
    weights = [int(x) for x in rng.integers(1, 6, size=K)]
    Y = torch.empty((K, P), dtype=torch.int32, device=DEV)
    E = np.empty((K, P), U32)
    stats = torch.zeros(2, dtype=torch.int32, device=DEV)
    for k, wid in enumerate(ids):
        add, sub = secagg_client_streams(wid, ids, rnd)
        _native().secagg_mask(_dev(W[k]), _dev(base), P, f, b, weights[k], _table(add), _table(sub),
                              SEED, Y[k], stats)
        E[k] = R.encode(W[k], base, f, b, weights[k])[0]
    assert stats.tolist() == [0, 0]
    assert not np.array_equal(_bits(Y), E)
    threshold = K // 2 + 1
    for n_drop in sorted({0, 1, K - threshold}):
        gone_rows = sorted(int(r) for r in rng.choice(K, size=n_drop, replace=False))
        rows = [int(r) for r in rng.permutation(K) if r not in gone_rows]
        alive, gone = [ids[r] for r in rows], [ids[r] for r in gone_rows]
        total = float(sum(weights[r] for r in rows))
        want_S = R.ring_sum(E[rows])
        add, sub = secagg_server_streams(alive, gone, rnd)
        out, S = run_unmask(Y, rows, add, sub, base, f, total, P)
        assert np.array_equal(S, want_S), n_drop
        assert np.array_equal(out, R.decode(want_S, base, f, total)), n_drop
        if n_drop:  # without the recovery streams the sum stays masked: the masks are not zero
            add, sub = secagg_server_streams(alive, [], rnd)
            _, S = run_unmask(Y, rows, add, sub, base, f, total, P)
            assert not np.array_equal(S, want_S)


# ------------------------------------------------------------------ refusals
def test_entry_points_refuse_and_leave_the_outputs_untouched():
    N = _native()
    L = N.lib()
    P = 64
    y = torch.full((P,), -1, dtype=torch.int32, device=DEV)
    stats = torch.full((2,), -1, dtype=torch.int32, device=DEV)
    out = torch.full((P,), -7.0, device=DEV)
    sum_out = torch.full((P,), -1, dtype=torch.int32, device=DEV)
    w, base = torch.zeros(P, device=DEV), torch.zeros(P, device=DEV)
    Y = torch.zeros((3, P), dtype=torch.int32, device=DEV)
    rows = torch.arange(3, dtype=torch.int32, device=DEV)
    table = _table(STREAMS[:8])
    real_m = dict(w=N._ptr(w), base=N._ptr(base), add=N._ptr(table), sub=N._ptr(table), y=N._ptr(y),
                  stats=N._ptr(stats))
    real_u = dict(Y=N._ptr(Y), rows=N._ptr(rows), add=N._ptr(table), sub=N._ptr(table),
                  base=N._ptr(base), out=N._ptr(out), sum_out=N._ptr(sum_out))
    for kw, status, text in MASK_ERRORS:
        rc, msg = mask_call(L, **{**real_m, **kw})
        assert rc == status and text in msg, (kw, rc, msg)
    for kw, status, text in UNMASK_ERRORS:
        rc, msg = unmask_call(L, **{**real_u, **kw})
        assert rc == status and text in msg, (kw, rc, msg)
    assert mask_call(L, **{**real_m, "P": 0})[0] == 0  # launches nothing
    assert unmask_call(L, **{**real_u, "P": 0})[0] == 0
    torch.cuda.synchronize()
    assert (y == -1).all() and (stats == -1).all() and (out == -7.0).all() and (sum_out == -1).all()
    # the wrappers' own refusals, on device tensors
    with pytest.raises(RuntimeError, match="y and base overlap"):
        N.secagg_mask(w, base, P, 16, 20, 1, None, None, 0, base.view(torch.int32), stats)
    with pytest.raises(RuntimeError, match="is on cpu"):
        N.secagg_mask(w, base, P, 16, 20, 1, torch.zeros(1, dtype=torch.int64), None, 0, y, stats)
    with pytest.raises(RuntimeError, match="K=65 rows"):
        N.secagg_unmask(Y, torch.zeros(65, dtype=torch.int32, device=DEV), None, None, 0, base, 16,
                        3.0, P, out)
    assert (y == -1).all() and (out == -7.0).all()


# -------------------------------------------------- server and worker on the device
def device_run(order_of_round, weighted):
    from distributed_learning_simulator_amd.servers.fed_secagg_server import FedSecAggServer
    from distributed_learning_simulator_amd.workers.fed_secagg_worker import FedSecAggWorker
    bits, f = (12, 8) if weighted else (20, 16)
    server = FedSecAggServer(initial_model=initial_model(), tester=None, worker_number=4,
                             synchronous=True, device=DEV, secagg_dropouts=(2,), secagg_seed=SEED,
                             secagg_bits=bits, secagg_frac_bits=f)
    workers = {i: FedSecAggWorker(worker_id=i, trainer=FakeTrainer(make_model(10 + i).to(DEV), NS[i]),
                                  worker_data_queue=server.worker_data_queue, round=2,
                                  participants=range(4), secagg_weighted=weighted,
                                  secagg_seed=SEED, secagg_bits=bits, secagg_frac_bits=f)
               for i in range(4)}
    for i, w in workers.items():
        w.load_model(server.worker_data_queue.get_result(consumer=i))
    lay = server.layout
    rng = np.random.default_rng(17)
    models = []
    for order in order_of_round:
        prev = lay.flatten(server.prev_model, device=DEV).cpu().numpy()
        E, payloads = {}, {}
        for wid in range(4):  # the same training in every run
            with torch.no_grad():
                for p in workers[wid].trainer.model.parameters():
                    p += torch.from_numpy((rng.standard_normal(tuple(p.shape)) * 0.05)
                                          .astype(F32)).to(DEV)
            wflat = lay.flatten(dict(workers[wid].trainer.model.named_parameters()),
                                device=DEV).cpu().numpy()
            E[wid] = R.encode(wflat, prev, f, bits, NS[wid] if weighted else 1)[0]
            payloads[wid] = workers[wid].masked_update(NS[wid])
            assert payloads[wid].y.device.type == "cuda" and payloads[wid].saturated == 0
        for wid in order:
            server.worker_data_queue.add_task((wid, NS[wid], payloads[wid]))
        alive = [0, 1, 3]
        total = sum(NS[w] for w in alive) if weighted else 3
        ref = R.decode(R.ring_sum(np.stack([E[w] for w in alive])), prev, f, total)
        got = lay.flatten(server.prev_model, device=DEV).cpu().numpy()
        assert np.array_equal(got.view(U32), ref)
        assert server.last_secagg["survivors"] == (0, 1, 3) and server.last_secagg["dropped"] == (2,)
        assert server.last_secagg["total"] == total and server.last_secagg["streams_removed"] == 6
        for wid in range(4):
            workers[wid].load_model(server.worker_data_queue.get_result(consumer=wid))
        models.append(got.copy())
    assert server.round == len(order_of_round)
    return models


@pytest.mark.parametrize("weighted", [False, True])
def test_server_and_worker_on_the_device(weighted):
    a = device_run(([0, 1, 2, 3], [2, 0, 3, 1]), weighted)
    b = device_run(([3, 2, 1, 0], [1, 3, 0, 2]), weighted)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(U32), y.view(U32))
    assert not np.array_equal(a[0], a[1])


def test_simulator_run_with_dropouts(tmp_path):
    from distributed_learning_simulator_amd import simulator
    cfg = simulator.get_config(
        ["--distributed_algorithm", "fed_secagg", "--worker_number", "3", "--round", "2",
         "--secagg_dropouts", "1", "--secagg_seed", "7", "--train_size", "192", "--test_size",
         "64", "--log_dir", str(tmp_path)])
    server = simulator.run(cfg)
    assert server.round == 2 and server.last_secagg["survivors"] == (0, 2)
    assert server.last_secagg["dropped"] == (1,) and server.last_secagg["streams_removed"] == 4
    assert server.last_secagg["total"] == 2
    for v in server.prev_model.values():
        assert bool(torch.isfinite(v).all())
