"""GPU: dls_topk_compress_f32 and dls_sparse_fedavg_f32 against tests/topk_ref.py, bit for
bit (idx exactly, val / residual / out as uint32 views, stats); FedTopKServer and one
fed_topk simulation.  No tolerances anywhere."""
import logging
import math

import numpy as np
import pytest
import torch

from tests import topk_ref
from tests.topk_ref import bits

pytestmark = pytest.mark.gpu

F32 = np.float32
BIG = (1 << 20) + 68


def _dev():
    return torch.device("cuda", 0)


def run_compress(w, base, e, k, stream=None, ws_fill=0xFF):
    """The device outputs of one call as numpy: idx, val, e_new, stats.  The workspace is
    filled with ``ws_fill`` bytes first: it may hold garbage on entry."""
    from distributed_learning_simulator_amd import _native
    dev = _dev()
    P = w.size
    tw, tb, te = (torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(dev) for a in (w, base, e))
    ws = _native.topk_workspace(P, dev)
    ws.fill_(ws_fill)
    idx = torch.full((k,), -1, dtype=torch.int32, device=dev)
    val = torch.full((k,), 123.0, dtype=torch.float32, device=dev)
    stats = torch.full((2,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    if stream is None:
        _native.topk_compress(tw, tb, te, k, P, idx, val, stats, ws)
    else:
        with torch.cuda.stream(stream):
            _native.topk_compress(tw, tb, te, k, P, idx, val, stats, ws, stream=stream)
    torch.cuda.synchronize()
    return idx.cpu().numpy(), val.cpu().numpy(), te.cpu().numpy(), stats.cpu().numpy()


def check_split(w, base, e, k, got):
    """The exact-split invariant on the device outputs, independent of the reference's
    selection: every u[j] is in exactly one of val and the new residual, bit for bit."""
    idx, val, e_new, _ = got
    u = topk_ref.update(w, base, e)
    assert idx.size == k and np.all(np.diff(idx.astype(np.int64)) > 0)
    assert idx[0] >= 0 and idx[-1] < u.size
    sent = np.zeros(u.size, bool)
    sent[idx] = True
    assert np.array_equal(bits(val), bits(u[idx]))
    assert np.array_equal(bits(e_new[sent]), np.zeros(k, np.uint32))  # +0.0
    assert np.array_equal(bits(e_new[~sent]), bits(u[~sent]))


def check(w, base, e, k, got=None):
    got = run_compress(w, base, e, k) if got is None else got
    idx, val, e_new, nonfinite = topk_ref.compress(w, base, e, k)
    assert np.array_equal(got[0], idx)
    assert np.array_equal(bits(got[1]), bits(val))
    assert np.array_equal(bits(got[2]), bits(e_new))
    assert got[3].tolist() == [k, nonfinite]
    check_split(w, base, e, k, got)
    return got


def gaussian(P, rng):
    w = (rng.standard_normal(P) * 10.0 ** rng.uniform(-6, 2, P)).astype(F32)
    base = (rng.standard_normal(P) * 0.1).astype(F32)
    e = (rng.standard_normal(P) * 1e-3).astype(F32)
    return w, base, e


def zeros(P):
    return np.zeros(P, F32)


@pytest.mark.parametrize("P", [4, 64, 4100, 65540, BIG])
def test_compress_sizes(P):
    """One lane, one wave, a ragged last block, many blocks, more blocks than CUs."""
    rng = np.random.default_rng(P)
    w, base, e = gaussian(P, rng)
    for k in sorted({1, 2, P // 2, P - 1, P, math.ceil(0.01 * P)}):
        if 1 <= k <= P:
            check(w, base, e, k)


def family(name, P, rng):
    if name == "gaussian":
        return gaussian(P, rng)
    if name == "lowbits":  # keys that differ in the lowest bits only: the last pass decides
        b = (np.uint32(0x3F800000) + rng.permutation(P).astype(np.uint32))
        sign = rng.integers(0, 2, P).astype(np.uint32) << np.uint32(31)
        return (b | sign).view(F32), zeros(P), zeros(P)
    if name == "pow2":  # the first pass decides
        w = np.ldexp(F32(1.0), rng.integers(-40, 41, P)).astype(F32)
        return w * rng.choice(np.array([-1.0, 1.0], F32), P), zeros(P), zeros(P)
    if name == "zeros":  # all zeros, some -0.0 (from w = -0.0, base = +0.0, e = -0.0)
        w, e = zeros(P), zeros(P)
        neg = rng.random(P) < 0.3
        w[neg] = F32(-0.0)
        e[neg] = F32(-0.0)
        return w, zeros(P), e
    if name == "denormal":
        b = rng.integers(1, 0x00800000, P).astype(np.uint32)
        sign = rng.integers(0, 2, P).astype(np.uint32) << np.uint32(31)
        return (b | sign).view(F32), zeros(P), zeros(P)
    if name == "residual":  # the residual's addition changes which coordinates win
        w = (rng.standard_normal(P) * 1e-3).astype(F32)
        base = (rng.standard_normal(P) * 1e-3).astype(F32)
        e = zeros(P)
        at = rng.choice(P, P // 50, replace=False)
        e[at] = (rng.standard_normal(at.size) * 1e-2).astype(F32)
        return w, base, e
    raise AssertionError(name)


@pytest.mark.parametrize("name", ["gaussian", "lowbits", "pow2", "zeros", "denormal", "residual"])
def test_compress_value_families(name):
    P = 65540
    rng = np.random.default_rng(len(name))
    w, base, e = family(name, P, rng)
    if name == "zeros":
        assert (bits(topk_ref.update(w, base, e)) == 0x80000000).any()
    if name == "residual":  # ... it does change the winners
        k = P // 100
        assert not np.array_equal(topk_ref.compress(w, base, e, k)[0],
                                  topk_ref.compress(w, base, zeros(P), k)[0])
    for k in (1, math.ceil(0.01 * P), P // 3, P - 1):
        check(w, base, e, k)


@pytest.mark.parametrize("P", [65540, BIG])
def test_compress_threshold_group(P):
    """Eight magnitudes with random signs: the threshold group holds about P / 8 entries
    spread over every block; k at its first element, in its middle and at its last."""
    rng = np.random.default_rng(8)
    mags = np.array([0.5, 0.75, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], F32)
    pick = rng.integers(0, 8, P)
    w = mags[pick] * rng.choice(np.array([-1.0, 1.0], F32), P)
    above = int((pick > 4).sum())          # the entries larger than 2.0
    group = int((pick == 4).sum())
    assert group > P // 10 and (pick[:4096] == 4).any() and (pick[-68:] == 4).any()
    for k in (above + 1, above + group // 2, above + group):
        got = check(w, zeros(P), zeros(P), k)
        # the group's members that were sent are its lowest indices
        members = np.flatnonzero(pick == 4)
        assert np.array_equal(np.intersect1d(got[0], members), members[:k - above])


def test_compress_nonfinite():
    """Three NaNs, a +inf and a -inf: counted, and they take selected slots first."""
    P, k = 4100, 9
    rng = np.random.default_rng(5)
    w, base, e = gaussian(P, rng)
    e[:] = 0
    where = [3, 2049, 4099, 64, 4000]
    w[where[:3]] = np.nan
    w[where[3]] = np.inf
    w[where[4]] = -np.inf
    got = check(w, base, e, k)
    assert got[3].tolist() == [k, 5]
    assert set(where) <= set(got[0].tolist())
    got = check(w, base, e, 4)  # fewer slots than non-finite values: the NaNs, then index order
    assert set(got[0].tolist()) == {3, 2049, 4099, 64}


def test_compress_is_deterministic_and_stream_independent():
    P, k = 65540, 700
    rng = np.random.default_rng(11)
    w, base, e = gaussian(P, rng)
    a = run_compress(w, base, e, k)
    b = run_compress(w, base, e, k)
    c = run_compress(w, base, e, k, stream=torch.cuda.Stream(_dev()))
    for other in (b, c):
        assert np.array_equal(a[0], other[0]) and np.array_equal(bits(a[1]), bits(other[1]))
        assert np.array_equal(bits(a[2]), bits(other[2])) and np.array_equal(a[3], other[3])
    check(w, base, e, k, got=c)


# ------------------------------------------------------------------ sparse FedAvg
def run_sparse(base, payloads, ns):
    from distributed_learning_simulator_amd import _native
    dev = _dev()
    off = np.cumsum([0] + [len(i) for i, _ in payloads]).astype(np.int64)
    idx = np.concatenate([i for i, _ in payloads]).astype(np.int32)
    val = np.concatenate([v for _, v in payloads]).astype(F32)
    out = torch.full((base.size,), 7.0, dtype=torch.float32, device=dev)
    _native.sparse_fedavg(torch.from_numpy(base).to(dev), torch.from_numpy(idx).to(dev),
                          torch.from_numpy(val).to(dev), torch.from_numpy(off).to(dev),
                          torch.tensor([float(n) for n in ns], dtype=torch.float32, device=dev),
                          float(sum(ns)), base.size, out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def subset(P, ratio, rng):
    return np.flatnonzero(rng.random(P) < ratio).astype(np.int32)


def edges(P):
    """The first and last coordinate and both sides of every multiple of 256 (so of 4096)."""
    m = np.arange(256, P, 256)
    return np.unique(np.concatenate([[0, P - 1], m - 1, m])).astype(np.int32)


def make_payloads(kind, K, P, rng):
    if kind in ("r01", "r50"):
        sets = [subset(P, 0.01 if kind == "r01" else 0.5, rng) for _ in range(K)]
    elif kind == "same":  # every client sends the same coordinates: chains of full length
        sets = [subset(P, 0.1, rng)] * K
    elif kind == "disjoint":
        sets = [np.arange(i, P, K, dtype=np.int32) for i in range(K)]
    else:  # mixed: an empty segment, a client that sent everything, tile edges
        sets = [[np.zeros(0, np.int32), np.arange(P, dtype=np.int32), edges(P)][i % 3]
                for i in range(K)]
    return [(s, (rng.standard_normal(s.size) * 0.05).astype(F32)) for s in sets]


@pytest.mark.parametrize("P", [64, 4100, (1 << 18) + 4])
@pytest.mark.parametrize("K", [1, 2, 7, 100])
def test_sparse_fedavg(K, P):
    rng = np.random.default_rng(1000 * K + P % 997)
    base = (rng.standard_normal(P) * 0.1).astype(F32)
    base[rng.random(P) < 0.05] = F32(-0.0)
    ns = [int(n) for n in rng.integers(100, 1001, K)]
    for kind in ("r01", "r50", "same", "disjoint", "mixed"):
        pay = make_payloads(kind, K, P, rng)
        ref = topk_ref.sparse_fedavg(base, pay, ns)
        got = run_sparse(base, pay, ns)
        assert np.array_equal(bits(got), bits(ref)), kind
        if kind == "r01":  # an untouched -0.0 stays -0.0; the same bits on a repeat
            sent = np.zeros(P, bool)
            for i, _ in pay:
                sent[i] = True
            quiet = ~sent & (bits(base) == 0x80000000)
            assert np.all(bits(got)[quiet] == 0x80000000)
            assert quiet.any() or P == 64
            assert np.array_equal(bits(run_sparse(base, pay, ns)), bits(got))
        if K > 1 and kind in ("r50", "same"):  # the other client order: the reference's bits for it
            rev, nrev = pay[::-1], ns[::-1]
            other = run_sparse(base, rev, nrev)
            assert np.array_equal(bits(other), bits(topk_ref.sparse_fedavg(base, rev, nrev))), kind


def test_sparse_fedavg_single_client_weight_one():
    P = 4100
    rng = np.random.default_rng(3)
    base = (rng.standard_normal(P) * 0.1).astype(F32)
    base[7] = F32(-0.0)
    idx = np.setdiff1d(np.arange(P, dtype=np.int32), [7]).astype(np.int32)
    pay = [(idx, (rng.standard_normal(idx.size) * 0.05).astype(F32))]
    got = run_sparse(base, pay, [1])
    assert np.array_equal(bits(got), bits(topk_ref.sparse_fedavg(base, pay, [1])))
    assert bits(got)[7] == 0x80000000
    assert np.array_equal(bits(got[idx]), bits(base[idx] + pay[0][1]))  # fl(fl(v * 1) / 1) = v


# ------------------------------------------------------------------ server, simulator
def test_server_round_on_device():
    """One FedTopKServer round: payloads from topk_compress on the device, arriving out of
    id order; the broadcast model is the numpy reference's, bit for bit."""
    from distributed_learning_simulator_amd import _native
    from distributed_learning_simulator_amd.layout import ParameterLayout
    from distributed_learning_simulator_amd.servers.fed_topk_server import FedTopKServer
    from distributed_learning_simulator_amd.workers.fed_topk_worker import SparseUpdate
    dev = _dev()
    g = torch.Generator().manual_seed(2)
    initial = {"w": torch.randn(37, 11, generator=g), "b": torch.randn(70, generator=g)}
    layout = ParameterLayout.from_dict(initial)
    server = FedTopKServer(initial_model=initial, tester=None, worker_number=3, synchronous=True,
                           device=dev)
    base = layout.flatten(initial, device=dev)
    for wid in range(3):  # every worker takes the initial broadcast
        first = server.worker_data_queue.get_result(consumer=wid)
        assert all(torch.equal(first[n].cpu(), initial[n]) for n in initial)
    k, ns, order, sent = 40, {0: 300, 1: 120, 2: 777}, [2, 0, 1], {}
    for wid in order:
        trained = {n: v + 0.01 * torch.randn(v.shape, generator=g) for n, v in initial.items()}
        w = layout.flatten(trained, device=dev)
        e = torch.zeros(layout.P, device=dev)
        idx = torch.empty(k, dtype=torch.int32, device=dev)
        val = torch.empty(k, dtype=torch.float32, device=dev)
        stats = torch.empty(2, dtype=torch.int32, device=dev)
        _native.topk_compress(w, base, e, k, layout.P, idx, val, stats,
                              _native.topk_workspace(layout.P, dev))
        assert stats.tolist() == [k, 0]
        ri, rv, _, _ = topk_ref.compress(w.cpu().numpy(), base.cpu().numpy(), np.zeros(layout.P, F32), k)
        assert np.array_equal(idx.cpu().numpy(), ri) and np.array_equal(bits(val.cpu().numpy()), bits(rv))
        sent[wid] = (ri, rv)
        server.worker_data_queue.add_task((wid, ns[wid], SparseUpdate(idx, val, layout.P)))
    model = server.worker_data_queue.get_result(consumer=0)
    ref = topk_ref.sparse_fedavg(base.cpu().numpy(), [sent[i] for i in order], [ns[i] for i in order])
    flat = layout.flatten(model, device=dev).cpu().numpy()
    assert np.array_equal(bits(flat), bits(ref))
    assert server.round == 1 and server.payload_counts == [{2: k, 0: k, 1: k}]


def test_fed_topk_simulation(tmp_path, caplog):
    from distributed_learning_simulator_amd import simulator
    from distributed_learning_simulator_amd.workers.fed_topk_worker import topk_count
    cfg = simulator.get_config(["--distributed_algorithm", "fed_topk", "--worker_number", "4",
                                "--round", "2", "--model_name", "LeNet5", "--train_size", "512",
                                "--test_size", "256", "--topk_ratio", "0.05",
                                "--log_dir", str(tmp_path / "log")])
    with caplog.at_level(logging.INFO, logger="distributed_learning_simulator_amd"):
        server = simulator.run(cfg)
    assert server.round == 2
    k = topk_count(0.05, server.layout.numel)
    assert server.payload_counts == [{w: k for w in c} for c in server.payload_counts]
    assert [sorted(c) for c in server.payload_counts] == [[0, 1, 2, 3]] * 2
    acc = server.get_metric(server.prev_model)
    assert math.isfinite(float(acc))
    assert any("uplink" in r.getMessage() and "ratio" in r.getMessage() for r in caplog.records)
    assert any("compression ratio" in r.getMessage() for r in caplog.records)
