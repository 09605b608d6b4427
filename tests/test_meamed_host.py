"""CPU checks of the mean around the median and of Bulyan: the numpy reference the
GPU tests compare with (against a brute force, and the prefix property that lets
the kernel count instead of search), ``bulyan_select`` on hand-made matrices, the
argument validation of dls_mean_around_median_f32 and its Python wrapper (both run
before any device call), the servers' validation, the simulator flags and a full
FedServer round on CPU doubles."""
import ctypes
import itertools
import math

import numpy as np
import pytest
import torch

from tests import cpu_doubles
from tests import meamed_ref as M
from tests import robust_ref as R

CPU = torch.device("cpu")
NEG0, POS0, QNAN = 0x80000000, 0x00000000, 0x7FC00000
FMAX = 0x7F7FFFFF
# +-0, +-inf, two NaNs, +-denormal, +-FLT_MAX, +-1 and 3
POOL = np.array([POS0, NEG0, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFABCDEF, 0x00000001,
                 0x80000001, FMAX, FMAX | 0x80000000, 0x3F800000, 0xBF800000, 0x40400000],
                np.uint32)


def f32_bits(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


# ------------------------------------------------------------------ reference
def test_reference_by_hand():
    # the window slides to the cluster: the trimmed mean would keep 1, 2, 3
    assert M.column([0.0, 1.0, 2.0, 3.0, 100.0], 3) == f32_bits(2.0)
    assert M.column([-100.0, 0.0, 10.0, 11.0, 12.0], 3) == f32_bits(11.0)
    assert M.column([-100.0, -50.0, 10.0, 11.0, 12.0], 2) == f32_bits(10.5)
    # an exact tie keeps the lower value: 1 and 3 are equally far from 2
    assert M.column([1.0, 2.0, 3.0], 2) == f32_bits(1.5)
    assert M.column([3.0, 1.0, 2.0, 4.0], 2) == f32_bits(2.5)  # med 2.5, 2 and 3 nearest
    assert M.column([3.0, 1.0, 2.0, 4.0], 3) == f32_bits(2.0)  # 1 | 4 tie: the lower stays
    # keep == 1: the kept value's own bits
    assert M.column_bits([NEG0, NEG0, f32_bits(5.0)], 1) == NEG0
    assert M.column_bits([f32_bits(7.0)], 1) == f32_bits(7.0)
    # NaNs sit on top and are never compared true: at most K - keep of them are dropped
    nan = 0xFFC00001
    assert M.column_bits([nan, f32_bits(1.0), f32_bits(2.0), f32_bits(3.0), nan], 3) == f32_bits(2.0)
    assert M.column_bits([nan, f32_bits(1.0), f32_bits(2.0), f32_bits(3.0), nan], 4) == QNAN
    assert M.column_bits([nan, nan, nan, f32_bits(1.0), f32_bits(2.0)], 2) == f32_bits(1.5)  # NaN median
    assert M.column_bits([FMAX, FMAX, FMAX], 3) == 0x7F800000  # the kept sum overflows
    # keep == 1 and the median: a finite median comes back with its value, but the steps
    # are the contract where the median is a zero among zeros of both signs, infinite
    # or a NaN (an exact tie keeps the lower value, a comparison with a NaN is false)
    assert M.column([5.0, 1.0, 3.0], 1) == f32_bits(3.0)
    assert M.column_bits([NEG0, POS0, POS0], 1) == NEG0
    assert M.column_bits([f32_bits(1.0), 0x7F800000, 0x7F800000], 1) == f32_bits(1.0)
    assert M.column_bits([f32_bits(1.0), nan, nan], 1) == f32_bits(1.0)


def test_reference_matches_the_keep_smallest_distances():
    """Odd K (an even K always ties: lo and hi are equidistant from the median), the
    columns whose fp32 distances to the median are pairwise distinct: the window is
    the ``keep`` values of smallest distance."""
    rng = np.random.default_rng(2018)
    total = skipped = checked = 0
    for K in range(1, 20, 2):
        P = 1500
        X = (rng.standard_normal((K, P)) * 10.0 ** rng.integers(-3, 4, (1, P))).astype(np.float32)
        keep = rng.integers(1, K + 1, P)
        v = M.sorted_values(X)
        med = M.median_of_sorted(v)
        dist = np.abs((v - med).astype(np.float32))
        distinct = np.array([len(set(dist[:, p].tolist())) == K for p in range(P)])
        total += P
        skipped += int((~distinct).sum())
        for k in range(1, K + 1):
            cols = np.flatnonzero(distinct & (keep == k))
            if cols.size == 0:
                continue
            s = M.window_start(v[:, cols], med[cols], k)
            near = np.sort(np.argsort(dist[:, cols], axis=0, kind="stable")[:k], axis=0)
            assert np.array_equal(near, s[None, :] + np.arange(k)[:, None]), (K, k)
            want = R.trimmed_mean_bits(np.take_along_axis(v[:, cols], near, axis=0), 0)
            assert np.array_equal(M.mean_around_median_bits(X[:, cols], k), want), (K, k)
            checked += cols.size
    assert skipped <= 0.05 * total, (skipped, total)
    assert checked == total - skipped and checked > 14000


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_true_comparisons_form_a_prefix(K):
    """Every column of K special values, every keep: the number of true comparisons is
    the first false index (what the kernel computes instead of searching)."""
    X = np.array(list(itertools.product(POOL.tolist(), repeat=K)), np.uint32).T.copy()
    v = M.sorted_values(X)
    med = M.median_of_sorted(v)
    for keep in range(1, K + 1):
        c = M.comparisons(v, med, keep)
        assert np.array_equal(c.sum(axis=0), M.window_start(v, med, keep)), keep


def test_reference_consequences():
    rng = np.random.default_rng(7)
    for K in (1, 2, 5, 8, 13):
        X = (rng.standard_normal((K, 512)) * 100).astype(np.float32)
        X.view(np.uint32)[:, :128][rng.random((K, 128)) < 0.3] = rng.choice(POOL, 1)[0]
        X.view(np.uint32)[:, 128:256] = rng.choice(POOL, (K, 128))
        assert np.array_equal(M.mean_around_median_bits(X, K), R.trimmed_mean_bits(X, 0))
        if K % 2:  # keep == 1 is the median wherever the median is finite and not a zero
            med = R.median_bits(X)
            ok = np.isfinite(med.view(np.float32)) & (med.view(np.float32) != 0)
            assert ok.sum() > 256
            assert np.array_equal(M.mean_around_median_bits(X, 1)[ok], med[ok])
        for keep in range(1, K + 1):
            want = M.mean_around_median_bits(X, keep)
            assert np.array_equal(M.mean_around_median_bits(X[rng.permutation(K)], keep), want)


# -------------------------------------------------------------- bulyan_select
def _line(points):
    return [[float((a - b) ** 2) for b in points] for a in points]


def test_bulyan_select_no_byzantine():
    from distributed_learning_simulator_amd.aggregation import bulyan_select
    D = [[float("nan")] * 3 for _ in range(3)]  # never looked at
    assert bulyan_select(D, [9, 4, 7], 0) == ([4, 7, 9], {})


@pytest.mark.parametrize("f", [1, 2])
def test_bulyan_select_smallest_k_and_far_clients(f):
    from distributed_learning_simulator_amd.aggregation import bulyan_select
    K = 4 * f + 3
    pts = [0.1 * i for i in range(K - f)] + [1000.0 + 50.0 * i for i in range(f)]
    ids = [100 + i for i in range(K)]
    selected, scores = bulyan_select(_line(pts), ids, f)
    assert len(selected) == K - 2 * f == len(set(selected)) and set(scores) == set(selected)
    assert not set(selected) & set(ids[K - f:])  # the far clients are never picked
    assert all(math.isfinite(s) and s >= 0 for s in scores.values())
    # the first pick by hand: r = K, c = K - f - 2 nearest neighbours
    D = _line(pts)
    first = min(range(K), key=lambda i: (sum(sorted(D[i][j] for j in range(K) if j != i)[:K - f - 2]),
                                         ids[i]))
    assert selected[0] == ids[first]
    # permuting ids and D together: the same picks in the same order
    perm = [(3 * i + 1) % K for i in range(K)]
    Dp = [[D[a][b] for b in perm] for a in perm]
    sel2, sc2 = bulyan_select(Dp, [ids[a] for a in perm], f)
    assert sel2 == selected and sc2 == scores
    with pytest.raises(ValueError, match="4\\*byzantine \\+ 3 <= K"):
        bulyan_select([row[:K - 1] for row in D[:K - 1]], ids[:K - 1], f)


def test_bulyan_select_scores_by_hand():
    from distributed_learning_simulator_amd.aggregation import bulyan_select
    # K = 7, f = 1: theta = 5 picks, c = r - 3 = 4, 3, 2, 1, 1 (never below one)
    pts = [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 100.0]
    D = _line(pts)
    selected, scores = bulyan_select(D, list(range(7)), 1)
    # pick 1: client 2 and 3 tie at 1 + 1 + 4 + 4 = 10: the lower id
    assert selected[0] == 2 and scores[2] == 10.0
    # R = {0,1,3,4,5,6}, c = 3: client 3 -> 1 + 4 + 4 = 9, client 4 -> 1 + 1 + 9 = 11
    assert selected[1] == 3 and scores[3] == 9.0
    # R = {0,1,4,5,6}, c = 2: 0 -> 1 + 16, 1 -> 1 + 9, 4 -> 1 + 9, 5 -> 1 + 16: id breaks the tie
    assert selected[2] == 1 and scores[1] == 10.0
    # R = {0,4,5,6}, c = 1: 4 and 5 at distance 1
    assert selected[3] == 4 and scores[4] == 1.0
    # R = {0,5,6}, c = max(3 - 3, 1) = 1: 0 -> 25, 5 -> 25: the lower id
    assert selected[4] == 0 and scores[0] == 25.0
    assert 6 not in selected


def test_bulyan_select_ties_go_to_the_id_not_the_position():
    from distributed_learning_simulator_amd.aggregation import bulyan_select
    D = [[0.0 if a == b else 1.0 for b in range(7)] for a in range(7)]  # everybody ties
    ids = [5, 3, 9, 1, 8, 2, 7]
    selected, scores = bulyan_select(D, ids, 1)
    assert selected == [1, 2, 3, 5, 7] and all(scores[i] in (4.0, 3.0, 2.0, 1.0) for i in selected)
    assert bulyan_select(D, ids[::-1], 1)[0] == selected
    assert bulyan_select(D, ["b", "a", "g", "c", "e", "d", "f"], 1)[0] == ["a", "b", "c", "d", "e"]


def test_bulyan_select_non_finite_entries():
    from distributed_learning_simulator_amd.aggregation import bulyan_select
    pts = [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0]
    D = _line(pts)
    for j in range(7):  # client 6's row holds inf / NaN / -inf: all count as +inf
        D[6][j] = D[j][6] = (float("inf"), float("nan"), float("-inf"))[j % 3]
    D[6][6] = 0.0
    selected, scores = bulyan_select(D, list(range(7)), 1)
    assert 6 not in selected and len(selected) == 5
    assert all(math.isfinite(s) for s in scores.values())
    # numpy and torch matrices are accepted
    assert bulyan_select(np.array(D), list(range(7)), 1)[0] == selected
    assert bulyan_select(torch.tensor(D, dtype=torch.float64), list(range(7)), 1)[0] == selected
    # three clean clients among seven: after they are gone nobody has a finite neighbour
    bad = [[0.0 if a == b else (float((a - b) ** 2) if a < 3 and b < 3 else float("nan"))
            for b in range(7)] for a in range(7)]
    with pytest.raises(ValueError, match="could select only [0-9] of theta=5"):
        bulyan_select(bad, list(range(7)), 1)


def test_bulyan_select_value_errors():
    from distributed_learning_simulator_amd.aggregation import bulyan_select
    D = _line([float(i) for i in range(7)])
    with pytest.raises(ValueError, match="4\\*byzantine \\+ 3 <= K \\(byzantine=2, K=7\\)"):
        bulyan_select(D, list(range(7)), 2)
    with pytest.raises(ValueError, match="4\\*byzantine \\+ 3 <= K"):
        bulyan_select(D, list(range(7)), -1)
    with pytest.raises(ValueError, match="\\[7, 7\\] matrix"):
        bulyan_select([row[:6] for row in D], list(range(7)), 1)
    with pytest.raises(ValueError, match="\\[7, 7\\] matrix"):
        bulyan_select(D[:6], list(range(7)), 1)
    with pytest.raises(ValueError, match="4\\*byzantine \\+ 3 <= K"):
        bulyan_select([[0.0, 1.0], [1.0, 0.0]], [0, 1], 0)


# ------------------------------------------------------------------------ ABI
def test_abi_rejects_bad_arguments_without_gpu():
    from distributed_learning_simulator_amd import _native
    L = _native.lib()
    d = ctypes.c_void_p(256)  # 16-byte aligned, never dereferenced
    f = L.dls_mean_around_median_f32
    err = L.dls_last_error
    for U, rows, out in ((None, d, d), (d, None, d), (d, d, None)):
        assert f(U, 64, rows, 3, 1, 64, out, None) == -1 and b"null pointer" in err()
    assert f(d, 64, d, 0, 1, 64, d, None) == -1 and b"DLS_ROBUST_MAX_K=64" in err()
    assert f(d, 64, d, 65, 1, 64, d, None) == -1 and b"DLS_ROBUST_MAX_K=64" in err()
    assert f(d, 64, d, 5, 0, 64, d, None) == -1 and b"keep=0 (1 <= keep <= K=5)" in err()
    assert f(d, 64, d, 5, 6, 64, d, None) == -1 and b"keep=6 (1 <= keep <= K=5)" in err()
    assert f(d, 64, d, 5, -1, 64, d, None) == -1 and b"keep=-1" in err()
    assert f(d, 64, d, 3, 1, 62, d, None) == -2 and b"multiples of 4" in err()
    assert f(d, 60, d, 3, 1, 64, d, None) == -2 and b"multiples of 4" in err()
    assert f(d, 62, d, 3, 1, 60, d, None) == -2
    assert f(d, 64, d, 3, 1, 64, ctypes.c_void_p(260), None) == -2 and b"alignment" in err()
    assert f(ctypes.c_void_p(264), 64, d, 3, 1, 64, d, None) == -2 and b"alignment" in err()
    assert b"dls_mean_around_median_f32" in err()
    assert f(d, 64, d, 3, 3, 0, d, None) == 0  # P == 0: nothing to do, no launch


def test_wrapper_validates_before_the_library_call():
    from distributed_learning_simulator_amd import _native
    U = torch.zeros(8, 64)
    out = torch.zeros(64)
    rows = torch.arange(5, dtype=torch.int32)
    bad = [
        (dict(U=U.double()), "U must be"),
        (dict(U=torch.zeros(8, 128)[:, ::2]), "U must be"),
        (dict(rows=rows.long()), "rows must be"),
        (dict(rows=torch.zeros(0, dtype=torch.int32)), "ROBUST_MAX_K"),
        (dict(rows=torch.zeros(65, dtype=torch.int32)), "ROBUST_MAX_K=64"),
        (dict(keep=0), "keep=0 \\(1 <= keep <= K=5\\)"),
        (dict(keep=6), "keep=6 \\(1 <= keep <= K=5\\)"),
        (dict(P=62), "multiple of 4"),
        (dict(P=68), "row length"),
        (dict(out=torch.zeros(32)), "out must be"),
        (dict(out=out.double()), "out must be"),
        (dict(U=torch.zeros(8, 66)[:, :64]), "row pitch"),
        (dict(out=torch.zeros(68)[1:65]), "16-byte aligned"),
    ]
    for change, what in bad:
        kw = dict(U=U, rows=rows, keep=3, P=64, out=out)
        kw.update(change)
        with pytest.raises(RuntimeError, match="mean_around_median: .*" + what):
            _native.mean_around_median(kw["U"], kw["rows"], kw["keep"], kw["P"], kw["out"])
    # valid operands reach the library, which has no CPU path
    with pytest.raises(RuntimeError, match="not on the GPU"):
        _native.mean_around_median(U, rows, 3, 64, out)


# -------------------------------------------------------------------- servers
def _np_mean_around_median(U, rows, keep, P, out, stream=None):
    X = U.detach().numpy()[rows.numpy().astype(np.int64), :P]
    out[:P].copy_(torch.from_numpy(M.mean_around_median_bits(X, keep).view(np.float32)))
    return out


def _np_pairwise_sqdist(U, rows, P, out=None, stream=None):
    X = U.detach().numpy()[rows.numpy().astype(np.int64), :P].astype(np.float64)
    with np.errstate(all="ignore"):
        D = ((X[:, None, :] - X[None, :, :]) ** 2).sum(axis=2)
    np.fill_diagonal(D, 0.0)
    return torch.from_numpy(D)


@pytest.fixture
def doubles(monkeypatch):
    from distributed_learning_simulator_amd import _native
    cpu_doubles.install(monkeypatch)
    calls = {"mean_around_median": 0, "pairwise_sqdist": 0}

    def counted(name, fn):
        def run(*a, **kw):
            calls[name] += 1
            return fn(*a, **kw)
        return run

    monkeypatch.setattr(_native, "mean_around_median",
                        counted("mean_around_median", _np_mean_around_median))
    monkeypatch.setattr(_native, "pairwise_sqdist", counted("pairwise_sqdist", _np_pairwise_sqdist))
    return calls


def _fed(**kw):
    from distributed_learning_simulator_amd.servers.fed_server import FedServer
    return FedServer(tester=None, device=CPU, synchronous=True, **kw)


def test_fed_server_accepts_the_rules(doubles):
    s = _fed(worker_number=11, aggregation_rule="bulyan", byzantine=2)
    assert (s.aggregation_rule, s.byzantine, s.krum_select) == ("bulyan", 2, None)
    assert s.last_selection == () and s.last_scores == {}
    s.stop()
    s = _fed(worker_number=5, aggregation_rule="mean_around_median", byzantine=2)
    assert (s.aggregation_rule, s.byzantine) == ("mean_around_median", 2)
    s.stop()
    _fed(worker_number=3, aggregation_rule="bulyan").stop()
    _fed(worker_number=64, aggregation_rule="bulyan", byzantine=15).stop()
    _fed(worker_number=1, aggregation_rule="mean_around_median").stop()


@pytest.mark.parametrize("kw, what", [
    (dict(aggregation_rule="bulyan", byzantine=2), "4\\*byzantine \\+ 3 <= worker_number"),
    (dict(aggregation_rule="bulyan", byzantine=1, worker_number=6),
     "byzantine=1 is too many for worker_number=6"),
    (dict(aggregation_rule="mean_around_median", byzantine=5), "2\\*byzantine < worker_number"),
    (dict(aggregation_rule="mean_around_median", byzantine=1, worker_number=2),
     "byzantine=1 leaves no majority of worker_number=2"),
    (dict(aggregation_rule="bulyan", byzantine=-1), "non-negative"),
    (dict(aggregation_rule="mean_around_median", byzantine=1.5), "non-negative integer"),
    (dict(aggregation_rule="bulyan", byzantine=1, krum_select=3),
     "krum_select=3 needs aggregation_rule='multi_krum'"),
    (dict(aggregation_rule="mean_around_median", krum_select=1),
     "needs aggregation_rule='multi_krum'"),
    (dict(aggregation_rule="bulyan", trim=1), "trim=1 needs aggregation_rule='trimmed_mean'"),
    (dict(aggregation_rule="bulyan", worker_number=65), "ROBUST_MAX_K=64"),
    (dict(aggregation_rule="mean_around_median", worker_number=65), "ROBUST_MAX_K=64"),
    (dict(aggregation_rule="bulyan", aggregation_mode="fma"), "aggregation_rule='mean' only"),
    (dict(aggregation_rule="mean_around_median", aggregation_mode="fma"),
     "aggregation_rule='mean' only"),
    # the other rules keep multi-Krum's message
    (dict(byzantine=1), "byzantine=1 / krum_select=None needs aggregation_rule='multi_krum'"),
    (dict(aggregation_rule="median", byzantine=2),
     "byzantine=2 / krum_select=None needs aggregation_rule='multi_krum', not 'median'"),
    (dict(aggregation_rule="trimmed_mean", trim=1, byzantine=1),
     "needs aggregation_rule='multi_krum'"),
    (dict(aggregation_rule="geometric_median", byzantine=1), "needs aggregation_rule='multi_krum'"),
    (dict(aggregation_rule="centered_clip", byzantine=1), "needs aggregation_rule='multi_krum'"),
])
def test_fed_server_rejects(kw, what):
    """Every case raises before the GPU is needed (no doubles installed)."""
    args = dict(worker_number=10)
    args.update(kw)
    with pytest.raises(ValueError, match=what):
        _fed(**args)


@pytest.mark.parametrize("algo", ["fed_quant", "GTG_shapley_value", "multiround_shapley_value"])
@pytest.mark.parametrize("rule", ["bulyan", "mean_around_median"])
def test_other_servers_reject_the_rules(algo, rule, doubles):
    from distributed_learning_simulator_amd import factory
    with pytest.raises(ValueError, match="does not support aggregation_rule.*FedServer"):
        factory.get_server(algo, sharded=False, tester=None, worker_number=8, synchronous=True,
                           device=CPU, aggregation_rule=rule, byzantine=1)


@pytest.mark.parametrize("rule", ["bulyan", "mean_around_median"])
def test_sharded_server_rejects_the_rules(rule, doubles):
    from distributed_learning_simulator_amd import factory
    with pytest.raises(ValueError, match="does not support aggregation_rule.*FedServer"):
        factory.get_server("fed", sharded=True, tester=None, worker_number=8, synchronous=True,
                           device=CPU, aggregation_rule=rule, byzantine=1)


def _clients(n, bad):
    g = torch.Generator().manual_seed(3)
    base = {"w": torch.randn(6, 10, generator=g), "b": torch.randn(7, generator=g)}
    out = []
    for i in range(n):
        d = {k: v + 0.01 * torch.randn(v.shape, generator=g) for k, v in base.items()}
        if i in bad:
            fill = (float("inf"), float("nan"), 1e30, -1e30)[i % 4]
            d = {k: torch.full_like(v, fill) for k, v in d.items()}
            d["w"][0, 0] = -1e30
        out.append(d)
    return out


def _round(clients, order, **kw):
    server = _fed(worker_number=len(clients), **kw)
    q = server.worker_data_queue
    for w in order:
        q.add_task((w, 100 + 7 * w, clients[w]))
    for w in range(len(clients)):
        q.get_result(consumer=w)  # the initial broadcast
    agg = q.get_result(consumer=0)
    server.stop()
    return server, agg


def test_fed_server_bulyan_round_on_cpu_doubles(doubles):
    from distributed_learning_simulator_amd.layout import ParameterLayout
    bad = (2, 9)
    clients = _clients(11, bad)
    lay = ParameterLayout.from_dict(clients[0])
    X = np.stack([lay.flatten(c).numpy() for c in clients])
    server, agg = _round(clients, [4, 0, 9, 2, 7, 10, 1, 3, 8, 6, 5], aggregation_rule="bulyan",
                         byzantine=2)
    assert doubles == {"mean_around_median": 1, "pairwise_sqdist": 1}
    sel = server.last_selection
    assert isinstance(sel, tuple) and len(sel) == 7 == len(set(sel)) and not set(sel) & set(bad)
    assert set(server.last_scores) == set(sel)
    assert all(math.isfinite(s) for s in server.last_scores.values())
    assert all(torch.isfinite(v).all() for v in agg.values())
    want = M.mean_around_median_bits(X[sorted(sel)], 3)
    flat = lay.flatten(agg).numpy().view(np.uint32)
    assert np.array_equal(flat, want)
    assert np.array_equal(lay.flatten(server.prev_model).numpy().view(np.uint32), want)
    # another arrival order: the same picks in the same order, the same bits
    server2, agg2 = _round(clients, [10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0], aggregation_rule="bulyan",
                           byzantine=2)
    assert server2.last_selection == sel and server2.last_scores == server.last_scores
    assert np.array_equal(lay.flatten(agg2).numpy().view(np.uint32), want)


def test_fed_server_bulyan_without_byzantine_skips_the_distances(doubles):
    from distributed_learning_simulator_amd.layout import ParameterLayout
    clients = _clients(3, ())
    lay = ParameterLayout.from_dict(clients[0])
    X = np.stack([lay.flatten(c).numpy() for c in clients])
    server, agg = _round(clients, [2, 0, 1], aggregation_rule="bulyan")
    assert doubles == {"mean_around_median": 1, "pairwise_sqdist": 0}
    assert server.last_selection == (0, 1, 2) and server.last_scores == {}
    assert np.array_equal(lay.flatten(agg).numpy().view(np.uint32), R.trimmed_mean_bits(X, 0))


def test_fed_server_mean_around_median_round_and_subsets(doubles):
    from distributed_learning_simulator_amd.layout import ParameterLayout
    clients = _clients(10, (3, 7))
    lay = ParameterLayout.from_dict(clients[0])
    X = np.stack([lay.flatten(c).numpy() for c in clients])
    server, agg = _round(clients, [4, 0, 9, 2, 7, 1, 3, 8, 6, 5],
                         aggregation_rule="mean_around_median", byzantine=2)
    assert doubles == {"mean_around_median": 1, "pairwise_sqdist": 0}
    assert all(torch.isfinite(v).all() for v in agg.values())
    assert np.array_equal(lay.flatten(agg).numpy().view(np.uint32),
                          M.mean_around_median_bits(X, 8))
    # a subset runs the rule with its own K
    s = _fed(worker_number=10, aggregation_rule="mean_around_median", byzantine=2)
    for w in (5, 3, 0, 7, 9, 1):
        s.parameters[w] = (50 + w, clients[w])
    model = s.get_subset_model((9, 3, 0, 7, 5))
    assert np.array_equal(lay.flatten(model).numpy().view(np.uint32),
                          M.mean_around_median_bits(X[[9, 3, 0, 7, 5]], 3))
    with pytest.raises(ValueError, match="2\\*byzantine < len\\(subset\\)"):
        s.get_subset_model((0, 1, 5, 9))
    s.stop()
    s = _fed(worker_number=10, aggregation_rule="bulyan", byzantine=1)
    for w in range(8):
        s.parameters[w] = (50 + w, clients[w])
    model = s.get_subset_model((6, 3, 0, 1, 2, 5, 4))  # K = 7: theta = 5, keep = 3
    assert 3 not in s.last_selection and len(s.last_selection) == 5
    assert np.array_equal(lay.flatten(model).numpy().view(np.uint32),
                          M.mean_around_median_bits(X[sorted(s.last_selection)], 3))
    with pytest.raises(ValueError, match="4\\*byzantine \\+ 3 <= len\\(subset\\)"):
        s.get_subset_model((0, 1, 2, 4, 5, 6))
    s.stop()


def test_store_bulyan_needs_distinct_ids(doubles):
    from distributed_learning_simulator_amd.aggregation import ClientUpdateStore
    from distributed_learning_simulator_amd.layout import ParameterLayout
    store = ClientUpdateStore(ParameterLayout([("a", (64,))]), CPU, capacity=7)
    with pytest.raises(ValueError, match="one distinct id per row"):
        store.bulyan(list(range(7)), [0, 1, 2, 3, 4, 5, 5], 1)
    with pytest.raises(ValueError, match="one distinct id per row"):
        store.bulyan(list(range(7)), [0, 1, 2], 1)
    with pytest.raises(ValueError, match="4\\*byzantine \\+ 3 <= K"):
        store.bulyan(list(range(6)), list(range(6)), 1)


# ------------------------------------------------------------------ simulator
def test_simulator_flags():
    from distributed_learning_simulator_amd.simulator import get_config, server_kwargs
    base = ["--worker_number", "7", "--round", "1", "--distributed_algorithm"]
    cfg = get_config(base + ["fed", "--aggregation_rule", "bulyan", "--byzantine", "1"])
    assert (cfg.aggregation_rule, cfg.byzantine) == ("bulyan", 1)
    assert server_kwargs(cfg) == {"aggregation_mode": "exact", "aggregation_rule": "bulyan",
                                  "trim": 0, "byzantine": 1}
    cfg = get_config(base + ["fed", "--aggregation_rule", "mean_around_median", "--byzantine", "2"])
    assert server_kwargs(cfg) == {"aggregation_mode": "exact", "trim": 0, "byzantine": 2,
                                  "aggregation_rule": "mean_around_median"}
    assert server_kwargs(get_config(base + ["fed", "--aggregation_rule", "bulyan"])) == \
        {"aggregation_mode": "exact", "aggregation_rule": "bulyan", "trim": 0, "byzantine": 0}
    with pytest.raises(SystemExit):  # the vote has no mean to replace
        get_config(base + ["sign_SGD", "--aggregation_rule", "bulyan"])


def test_source_plumbing():
    """The symbol is declared, bound and part of the hashed sources."""
    from distributed_learning_simulator_amd import _native
    assert "dls_mean_around_median_f32" in _native.SIGNATURES
    assert _native.SIGNATURES["dls_mean_around_median_f32"] == \
        _native.SIGNATURES["dls_trimmed_mean_f32"]
    assert "robust.hip" in _native.CSRC_HASHED
    assert _native.lib().dls_source_hash().decode() == _native.source_hash()
