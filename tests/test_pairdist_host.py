"""CPU checks of the pairwise-distance / multi-Krum feature: the numpy reference the
GPU tests compare with, ``aggregation.multi_krum_select``, the argument validation of
dls_pairwise_sqdist_f32 and its Python wrapper (both run before any device call),
the servers' constructor validation, the simulator flags and the build plumbing."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import cpu_doubles
from tests import pairdist_ref as PR

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")


# ------------------------------------------------------------------ reference
def test_reference_three_points_by_hand():
    X = np.array([[0, 0, 0, 0], [3, 4, 0, 0], [0, 0, 0, 1]], np.float32)
    assert PR.sqdist(X).tolist() == [[0.0, 25.0, 1.0], [25.0, 0.0, 26.0], [1.0, 26.0, 0.0]]
    # f = 0: K - f - 2 = 1 nearest neighbour each
    assert PR.krum_scores(PR.sqdist(X), 0).tolist() == [1.0, 25.0, 1.0]
    sel, scores, bits = PR.multi_krum_ref(X, [7, 5, 2], 0, 2)
    assert sel == [2, 7] and scores == {7: 1.0, 5: 25.0, 2: 1.0}  # the tie goes to the lower id
    assert np.array_equal(bits, np.array([0, 0, 0, 0.5], np.float32).view(np.uint32))


def test_reference_five_points_by_hand():
    # points on a line at 0, 1, 2, 4 and 100
    X = np.zeros((5, 4), np.float32)
    X[:, 0] = [0, 1, 2, 4, 100]
    D = PR.sqdist(X)
    assert D[0].tolist() == [0.0, 1.0, 4.0, 16.0, 10000.0]
    assert D[3].tolist() == [16.0, 9.0, 4.0, 0.0, 9216.0]
    # f = 1: the 2 nearest neighbours: 1+4, 1+1, 1+4, 4+9, 96^2+98^2
    assert PR.krum_scores(D, 1).tolist() == [5.0, 2.0, 5.0, 13.0, 9216.0 + 9604.0]
    sel, _, bits = PR.multi_krum_ref(X, [0, 1, 2, 3, 4], 1, 4)
    assert sel == [1, 0, 2, 3]
    assert bits[0] == np.float32(7.0 / 4.0).view(np.uint32)
    sel1, _, bits1 = PR.multi_krum_ref(X, [0, 1, 2, 3, 4], 1, 1)
    assert sel1 == [1] and np.array_equal(bits1, X[1].view(np.uint32))  # Krum: the row's bits


def test_reference_non_finite_rows():
    X = np.ones((4, 4), np.float32)
    X[1, 2] = np.inf
    X[2, 0] = np.nan
    D = PR.sqdist(X)
    assert D[0, 3] == 0.0 and D[0, 1] == np.inf and np.isnan(D[0, 2]) and not np.isfinite(D[1, 2])
    assert (np.diag(D) == 0).all()


# ---------------------------------------------------------- multi_krum_select
def _select(*a):
    from distributed_learning_simulator_amd.aggregation import multi_krum_select
    return multi_krum_select(*a)


def _line(points):
    X = np.zeros((len(points), 4), np.float32)
    X[:, 0] = points
    return X


def test_select_rejects_an_outlier_and_matches_the_reference():
    X = _line([0, 1, 2, 4, 100])
    ids = [10, 11, 12, 13, 14]
    sel, scores = _select(PR.sqdist(X), ids, 1, 4)
    assert sel == [11, 10, 12, 13] and 14 not in sel
    assert scores == [5.0, 2.0, 5.0, 13.0, 18820.0]
    want, wscores, _ = PR.multi_krum_ref(X, ids, 1, 4)
    assert sel == want and dict(zip(ids, scores)) == wscores
    assert _select(PR.sqdist(X).tolist(), ids, 1, 1)[0] == [11]  # nested lists do as well
    rng = np.random.default_rng(0)
    Y = rng.standard_normal((9, 64)).astype(np.float32)
    Y[4] += 30.0
    for f, m in ((0, 9), (1, 8), (3, 1), (3, 6)):
        sel, scores = _select(PR.sqdist(Y), list(range(9)), f, m)
        want, wscores, _ = PR.multi_krum_ref(Y, list(range(9)), f, m)
        assert sel == want and 4 not in sel[:8]
        assert np.allclose(scores, [wscores[i] for i in range(9)], rtol=1e-12)


def test_select_maps_non_finite_entries_to_inf():
    D = PR.sqdist(_line([0, 1, 2, 4, 5]))
    D[4, :4] = [NAN, INF, -INF, NAN]
    D[:4, 4] = [NAN, INF, -INF, NAN]
    sel, scores = _select(D, [0, 1, 2, 3, 4], 1, 4)
    assert scores[4] == INF and all(np.isfinite(scores[:4])) and sel == [1, 0, 2, 3]
    # the bad distance is each clean client's largest: it never enters their scores
    assert scores[:4] == [5.0, 2.0, 5.0, 13.0]
    with pytest.raises(ValueError, match="fewer than select=4 clients have a finite score"):
        D2 = D.copy()
        D2[3, :3] = D2[:3, 3] = NAN  # now clients 3 and 4 are both at +inf from everyone
        _select(D2, [0, 1, 2, 3, 4], 1, 4)


def test_select_breaks_ties_by_id_not_by_arrival():
    # clients 20 and 3 hold the same update: identical rows of D, identical scores
    X = _line([1, 0, 1, 2, 50, 3])
    ids = [20, 8, 3, 5, 9, 6]
    D = PR.sqdist(X)
    sel, scores = _select(D, ids, 1, 1)
    assert scores[0] == scores[2] and sel == [3]
    first = _select(D, ids, 1, 4)
    rng = np.random.default_rng(1)
    for _ in range(5):
        p = rng.permutation(6)
        sel_p, scores_p = _select(D[np.ix_(p, p)], [ids[k] for k in p], 1, 4)
        assert sel_p == first[0]
        assert dict(zip([ids[k] for k in p], scores_p)) == dict(zip(ids, first[1]))


@pytest.mark.parametrize("K, f, m, what", [
    (4, 1, 1, "2\\*byzantine \\+ 3 <= K"),
    (2, 0, 1, "2\\*byzantine \\+ 3 <= K"),
    (5, 1, 0, "select=0 must be in 1\\.\\.K - byzantine = 4"),
    (5, 1, 5, "select=5 must be in 1\\.\\.K - byzantine = 4"),
])
def test_select_value_errors(K, f, m, what):
    D = PR.sqdist(_line(list(range(K))))
    with pytest.raises(ValueError, match=what):
        _select(D, list(range(K)), f, m)
    with pytest.raises(ValueError, match="D must be"):
        _select(D[:, :-1], list(range(K)), 0, 1)


# ------------------------------------------------------------------------ ABI
def test_abi_rejects_bad_arguments_without_gpu():
    from distributed_learning_simulator_amd import _native
    L = _native.lib()
    d = ctypes.c_void_p(256)  # 16-byte aligned, never dereferenced
    f, ws, err = L.dls_pairwise_sqdist_f32, L.dls_pairwise_sqdist_workspace, L.dls_last_error
    for U, rows, D, work in ((None, d, d, d), (d, None, d, d), (d, d, None, d), (d, d, d, None)):
        assert f(U, 64, rows, 3, 64, D, work, None) == -1 and b"null pointer" in err()
    assert f(d, 64, d, 0, 64, d, d, None) == -1 and b"DLS_ROBUST_MAX_K=64" in err()
    assert f(d, 64, d, 65, 64, d, d, None) == -1 and b"DLS_ROBUST_MAX_K=64" in err()
    assert f(d, 64, d, 3, -4, d, d, None) == -1
    assert f(d, 64, d, 3, 62, d, d, None) == -2 and b"multiples of 4" in err()
    assert f(d, 60, d, 3, 64, d, d, None) == -2
    assert f(d, 66, d, 3, 64, d, d, None) == -2
    assert f(ctypes.c_void_p(260), 64, d, 3, 64, d, d, None) == -2 and b"alignment" in err()
    assert f(d, 64, d, 3, 64, ctypes.c_void_p(260), d, None) == -2 and b"alignment" in err()
    assert ws(0, 64) == -1 and ws(65, 64) == -1 and ws(3, -1) == -1
    # the workspace is a function of K and P alone, and never empty
    sizes = {(K, P): ws(K, P) for K in (1, 8, 9, 64) for P in (0, 4, 70004, 11174016)}
    assert all(v >= 32768 and v % 32768 == 0 for v in sizes.values())
    assert sizes == {(K, P): ws(K, P) for K in (1, 8, 9, 64) for P in (0, 4, 70004, 11174016)}
    assert sizes[(64, 11174016)] <= 64 << 20


def test_wrapper_validates_before_the_library_call():
    from distributed_learning_simulator_amd import _native
    U = torch.zeros(8, 64)
    rows = torch.arange(5, dtype=torch.int32)
    out = torch.zeros(5, 5, dtype=torch.float64)
    bad = [
        (dict(U=U.double()), "U must be"),
        (dict(U=torch.zeros(8, 128)[:, ::2]), "U must be"),
        (dict(U=torch.zeros(64)), "U must be"),
        (dict(rows=rows.long()), "rows must be"),
        (dict(rows=torch.arange(10, dtype=torch.int32)[::2]), "rows must be"),
        (dict(rows=torch.zeros(0, dtype=torch.int32)), "ROBUST_MAX_K"),
        (dict(rows=torch.zeros(65, dtype=torch.int32)), "ROBUST_MAX_K=64"),
        (dict(P=62), "multiple of 4"),
        (dict(P=-4), "multiple of 4"),
        (dict(P=68), "row length"),
        (dict(U=torch.zeros(8, 66)[:, :64]), "row pitch"),
        (dict(out=torch.zeros(5, 5)), "out must be"),
        (dict(out=torch.zeros(4, 5, dtype=torch.float64)), "out must be"),
        (dict(out=torch.zeros(5, 10, dtype=torch.float64)[:, ::2]), "out must be"),
        (dict(out=torch.zeros(5, 5, dtype=torch.float64, device="meta")), "out is on meta"),
        (dict(rows=torch.zeros(5, dtype=torch.int32, device="meta")), "rows is on meta"),
        (dict(U=torch.zeros(8 * 64 + 1)[1:].view(8, 64)), "16-byte aligned"),
    ]
    for change, what in bad:
        kw = dict(U=U, rows=rows, P=64, out=out)
        kw.update(change)
        with pytest.raises(RuntimeError, match="pairwise_sqdist: .*" + what):
            _native.pairwise_sqdist(kw["U"], kw["rows"], kw["P"], out=kw["out"])
    # valid operands reach the library, which has no CPU path
    with pytest.raises(RuntimeError, match="not on the GPU"):
        _native.pairwise_sqdist(U, rows, 64, out=out)
    with pytest.raises(RuntimeError, match="not on the GPU"):
        _native.pairwise_sqdist(U, rows, 64)


# -------------------------------------------------------------------- servers
@pytest.fixture
def doubles(monkeypatch):
    cpu_doubles.install(monkeypatch)


def _fed(**kw):
    from distributed_learning_simulator_amd.servers.fed_server import FedServer
    return FedServer(tester=None, device=CPU, synchronous=True, **kw)


def test_fed_server_accepts_multi_krum(doubles):
    s = _fed(worker_number=10, aggregation_rule="multi_krum", byzantine=2)
    assert (s.aggregation_rule, s.byzantine, s.krum_select) == ("multi_krum", 2, None)
    assert s.last_selection == () and s.last_scores == {}
    s.stop()
    s = _fed(worker_number=7, aggregation_rule="multi_krum", byzantine=2, krum_select=1)
    assert (s.byzantine, s.krum_select, s.trim) == (2, 1, 0)
    s.stop()
    s = _fed(worker_number=64, aggregation_rule="multi_krum", byzantine=30, krum_select=34)
    s.stop()
    s = _fed(worker_number=3, aggregation_rule="multi_krum")  # f = 0 is allowed
    s.stop()
    s = _fed(worker_number=10)  # the defaults of the other rules are untouched
    assert (s.aggregation_rule, s.trim, s.byzantine, s.krum_select) == ("mean", 0, 0, None)
    s.stop()


@pytest.mark.parametrize("kw, what", [
    (dict(aggregation_rule="krum"), "aggregation_rule must be one of"),
    (dict(aggregation_rule="multi_krum", byzantine=-1), "byzantine must be a non-negative integer"),
    (dict(aggregation_rule="multi_krum", byzantine=1.0), "byzantine must be a non-negative integer"),
    (dict(aggregation_rule="multi_krum", byzantine=True), "byzantine must be a non-negative integer"),
    (dict(aggregation_rule="multi_krum", krum_select=True), "krum_select must be an integer"),
    (dict(aggregation_rule="multi_krum", krum_select=2.0), "krum_select must be an integer"),
    (dict(byzantine=1), "byzantine=1 / krum_select=None needs aggregation_rule='multi_krum'"),
    (dict(aggregation_rule="median", krum_select=3),
     "byzantine=0 / krum_select=3 needs aggregation_rule='multi_krum'"),
    (dict(aggregation_rule="trimmed_mean", trim=1, byzantine=2),
     "byzantine=2 / krum_select=None needs aggregation_rule='multi_krum'"),
    (dict(aggregation_rule="multi_krum", trim=1), "trim=1 needs aggregation_rule='trimmed_mean'"),
    (dict(aggregation_rule="multi_krum", byzantine=4), "2\\*byzantine \\+ 3 <= worker_number"),
    (dict(aggregation_rule="multi_krum", worker_number=2), "2\\*byzantine \\+ 3 <= worker_number"),
    (dict(aggregation_rule="multi_krum", byzantine=2, krum_select=0),
     "krum_select=0 must be in 1\\.\\.worker_number - byzantine = 8"),
    (dict(aggregation_rule="multi_krum", byzantine=2, krum_select=9),
     "krum_select=9 must be in 1\\.\\.worker_number - byzantine = 8"),
    (dict(aggregation_rule="multi_krum", worker_number=65), "ROBUST_MAX_K=64"),
    (dict(aggregation_rule="multi_krum", aggregation_mode="fma"), "aggregation_rule='mean' only"),
])
def test_fed_server_rejects(kw, what):
    """Every case raises before the GPU is needed (no doubles installed)."""
    args = dict(worker_number=10)
    args.update(kw)
    with pytest.raises(ValueError, match=what):
        _fed(**args)


def test_subset_too_small_for_byzantine(doubles):
    s = _fed(worker_number=10, aggregation_rule="multi_krum", byzantine=2)
    for w in range(6):
        s.parameters[w] = (10, {"w": torch.full((4, 4), float(w))})
    with pytest.raises(ValueError, match="2\\*byzantine \\+ 3 <= len\\(subset\\)"):
        s.get_subset_model([0, 1, 2, 3, 4, 5])
    s.stop()


@pytest.mark.parametrize("algo", ["fed_quant", "GTG_shapley_value", "multiround_shapley_value"])
def test_other_servers_reject_multi_krum(algo, doubles):
    from distributed_learning_simulator_amd import factory
    with pytest.raises(ValueError, match="does not support aggregation_rule.*FedServer"):
        factory.get_server(algo, sharded=False, tester=None, worker_number=5, synchronous=True,
                           device=CPU, aggregation_rule="multi_krum", byzantine=1)
    with pytest.raises(ValueError, match="needs aggregation_rule='multi_krum'"):
        factory.get_server(algo, sharded=False, tester=None, worker_number=5, synchronous=True,
                           device=CPU, byzantine=1)


@pytest.mark.parametrize("algo", ["fed", "fed_quant", "GTG_shapley_value",
                                  "multiround_shapley_value"])
def test_sharded_servers_reject_multi_krum(algo, doubles):
    from distributed_learning_simulator_amd import factory
    with pytest.raises(ValueError, match="does not support aggregation_rule.*FedServer"):
        factory.get_server(algo, sharded=True, tester=None, worker_number=5, synchronous=True,
                           device=CPU, aggregation_rule="multi_krum")


# ------------------------------------------------------------------ simulator
def test_simulator_flags():
    from distributed_learning_simulator_amd.simulator import get_config, server_kwargs
    base = ["--worker_number", "5", "--round", "1", "--distributed_algorithm"]
    cfg = get_config(base + ["fed", "--aggregation_rule", "multi_krum", "--byzantine", "1"])
    assert (cfg.aggregation_rule, cfg.byzantine, cfg.krum_select) == ("multi_krum", 1, None)
    assert server_kwargs(cfg) == {"aggregation_mode": "exact", "aggregation_rule": "multi_krum",
                                  "trim": 0, "byzantine": 1, "krum_select": None}
    cfg = get_config(base + ["fed", "--aggregation_rule", "multi_krum", "--byzantine", "1",
                             "--krum_select", "1"])
    assert server_kwargs(cfg) == {"aggregation_mode": "exact", "aggregation_rule": "multi_krum",
                                  "trim": 0, "byzantine": 1, "krum_select": 1}
    # the other rules' dicts hold neither new key
    cfg = get_config(base + ["fed"])
    assert (cfg.byzantine, cfg.krum_select) == (0, None)
    assert server_kwargs(cfg) == {"aggregation_mode": "exact"}
    assert server_kwargs(get_config(base + ["fed", "--aggregation_rule", "median"])) == \
        {"aggregation_mode": "exact", "aggregation_rule": "median", "trim": 0}
    assert server_kwargs(get_config(base + ["fed", "--aggregation_rule", "trimmed_mean",
                                            "--trim", "1"])) == \
        {"aggregation_mode": "exact", "aggregation_rule": "trimmed_mean", "trim": 1}
    assert server_kwargs(get_config(base + ["sign_SGD"])) == {}
    with pytest.raises(SystemExit):
        get_config(base + ["fed", "--aggregation_rule", "krum"])
    with pytest.raises(SystemExit):
        get_config(base + ["fed", "--aggregation_rule", "multi_krum", "--byzantine", "one"])
    with pytest.raises(SystemExit):  # the vote has no mean to replace
        get_config(base + ["sign_SGD", "--aggregation_rule", "multi_krum"])


# ------------------------------------------------------------ source plumbing
def test_source_plumbing():
    from distributed_learning_simulator_amd import _native
    csrc = os.path.join(ROOT, "distributed_learning_simulator_amd", "csrc")
    with open(os.path.join(csrc, "Makefile")) as fh:
        srcs = next(line for line in fh if line.startswith("SRCS :=")).split()[2:]
    assert srcs[srcs.index("robust.hip") + 1] == "pairdist.hip"
    hashed = _native.CSRC_HASHED
    assert hashed[hashed.index("robust.hip") + 1] == "pairdist.hip"
    assert hashed[:len(srcs)] == srcs
    with open(os.path.join(ROOT, "include", "dls_hip.h")) as fh:
        header = fh.read()
    assert "int64_t dls_pairwise_sqdist_workspace(int32_t K, int64_t P);" in header
    assert "int dls_pairwise_sqdist_f32(const float *U, int64_t ldu, const int32_t *rows" in header
    assert "#define DLS_ABI_VERSION 2" in header
    for name in ("dls_pairwise_sqdist_workspace", "dls_pairwise_sqdist_f32"):
        assert name in _native.SIGNATURES
    with open(os.path.join(csrc, "pairdist.hip")) as fh:
        assert "getenv" not in fh.read()


# ------------------------------------------------------------------ the launch plan
def test_launch_shape_constant_matches_the_header():
    import re
    from distributed_learning_simulator_amd import _native
    with open(os.path.join(ROOT, "include", "dls_hip.h")) as fh:
        macros = dict(re.findall(r"#define DLS_PAIRDIST_(\w+) (\d+)", fh.read()))
    assert {k: int(v) for k, v in macros.items()} == {"MAX_WAVES": _native.PAIRDIST_MAX_WAVES}


def test_reference_integer_rows_are_exact():
    """sqdist_int against the term-by-term sum in Python integers, and against sqdist."""
    X = PR.int_rows(5, 1000, seed=0)
    assert X.dtype == np.int8 and X.min() == -8 and X.max() == 8
    assert (X[0] % 2 == 0).all() and (X[1] % 2 != 0).all()
    want = [[sum((int(x) - int(y)) ** 2 for x, y in zip(a, b)) for b in X] for a in X]
    D = PR.sqdist_int(X, block=300)  # several blocks, a ragged last one
    assert D.dtype == np.float64 and D.tolist() == want
    assert np.array_equal(D, PR.sqdist(X.astype(np.float32))) and D[0, 1] >= 1000


def test_plan_model_matches_the_workspace_query():
    """pairdist_ref.plan against dls_pairwise_sqdist_workspace (a host function) for every
    grid, on both sides of each multiple of the wave cap."""
    from distributed_learning_simulator_amd import _native
    ws = _native.lib().dls_pairwise_sqdist_workspace
    W = _native.PAIRDIST_MAX_WAVES
    assert [PR.period(K) for K in (1, 8, 9, 16, 17, 32, 33, 64)] == \
        [7680, 7680, 1920, 1920, 448, 448, 96, 96]
    for K in (1, 2, 8, 9, 16, 17, 32, 33, 64):
        per = PR.period(K)
        sizes = {0, 4, per - 4, per, per + 4, 70004, 11_173_964}
        for n in (W - 1, W, W + 1, 2 * W - 1, 2 * W, 2 * W + 1, 3 * W, 3 * W + 1):
            sizes |= {n * per - 4, n * per, n * per + 4}
        for P in sorted(sizes):
            assert ws(K, P) == PR.workspace_bytes(K, P), (K, P)
            _, periods, ppw, nW = PR.plan(K, P)
            assert nW <= W and ppw * nW >= periods and (ppw - 1) * nW < periods
        assert [PR.plan(K, W * per + d)[2] for d in (0, 4)] == [1, 2]
        assert [PR.plan(K, 2 * W * per + d)[2] for d in (0, 4)] == [2, 3]
    assert PR.plan(9, 11_173_964) == (1920, 5820, 3, 1940)
    assert PR.plan(17, 920004)[1:3] == (2054, 2) and PR.plan(64, 200004)[1:3] == (2084, 2)


def test_scale_shapes_reach_the_paths_they_are_named_for():
    """One shape per block grid with several periods per wave and a tail that ends inside
    a tile: a change to the cap or the tile geometry fails here, not by silently
    un-testing the GPU path."""
    assert [PR.block_grid(K) for K, _ in PR.SCALE_SHAPES] == [1, 2, 4, 8]
    for (K, P), ppw in zip(PR.SCALE_SHAPES, PR.SCALE_PPW):
        per, periods, got, nW = PR.plan(K, P)
        assert got == ppw >= 2 and P % 4 == 0 and P % PR.tile(K) != 0
        assert nW < periods  # some wave does take a second period
    assert sorted(PR.SCALE_PPW) == [2, 2, 3, 3]
    assert PR.SCALE_SHAPES[1] == (9, 11_173_964)
    # "just over": one period less and the wave count is back under the cap's multiple
    for (K, P), ppw in zip(PR.SCALE_SHAPES, PR.SCALE_PPW):
        if K != 9:
            assert PR.plan(K, P - PR.period(K))[2] == ppw - 1
