"""CPU checks of the geometric-median feature: ``aggregation.weiszfeld_weights``
against the numpy reference tests/geomedian_ref.py, the argument validation of
dls_rows_sqdist_to_f32 / dls_weiszfeld_step_f32 and their Python wrappers (all of it
runs before any device call), the servers' constructor validation, the simulator
flags and the build plumbing."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import cpu_doubles
from tests import geomedian_ref as GR

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")


def _weights(*a):
    from distributed_learning_simulator_amd.aggregation import weiszfeld_weights
    return weiszfeld_weights(*a)


# ------------------------------------------------------------------ reference
def test_reference_by_hand():
    X = np.array([[1, 2, 0, 0], [3, -1, 0, 0]], np.float32)
    z = np.array([1, -1, 0, 0], np.float32)
    assert GR.sqdist_to(X, z).tolist() == [9.0, 4.0]
    kept, w = GR.weights([9.0, 4.0], 1e-6)  # beta = 1/3, 1/2: weights 2/5, 3/5
    assert kept == [0, 1] and w.dtype == np.float32
    assert w.tolist() == [float(np.float32(0.4)), float(np.float32(0.6))]
    assert _weights([9.0, 4.0], 1e-6) == (kept, w.tolist())  # the package agrees
    # one rounding per product and per sum
    a, b = np.float32(1.0 + 2.0 ** -23), np.float32(3.0)
    got = GR.step_bits(np.array([[a], [b]], np.float32), w)
    want = np.float32(np.float32(w[0] * a) + np.float32(w[1] * b))
    assert got[0] == want.view(np.uint32)
    neg0 = np.array([[-0.0, 5.0]], np.float32)
    assert np.array_equal(GR.step_bits(neg0, [1.0]), neg0.view(np.uint32)[0])
    # the geometric median of three collinear points is the middle one
    P3 = np.zeros((3, 4))
    P3[:, 0] = [0.0, 1.0, 10.0]
    zz, obj = GR.weiszfeld64(P3, 50, 1e-9, z0=np.array([3.0, 0, 0, 0]))
    assert abs(zz[0] - 1.0) < 1e-6 and obj[-1] <= obj[0] and abs(obj[-1] - 10.0) < 1e-6


# ----------------------------------------------------------- weiszfeld_weights
def test_weights_match_the_reference():
    rng = np.random.default_rng(0)
    for K in (1, 2, 5, 17, 64):
        d2 = (rng.random(K) * 10.0 ** rng.integers(-6, 6, K)).tolist()
        for nu in (1e-6, 0.5, 3):
            kept, w = _weights(d2, nu)
            rkept, rw = GR.weights(d2, nu)
            assert kept == rkept == list(range(K))
            assert np.array_equal(np.array(w, np.float32).view(np.uint32), rw.view(np.uint32))
            # float32-representable, and a partition of one within K * 2^-24
            assert all(float(np.float32(v)) == v for v in w)
            assert abs(sum(w) - 1.0) <= K * 2.0 ** -24


def test_weights_equal_distances_and_clamp():
    kept, w = _weights([4.0] * 7, 1e-6)
    assert kept == list(range(7)) and len(set(w)) == 1 and w[0] == float(np.float32(1.0 / 7.0))
    # a zero distance is clamped by nu: beta = 1 / nu, not a division by zero
    kept, w = _weights([0.0, 1.0], 0.25)
    assert kept == [0, 1] and w == [float(np.float32(0.8)), float(np.float32(0.2))]
    kept, w = _weights([0.0, 0.0, 1e-20], 1e-6)  # all below nu: equal weights
    assert len(set(w)) == 1
    assert _weights([0.0], 1e-6) == ([0], [1.0])
    assert _weights(np.array([9.0, 4.0]), 1e-6)[1] == GR.weights([9.0, 4.0], 1e-6)[1].tolist()
    assert _weights(torch.tensor([9.0, 4.0], dtype=torch.float64), 1e-6)[0] == [0, 1]


def test_weights_drop_non_finite_and_negative():
    d2 = [1.0, INF, 4.0, NAN, -1.0, -INF, 9.0]
    kept, w = _weights(d2, 1e-6)
    assert kept == [0, 2, 6]
    assert w == _weights([1.0, 4.0, 9.0], 1e-6)[1]
    rkept, rw = GR.weights(d2, 1e-6)
    assert kept == rkept and w == rw.tolist()
    assert _weights([-0.0, NAN], 1.0) == ([0], [1.0])  # -0.0 is a distance of zero


def test_weights_value_errors():
    for d2 in ([], [NAN], [INF, -1.0, NAN]):
        with pytest.raises(ValueError, match="no client has a finite distance"):
            _weights(d2, 1e-6)
    for nu in (0, 0.0, -1e-6, INF, NAN, True, "1e-6", None):
        with pytest.raises(ValueError, match="nu must be a positive finite number"):
            _weights([1.0, 2.0], nu)


# ------------------------------------------------------------------------ ABI
def test_abi_rejects_bad_arguments_without_gpu():
    from distributed_learning_simulator_amd import _native
    L = _native.lib()
    d = ctypes.c_void_p(256)  # 16-byte aligned, never dereferenced
    odd, odd8 = ctypes.c_void_p(260), ctypes.c_void_p(264)
    err, ws = L.dls_last_error, L.dls_weiszfeld_workspace

    def dist(U=d, ldu=64, rows=d, K=3, P=64, z=d, out=d, work=d):
        return L.dls_rows_sqdist_to_f32(U, ldu, rows, K, P, z, out, work, None)

    def step(U=d, ldu=64, rows=d, K=3, w=d, P=64, z=d, out=d, work=d):
        return L.dls_weiszfeld_step_f32(U, ldu, rows, K, w, P, z, out, work, None)

    for f, name in ((dist, b"dls_rows_sqdist_to_f32"), (step, b"dls_weiszfeld_step_f32")):
        for arg in ("U", "rows", "z", "out", "work"):
            assert f(**{arg: None}) == -1 and b"null pointer" in err() and name in err()
        assert f(K=0) == -1 and b"DLS_ROBUST_MAX_K=64" in err()
        assert f(K=65) == -1 and b"DLS_ROBUST_MAX_K=64" in err()
        assert f(P=-4) == -1
        assert f(P=62) == -2 and b"multiples of 4" in err()
        assert f(ldu=60) == -2 and f(ldu=66) == -2
        for arg in ("U", "z", "work"):
            assert f(**{arg: odd}) == -2 and b"alignment" in err()
            assert f(**{arg: odd8}) == -2
        assert f(out=odd) == -2 and b"alignment" in err()
    assert step(w=None) == -1 and b"null pointer" in err()
    assert ws(0, 64) == -1 and ws(65, 64) == -1 and ws(3, -1) == -1
    # the workspace is a function of K and P alone, never empty: 512 bytes per wave
    shapes = [(K, P) for K in (1, 32, 33, 64) for P in (0, 4, 70004, 11174016)]
    sizes = {s: ws(*s) for s in shapes}
    assert all(v >= 512 and v % 512 == 0 for v in sizes.values())
    assert sizes == {s: ws(*s) for s in shapes}
    assert sizes[(64, 11174016)] <= 1 << 20 and sizes[(1, 4)] == 512


def test_wrappers_validate_before_the_library_call():
    from distributed_learning_simulator_amd import _native
    U = torch.zeros(8, 64)
    rows = torch.arange(5, dtype=torch.int32)
    z = torch.zeros(64)
    w = torch.full((5,), 0.2)
    out = torch.zeros(5, dtype=torch.float64)
    common = [
        (dict(U=U.double()), "U must be"),
        (dict(U=torch.zeros(8, 128)[:, ::2]), "U must be"),
        (dict(U=torch.zeros(64)), "U must be"),
        (dict(rows=rows.long()), "rows must be"),
        (dict(rows=torch.arange(10, dtype=torch.int32)[::2]), "rows must be"),
        (dict(P=62), "multiple of 4"),
        (dict(P=-4), "multiple of 4"),
        (dict(P=68), "row length"),
        (dict(U=torch.zeros(8, 66)[:, :64]), "row pitch"),
        (dict(z=z.double()), "z must be"),
        (dict(z=torch.zeros(60)), "z must be"),
        (dict(z=torch.zeros(128)[::2]), "z must be"),
        (dict(z=torch.zeros(64, device="meta")), "z is on meta"),
        (dict(out=torch.zeros(5)), "must be a contiguous fp64"),
        (dict(out=torch.zeros(4, dtype=torch.float64)), "must be a contiguous fp64"),
        (dict(out=torch.zeros(10, dtype=torch.float64)[::2]), "must be a contiguous fp64"),
        (dict(out=torch.zeros(5, dtype=torch.float64, device="meta")), "is on meta"),
        (dict(rows=torch.zeros(5, dtype=torch.int32, device="meta")), "rows is on meta"),
        (dict(U=torch.zeros(8 * 64 + 1)[1:].view(8, 64)), "16-byte aligned"),
        (dict(z=torch.zeros(65)[1:]), "16-byte aligned"),
    ]
    for change, what in common:
        kw = dict(U=U, rows=rows, P=64, z=z, out=out, w=w)
        kw.update(change)
        with pytest.raises(RuntimeError, match="rows_sqdist_to: .*" + what):
            _native.rows_sqdist_to(kw["U"], kw["rows"], kw["P"], kw["z"], out=kw["out"])
        with pytest.raises(RuntimeError, match="weiszfeld_step: .*" + what):
            _native.weiszfeld_step(kw["U"], kw["rows"], kw["w"], kw["P"], kw["z"], dist2=kw["out"])
    for r in (torch.zeros(0, dtype=torch.int32), torch.zeros(65, dtype=torch.int32)):
        with pytest.raises(RuntimeError, match="rows_sqdist_to: .*ROBUST_MAX_K=64"):
            _native.rows_sqdist_to(U, r, 64, z)
        with pytest.raises(RuntimeError, match="weiszfeld_step: .*ROBUST_MAX_K=64"):
            _native.weiszfeld_step(U, r, w, 64, z)
    for bad_w in (w.double(), torch.zeros(4), torch.zeros(10)[::2], torch.zeros(5, 1)):
        with pytest.raises(RuntimeError, match="weiszfeld_step: w must be"):
            _native.weiszfeld_step(U, rows, bad_w, 64, z)
    with pytest.raises(RuntimeError, match="weiszfeld_step: w is on meta"):
        _native.weiszfeld_step(U, rows, torch.zeros(5, device="meta"), 64, z)
    # valid operands reach the library, which has no CPU path
    with pytest.raises(RuntimeError, match="not on the GPU"):
        _native.rows_sqdist_to(U, rows, 64, z, out=out)
    with pytest.raises(RuntimeError, match="not on the GPU"):
        _native.weiszfeld_step(U, rows, w, 64, z)


# -------------------------------------------------------------------- servers
@pytest.fixture
def doubles(monkeypatch):
    cpu_doubles.install(monkeypatch)


def _fed(**kw):
    from distributed_learning_simulator_amd.servers.fed_server import FedServer
    return FedServer(tester=None, device=CPU, synchronous=True, **kw)


def test_fed_server_accepts_geometric_median(doubles):
    s = _fed(worker_number=10, aggregation_rule="geometric_median")
    assert (s.aggregation_rule, s.gm_iters, s.gm_nu) == ("geometric_median", 3, 1e-6)
    assert s.last_distances == {} and s.last_rejected == ()
    s.stop()
    s = _fed(worker_number=64, aggregation_rule="geometric_median", gm_iters=1, gm_nu=2)
    assert (s.gm_iters, s.gm_nu, s.trim, s.byzantine, s.krum_select) == (1, 2.0, 0, 0, None)
    s.stop()
    s = _fed(worker_number=1, aggregation_rule="geometric_median", gm_iters=10, gm_nu=1e-3)
    s.stop()
    for rule in ("mean", "median"):  # the defaults, spelled out, suit every rule
        s = _fed(worker_number=10, aggregation_rule=rule, gm_iters=3, gm_nu=1e-6)
        assert (s.aggregation_rule, s.gm_iters, s.gm_nu) == (rule, 3, 1e-6)
        s.stop()


@pytest.mark.parametrize("kw, what", [
    (dict(aggregation_rule="geomedian"), "aggregation_rule must be one of .*'geometric_median'"),
    (dict(gm_iters=5), "gm_iters=5 / gm_nu=1e-06 needs aggregation_rule='geometric_median'"),
    (dict(gm_nu=1e-3), "gm_iters=3 / gm_nu=0.001 needs aggregation_rule='geometric_median'"),
    (dict(aggregation_rule="median", gm_iters=2), "needs aggregation_rule='geometric_median'"),
    (dict(aggregation_rule="multi_krum", byzantine=1, gm_nu=1.0),
     "needs aggregation_rule='geometric_median'"),
    (dict(aggregation_rule="trimmed_mean", trim=1, gm_iters=1),
     "needs aggregation_rule='geometric_median'"),
    (dict(aggregation_rule="geometric_median", gm_iters=0), "gm_iters must be a positive integer"),
    (dict(aggregation_rule="geometric_median", gm_iters=-1), "gm_iters must be a positive integer"),
    (dict(aggregation_rule="geometric_median", gm_iters=2.0), "gm_iters must be a positive integer"),
    (dict(aggregation_rule="geometric_median", gm_iters=True), "gm_iters must be a positive integer"),
    (dict(aggregation_rule="geometric_median", gm_iters=None), "gm_iters must be a positive integer"),
    (dict(aggregation_rule="geometric_median", gm_nu=0.0), "gm_nu must be a positive finite"),
    (dict(aggregation_rule="geometric_median", gm_nu=-1e-6), "gm_nu must be a positive finite"),
    (dict(aggregation_rule="geometric_median", gm_nu=INF), "gm_nu must be a positive finite"),
    (dict(aggregation_rule="geometric_median", gm_nu=NAN), "gm_nu must be a positive finite"),
    (dict(aggregation_rule="geometric_median", gm_nu="1e-6"), "gm_nu must be a positive finite"),
    (dict(aggregation_rule="geometric_median", gm_nu=True), "gm_nu must be a positive finite"),
    (dict(aggregation_rule="geometric_median", trim=1), "trim=1 needs aggregation_rule='trimmed_mean'"),
    (dict(aggregation_rule="geometric_median", byzantine=1),
     "needs aggregation_rule='multi_krum'"),
    (dict(aggregation_rule="geometric_median", aggregation_mode="fma"),
     "aggregation_rule='mean' only"),
    (dict(aggregation_rule="geometric_median", worker_number=65), "ROBUST_MAX_K=64"),
])
def test_fed_server_rejects(kw, what):
    """Every case raises before the GPU is needed (no doubles installed)."""
    args = dict(worker_number=10)
    args.update(kw)
    with pytest.raises(ValueError, match=what):
        _fed(**args)


@pytest.mark.parametrize("algo", ["fed_quant", "GTG_shapley_value", "multiround_shapley_value"])
def test_other_servers_reject_geometric_median(algo, doubles):
    from distributed_learning_simulator_amd import factory
    with pytest.raises(ValueError, match="does not support aggregation_rule='geometric_median'"
                                         ".*FedServer"):
        factory.get_server(algo, sharded=False, tester=None, worker_number=5, synchronous=True,
                           device=CPU, aggregation_rule="geometric_median", gm_iters=2)
    with pytest.raises(ValueError, match="needs aggregation_rule='geometric_median'"):
        factory.get_server(algo, sharded=False, tester=None, worker_number=5, synchronous=True,
                           device=CPU, gm_iters=2)


@pytest.mark.parametrize("algo", ["fed", "fed_quant", "GTG_shapley_value",
                                  "multiround_shapley_value"])
def test_sharded_servers_reject_geometric_median(algo, doubles):
    from distributed_learning_simulator_amd import factory
    with pytest.raises(ValueError, match="does not support aggregation_rule='geometric_median'"
                                         ".*FedServer"):
        factory.get_server(algo, sharded=True, tester=None, worker_number=5, synchronous=True,
                           device=CPU, aggregation_rule="geometric_median")


# ------------------------------------------------------------------ simulator
def test_simulator_flags():
    from distributed_learning_simulator_amd.simulator import get_config, server_kwargs
    base = ["--worker_number", "5", "--round", "1", "--distributed_algorithm"]
    cfg = get_config(base + ["fed", "--aggregation_rule", "geometric_median"])
    assert (cfg.aggregation_rule, cfg.gm_iters, cfg.gm_nu) == ("geometric_median", 3, 1e-6)
    assert server_kwargs(cfg) == {"aggregation_mode": "exact",
                                  "aggregation_rule": "geometric_median", "trim": 0,
                                  "gm_iters": 3, "gm_nu": 1e-6}
    cfg = get_config(base + ["fed", "--aggregation_rule", "geometric_median", "--gm_iters", "5",
                             "--gm_nu", "1e-3"])
    assert server_kwargs(cfg) == {"aggregation_mode": "exact",
                                  "aggregation_rule": "geometric_median", "trim": 0,
                                  "gm_iters": 5, "gm_nu": 1e-3}
    # the other rules' dicts hold neither new key
    cfg = get_config(base + ["fed"])
    assert (cfg.gm_iters, cfg.gm_nu) == (3, 1e-6)
    assert server_kwargs(cfg) == {"aggregation_mode": "exact"}
    assert server_kwargs(get_config(base + ["fed", "--aggregation_rule", "median"])) == \
        {"aggregation_mode": "exact", "aggregation_rule": "median", "trim": 0}
    assert server_kwargs(get_config(base + ["fed", "--aggregation_rule", "trimmed_mean",
                                            "--trim", "1"])) == \
        {"aggregation_mode": "exact", "aggregation_rule": "trimmed_mean", "trim": 1}
    assert server_kwargs(get_config(base + ["fed", "--aggregation_rule", "multi_krum",
                                            "--byzantine", "1"])) == \
        {"aggregation_mode": "exact", "aggregation_rule": "multi_krum", "trim": 0,
         "byzantine": 1, "krum_select": None}
    assert server_kwargs(get_config(base + ["sign_SGD"])) == {}
    with pytest.raises(SystemExit):
        get_config(base + ["fed", "--aggregation_rule", "geomedian"])
    with pytest.raises(SystemExit):
        get_config(base + ["fed", "--aggregation_rule", "geometric_median", "--gm_iters", "three"])
    with pytest.raises(SystemExit):  # the vote has no mean to replace
        get_config(base + ["sign_SGD", "--aggregation_rule", "geometric_median"])
    from distributed_learning_simulator_amd import simulator
    assert "--aggregation_rule geometric_median" in simulator.__doc__


# ------------------------------------------------------------ source plumbing
def test_source_plumbing():
    from distributed_learning_simulator_amd import _native
    csrc = os.path.join(ROOT, "distributed_learning_simulator_amd", "csrc")
    with open(os.path.join(csrc, "Makefile")) as fh:
        srcs = next(line for line in fh if line.startswith("SRCS :=")).split()[2:]
    assert "weiszfeld.hip" in srcs
    assert _native.CSRC_HASHED[:len(srcs)] == srcs
    with open(os.path.join(ROOT, "include", "dls_hip.h")) as fh:
        header = fh.read()
    assert "int64_t dls_weiszfeld_workspace(int32_t K, int64_t P);" in header
    assert "int dls_rows_sqdist_to_f32(const float *U, int64_t ldu, const int32_t *rows" in header
    assert "int dls_weiszfeld_step_f32(const float *U, int64_t ldu, const int32_t *rows" in header
    assert "#define DLS_ABI_VERSION 2" in header
    L = _native.lib()
    for name in ("dls_weiszfeld_workspace", "dls_rows_sqdist_to_f32", "dls_weiszfeld_step_f32"):
        assert name in _native.SIGNATURES and hasattr(L, name)
    with open(os.path.join(csrc, "weiszfeld.hip")) as fh:
        src = fh.read()
    assert "getenv" not in src and "atomic" not in src.lower().replace("no atomics", "")
