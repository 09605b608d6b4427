"""CPU checks of the centered-clipping feature: ``aggregation.clip_scales`` against the
numpy reference tests/centered_clip_ref.py, the argument validation of
dls_centered_clip_step_f32 and its Python wrapper (all of it runs before any device
call), the servers' constructor validation, the simulator flags and the build
plumbing."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import centered_clip_ref as CR
from tests import cpu_doubles

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")


def _scales(*a):
    from distributed_learning_simulator_amd.aggregation import clip_scales
    return clip_scales(*a)


# ------------------------------------------------------------------ reference
def test_reference_by_hand():
    X = np.array([[4, 0, 0, 0], [0, 3, 0, 0]], np.float32)
    z = np.zeros(4, np.float32)
    assert CR.sqdist_to(X, z).tolist() == [16.0, 9.0]
    kept, s, c = CR.scales([16.0, 9.0], 3.0)  # distances 4 and 3: 3/4 and 1
    assert kept == [0, 1] and s.tolist() == [0.75, 1.0] and c.dtype == np.float32
    assert c.tolist() == [0.375, 0.5]
    assert _scales([16.0, 9.0], 3.0) == (kept, s.tolist(), c.tolist())  # the package agrees
    # both clipped differences have length tau = 3: the step is their mean
    got = CR.step_bits(X, c, z).view(np.float32)
    assert got.tolist() == [1.5, 1.5, 0.0, 0.0]
    # one rounding per difference, product, sum and the final add
    a, b, z0 = np.float32(1.0 + 2.0 ** -23), np.float32(3.0), np.float32(0.1)
    c2 = np.array([0.3, 0.7], np.float32)
    got = CR.step_bits(np.array([[a], [b]], np.float32), c2, np.array([z0], np.float32))
    want = np.float32(z0 + np.float32(np.float32(c2[0] * np.float32(a - z0))
                                      + np.float32(c2[1] * np.float32(b - z0))))
    assert got[0] == want.view(np.uint32)
    # fp64: one far client moves the iterate by tau / K per step and no further
    Y = np.zeros((4, 4))
    Y[3, 0] = 1e6
    v, ss, moved = CR.centered_clip64(Y, np.zeros(4), 2.0, 3)
    assert ss[0].tolist() == [1.0, 1.0, 1.0, 2.0 / 1e6] and abs(moved[0] - 0.5) < 1e-12
    assert 0 < v[0] < 1.5 and all(m <= 0.5 + 1e-12 for m in moved)
    # everyone inside the radius: one step is the mean
    v, ss, _ = CR.centered_clip64(X, np.zeros(4), 5.0, 1)
    assert v.tolist() == [2.0, 1.5, 0.0, 0.0] and ss[0].tolist() == [1.0, 1.0]


# ---------------------------------------------------------------- clip_scales
def test_scales_match_the_reference():
    rng = np.random.default_rng(0)
    for K in (1, 2, 5, 17, 64):
        d2 = (rng.random(K) * 10.0 ** rng.integers(-6, 6, K)).tolist()
        for tau in (1e-3, 0.5, 3, 1e4):
            kept, s, c = _scales(d2, tau)
            rkept, rs, rc = CR.scales(d2, tau)
            assert kept == rkept == list(range(K))
            assert np.array_equal(np.array(s).view(np.uint64), rs.view(np.uint64))
            assert np.array_equal(np.array(c, np.float32).view(np.uint32), rc.view(np.uint32))
            assert all(float(np.float32(v)) == v for v in c)  # float32-representable
            assert all(0.0 < v <= 1.0 for v in s)
            assert all(type(v) is float for v in s) and all(type(v) is float for v in c)


def test_scales_inside_on_and_outside_the_radius():
    # distances 1 (inside), 2 (on the radius: not clipped), 4 (outside) and 0
    kept, s, c = _scales([1.0, 4.0, 16.0, 0.0], 2.0)
    assert kept == [0, 1, 2, 3] and s == [1.0, 1.0, 0.5, 1.0]
    assert c == [0.25, 0.25, 0.125, 0.25]
    kept, s, c = _scales([0.0], 1e-6)
    assert (kept, s, c) == ([0], [1.0], [1.0])
    kept, s, c = _scales([9.0] * 3, 1)  # an int radius; 1/9 rounded to fp32
    assert s == [1.0 / 3.0] * 3 and c == [float(np.float32(1.0 / 9.0))] * 3
    assert _scales(np.array([16.0, 9.0]), 3.0)[1] == [0.75, 1.0]
    assert _scales(torch.tensor([16.0, 9.0], dtype=torch.float64), 3.0)[0] == [0, 1]
    # just outside: tau / d, not 1
    d = 2.0 * (1.0 + 2.0 ** -40)
    assert _scales([d * d], 2.0)[1][0] < 1.0


def test_scales_drop_non_finite_and_negative():
    d2 = [1.0, INF, 4.0, NAN, -1.0, -INF, 16.0]
    kept, s, c = _scales(d2, 2.0)
    assert kept == [0, 2, 6] and s == [1.0, 1.0, 0.5]
    assert c == _scales([1.0, 4.0, 16.0], 2.0)[2]  # divided by the number kept
    rkept, rs, rc = CR.scales(d2, 2.0)
    assert kept == rkept and s == rs.tolist() and c == rc.tolist()
    assert _scales([-0.0, NAN], 1.0) == ([0], [1.0], [1.0])  # -0.0 is a distance of zero


def test_scales_value_errors():
    for d2 in ([], [NAN], [INF, -1.0, NAN]):
        with pytest.raises(ValueError, match="no client has a finite distance"):
            _scales(d2, 1.0)
    for tau in (0, 0.0, -1e-6, INF, NAN, True, "1.0", None):
        with pytest.raises(ValueError, match="tau must be a positive finite number"):
            _scales([1.0, 2.0], tau)


# ------------------------------------------------------------------------ ABI
def test_abi_rejects_bad_arguments_without_gpu():
    from distributed_learning_simulator_amd import _native
    L = _native.lib()
    d = ctypes.c_void_p(256)  # 16-byte aligned, never dereferenced
    odd, odd8 = ctypes.c_void_p(260), ctypes.c_void_p(264)
    err = L.dls_last_error
    name = b"dls_centered_clip_step_f32"

    def step(U=d, ldu=64, rows=d, K=3, c=d, P=64, z=d, out=d, work=d):
        return L.dls_centered_clip_step_f32(U, ldu, rows, K, c, P, z, out, work, None)

    for arg in ("U", "rows", "c", "z", "out", "work"):
        assert step(**{arg: None}) == -1 and b"null pointer" in err() and name in err()
    assert step(K=0) == -1 and b"DLS_ROBUST_MAX_K=64" in err() and name in err()
    assert step(K=65) == -1 and b"DLS_ROBUST_MAX_K=64" in err() and name in err()
    assert step(P=-4) == -1 and name in err()
    assert step(P=62) == -2 and b"multiples of 4" in err() and name in err()
    assert step(ldu=60) == -2 and name in err()
    assert step(ldu=66) == -2 and name in err()
    for arg in ("U", "z", "work"):
        assert step(**{arg: odd}) == -2 and b"alignment" in err() and name in err()
        assert step(**{arg: odd8}) == -2
    assert step(out=odd) == -2 and b"alignment" in err() and name in err()
    assert step(c=ctypes.c_void_p(258)) == -2 and b"alignment" in err()


def test_wrapper_validates_before_the_library_call():
    from distributed_learning_simulator_amd import _native
    U = torch.zeros(8, 64)
    rows = torch.arange(5, dtype=torch.int32)
    z = torch.zeros(64)
    c = torch.full((5,), 0.2)
    out = torch.zeros(5, dtype=torch.float64)
    cases = [
        (dict(U=U.double()), "U must be"),
        (dict(U=torch.zeros(8, 128)[:, ::2]), "U must be"),
        (dict(U=torch.zeros(64)), "U must be"),
        (dict(rows=rows.long()), "rows must be"),
        (dict(rows=torch.arange(10, dtype=torch.int32)[::2]), "rows must be"),
        (dict(rows=torch.zeros(0, dtype=torch.int32)), "ROBUST_MAX_K=64"),
        (dict(rows=torch.zeros(65, dtype=torch.int32)), "ROBUST_MAX_K=64"),
        (dict(P=62), "multiple of 4"),
        (dict(P=-4), "multiple of 4"),
        (dict(P=68), "row length"),
        (dict(U=torch.zeros(8, 66)[:, :64]), "row pitch"),
        (dict(c=c.double()), "c must be"),
        (dict(c=torch.zeros(4)), "c must be"),
        (dict(c=torch.zeros(10)[::2]), "c must be"),
        (dict(c=torch.zeros(5, 1)), "c must be"),
        (dict(c=torch.zeros(5, device="meta")), "c is on meta"),
        (dict(z=z.double()), "z must be"),
        (dict(z=torch.zeros(60)), "z must be"),
        (dict(z=torch.zeros(128)[::2]), "z must be"),
        (dict(z=torch.zeros(64, device="meta")), "z is on meta"),
        (dict(out=torch.zeros(5)), "dist2 must be a contiguous fp64"),
        (dict(out=torch.zeros(4, dtype=torch.float64)), "dist2 must be a contiguous fp64"),
        (dict(out=torch.zeros(10, dtype=torch.float64)[::2]), "dist2 must be a contiguous fp64"),
        (dict(out=torch.zeros(5, dtype=torch.float64, device="meta")), "dist2 is on meta"),
        (dict(rows=torch.zeros(5, dtype=torch.int32, device="meta")), "rows is on meta"),
        (dict(U=torch.zeros(8 * 64 + 1)[1:].view(8, 64)), "16-byte aligned"),
        (dict(z=torch.zeros(65)[1:]), "16-byte aligned"),
    ]
    for change, what in cases:
        kw = dict(U=U, rows=rows, P=64, z=z, out=out, c=c)
        kw.update(change)
        with pytest.raises(RuntimeError, match="centered_clip_step: .*" + what):
            _native.centered_clip_step(kw["U"], kw["rows"], kw["c"], kw["P"], kw["z"],
                                       dist2=kw["out"])
    # valid operands reach the library, which has no CPU path
    with pytest.raises(RuntimeError, match="not on the GPU"):
        _native.centered_clip_step(U, rows, c, 64, z)
    with pytest.raises(RuntimeError, match="not on the GPU"):
        _native.centered_clip_step(U, rows, c, 64, z, dist2=out)


# -------------------------------------------------------------------- servers
@pytest.fixture
def doubles(monkeypatch):
    cpu_doubles.install(monkeypatch)


def _fed(**kw):
    from distributed_learning_simulator_amd.servers.fed_server import FedServer
    return FedServer(tester=None, device=CPU, synchronous=True, **kw)


def test_fed_server_accepts_centered_clip(doubles):
    s = _fed(worker_number=10, aggregation_rule="centered_clip")
    assert (s.aggregation_rule, s.cc_tau, s.cc_iters) == ("centered_clip", 10.0, 3)
    assert s.last_distances == {} and s.last_rejected == () and s.last_clip_scales == {}
    assert (s.gm_iters, s.gm_nu, s.trim, s.byzantine, s.krum_select) == (3, 1e-6, 0, 0, None)
    s.stop()
    s = _fed(worker_number=64, aggregation_rule="centered_clip", cc_tau=2, cc_iters=1)
    assert (s.cc_tau, s.cc_iters) == (2.0, 1) and type(s.cc_tau) is float
    s.stop()
    s = _fed(worker_number=1, aggregation_rule="centered_clip", cc_tau=1e-3, cc_iters=10)
    s.stop()
    for rule in ("mean", "median", "geometric_median"):  # the defaults suit every rule
        s = _fed(worker_number=10, aggregation_rule=rule, cc_tau=10.0, cc_iters=3)
        assert (s.aggregation_rule, s.cc_tau, s.cc_iters) == (rule, 10.0, 3)
        s.stop()


@pytest.mark.parametrize("kw, what", [
    (dict(aggregation_rule="clip"), "aggregation_rule must be one of .*'centered_clip'"),
    (dict(cc_iters=5), "cc_tau=10.0 / cc_iters=5 needs aggregation_rule='centered_clip'"),
    (dict(cc_tau=1.0), "cc_tau=1.0 / cc_iters=3 needs aggregation_rule='centered_clip'"),
    (dict(aggregation_rule="median", cc_iters=2), "needs aggregation_rule='centered_clip'"),
    (dict(aggregation_rule="multi_krum", byzantine=1, cc_tau=1.0),
     "needs aggregation_rule='centered_clip'"),
    (dict(aggregation_rule="trimmed_mean", trim=1, cc_iters=1),
     "needs aggregation_rule='centered_clip'"),
    (dict(aggregation_rule="geometric_median", cc_tau=0.5),
     "needs aggregation_rule='centered_clip'"),
    (dict(aggregation_rule="centered_clip", cc_iters=0), "cc_iters must be a positive integer"),
    (dict(aggregation_rule="centered_clip", cc_iters=-1), "cc_iters must be a positive integer"),
    (dict(aggregation_rule="centered_clip", cc_iters=2.0), "cc_iters must be a positive integer"),
    (dict(aggregation_rule="centered_clip", cc_iters=True), "cc_iters must be a positive integer"),
    (dict(aggregation_rule="centered_clip", cc_iters=None), "cc_iters must be a positive integer"),
    (dict(aggregation_rule="centered_clip", cc_tau=0.0), "cc_tau must be a positive finite"),
    (dict(aggregation_rule="centered_clip", cc_tau=-1.0), "cc_tau must be a positive finite"),
    (dict(aggregation_rule="centered_clip", cc_tau=INF), "cc_tau must be a positive finite"),
    (dict(aggregation_rule="centered_clip", cc_tau=NAN), "cc_tau must be a positive finite"),
    (dict(aggregation_rule="centered_clip", cc_tau="10"), "cc_tau must be a positive finite"),
    (dict(aggregation_rule="centered_clip", cc_tau=True), "cc_tau must be a positive finite"),
    (dict(aggregation_rule="centered_clip", trim=1), "trim=1 needs aggregation_rule='trimmed_mean'"),
    (dict(aggregation_rule="centered_clip", byzantine=1), "needs aggregation_rule='multi_krum'"),
    (dict(aggregation_rule="centered_clip", gm_iters=2),
     "needs aggregation_rule='geometric_median'"),
    (dict(aggregation_rule="centered_clip", aggregation_mode="fma"),
     "aggregation_rule='mean' only"),
    (dict(aggregation_rule="centered_clip", worker_number=65), "ROBUST_MAX_K=64"),
])
def test_fed_server_rejects(kw, what):
    """Every case raises before the GPU is needed (no doubles installed)."""
    args = dict(worker_number=10)
    args.update(kw)
    with pytest.raises(ValueError, match=what):
        _fed(**args)


@pytest.mark.parametrize("algo", ["fed_quant", "GTG_shapley_value", "multiround_shapley_value"])
def test_other_servers_reject_centered_clip(algo, doubles):
    from distributed_learning_simulator_amd import factory
    with pytest.raises(ValueError, match="does not support aggregation_rule='centered_clip'"
                                         ".*FedServer"):
        factory.get_server(algo, sharded=False, tester=None, worker_number=5, synchronous=True,
                           device=CPU, aggregation_rule="centered_clip", cc_iters=2)
    with pytest.raises(ValueError, match="needs aggregation_rule='centered_clip'"):
        factory.get_server(algo, sharded=False, tester=None, worker_number=5, synchronous=True,
                           device=CPU, cc_tau=1.0)


@pytest.mark.parametrize("algo", ["fed", "fed_quant", "GTG_shapley_value",
                                  "multiround_shapley_value"])
def test_sharded_servers_reject_centered_clip(algo, doubles):
    from distributed_learning_simulator_amd import factory
    with pytest.raises(ValueError, match="does not support aggregation_rule='centered_clip'"
                                         ".*FedServer"):
        factory.get_server(algo, sharded=True, tester=None, worker_number=5, synchronous=True,
                           device=CPU, aggregation_rule="centered_clip")


# ------------------------------------------------------------------ simulator
def test_simulator_flags():
    from distributed_learning_simulator_amd.simulator import get_config, server_kwargs
    base = ["--worker_number", "5", "--round", "1", "--distributed_algorithm"]
    cfg = get_config(base + ["fed", "--aggregation_rule", "centered_clip"])
    assert (cfg.aggregation_rule, cfg.cc_tau, cfg.cc_iters) == ("centered_clip", 10.0, 3)
    assert server_kwargs(cfg) == {"aggregation_mode": "exact",
                                  "aggregation_rule": "centered_clip", "trim": 0,
                                  "cc_tau": 10.0, "cc_iters": 3}
    cfg = get_config(base + ["fed", "--aggregation_rule", "centered_clip", "--cc_tau", "0.5",
                             "--cc_iters", "1"])
    assert server_kwargs(cfg) == {"aggregation_mode": "exact",
                                  "aggregation_rule": "centered_clip", "trim": 0,
                                  "cc_tau": 0.5, "cc_iters": 1}
    # the other rules' dicts hold neither new key
    cfg = get_config(base + ["fed"])
    assert (cfg.cc_tau, cfg.cc_iters) == (10.0, 3)
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
    assert server_kwargs(get_config(base + ["fed", "--aggregation_rule", "geometric_median"])) == \
        {"aggregation_mode": "exact", "aggregation_rule": "geometric_median", "trim": 0,
         "gm_iters": 3, "gm_nu": 1e-6}
    assert server_kwargs(get_config(base + ["sign_SGD"])) == {}
    with pytest.raises(SystemExit):
        get_config(base + ["fed", "--aggregation_rule", "clip"])
    with pytest.raises(SystemExit):
        get_config(base + ["fed", "--aggregation_rule", "centered_clip", "--cc_iters", "three"])
    with pytest.raises(SystemExit):  # the vote has no mean to replace
        get_config(base + ["sign_SGD", "--aggregation_rule", "centered_clip"])
    from distributed_learning_simulator_amd import simulator
    assert "--aggregation_rule centered_clip" in simulator.__doc__


# ------------------------------------------------------------ source plumbing
def test_source_plumbing():
    from distributed_learning_simulator_amd import _native
    with open(os.path.join(ROOT, "include", "dls_hip.h")) as fh:
        header = fh.read()
    assert "int dls_centered_clip_step_f32(const float *U, int64_t ldu, const int32_t *rows" \
        in header
    assert "#define DLS_ABI_VERSION 2" in header
    L = _native.lib()
    assert "dls_centered_clip_step_f32" in _native.SIGNATURES
    assert hasattr(L, "dls_centered_clip_step_f32")
    # the step's operands are the Weiszfeld step's: one plan, one workspace function
    assert _native.SIGNATURES["dls_centered_clip_step_f32"] == \
        _native.SIGNATURES["dls_weiszfeld_step_f32"]
    assert L.dls_abi_version() == 2
    assert L.dls_source_hash().decode() == _native.source_hash()
    csrc = os.path.join(ROOT, "distributed_learning_simulator_amd", "csrc")
    with open(os.path.join(csrc, "weiszfeld.hip")) as fh:
        src = fh.read()
    assert 'extern "C" int dls_centered_clip_step_f32(' in src
    assert "getenv" not in src and "atomic" not in src.lower().replace("no atomics", "")
