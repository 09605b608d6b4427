"""CPU checks of the server optimizers (FedAvgM, FedAdagrad, FedAdam, FedYogi): the numpy
reference the GPU tests compare with against closed forms, FedServer's constructor
validation, the servers that refuse, the simulator flags, and the operand checks of
the Python wrapper and of dls_server_opt_step_f32, which all run before any device
call."""
import ctypes

import numpy as np
import pytest
import torch

from tests import cpu_doubles
from tests import server_opt_ref as R

CPU = torch.device("cpu")
F = np.float32
ADAPTIVE = ("adagrad", "adam", "yogi")


@pytest.fixture
def doubles(monkeypatch):
    cpu_doubles.install(monkeypatch)


# ------------------------------------------------------------------ reference
def test_reference_coefficients_are_rounded_once():
    lr, b1, o1, b2, o2, tau = R.coeffs(0.01, 0.9, 0.99, 1e-3)
    assert all(isinstance(c, np.float32) for c in (lr, b1, o1, b2, o2, tau))
    assert o1 == F(1.0 - float(F(0.9))) and o2 == F(1.0 - float(F(0.99)))
    assert R.v_start(1e-3) == F(float(F(1e-3)) ** 2)
    from distributed_learning_simulator_amd import _native
    got = _native.server_opt_coeffs(0.01, 0.9, 0.99, 1e-3)
    assert [float(c) for c in (lr, b1, o1, b2, o2, tau)] == list(got)
    assert _native.fl32(float(R.v_start(1e-3))) == float(R.v_start(1e-3))


def test_reference_sgd_without_momentum_is_the_aggregate_up_to_one_rounding():
    rng = np.random.default_rng(0)
    agg, x = rng.standard_normal(257).astype(F), rng.standard_normal(257).astype(F)
    out, m1 = R.sgd(agg, x, None, R.coeffs(1.0, 0.0, 0.99, 1e-3))
    assert np.array_equal(R.bits(m1), R.bits(agg - x))
    assert np.array_equal(R.bits(out), R.bits(x + (agg - x)))
    # with a momentum buffer: m' = fl(fl(beta1 * m) + d)
    m = rng.standard_normal(257).astype(F)
    c = R.coeffs(0.5, 0.9, 0.99, 1e-3)
    out, m1 = R.sgd(agg, x, m, c)
    assert np.array_equal(R.bits(m1), R.bits((c[1] * m).astype(F) + (agg - x)))
    assert np.array_equal(R.bits(out), R.bits(x + (c[0] * m1).astype(F)))


@pytest.mark.parametrize("name", ADAPTIVE)
def test_reference_first_adaptive_step_matches_the_float64_formula(name):
    """From m = 0, v = tau^2 the applied update out - x (in float64) is within 2^-20
    relative of the float64 formula on the fp32 d: at most nine roundings of 2^-24 each
    lie between them (omb1*d, beta1*m + ., d*d, two or three for v', the square root,
    the sum with tau, lr*m', the division; the final x + . is taken out by comparing
    against x + update rounded once below)."""
    rng = np.random.default_rng(1)
    lr, b1, b2, tau = 0.01, 0.9, 0.99, 1e-3
    c = R.coeffs(lr, b1, b2, tau)
    n = 4096
    x = np.zeros(n, F)  # out - x is then the rounded update itself
    agg = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 1, n)).astype(F)
    m = np.zeros(n, F)
    v = np.full(n, R.v_start(tau), F)
    out, m1, v1 = R.step(R.KINDS[name], agg, x, m, v, c)
    d = (agg - x).astype(np.float64)
    lr64, b164, o164, b264, o264, tau64 = (float(t) for t in c)
    v0 = float(R.v_start(tau))
    m64 = o164 * d
    d2 = d * d
    v64 = {"adagrad": v0 + d2, "adam": b264 * v0 + o264 * d2,
           "yogi": v0 - o264 * d2 * np.sign(v0 - d2)}[name]
    upd = lr64 * m64 / (np.sqrt(v64) + tau64)
    got = out.astype(np.float64) - x.astype(np.float64)
    rel = np.abs(got - upd) / np.abs(upd)
    assert float(rel.max()) <= 2.0 ** -20, float(rel.max())
    assert np.all(np.abs(m1.astype(np.float64) - m64) <= 2.0 ** -22 * np.abs(m64))


def test_reference_yogi_keeps_v_where_it_equals_d2_and_moves_it_either_side():
    c = R.coeffs(0.01, 0.9, 0.99, 1e-3)
    o2 = c[4]
    d = np.array([2.0, 2.0, 2.0], F)
    x = np.zeros(3, F)
    v = np.array([4.0, 5.0, 3.0], F)  # v == d2, v > d2, v < d2
    _, _, v1 = R.yogi(d, x, np.zeros(3, F), v, c)
    step = F(o2 * F(4.0))
    assert v1[0] == F(4.0)
    assert v1[1] == F(F(5.0) - step) and v1[1] < 5.0
    assert v1[2] == F(F(3.0) + step) and v1[2] > 3.0


def test_reference_zero_everything_stays_zero():
    """The padding's case: d = 0, m = 0, v = 0 gives the update 0 / tau = 0."""
    z = np.zeros(8, F)
    for name in ADAPTIVE:
        out, m1, v1 = R.step(R.KINDS[name], z, z, z, z, R.coeffs(0.01, 0.9, 0.99, 1e-3))
        assert not R.bits(out).any() and not R.bits(m1).any() and not R.bits(v1).any()
    out, m1, _ = R.step(R.SGD, z, z, z, None, R.coeffs(1.0, 0.9, 0.99, 1e-3))
    assert not R.bits(out).any() and not R.bits(m1).any()


def test_reference_driver_chains_steps():
    rng = np.random.default_rng(2)
    aggs = [rng.standard_normal(33).astype(F) for _ in range(3)]
    x, m = rng.standard_normal(33).astype(F), np.zeros(33, F)
    v = np.full(33, R.v_start(1e-3), F)
    c = R.coeffs(0.01, 0.9, 0.99, 1e-3)
    trail = R.run(R.ADAM, aggs, x, m, v, c)
    o1, m1, v1 = R.adam(aggs[0], x, m, v, c)
    o2, m2, v2 = R.adam(aggs[1], o1, m1, v1, c)
    assert np.array_equal(R.bits(trail[1][0]), R.bits(o2))
    assert np.array_equal(R.bits(trail[1][2]), R.bits(v2)) and len(trail) == 3
    assert R.same_bits(np.array([np.nan, 1.0], F), np.array([np.nan, 1.0], F))
    assert not R.same_bits(np.array([0.0], F), np.array([-0.0], F))


# ----------------------------------------------------------------- validation
def _check(**kw):
    from distributed_learning_simulator_amd.servers.fed_server import FedServer
    return FedServer._check_server_opt(kw.pop("optimizer", None), **kw)


def test_defaults_are_resolved_per_optimizer():
    assert _check() is None
    assert _check(optimizer="sgd") == (1.0, 0.0, 0.99, 1e-3)
    for name in ADAPTIVE:
        assert _check(optimizer=name) == (0.01, 0.9, 0.99, 1e-3)
    assert _check(optimizer="sgd", server_lr=0.5, server_momentum=0.9) == (0.5, 0.9, 0.99, 1e-3)
    assert _check(optimizer="yogi", server_lr=1, server_momentum=0, server_beta2=0.5,
                  server_tau=0.1) == (1.0, 0.0, 0.5, 0.1)


@pytest.mark.parametrize("kw, text", [
    (dict(optimizer="fedprox"), "server_optimizer must be None or one of"),
    (dict(optimizer="adam", server_lr=0.0), "server_lr must be a positive finite number"),
    (dict(optimizer="adam", server_lr=-1.0), "server_lr must be a positive finite number"),
    (dict(optimizer="adam", server_lr=float("inf")), "server_lr must be a positive finite"),
    (dict(optimizer="adam", server_lr=float("nan")), "server_lr must be a positive finite"),
    (dict(optimizer="adam", server_lr="0.1"), "server_lr must be a positive finite number"),
    (dict(optimizer="adam", server_lr=True), "server_lr must be a positive finite number"),
    (dict(optimizer="adam", server_lr=1e-60), "positive"),  # zero in fp32
    (dict(optimizer="adam", server_tau=0.0), "server_tau must be a positive finite number"),
    (dict(optimizer="adam", server_tau=float("nan")), "server_tau must be a positive finite"),
    (dict(optimizer="adam", server_tau=None), "server_tau must be a positive finite number"),
    (dict(optimizer="sgd", server_momentum=1.0), "server_momentum must be in [0, 1)"),
    (dict(optimizer="sgd", server_momentum=-0.1), "server_momentum must be in [0, 1)"),
    (dict(optimizer="sgd", server_momentum=float("nan")), "server_momentum must be a finite"),
    (dict(optimizer="adam", server_momentum=1.0 - 1e-12), "below 1"),  # 1.0 in fp32
    (dict(optimizer="adam", server_beta2=1.0), "server_beta2 must be in [0, 1)"),
    (dict(optimizer="adam", server_beta2=-1e-9), "server_beta2 must be in [0, 1)"),
    (dict(optimizer="yogi", server_beta2=None), "server_beta2 must be a finite number"),
])
def test_bad_values_are_refused(kw, text):
    with pytest.raises(ValueError) as e:
        _check(**kw)
    assert text in str(e.value), str(e.value)


@pytest.mark.parametrize("kw, text", [
    (dict(server_lr=0.1), "server_lr=0.1 needs server_optimizer set"),
    (dict(server_momentum=0.9), "server_momentum=0.9 needs server_optimizer set"),
    (dict(server_beta2=0.9), "server_beta2=0.9 needs server_optimizer in ['adam', 'yogi']"),
    (dict(server_tau=0.1), "server_tau=0.1 needs server_optimizer in ['adagrad', 'adam', 'yogi']"),
    (dict(optimizer="sgd", server_beta2=0.9), "server_beta2=0.9 needs server_optimizer in"),
    (dict(optimizer="sgd", server_tau=0.1), "server_tau=0.1 needs server_optimizer in"),
    (dict(optimizer="adagrad", server_beta2=0.9), "not 'adagrad'"),
])
def test_a_parameter_without_its_optimizer_is_refused(kw, text):
    with pytest.raises(ValueError) as e:
        _check(**kw)
    assert text in str(e.value), str(e.value)
    assert repr(kw.get("optimizer")) in str(e.value)


def test_the_constructor_runs_the_check_before_anything_else(doubles):
    from distributed_learning_simulator_amd import factory
    with pytest.raises(ValueError, match="server_tau=0.5 needs server_optimizer"):
        factory.get_server("fed", sharded=False, tester=None, worker_number=4, synchronous=True,
                           device=CPU, server_optimizer="sgd", server_tau=0.5)
    server = factory.get_server("fed", sharded=False, tester=None, worker_number=4,
                                synchronous=True, device=CPU, server_optimizer="yogi",
                                server_lr=0.1)
    try:
        assert server.server_optimizer == "yogi" and server.server_lr == 0.1
        assert (server.server_momentum, server.server_beta2, server.server_tau) == \
            (0.9, 0.99, 1e-3)
        assert server.server_opt_state == {"step": 0, "m": None, "v": None}
        assert server.last_server_step == {}
        server.reset_server_optimizer()  # nothing to reset yet
    finally:
        server.stop()
    plain = factory.get_server("fed", sharded=False, tester=None, worker_number=4,
                               synchronous=True, device=CPU)
    try:
        assert plain.server_optimizer is None and plain.server_opt_state is None
    finally:
        plain.stop()


@pytest.mark.parametrize("algo, why", [
    ("fed_quant", "re-quantized"),
    ("GTG_shapley_value", "picks or records the round model"),
    ("multiround_shapley_value", "picks or records the round model"),
])
def test_other_servers_refuse_a_server_optimizer(algo, why, doubles):
    from distributed_learning_simulator_amd import factory
    with pytest.raises(ValueError) as e:
        factory.get_server(algo, sharded=False, tester=None, worker_number=4, synchronous=True,
                           device=CPU, server_optimizer="adam")
    msg = str(e.value)
    assert "does not support server_optimizer='adam'" in msg and why in msg
    assert "the one-process FedServer (factory.get_server('fed', ...))" in msg
    # a parameter alone is refused as for FedServer, and the default is untouched
    with pytest.raises(ValueError, match="server_lr=0.5 needs server_optimizer set"):
        factory.get_server(algo, sharded=False, tester=None, worker_number=4, synchronous=True,
                           device=CPU, server_lr=0.5)
    factory.get_server(algo, sharded=False, tester=None, worker_number=4, synchronous=True,
                       device=CPU).stop()


@pytest.mark.parametrize("algo", ["fed", "fed_quant", "GTG_shapley_value",
                                  "multiround_shapley_value"])
def test_sharded_servers_refuse_a_server_optimizer(algo, doubles):
    from distributed_learning_simulator_amd import factory
    with pytest.raises(ValueError) as e:
        factory.get_server(algo, sharded=True, tester=None, worker_number=4, synchronous=True,
                           device=CPU, server_optimizer="sgd")
    msg = str(e.value)
    assert "does not support server_optimizer='sgd'" in msg
    assert "identical on every rank" in msg and "Sharded" in msg
    factory.get_server(algo, sharded=True, tester=None, worker_number=4, synchronous=True,
                       device=CPU).stop()


def test_sign_sgd_has_no_such_parameter(doubles):
    from distributed_learning_simulator_amd import factory
    with pytest.raises(TypeError, match="server_optimizer"):
        factory.get_server("sign_SGD", sharded=False, tester=None, worker_number=4,
                           synchronous=True, device=CPU, server_optimizer="sgd")


# ------------------------------------------------------------------ simulator
def test_simulator_flags():
    from distributed_learning_simulator_amd.simulator import get_config, server_kwargs
    base = ["--worker_number", "4", "--round", "1", "--distributed_algorithm"]
    cfg = get_config(base + ["fed"])
    assert cfg.server_optimizer is None and cfg.server_lr is None and cfg.server_tau is None
    assert server_kwargs(cfg) == {"aggregation_mode": "exact"}
    assert server_kwargs(get_config(base + ["fed", "--server_optimizer", "yogi", "--server_lr",
                                            "0.01"])) == \
        {"aggregation_mode": "exact", "server_optimizer": "yogi", "server_lr": 0.01}
    assert server_kwargs(get_config(base + ["fed", "--server_optimizer", "adam",
                                            "--server_momentum", "0.5", "--server_beta2", "0.9",
                                            "--server_tau", "0.01", "--aggregation_rule",
                                            "median"])) == \
        {"aggregation_mode": "exact", "aggregation_rule": "median", "trim": 0,
         "server_optimizer": "adam", "server_momentum": 0.5, "server_beta2": 0.9,
         "server_tau": 0.01}
    # a parameter alone reaches the server, which refuses it
    assert server_kwargs(get_config(base + ["fed", "--server_lr", "0.5"])) == \
        {"aggregation_mode": "exact", "server_lr": 0.5}
    assert server_kwargs(get_config(base + ["sign_SGD"])) == {}
    with pytest.raises(SystemExit):
        get_config(base + ["fed", "--server_optimizer", "lamb"])
    with pytest.raises(SystemExit):
        get_config(base + ["fed", "--server_optimizer", "adam", "--server_lr", "fast"])
    for flags in (["--server_optimizer", "sgd"], ["--server_lr", "0.5"],
                  ["--server_momentum", "0.9"], ["--server_beta2", "0.9"],
                  ["--server_tau", "0.1"]):
        with pytest.raises(SystemExit):  # the vote is no model to step
            get_config(base + ["sign_SGD"] + flags)


# -------------------------------------------------------------------- wrapper
def _vecs(n=16):
    return [torch.zeros(n) for _ in range(5)]


def _call(kind, agg, x, m, v, out, P, lr=0.01, beta1=0.9, beta2=0.99, tau=1e-3):
    from distributed_learning_simulator_amd import _native
    return _native.server_opt_step(kind, agg, x, m, v, out, P, lr, beta1, beta2, tau)


def test_wrapper_checks_run_before_any_device_call():
    from distributed_learning_simulator_amd import _native
    ADAM, SGD = _native.SERVER_OPT_ADAM, _native.SERVER_OPT_SGD
    agg, x, m, v, out = _vecs()
    cases = [
        ((7, agg, x, m, v, out, 16), {}, "kind=7"),
        ((True, agg, x, m, v, out, 16), {}, "kind=True"),
        ((ADAM, agg, x, m, v, out, -1), {}, "P=-1"),
        ((ADAM, agg.double(), x, m, v, out, 16), {}, "agg must be an fp32 vector"),
        ((ADAM, agg, x, m, v.to(torch.float16), out, 16), {}, "v must be an fp32 vector"),
        ((ADAM, agg, x, m, v, out.int(), 16), {}, "out must be an fp32 vector"),
        ((ADAM, agg, x[:15], m, v, out, 16), {}, "x must be an fp32 vector of at least P=16"),
        ((ADAM, agg, x, torch.zeros(32)[::2], v, out, 16), {}, "m must be an fp32 vector"),
        ((ADAM, agg, x, m, v, torch.zeros(4, 4), 16), {}, "out must be an fp32 vector"),
        ((ADAM, agg, x, m, None, out, 16), {}, "needs v"),
        ((ADAM, agg, x, None, v, out, 16), {}, "m may be None"),
        ((SGD, agg, x, m, v, out, 16), {}, "v must be None"),
        ((SGD, agg, x, None, None, out, 16), {}, "m may be None"),  # beta1 = 0.9
        ((ADAM, agg, x, m, v, out, 16), {"lr": float("inf")}, "must be finite"),
        ((ADAM, agg, x, m, v, out, 16), {"lr": 1e39}, "must be finite"),  # inf in fp32
        ((ADAM, agg, x, m, v, out, 16), {"beta1": float("nan")}, "must be finite"),
        ((ADAM, agg, x, m, v, out, 16), {"beta2": float("-inf")}, "must be finite"),
        ((ADAM, agg, x, m, v, out, 16), {"tau": float("nan")}, "must be finite"),
    ]
    for args, kw, text in cases:
        with pytest.raises(RuntimeError) as e:
            _call(*args, **kw)
        assert text in str(e.value), (text, str(e.value))
    # overlap: out may be x itself, anything else is refused, a partial overlap of the
    # two included
    buf = torch.zeros(40)
    for args, text in [
        ((ADAM, agg, buf[:16], m, v, buf[8:24], 16), "x and out overlap"),
        ((ADAM, agg, buf[1:17], m, v, buf[:16], 16), "x and out overlap"),
        ((ADAM, agg, x, m, v, agg, 16), "agg and out overlap"),
        ((ADAM, agg, x, buf[:16], buf[15:31], out, 16), "m and v overlap"),
        ((ADAM, x, x, m, v, out, 16), "agg and x overlap"),
        ((ADAM, agg, x, m, m, out, 16), "m and v overlap"),
    ]:
        with pytest.raises(RuntimeError) as e:
            _call(*args)
        assert text in str(e.value), (text, str(e.value))
    # only the first P elements count
    with pytest.raises(RuntimeError, match="not on the GPU"):
        _call(ADAM, agg, buf[:16], m, v, buf[8:24], 8)
    # every operand check passed: what is left is the CPU tensor itself
    for args in [(ADAM, agg, x, m, v, out, 16), (ADAM, agg, x, m, v, x, 16),
                 (SGD, agg, x, m, None, out, 16), (ADAM, agg, x, m, v, out, 0)]:
        with pytest.raises(RuntimeError, match="not on the GPU"):
            _call(*args)
    with pytest.raises(RuntimeError, match="not on the GPU"):
        _call(SGD, agg, x, None, None, out, 16, beta1=0.0)


def test_launch_shape_constants_match_the_header():
    import os
    import re
    from distributed_learning_simulator_amd import _native
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                             "include", "dls_hip.h")).read()
    macros = dict(re.findall(r"#define DLS_SERVER_OPT_(\w+) (\d+)", text))
    assert {k: int(v) for k, v in macros.items()} == {
        "SGD": _native.SERVER_OPT_SGD, "ADAGRAD": _native.SERVER_OPT_ADAGRAD,
        "ADAM": _native.SERVER_OPT_ADAM, "YOGI": _native.SERVER_OPT_YOGI,
        "BLOCK": _native.SERVER_OPT_BLOCK, "MAX_BLOCKS": _native.SERVER_OPT_MAX_BLOCKS,
        "UNROLL": _native.SERVER_OPT_UNROLL}
    assert _native.SERVER_OPT_KINDS == R.KINDS


# ---------------------------------------------------------------------- C-ABI
def test_c_abi_checks_run_before_any_device_call():
    """rc -1 and dls_last_error for null pointers, a bad kind, v given for SGD, a missing
    v or m, a negative P, a non-finite coefficient and overlapping operands; rc -2 for a
    pointer that is not 4-byte aligned.  The pointers are never dereferenced."""
    from distributed_learning_simulator_amd import _native
    L = _native.lib()
    f = L.dls_server_opt_step_f32
    err = lambda: L.dls_last_error().decode()
    a, x, m, v, o = (ctypes.c_void_p(4096 * (i + 1)) for i in range(5))
    co = (0.01, 0.9, 0.1, 0.99, 0.01, 1e-3)

    def call(kind, a, x, m, v, o, P=64, co=co):
        return f(kind, a, x, m, v, o, P, *co, None)

    assert call(2, None, x, m, v, o) == -1 and "null pointer" in err()
    assert call(2, a, None, m, v, o) == -1 and "null pointer" in err()
    assert call(2, a, x, m, v, None) == -1 and "null pointer" in err()
    assert call(2, a, x, None, v, o) == -1 and "null pointer (m" in err()
    assert call(1, a, x, m, None, o) == -1 and "null pointer (v" in err()
    assert call(0, a, x, None, None, o) == -1 and "null pointer (m" in err()  # beta1 != 0
    assert call(4, a, x, m, v, o) == -1 and "kind=4" in err()
    assert call(-1, a, x, m, v, o) == -1 and "kind=-1" in err()
    assert call(0, a, x, m, v, o) == -1 and "v must be null" in err()
    assert call(3, a, x, m, v, o, P=-1) == -1 and "P=-1" in err()
    for i in range(6):
        for bad in (float("nan"), float("inf")):
            c2 = list(co)
            c2[i] = bad
            assert call(3, a, x, m, v, o, co=c2) == -1 and "non-finite coefficient" in err()
    assert call(2, a, x, m, v, ctypes.c_void_p(4096 + 8)) == -1 and "overlap" in err()
    assert call(2, a, a, m, v, o) == -1 and "overlap" in err()
    assert call(2, a, x, m, m, o) == -1 and "overlap" in err()
    assert call(2, a, x, m, v, a) == -1 and "overlap" in err()
    assert call(2, a, x, m, v, ctypes.c_void_p(4096 * 5 + 2)) == -2 and "alignment" in err()
    # nothing to do: no launch, no device call, whatever the pointers are
    assert call(2, a, x, m, v, o, P=0) == 0
    assert call(2, a, x, m, v, x, P=0) == 0
    assert call(0, a, x, None, None, o, P=0, co=(1.0, 0.0, 1.0, 0.0, 1.0, 0.0)) == 0
