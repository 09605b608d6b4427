"""CPU checks of the robust aggregation rules (coordinate-wise trimmed mean and
median): the numpy reference the GPU tests compare with, the argument validation
of dls_trimmed_mean_f32 and its Python wrapper (both run before any device call),
the servers' constructor validation and the simulator flags."""
import ctypes

import numpy as np
import pytest
import torch

from tests import cpu_doubles
from tests import robust_ref as R

CPU = torch.device("cpu")
NEG0, POS0, QNAN = 0x80000000, 0x00000000, 0x7FC00000


def f32_bits(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


# ------------------------------------------------------------------ reference
def test_reference_medians_odd_and_even():
    assert R.column([5.0, 1.0, 3.0], 1) == f32_bits(3.0)  # odd K: the middle element
    assert R.column([7.0, -2.0, 9.0, 1.0, 4.0], 2) == f32_bits(4.0)
    assert R.column([4.0, 1.0, 2.0, 8.0], 1) == f32_bits(3.0)  # even K: fl(fl(2 + 4) / 2)
    # one rounding in the sum, one in the division
    a, b = np.float32(1.0), np.float32(1.0 + 2.0 ** -23)
    assert R.column([b, a], 0) == f32_bits(np.float32(np.float32(a + b) / np.float32(2)))
    assert int(R.median_bits(np.array([[4.0], [1.0], [2.0], [8.0]], np.float32))[0]) == f32_bits(3.0)


def test_reference_trim_zero_is_the_ascending_unweighted_mean():
    vals = [np.float32(1e8), np.float32(1.0), np.float32(-1e8), np.float32(3.0)]
    acc = np.float32(-1e8)
    for v in (np.float32(1.0), np.float32(3.0), np.float32(1e8)):
        acc = np.float32(acc + v)
    assert R.column(vals, 0) == f32_bits(np.float32(acc / np.float32(4)))
    assert R.column(vals, 1) == f32_bits(2.0)


def test_reference_signed_zeros():
    # -0.0 sorts below +0.0; with m == 1 the kept value's own bits come back
    assert R.column_bits([POS0, NEG0, POS0], 1) == POS0
    assert R.column_bits([NEG0, POS0, NEG0], 1) == NEG0
    assert R.column_bits([NEG0], 0) == NEG0
    assert R.column_bits([f32_bits(1.0), NEG0, f32_bits(-1.0)], 1) == NEG0
    assert R.column_bits([NEG0, NEG0], 0) == NEG0  # fl(-0 + -0) / 2
    assert R.column_bits([NEG0, POS0], 0) == POS0


def test_reference_nan_order_and_canonical_result():
    inf, ninf = f32_bits(np.inf), f32_bits(-np.inf)
    nans = [0x7FC00000, 0xFFC00001, 0x7F800001, 0xFFFFFFFF]
    k = R.keys(np.array([ninf, f32_bits(-1.0), NEG0, POS0, f32_bits(1.0), inf] + nans, np.uint32))
    assert list(k[:6]) == sorted(k[:6]) and len(set(k[:6])) == 6
    assert all(x == 0xFFFFFFFF for x in k[6:]) and k[5] < 0xFFFFFFFF  # every NaN above +inf
    # NaN (either sign, odd payload) trimmed away: a finite result
    for nan in nans:
        assert R.column_bits([nan, f32_bits(1.0), f32_bits(2.0), f32_bits(3.0), f32_bits(-9.0)], 1) \
            == f32_bits(2.0)
        # a NaN inside the kept window: the canonical quiet NaN
        assert R.column_bits([nan, f32_bits(1.0), f32_bits(2.0)], 0) == QNAN
        assert R.column_bits([nan, nan, f32_bits(2.0)], 1) == QNAN
        assert R.column_bits([nan], 0) == QNAN
    # +inf is an ordinary value below the NaNs
    assert R.column_bits([nans[1], inf, f32_bits(2.0)], 1) == inf
    assert R.column_bits([inf, ninf], 0) == QNAN  # inf + -inf inside the sum
    big = f32_bits(np.finfo(np.float32).max)
    assert R.column_bits([big, big, f32_bits(1.0)], 0) == inf  # the kept sum overflows


def test_reference_is_permutation_invariant():
    rng = np.random.default_rng(5)
    X = rng.standard_normal((9, 64)).astype(np.float32)
    want = R.trimmed_mean_bits(X, 2)
    for _ in range(3):
        assert np.array_equal(R.trimmed_mean_bits(X[rng.permutation(9)], 2), want)


# ------------------------------------------------------------------------ ABI
def test_abi_rejects_bad_arguments_without_gpu():
    from distributed_learning_simulator_amd import _native
    L = _native.lib()
    d = ctypes.c_void_p(256)  # 16-byte aligned, never dereferenced
    f = L.dls_trimmed_mean_f32
    err = L.dls_last_error
    assert _native.ROBUST_MAX_K == 64
    for U, rows, out in ((None, d, d), (d, None, d), (d, d, None)):
        assert f(U, 64, rows, 3, 1, 64, out, None) == -1 and b"null pointer" in err()
    assert f(d, 64, d, 0, 0, 64, d, None) == -1 and b"DLS_ROBUST_MAX_K=64" in err()
    assert f(d, 64, d, 65, 0, 64, d, None) == -1 and b"DLS_ROBUST_MAX_K=64" in err()
    assert f(d, 64, d, 5, -1, 64, d, None) == -1 and b"2*trim < K" in err()
    assert f(d, 64, d, 4, 2, 64, d, None) == -1 and b"2*trim < K" in err()
    assert f(d, 64, d, 5, 2**30, 64, d, None) == -1 and b"2*trim < K" in err()
    assert f(d, 64, d, 3, 1, 62, d, None) == -2 and b"multiples of 4" in err()
    assert f(d, 60, d, 3, 1, 64, d, None) == -2
    assert f(d, 64, d, 3, 1, 64, ctypes.c_void_p(260), None) == -2 and b"alignment" in err()
    assert f(d, 64, d, 3, 1, 0, d, None) == 0  # P == 0: nothing to do, no launch


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
        (dict(trim=-1), "trim=-1"),
        (dict(trim=3), "2\\*trim < K=5"),
        (dict(P=62), "multiple of 4"),
        (dict(P=68), "row length"),
        (dict(out=torch.zeros(32)), "out must be"),
        (dict(out=out.double()), "out must be"),
        (dict(U=torch.zeros(8, 66)[:, :64]), "row pitch"),
        (dict(out=torch.zeros(68)[1:65]), "16-byte aligned"),
    ]
    for change, what in bad:
        kw = dict(U=U, rows=rows, trim=1, P=64, out=out)
        kw.update(change)
        with pytest.raises(RuntimeError, match="trimmed_mean: .*" + what):
            _native.trimmed_mean(kw["U"], kw["rows"], kw["trim"], kw["P"], kw["out"])
    # valid operands reach the library, which has no CPU path
    with pytest.raises(RuntimeError, match="not on the GPU"):
        _native.trimmed_mean(U, rows, 1, 64, out)


# -------------------------------------------------------------------- servers
@pytest.fixture
def doubles(monkeypatch):
    cpu_doubles.install(monkeypatch)


def _fed(**kw):
    from distributed_learning_simulator_amd.servers.fed_server import FedServer
    return FedServer(tester=None, device=CPU, synchronous=True, **kw)


def test_fed_server_accepts_the_rules(doubles):
    s = _fed(worker_number=10)
    assert s.aggregation_rule == "mean" and s.trim == 0
    s.stop()
    s = _fed(worker_number=10, aggregation_rule="trimmed_mean", trim=2)
    assert (s.aggregation_rule, s.trim) == ("trimmed_mean", 2)
    s.stop()
    s = _fed(worker_number=64, aggregation_rule="median")
    assert s.aggregation_rule == "median"
    s.stop()
    s = _fed(worker_number=65, aggregation_mode="fma")  # the mean has no client limit
    s.stop()


@pytest.mark.parametrize("kw, what", [
    (dict(aggregation_rule="krum"), "aggregation_rule must be one of"),
    (dict(aggregation_rule="median", trim=1), "trim=1 needs aggregation_rule='trimmed_mean'"),
    (dict(trim=1), "trim=1 needs aggregation_rule='trimmed_mean'"),
    (dict(aggregation_rule="trimmed_mean", trim=5), "2\\*trim < worker_number"),
    (dict(aggregation_rule="trimmed_mean", trim=-1), "non-negative"),
    (dict(aggregation_rule="trimmed_mean", trim=1.5), "non-negative integer"),
    (dict(aggregation_rule="median", worker_number=65), "ROBUST_MAX_K=64"),
    (dict(aggregation_rule="trimmed_mean", worker_number=65), "ROBUST_MAX_K=64"),
    (dict(aggregation_rule="median", aggregation_mode="fma"), "aggregation_rule='mean' only"),
    (dict(aggregation_rule="trimmed_mean", trim=1, aggregation_mode="fma"),
     "aggregation_rule='mean' only"),
])
def test_fed_server_rejects(kw, what):
    """Every case raises before the GPU is needed (no doubles installed)."""
    args = dict(worker_number=10)
    args.update(kw)
    with pytest.raises(ValueError, match=what):
        _fed(**args)


def test_subset_too_small_for_trim(doubles):
    s = _fed(worker_number=10, aggregation_rule="trimmed_mean", trim=2)
    for w in range(4):
        s.parameters[w] = (10, {"w": torch.full((4, 4), float(w))})
    with pytest.raises(ValueError, match="2\\*trim < len\\(subset\\)"):
        s.get_subset_model([0, 1, 2, 3])
    s.stop()


@pytest.mark.parametrize("algo", ["fed_quant", "GTG_shapley_value", "multiround_shapley_value"])
@pytest.mark.parametrize("rule", ["median", "trimmed_mean"])
def test_other_servers_reject_the_robust_rules(algo, rule, doubles):
    from distributed_learning_simulator_amd import factory
    with pytest.raises(ValueError, match="does not support aggregation_rule.*FedServer"):
        factory.get_server(algo, sharded=False, tester=None, worker_number=4, synchronous=True,
                           device=CPU, aggregation_rule=rule)
    # the default is untouched
    factory.get_server(algo, sharded=False, tester=None, worker_number=4, synchronous=True,
                       device=CPU).stop()
    factory.get_server(algo, sharded=False, tester=None, worker_number=4, synchronous=True,
                       device=CPU, aggregation_rule="mean").stop()


@pytest.mark.parametrize("algo", ["fed", "fed_quant", "GTG_shapley_value",
                                  "multiround_shapley_value"])
def test_sharded_servers_reject_the_robust_rules(algo, doubles):
    from distributed_learning_simulator_amd import factory
    with pytest.raises(ValueError, match="does not support aggregation_rule.*FedServer"):
        factory.get_server(algo, sharded=True, tester=None, worker_number=4, synchronous=True,
                           device=CPU, aggregation_rule="median")
    factory.get_server(algo, sharded=True, tester=None, worker_number=4, synchronous=True,
                       device=CPU).stop()


# ------------------------------------------------------------------ simulator
def test_simulator_flags():
    from distributed_learning_simulator_amd.simulator import get_config, server_kwargs
    base = ["--worker_number", "4", "--round", "1", "--distributed_algorithm"]
    cfg = get_config(base + ["fed"])
    assert (cfg.aggregation_rule, cfg.trim) == ("mean", 0)
    assert server_kwargs(cfg) == {"aggregation_mode": "exact"}
    assert server_kwargs(get_config(base + ["fed", "--aggregation_mode", "fma"])) == \
        {"aggregation_mode": "fma"}
    assert server_kwargs(get_config(base + ["fed", "--aggregation_rule", "mean"])) == \
        {"aggregation_mode": "exact"}
    assert server_kwargs(get_config(base + ["sign_SGD"])) == {}
    assert server_kwargs(get_config(base + ["fed", "--aggregation_rule", "median"])) == \
        {"aggregation_mode": "exact", "aggregation_rule": "median", "trim": 0}
    assert server_kwargs(get_config(base + ["fed", "--aggregation_rule", "trimmed_mean",
                                            "--trim", "1"])) == \
        {"aggregation_mode": "exact", "aggregation_rule": "trimmed_mean", "trim": 1}
    with pytest.raises(SystemExit):
        get_config(base + ["fed", "--aggregation_rule", "krum"])
    with pytest.raises(SystemExit):
        get_config(base + ["fed", "--trim", "half"])
    with pytest.raises(SystemExit):  # the vote has no mean to replace
        get_config(base + ["sign_SGD", "--aggregation_rule", "median"])
