"""CPU checks of the Byzantine client attacks: ``alie_z`` and ``attack_coefficients``,
the numpy reference the GPU tests compare with (against the trimmed-mean reference,
by hand and under permutation), the argument validation of dls_craft_rows_f32, of its
Python wrapper and of the store methods (all before any device call), the servers'
validation, the simulator flags and FedServer rounds on CPU doubles."""
import ctypes
import math
import statistics

import numpy as np
import pytest
import torch

from tests import attack_ref as A
from tests import cpu_doubles
from tests import robust_ref as R

CPU = torch.device("cpu")
QNAN, INF = 0x7FC00000, 0x7F800000


def f32_bits(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


# ---------------------------------------------------------------- host functions
@pytest.mark.parametrize("n, f", [(50, 12), (10, 2), (10, 1)])
def test_alie_z_values(n, f):
    from distributed_learning_simulator_amd.aggregation import alie_z
    s = n // 2 + 1 - f
    want = statistics.NormalDist().inv_cdf((n - f - s) / (n - f))
    assert alie_z(n, f) == want
    if (n, f) == (10, 2):
        assert want == 0.0
    elif (n, f) == (10, 1):
        assert want < 0  # passed through, not clamped
    else:
        assert 0.3 < want < 0.4  # p = 24 / 38


@pytest.mark.parametrize("n, f", [(10, 0), (10, 10), (10, 11), (2, 1), (3, 2), (10, -1), (10, 6),
                                  (10.0, 2), (10, True)])
def test_alie_z_value_errors(n, f):
    from distributed_learning_simulator_amd.aggregation import alie_z
    # (2, 1), (3, 2): p = 0; (10, 6): s = 0, p = 1
    with pytest.raises(ValueError, match="alie_z"):
        alie_z(n, f)


def test_attack_coefficients():
    from distributed_learning_simulator_amd.aggregation import alie_z, attack_coefficients
    assert attack_coefficients("alie", 50, 12) == (1.0, -alie_z(50, 12), False)
    assert attack_coefficients("alie", 50, 12, z=1.5) == (1.0, -1.5, False)
    a, b, base = attack_coefficients("alie", 10, 2)
    assert (a, b, base) == (1.0, 0.0, False)  # z == 0: no deviation term at all
    assert attack_coefficients("alie", 10, 1)[1] > 0  # a negative z
    assert attack_coefficients("ipm", 10, 2) == (-0.1, 0.0, True)
    assert attack_coefficients("ipm", 10, 2, eps=2.5) == (-2.5, 0.0, True)
    assert attack_coefficients("ipm", 10, 2, z=7.0, eps=1) == (-1.0, 0.0, True)
    for bad in ("sign_flip", None, "ALIE"):
        with pytest.raises(ValueError, match="'alie' or 'ipm'"):
            attack_coefficients(bad, 10, 2)
    with pytest.raises(ValueError, match="z must be a finite number"):
        attack_coefficients("alie", 10, 2, z=float("nan"))
    with pytest.raises(ValueError, match="eps must be a finite number"):
        attack_coefficients("ipm", 10, 2, eps=float("inf"))
    with pytest.raises(ValueError, match="alie_z"):
        attack_coefficients("alie", 3, 2)


# ------------------------------------------------------------------ reference
def test_reference_by_hand():
    # mean 2, deviations -1, 0, 1: variance 2/3, all in fp32
    var = np.float32(2.0) / np.float32(3.0)
    sig = np.sqrt(var)
    assert A.column([3.0, 1.0, 2.0], 1.0, 0.0) == f32_bits(2.0)
    assert A.column([3.0, 1.0, 2.0], 1.0, -0.75) == f32_bits(np.float32(2.0) + np.float32(-0.75) * sig)
    assert A.column([3.0, 1.0, 2.0], -0.1, 0.0, base=1.0) == \
        f32_bits(np.float32(1.0) + np.float32(-0.1) * np.float32(1.0))
    assert A.column([3.0, 1.0, 2.0], 1.0, 0.5, base=1.0) == \
        f32_bits(np.float32(1.0) + (np.float32(1.0) + np.float32(0.5) * sig))
    # Kh == 1: the value's own bits, variance +0
    assert A.craft_bits(np.array([[0x80000000]], np.uint32), 1.0, 0.0)[0] == 0x80000000
    assert A.column([5.0], 1.0, -2.0) == f32_bits(5.0)
    # the variance overflows: inf with b != 0, a finite a * mu with b == 0 of either sign
    big = [3e38, -3e38, 1.0, -1.0]
    assert A.column(big, 1.0, 1.0) == INF
    assert A.column(big, 1.0, -1.0) == INF | 0x80000000
    assert A.column(big, 1.0, 0.0) == 0 and A.column(big, 1.0, -0.0) == 0
    assert A.column([3e38, 3e38], 1.0, 0.0) == INF  # the sum itself overflows
    assert A.column([3e38, 3e38], 1.0, 1.0) == INF  # mu = inf, d = -inf
    assert A.column([float("inf"), 1.0], 1.0, 1.0) == QNAN  # inf - inf in the deviations
    assert A.column([float("inf"), 1.0], 1.0, 0.0) == INF
    assert A.column([float("nan"), 1.0], 1.0, 0.0) == QNAN
    # a denormal variance: (x, -x) has variance exactly x * x
    x = np.float32(2.0 ** -70)
    assert A.column([x, -x], 0.0, 1.0) == f32_bits(np.sqrt(np.float32(2.0 ** -140)))
    assert A.column([x, -x], 0.0, 1.0) == f32_bits(2.0 ** -70)


def test_reference_fmaf_rounds_once():
    """Cases where rounding the fp64 sum to nearest first would give another fp32."""
    one = np.array([1.0], np.float32)
    # 2^-12 squared is 2^-24: 1 + 2^-23 + 2^-24 is a tie at an odd mantissa, up
    a = np.array([2.0 ** -12], np.float32)
    assert A.fmaf(a, a, one + np.float32(2.0 ** -23))[0] == np.float32(1.0 + 2.0 ** -22)
    # big^2 = 1 + 2^-11 + 2^-24 is an fp32 tie; an addend far below the fp64 ulp decides
    big = np.array([1.0 + 2.0 ** -12], np.float32)
    tiny = np.array([2.0 ** -80], np.float32)
    assert (big.astype(np.float64) ** 2 + tiny.astype(np.float64)).astype(np.float32)[0] == \
        np.float32(1.0 + 2.0 ** -11)  # two roundings: the tie goes to even
    assert A.fmaf(big, big, tiny)[0] == np.float32(1.0 + 2.0 ** -11 + 2.0 ** -23)
    assert A.fmaf(big, big, -tiny)[0] == np.float32(1.0 + 2.0 ** -11)
    assert A.fmaf(big, big, 0 * tiny)[0] == np.float32(1.0 + 2.0 ** -11)  # the exact tie
    # inf and NaN pass through
    inf = np.array([np.inf], np.float32)
    assert A.fmaf(inf, inf, one)[0] == np.inf and np.isnan(A.fmaf(inf, inf, -inf)[0])


def test_reference_against_the_trimmed_mean_and_permutations():
    rng = np.random.default_rng(2019)
    pool = np.array([0, 0x80000000, INF, 0xFF800000, 0x7FC00000, 0xFFABCDEF, 1, 0x80000001,
                     0x7F7FFFFF, 0xFF7FFFFF, 0x3F800000], np.uint32)
    for K in (1, 2, 5, 8, 13, 64):
        X = (rng.standard_normal((K, 512)) * 100).astype(np.float32)
        X.view(np.uint32)[:, :128][rng.random((K, 128)) < 0.3] = rng.choice(pool, 1)[0]
        X.view(np.uint32)[:, 128:256] = rng.choice(pool, (K, 128))
        base = (rng.standard_normal(512) * 100).astype(np.float32)
        # a = 1, b = 0, no base: the ascending mean
        assert np.array_equal(A.craft_bits(X, 1.0, 0.0), R.trimmed_mean_bits(X, 0))
        assert np.array_equal(A.craft_bits(X, 1.0, -0.0), R.trimmed_mean_bits(X, 0))
        for a, b, bs in ((1.0, -0.75, None), (-0.1, 0.0, base), (1.0, 0.5, base)):
            want = A.craft_bits(X, a, b, bs)
            for _ in range(3):
                assert np.array_equal(A.craft_bits(X[rng.permutation(K)], a, b, bs), want)
    # against fp64 on ordinary values
    X = rng.standard_normal((20, 256)).astype(np.float32)
    got = A.craft_bits(X, 1.0, -1.5).view(np.float32)
    want = X.astype(np.float64).mean(0) - 1.5 * X.astype(np.float64).std(0)
    assert np.abs(got - want).max() < 1e-5


def test_sign_flip_reference():
    x = np.array([1.0, -2.0, 0.0, 3.5], np.float32)
    base = np.array([0.5, 0.5, 0.5, 0.5], np.float32)
    assert np.array_equal(A.sign_flip_bits(x, 1.0, base).view(np.float32),
                          np.array([0.0, 3.0, 1.0, -2.5], np.float32))
    assert np.array_equal(A.sign_flip_bits(x, 2.0).view(np.uint32),
                          np.array([-2.0, 4.0, -0.0, -7.0], np.float32).view(np.uint32))


# ------------------------------------------------------------------------ ABI
def test_abi_rejects_bad_arguments_without_gpu():
    from distributed_learning_simulator_amd import _native
    L = _native.lib()
    d = ctypes.c_void_p(256)  # 16-byte aligned, never dereferenced
    f = L.dls_craft_rows_f32
    err = L.dls_last_error
    for U, h, a in ((None, d, d), (d, None, d), (d, d, None)):
        assert f(U, 64, h, 3, a, 1, 1.0, 0.0, None, 64, None) == -1 and b"null pointer" in err()
    assert f(d, 64, d, 0, d, 1, 1.0, 0.0, None, 64, None) == -1 and b"Kh=0" in err()
    assert f(d, 64, d, 65, d, 1, 1.0, 0.0, None, 64, None) == -1 and b"DLS_ROBUST_MAX_K=64" in err()
    assert f(d, 64, d, 3, d, 0, 1.0, 0.0, None, 64, None) == -1 and b"Ka=0" in err()
    assert f(d, 64, d, 3, d, 65, 1.0, 0.0, None, 64, None) == -1 and b"Ka=65" in err()
    for a, b in ((math.inf, 0.0), (math.nan, 0.0), (1.0, -math.inf), (1.0, math.nan)):
        assert f(d, 64, d, 3, d, 1, a, b, None, 64, None) == -1 and b"finite" in err()
    assert f(d, 64, d, 3, d, 1, 1.0, 0.0, None, -4, None) == -1 and b"P=-4" in err()
    assert f(d, 64, d, 3, d, 1, 1.0, 0.0, None, 62, None) == -2 and b"multiples of 4" in err()
    assert f(d, 60, d, 3, d, 1, 1.0, 0.0, None, 64, None) == -2 and b"multiples of 4" in err()
    assert f(d, 62, d, 3, d, 1, 1.0, 0.0, None, 60, None) == -2
    assert f(ctypes.c_void_p(264), 64, d, 3, d, 1, 1.0, 0.0, None, 64, None) == -2 \
        and b"alignment" in err()
    assert f(d, 64, d, 3, d, 1, 1.0, 0.0, ctypes.c_void_p(260), 64, None) == -2 \
        and b"alignment" in err()
    assert b"dls_craft_rows_f32" in err()
    assert f(d, 64, d, 3, d, 2, 1.0, -0.5, d, 0, None) == 0  # P == 0: nothing to do, no launch


def test_wrapper_validates_before_the_library_call():
    from distributed_learning_simulator_amd import _native
    U = torch.zeros(8, 64)
    h = torch.arange(5, dtype=torch.int32)
    at = torch.tensor([6, 7], dtype=torch.int32)
    bad = [
        (dict(U=U.double()), "U must be"),
        (dict(U=torch.zeros(8, 128)[:, ::2]), "U must be"),
        (dict(hrows=h.long()), "rows must be"),
        (dict(arows=at.long()), "rows must be"),
        (dict(hrows=torch.zeros(0, dtype=torch.int32)), "ROBUST_MAX_K"),
        (dict(arows=torch.zeros(65, dtype=torch.int32)), "ROBUST_MAX_K=64"),
        (dict(a=float("inf")), "must be finite"),
        (dict(b=float("nan")), "must be finite"),
        (dict(P=62), "multiple of 4"),
        (dict(P=68), "row length"),
        (dict(U=torch.zeros(8, 66)[:, :64]), "row pitch"),
        (dict(base=torch.zeros(32)), "base must be"),
        (dict(base=torch.zeros(64).double()), "base must be"),
        (dict(base=torch.zeros(68)[1:65]), "16-byte aligned"),
    ]
    for change, what in bad:
        kw = dict(U=U, hrows=h, arows=at, a=1.0, b=-0.5, P=64, base=None)
        kw.update(change)
        with pytest.raises(RuntimeError, match="craft_rows: .*" + what):
            _native.craft_rows(**kw)
    # valid operands reach the library, which has no CPU path
    with pytest.raises(RuntimeError, match="not on the GPU"):
        _native.craft_rows(U, h, at, 1.0, -0.5, 64, base=torch.zeros(64))


def test_source_plumbing():
    """The symbol is declared, bound and part of the hashed sources."""
    from distributed_learning_simulator_amd import _native
    assert "dls_craft_rows_f32" in _native.SIGNATURES
    assert "robust.hip" in _native.CSRC_HASHED and "dls_common.h" in _native.CSRC_HASHED
    assert _native.lib().dls_source_hash().decode() == _native.source_hash()
    assert _native.lib().dls_abi_version() == 2


# ---------------------------------------------------------------------- store
def _np_craft_rows(U, hrows, arows, a, b, P, base=None, stream=None):
    Un = U.detach().numpy()
    X = Un[hrows.numpy().astype(np.int64), :P]
    bs = None if base is None else base.detach().numpy()[:P]
    out = torch.from_numpy(A.craft_bits(X, a, b, bs).view(np.float32))
    for r in arows.tolist():
        U[r, :P].copy_(out)
    return U


def _np_trimmed_mean(U, rows, trim, P, out, stream=None):
    X = U.detach().numpy()[rows.numpy().astype(np.int64), :P]
    out[:P].copy_(torch.from_numpy(R.trimmed_mean_bits(X, trim).view(np.float32)))
    return out


@pytest.fixture
def doubles(monkeypatch):
    from distributed_learning_simulator_amd import _native
    cpu_doubles.install(monkeypatch)
    calls = {"craft_rows": 0}

    def craft(*a, **kw):
        calls["craft_rows"] += 1
        return _np_craft_rows(*a, **kw)

    monkeypatch.setattr(_native, "craft_rows", craft)
    monkeypatch.setattr(_native, "trimmed_mean", _np_trimmed_mean)
    return calls


def _store(rows=8, n=100):
    from distributed_learning_simulator_amd.aggregation import ClientUpdateStore
    from distributed_learning_simulator_amd.layout import ParameterLayout
    store = ClientUpdateStore(ParameterLayout([("a", (n,))]), CPU, capacity=rows)
    store.U.copy_(torch.randn(store.U.shape, generator=torch.Generator().manual_seed(5)))
    return store


def test_store_craft_checks_its_row_lists(doubles):
    store = _store()
    for honest, bad, what in (
            ([0, 1, 2], [2, 3], "rows \\[2\\] are both honest and attacker rows"),
            ([0, 1, 1], [3], "honest_rows holds a row twice"),
            ([0, 1], [3, 3], "attacker_rows holds a row twice"),
            ([], [3], "honest_rows holds 0 rows"),
            ([0], [], "attacker_rows holds 0 rows"),
            (list(range(65)), [70], "honest_rows holds 65 rows \\(1..ROBUST_MAX_K=64\\)"),
            ([0], list(range(1, 66)), "attacker_rows holds 65 rows"),
            ([0, 8], [1], "outside the store's 8 rows"),
            ([0], [-1], "outside the store's 8 rows")):
        with pytest.raises(ValueError, match="craft: .*" + what):
            store.craft(honest, bad, 1.0, 0.0)
    assert doubles["craft_rows"] == 0  # nothing reached the kernel wrapper


def test_store_craft_and_sign_flip_on_cpu_doubles(doubles):
    store = _store()
    before = store.U.numpy().copy()
    P = store.layout.P
    base = torch.randn(P, generator=torch.Generator().manual_seed(6))
    assert store.craft([5, 0, 3], [6, 1], 1.0, -0.75) is None
    want = A.craft_bits(before[[0, 3, 5]], 1.0, -0.75)
    after = store.U.numpy()
    assert np.array_equal(after[6].view(np.uint32), want)
    assert np.array_equal(after[1].view(np.uint32), want)
    keep = [0, 2, 3, 4, 5, 7]
    assert np.array_equal(after[keep].view(np.uint32), before[keep].view(np.uint32))
    store.craft([5, 0, 3], [2], -0.1, 0.0, base=base[64:96], cols=(64, 96))
    got = store.U.numpy()
    assert np.array_equal(got[2, 64:96].view(np.uint32),
                          A.craft_bits(before[[0, 3, 5], 64:96], -0.1, 0.0, base.numpy()[64:96]))
    assert np.array_equal(got[2, :64], before[2, :64]) and np.array_equal(got[2, 96:], before[2, 96:])
    # sign flip: three ops, with and without base
    x = store.U.numpy().copy()
    assert store.sign_flip([4, 7], 1.5, base=base) is None
    now = store.U.numpy()
    for r in (4, 7):
        assert np.array_equal(now[r].view(np.uint32), A.sign_flip_bits(x[r], 1.5, base.numpy()))
    store.sign_flip([0], 0.1)
    assert np.array_equal(store.U.numpy()[0].view(np.uint32), A.sign_flip_bits(x[0], 0.1))
    assert np.array_equal(store.U.numpy()[3], x[3])
    with pytest.raises(ValueError, match="listed twice"):
        store.sign_flip([1, 1], 1.0)
    with pytest.raises(ValueError, match="scale must be a finite number"):
        store.sign_flip([1], float("nan"))


# -------------------------------------------------------------------- servers
def _fed(**kw):
    from distributed_learning_simulator_amd.servers.fed_server import FedServer
    return FedServer(tester=None, device=CPU, synchronous=True, **kw)


def test_fed_server_accepts_the_attacks(doubles):
    s = _fed(worker_number=11, attack="alie", attackers=[7, 3])
    assert (s.attack, s.attackers, s.attack_z, s.last_attack) == ("alie", (3, 7), None, {})
    s.stop()
    s = _fed(worker_number=11, attack="alie", attackers={3}, attack_z=1)
    assert s.attack_z == 1.0
    s.stop()
    s = _fed(worker_number=5, attack="ipm", attackers=(4,), attack_eps=2.0)
    assert (s.attack, s.attackers, s.attack_eps) == ("ipm", (4,), 2.0)
    s.stop()
    s = _fed(worker_number=3, attack="sign_flip", attackers=(0, 1, 2), attack_scale=3.0)
    assert s.attack_scale == 3.0  # everybody may flip: nothing is crafted from honest rows
    s.stop()
    s = _fed(worker_number=3)
    assert (s.attack, s.attackers, s.last_attack) == (None, (), {})
    s.stop()
    _fed(worker_number=128, attack="ipm", attackers=tuple(range(64))).stop()
    _fed(worker_number=11, attack="alie", attackers=(3, 7), aggregation_rule="bulyan",
         byzantine=2).stop()


@pytest.mark.parametrize("kw, what", [
    (dict(attack="gaussian", attackers=(1,)), "attack must be None or one of"),
    (dict(attack="alie"), "attack='alie' needs attackers"),
    (dict(attack="ipm", attackers=()), "attack='ipm' needs attackers"),
    (dict(attackers=(1,)), "attackers=\\[1\\] needs an attack"),
    (dict(attack="alie", attackers=(1, 1)), "distinct worker ids"),
    (dict(attack="alie", attackers=(1, 10)), "worker ids in 0..worker_number - 1 = 9"),
    (dict(attack="alie", attackers=(-1,)), "non-negative integer worker ids"),
    (dict(attack="alie", attackers=(1.0,)), "non-negative integer worker ids"),
    (dict(attack="alie", attackers=3), "collection of worker ids"),
    (dict(attack="ipm", attackers=tuple(range(10))), "needs at least one honest worker"),
    (dict(attack="alie", attackers=tuple(range(10))), "needs at least one honest worker"),
    (dict(attack="ipm", attackers=(0,), worker_number=66), "at most ROBUST_MAX_K=64 honest"),
    (dict(attack="ipm", attackers=tuple(range(65)), worker_number=70),
     "at most ROBUST_MAX_K=64 attackers"),
    (dict(attack="alie", attackers=tuple(range(6))), "alie_z"),  # p = 1: give attack_z
    (dict(attack_z=1.0), "attack_z=1.0 needs attack='alie', not None"),
    (dict(attack="ipm", attackers=(1,), attack_z=1.0), "attack_z=1.0 needs attack='alie', not 'ipm'"),
    (dict(attack_eps=0.5), "attack_eps=0.5 needs attack='ipm', not None"),
    (dict(attack="alie", attackers=(1,), attack_eps=0.5), "needs attack='ipm', not 'alie'"),
    (dict(attack_scale=2.0), "attack_scale=2.0 needs attack='sign_flip', not None"),
    (dict(attack="ipm", attackers=(1,), attack_scale=2.0), "needs attack='sign_flip', not 'ipm'"),
    (dict(attack="alie", attackers=(1,), attack_z=float("nan")), "attack_z must be a finite number"),
    (dict(attack="ipm", attackers=(1,), attack_eps=float("inf")), "attack_eps must be a finite"),
    (dict(attack="sign_flip", attackers=(1,), attack_scale="2"), "attack_scale must be a finite"),
])
def test_fed_server_rejects(kw, what):
    """Every case raises before the GPU is needed (no doubles installed)."""
    args = dict(worker_number=10)
    args.update(kw)
    with pytest.raises(ValueError, match=what):
        _fed(**args)


def test_check_attack_class_methods():
    from distributed_learning_simulator_amd.distributed import (ShardedFedQuantServer,
                                                                ShardedFedServer,
                                                                ShardedMultiRoundShapleyValueServer)
    from distributed_learning_simulator_amd.servers.fed_quant_server import FedQuantServer
    from distributed_learning_simulator_amd.servers.fed_server import FedServer
    from distributed_learning_simulator_amd.servers.GTG_shapley_value_server import \
        GTGShapleyValueServer
    from distributed_learning_simulator_amd.servers.multiround_shapley_value_server import \
        MultiRoundShapleyValueServer
    for cls in (FedServer, GTGShapleyValueServer, MultiRoundShapleyValueServer):
        assert cls._attack_unsupported is None
        assert cls._check_attack("alie", [7, 3], worker_number=11) == (3, 7)
        assert cls._check_attack(None, ()) == ()
    for cls in (FedQuantServer, ShardedFedServer, ShardedFedQuantServer,
                ShardedMultiRoundShapleyValueServer):
        assert cls._check_attack(None, (), worker_number=8) == ()  # the default still passes
        with pytest.raises(ValueError, match=f"{cls.__name__} does not support attack='ipm'"):
            cls._check_attack("ipm", (1,), worker_number=8)
        with pytest.raises(ValueError, match="needs an attack"):  # the general checks come first
            cls._check_attack(None, (1,), worker_number=8)


@pytest.mark.parametrize("algo", ["fed_quant"])
def test_fed_quant_server_rejects_the_attacks(algo, doubles):
    from distributed_learning_simulator_amd import factory
    with pytest.raises(ValueError, match="does not support attack='alie'.*int payloads"):
        factory.get_server(algo, sharded=False, tester=None, worker_number=8, synchronous=True,
                           device=CPU, attack="alie", attackers=(1,))


@pytest.mark.parametrize("algo", ["fed", "fed_quant", "multiround_shapley_value"])
def test_sharded_servers_reject_the_attacks(algo, doubles):
    from distributed_learning_simulator_amd import factory
    with pytest.raises(ValueError, match="does not support attack='sign_flip'.*own clients"):
        factory.get_server(algo, sharded=True, tester=None, worker_number=8, synchronous=True,
                           device=CPU, attack="sign_flip", attackers=(1,))


def _clients(n):
    g = torch.Generator().manual_seed(3)
    base = {"w": torch.randn(6, 10, generator=g), "b": torch.randn(7, generator=g)}
    return [{k: v + 0.01 * torch.randn(v.shape, generator=g) for k, v in base.items()}
            for _ in range(n)]


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


def test_fed_server_alie_round_on_cpu_doubles(doubles):
    from distributed_learning_simulator_amd.layout import ParameterLayout
    clients = _clients(11)
    lay = ParameterLayout.from_dict(clients[0])
    X = np.stack([lay.flatten(c).numpy() for c in clients])
    order = [4, 0, 9, 2, 7, 10, 1, 3, 8, 6, 5]
    seen = {}

    from distributed_learning_simulator_amd.servers.fed_server import FedServer

    class Spy(FedServer):
        def get_subset_model(self, subset):
            seen.update({w: lay.flatten(self.parameters[w][1]).numpy().copy() for w in (3, 7, 4)})
            return super().get_subset_model(subset)

    server = Spy(tester=None, device=CPU, synchronous=True, worker_number=11, attack="alie",
                 attackers=(3, 7), attack_z=1.0)
    q = server.worker_data_queue
    for w in order:
        q.add_task((w, 100 + 7 * w, clients[w]))
    for w in range(11):
        q.get_result(consumer=w)
    agg = q.get_result(consumer=0)
    server.stop()
    assert doubles["craft_rows"] == 1
    honest = [w for w in range(11) if w not in (3, 7)]
    crafted = A.craft_bits(X[honest], 1.0, -1.0)
    assert np.array_equal(seen[3].view(np.uint32), crafted)
    assert np.array_equal(seen[7].view(np.uint32), crafted)
    assert np.array_equal(seen[4].view(np.uint32), X[4].view(np.uint32))
    assert server.last_attack == {"attack": "alie", "attackers": (3, 7), "a": 1.0, "b": -1.0,
                                  "z": 1.0}
    Y = X.copy()
    Y[[3, 7]] = crafted.view(np.float32)
    want = cpu_doubles.fedavg(torch.from_numpy(Y), torch.tensor(order, dtype=torch.int32),
                              torch.tensor([100.0 + 7 * w for w in order]),
                              float(sum(100 + 7 * w for w in order)), lay.P, torch.empty(lay.P))
    assert np.array_equal(lay.flatten(agg).numpy().view(np.uint32), want.numpy().view(np.uint32))
    # no attack: the same bits as a server built without the keywords
    _, a1 = _round(clients, order)
    _, a2 = _round(clients, order, attack=None, attackers=())
    assert np.array_equal(lay.flatten(a1).numpy().view(np.uint32),
                          lay.flatten(a2).numpy().view(np.uint32))
    assert doubles["craft_rows"] == 1


def test_fed_server_ipm_and_sign_flip_rounds_on_cpu_doubles(doubles):
    from distributed_learning_simulator_amd.layout import ParameterLayout
    clients = _clients(6)
    lay = ParameterLayout.from_dict(clients[0])
    X = np.stack([lay.flatten(c).numpy() for c in clients])
    n = np.array([100.0 + 7 * w for w in range(6)], np.float32)

    def mean(Y):
        return cpu_doubles.fedavg(torch.from_numpy(Y), torch.arange(6, dtype=torch.int32),
                                  torch.from_numpy(n), float(n.sum()), lay.P,
                                  torch.empty(lay.P)).numpy()

    for attack, kw in (("ipm", dict(attack_eps=0.5)), ("sign_flip", dict(attack_scale=2.0))):
        server = _fed(worker_number=6, attack=attack, attackers=(1, 4), **kw)
        q = server.worker_data_queue
        for w in range(6):
            q.get_result(consumer=w)
        prev = None
        for rnd in range(2):  # round 1 has no previous model, round 2 uses round 1's
            for w in range(6):
                q.add_task((w, 100 + 7 * w, clients[w]))
            agg = q.get_result(consumer=0)
            for w in range(1, 6):
                q.get_result(consumer=w)
            Y = X.copy()
            if attack == "ipm":
                Y[[1, 4]] = A.craft_bits(X[[0, 2, 3, 5]], -0.5, 0.0, prev).view(np.float32)
                assert server.last_attack == {"attack": "ipm", "attackers": (1, 4), "a": -0.5,
                                              "b": 0.0, "eps": 0.5}
            else:
                for w in (1, 4):
                    Y[w] = A.sign_flip_bits(X[w], 2.0, prev).view(np.float32)
                assert server.last_attack["scale"] == 2.0
            want = mean(Y)
            assert np.array_equal(lay.flatten(agg).numpy().view(np.uint32), want.view(np.uint32)), \
                (attack, rnd)
            prev = want
        assert server.round == 2
        server.stop()


# ------------------------------------------------------------------ simulator
def test_simulator_flags():
    from distributed_learning_simulator_amd.simulator import get_config, server_kwargs
    base = ["--worker_number", "11", "--round", "1", "--distributed_algorithm"]
    cfg = get_config(base + ["fed"])
    assert (cfg.attack, cfg.attackers, cfg.attack_z, cfg.attack_eps, cfg.attack_scale) == \
        (None, (), None, 0.1, 1.0)
    assert server_kwargs(cfg) == {"aggregation_mode": "exact"}
    # a parameter without --attack is not passed on
    assert server_kwargs(get_config(base + ["fed", "--attack_eps", "0.3"])) == \
        {"aggregation_mode": "exact"}
    cfg = get_config(base + ["fed", "--attack", "alie", "--attackers", "3,7", "--attack_z", "1.0"])
    assert server_kwargs(cfg) == {"aggregation_mode": "exact", "attack": "alie",
                                  "attackers": (3, 7), "attack_z": 1.0, "attack_eps": 0.1,
                                  "attack_scale": 1.0}
    cfg = get_config(base + ["fed", "--attack", "ipm", "--attackers", "5", "--attack_eps", "0.25",
                             "--aggregation_rule", "multi_krum", "--byzantine", "1"])
    assert server_kwargs(cfg) == {"aggregation_mode": "exact", "aggregation_rule": "multi_krum",
                                  "trim": 0, "byzantine": 1, "krum_select": None, "attack": "ipm",
                                  "attackers": (5,), "attack_z": None, "attack_eps": 0.25,
                                  "attack_scale": 1.0}
    cfg = get_config(base + ["multiround_shapley_value", "--attack", "sign_flip", "--attackers",
                             "0, 2", "--attack_scale", "4"])
    kw = server_kwargs(cfg)
    assert (kw["attack"], kw["attackers"], kw["attack_scale"], kw["utility_metric"]) == \
        ("sign_flip", (0, 2), 4.0, "acc")
    # the keyword arguments are the server's: they construct one
    from distributed_learning_simulator_amd.servers.fed_server import FedServer
    ok = {k: v for k, v in server_kwargs(get_config(
        base + ["fed", "--attack", "alie", "--attackers", "3,7"])).items() if k.startswith("attack")}
    assert FedServer._check_attack(ok["attack"], ok["attackers"], ok["attack_z"], ok["attack_eps"],
                                   ok["attack_scale"], 11) == (3, 7)
    with pytest.raises(SystemExit):  # the vote holds no fp32 rows
        get_config(base + ["sign_SGD", "--attack", "alie", "--attackers", "1"])
    with pytest.raises(SystemExit):
        get_config(base + ["fed", "--attack", "gaussian"])
    with pytest.raises(SystemExit):
        get_config(base + ["fed", "--attack", "alie", "--attackers", "a,b"])
    assert server_kwargs(get_config(base + ["sign_SGD"])) == {}
