"""CPU checks of the FoolsGold feature: ``aggregation.foolsgold_weights`` on hand-built
Gram matrices and against the numpy restatement tests/foolsgold_ref.py, the reference's
own exact sums, the argument validation of dls_rows_gram_f32 / dls_history_gram_f32 and
their wrappers (all of it runs before any device call), the servers' constructor
validation, the simulator flags and the build plumbing."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import cpu_doubles
from tests import foolsgold_ref as FR

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")


def _weights(*a, **kw):
    from distributed_learning_simulator_amd.aggregation import foolsgold_weights
    return foolsgold_weights(*a, **kw)


def _gram(X):
    X = np.asarray(X, np.float64)
    return X @ X.T


def _independent(K, P=4000, seed=0):
    return np.random.default_rng(seed).standard_normal((K, P))


# ------------------------------------------------------------------ reference
def test_reference_sums_are_exact():
    rng = np.random.default_rng(0)
    X = (rng.standard_normal((5, 301)) * 10.0 ** rng.integers(-6, 6, (5, 301))).astype(np.float32)
    assert np.array_equal(FR.gram_exact(X), FR.gram_exact_fsum(X))  # Sum2 against math.fsum
    assert np.array_equal(FR.abs_products(X), FR.gram_exact_fsum(np.abs(X)))
    Xg = FR.grid_rows(7, 1003, 1, corr=0.5)  # the matrix-product path
    assert np.array_equal(FR.gram_exact(Xg), FR.gram_exact_fsum(Xg))
    assert np.array_equal(FR.abs_products(Xg), FR.gram_exact_fsum(np.abs(Xg)))
    # one rounding per operation in the fold
    h, x, b = np.float32(0.1), np.float32(1.0 + 2.0 ** -23), np.float32(0.3)
    got = FR.fold_bits(np.array([[h]]), np.array([[x]]), np.array([b]))
    assert got[0, 0] == np.float32(h + np.float32(x - b)).view(np.uint32)
    assert FR.fold_bits(np.array([[h]]), np.array([[x]]))[0, 0] == np.float32(h + x).view(np.uint32)


# ---------------------------------------------------------- foolsgold_weights
def test_two_identical_clients_among_independent_ones():
    X = _independent(10)
    X[7] = X[3]
    alpha, info = _weights(_gram(X))
    assert alpha == [0.0 if i in (3, 7) else 1.0 for i in range(10)]
    assert all(type(a) is float for a in alpha) and info["rejected"] == []
    assert info["similarity"][3] == info["similarity"][7] == 1.0
    assert max(s for i, s in enumerate(info["similarity"]) if i not in (3, 7)) < 0.1
    ralpha, rsim, rrej = FR.weights(_gram(X))
    assert ralpha.tolist() == alpha and rrej == []
    assert np.allclose(rsim, info["similarity"], rtol=1e-12, atol=0)


def test_pardoning_keeps_an_honest_client_above_the_sybil_it_resembles():
    # sybils s0, s1 nearly alike (cosine 0.999); honest h resembles them (0.7); two others
    e = np.eye(6)
    s0 = e[0]
    s1 = 0.999 * e[0] + np.sqrt(1 - 0.999 ** 2) * e[1]
    h = 0.7 * e[0] + np.sqrt(0.51) * e[2]
    X = np.stack([s0, s1, h, e[3], e[4]])
    alpha, info = _weights(_gram(X))
    # pardoned: 0.7 * 0.7 / 0.999 instead of 0.7
    sim = 0.7 * 0.7 / 0.999
    assert abs(info["similarity"][2] - sim) < 1e-9
    assert alpha[0] == alpha[1] == 0.0 and alpha[3] == alpha[4] == 1.0
    want = np.log((1 - sim) / sim) + 0.5
    assert 0.0 < want < 1.0 and abs(alpha[2] - want) < 1e-6 and alpha[2] > alpha[0]
    # unpardoned, 1 - 0.7 would have mapped to weight 0 like the sybils
    assert np.log(0.3 / 0.7) + 0.5 < 0
    assert np.allclose(FR.weights(_gram(X))[0], alpha, rtol=1e-12, atol=0)
    # kappa scales the weight before the clip
    assert _weights(_gram(X), kappa=0.5)[0][2] == pytest.approx(0.5 * alpha[2])


def test_single_client_all_identical_and_zero_norm():
    alpha, info = _weights([[4.0]])
    assert alpha == [1.0] and info["rejected"] == [] and np.isnan(info["similarity"][0])
    assert _weights([[0.0]])[0] == [1.0]
    x = _independent(1)[0]
    alpha, info = _weights(_gram(np.stack([x] * 5)))
    assert alpha == [0.0] * 5 and info["similarity"] == [1.0] * 5
    # a zero-norm client has cosine 0 to everyone: full weight, and no division by zero
    X = _independent(4)
    X[2] = 0.0
    alpha, info = _weights(_gram(X))
    assert alpha == [1.0] * 4 and info["rejected"] == []
    assert info["similarity"][2] <= 0.0 + 1e-300 and FR.weights(_gram(X))[0].tolist() == alpha
    # two zero-norm clients are not sybils of each other
    X[1] = 0.0
    assert _weights(_gram(X))[0] == [1.0] * 4


def test_non_finite_diagonal_is_rejected():
    X = _independent(6)
    X[4] = X[1]
    G = _gram(X)
    G[2, :] = G[:, 2] = NAN
    G[5, :] = G[:, 5] = INF
    alpha, info = _weights(G)
    assert info["rejected"] == [2, 5] and alpha == [1.0, 0.0, 0.0, 1.0, 0.0, 0.0]
    assert np.isnan(info["similarity"][2]) and np.isnan(info["similarity"][5])
    ralpha, _, rrej = FR.weights(G)
    assert ralpha.tolist() == alpha and rrej == [2, 5]
    # only one finite client left: weight 1
    G = _gram(_independent(3))
    G[0, 0] = G[2, 2] = NAN
    assert _weights(G)[0] == [0.0, 1.0, 0.0]
    G[1, 1] = -1.0
    alpha, info = _weights(G)
    assert alpha == [0.0] * 3 and info["rejected"] == [0, 1, 2]


def test_permutation_invariance_and_the_reference():
    rng = np.random.default_rng(5)
    for K in (2, 3, 9, 33, 64):
        X = _independent(K, P=50, seed=K) + 0.8 * rng.standard_normal(50)[None, :]
        if K > 3:
            X[K - 1] = X[1] * 3.0  # a scaled twin
        G = _gram(X)
        for kappa in (0.5, 1.0, 4):
            alpha, info = _weights(G, kappa)
            assert all(0.0 <= a <= 1.0 for a in alpha)
            ralpha, rsim, _ = FR.weights(G, kappa)
            assert np.allclose(ralpha, alpha, rtol=1e-9, atol=1e-12)
            assert np.allclose(rsim, info["similarity"], rtol=1e-9, atol=1e-12)
            perm = rng.permutation(K)
            palpha, pinfo = _weights(G[np.ix_(perm, perm)], kappa)
            assert palpha == [alpha[i] for i in perm]
            assert pinfo["similarity"] == [info["similarity"][i] for i in perm]
    assert _weights(torch.tensor(G))[0] == _weights(G.tolist())[0]


def test_weights_value_errors():
    for kappa in (0, 0.0, -1.0, INF, NAN, True, "1", None):
        with pytest.raises(ValueError, match="kappa must be a positive finite number"):
            _weights([[1.0]], kappa)
    for G in ([], [[1.0, 2.0]], [[1.0, 0.0], [0.0]]):
        with pytest.raises(ValueError, match=r"G must be a \[K, K\] matrix"):
            _weights(G)


# ------------------------------------------------------------------------ ABI
def test_abi_rejects_bad_arguments_without_gpu():
    from distributed_learning_simulator_amd import _native
    L = _native.lib()
    d = ctypes.c_void_p(256)  # 16-byte aligned, never dereferenced
    odd, odd8 = ctypes.c_void_p(260), ctypes.c_void_p(264)
    err = L.dls_last_error

    def fold(U=d, ldu=64, rows=d, H=d, ldh=64, hrows=d, K=3, P=64, base=None, G=d, work=d):
        return L.dls_history_gram_f32(U, ldu, rows, H, ldh, hrows, K, P, base, G, work, None)

    def read(U=d, ldu=64, rows=d, K=3, P=64, base=None, G=d, work=d):
        return L.dls_rows_gram_f32(U, ldu, rows, K, P, base, G, work, None)

    for f, name, ptrs in ((fold, b"dls_history_gram_f32", ("U", "rows", "H", "hrows", "G", "work")),
                          (read, b"dls_rows_gram_f32", ("U", "rows", "G", "work"))):
        for arg in ptrs:
            assert f(**{arg: None}) == -1 and b"null pointer" in err() and name in err()
        assert f(K=0) == -1 and b"DLS_ROBUST_MAX_K=64" in err() and name in err()
        assert f(K=65) == -1 and b"DLS_ROBUST_MAX_K=64" in err()
        assert f(P=-4) == -1 and name in err()
        assert f(P=62) == -2 and b"multiples of 4" in err() and name in err()
        assert f(ldu=60) == -2 and f(ldu=66) == -2
        for arg in ("U", "base", "work"):
            assert f(**{arg: odd}) == -2 and b"alignment" in err() and name in err()
            assert f(**{arg: odd8}) == -2
        assert f(G=odd) == -2 and b"alignment" in err()
    assert fold(ldh=60) == -2 and fold(ldh=66) == -2 and fold(H=odd8) == -2
    assert L.dls_rows_gram_workspace(0, 64) == -1 and b"dls_rows_gram_workspace" in err()
    assert L.dls_rows_gram_workspace(65, 64) == -1 and L.dls_rows_gram_workspace(3, -4) == -1
    # the workspace is a function of K and P alone: 32 KiB per wave, at most 1024 waves
    # (a flush period is 7680 coordinates for K <= 8, 1920 / 448 / 96 for K <= 16 / 32 / 64)
    assert L.dls_rows_gram_workspace(1, 4) == 32768 == L.dls_rows_gram_workspace(8, 7680)
    assert L.dls_rows_gram_workspace(8, 7684) == 2 * 32768
    assert L.dls_rows_gram_workspace(16, 1924) == 2 * 32768 == L.dls_rows_gram_workspace(17, 452)
    assert L.dls_rows_gram_workspace(64, 1024 * 96) == 1024 * 32768
    assert L.dls_rows_gram_workspace(64, 1024 * 96 + 4) == 513 * 32768
    assert L.dls_rows_gram_workspace(10, 11_173_962 // 4 * 4 + 64) <= 1024 * 32768


def test_wrappers_validate_before_the_library_call():
    from distributed_learning_simulator_amd import _native
    U, H = torch.zeros(8, 64), torch.zeros(9, 64)
    rows = torch.arange(5, dtype=torch.int32)
    base = torch.zeros(64)
    out = torch.zeros(5, 5, dtype=torch.float64)
    cases = [
        (dict(U=U.double()), "U must be"),
        (dict(U=torch.zeros(64)), "U must be"),
        (dict(rows=rows.long()), "rows must be"),
        (dict(rows=torch.zeros(0, dtype=torch.int32)), "ROBUST_MAX_K=64"),
        (dict(rows=torch.zeros(65, dtype=torch.int32)), "ROBUST_MAX_K=64"),
        (dict(P=62), "multiple of 4"),
        (dict(P=68), "row length"),
        (dict(U=torch.zeros(8, 66)[:, :64]), "row pitch"),
        (dict(base=base.double()), "base must be"),
        (dict(base=torch.zeros(60)), "base must be"),
        (dict(base=torch.zeros(128)[::2]), "base must be"),
        (dict(base=torch.zeros(64, device="meta")), "base is on meta"),
        (dict(out=torch.zeros(5, 5)), "out must be a contiguous fp64"),
        (dict(out=torch.zeros(4, 5, dtype=torch.float64)), "out must be a contiguous fp64"),
        (dict(U=torch.zeros(8 * 64 + 1)[1:].view(8, 64)), "16-byte aligned"),
        (dict(base=torch.zeros(65)[1:]), "16-byte aligned"),
    ]
    for change, what in cases:
        kw = dict(U=U, rows=rows, P=64, base=base, out=out)
        kw.update(change)
        with pytest.raises(RuntimeError, match="rows_gram: .*" + what):
            _native.rows_gram(kw["U"], kw["rows"], kw["P"], base=kw["base"], out=kw["out"])
        with pytest.raises(RuntimeError, match="history_gram: .*" + what):
            _native.history_gram(kw["U"], kw["rows"], H, rows, kw["P"], base=kw["base"],
                                 out=kw["out"])
    for change, what in [
        (dict(H=H.double()), "H must be"),
        (dict(H=torch.zeros(9, 66)[:, :64]), "row pitch"),
        (dict(hrows=rows.long()), "hrows must be"),
        (dict(hrows=torch.arange(4, dtype=torch.int32)), "hrows holds 4 rows, rows holds 5"),
        (dict(H=torch.zeros(9 * 64 + 1)[1:].view(9, 64)), "16-byte aligned"),
        (dict(H=U), "must not overlap"),
    ]:
        kw = dict(H=H, hrows=rows)
        kw.update(change)
        with pytest.raises(RuntimeError, match="history_gram: .*" + what):
            _native.history_gram(U, rows, kw["H"], kw["hrows"], 64, base=base)
    # valid operands reach the library, which has no CPU path
    with pytest.raises(RuntimeError, match="not on the GPU"):
        _native.rows_gram(U, rows, 64, base=base)
    with pytest.raises(RuntimeError, match="not on the GPU"):
        _native.history_gram(U, rows, H, rows, 64)


# -------------------------------------------------------------------- servers
@pytest.fixture
def doubles(monkeypatch):
    cpu_doubles.install(monkeypatch)


def _fed(**kw):
    from distributed_learning_simulator_amd.servers.fed_server import FedServer
    return FedServer(tester=None, device=CPU, synchronous=True, **kw)


def test_fed_server_accepts_foolsgold(doubles):
    s = _fed(worker_number=10, aggregation_rule="foolsgold")
    assert (s.aggregation_rule, s.fg_kappa) == ("foolsgold", 1.0)
    assert s.last_weights == {} and s.last_similarity == {} and s.last_rejected == ()
    assert (s.cc_tau, s.cc_iters, s.gm_iters, s.trim, s.byzantine) == (10.0, 3, 3, 0, 0)
    s.reset_history()  # nothing to forget yet
    s.reset_history(3)
    with pytest.raises(ValueError, match="no folded round"):
        s._foolsgold(None, [0], [0])
    s.stop()
    s = _fed(worker_number=64, aggregation_rule="foolsgold", fg_kappa=2)
    assert s.fg_kappa == 2.0 and type(s.fg_kappa) is float
    s.stop()
    for rule in ("mean", "median", "centered_clip"):  # the default suits every rule
        s = _fed(worker_number=10, aggregation_rule=rule, fg_kappa=1.0)
        assert (s.aggregation_rule, s.fg_kappa) == (rule, 1.0)
        s.stop()


@pytest.mark.parametrize("kw, what", [
    (dict(aggregation_rule="fools_gold"), "aggregation_rule must be one of .*'foolsgold'"),
    (dict(fg_kappa=2.0), "fg_kappa=2.0 needs aggregation_rule='foolsgold', not 'mean'"),
    (dict(aggregation_rule="median", fg_kappa=0.5), "needs aggregation_rule='foolsgold'"),
    (dict(aggregation_rule="centered_clip", fg_kappa=0.5), "needs aggregation_rule='foolsgold'"),
    (dict(aggregation_rule="foolsgold", fg_kappa=0.0), "fg_kappa must be a positive finite"),
    (dict(aggregation_rule="foolsgold", fg_kappa=-1.0), "fg_kappa must be a positive finite"),
    (dict(aggregation_rule="foolsgold", fg_kappa=INF), "fg_kappa must be a positive finite"),
    (dict(aggregation_rule="foolsgold", fg_kappa=NAN), "fg_kappa must be a positive finite"),
    (dict(aggregation_rule="foolsgold", fg_kappa="1"), "fg_kappa must be a positive finite"),
    (dict(aggregation_rule="foolsgold", fg_kappa=True), "fg_kappa must be a positive finite"),
    (dict(aggregation_rule="foolsgold", fg_kappa=None), "fg_kappa must be a positive finite"),
    (dict(aggregation_rule="foolsgold", trim=1), "trim=1 needs aggregation_rule='trimmed_mean'"),
    (dict(aggregation_rule="foolsgold", byzantine=1), "needs aggregation_rule='multi_krum'"),
    (dict(aggregation_rule="foolsgold", cc_tau=1.0), "needs aggregation_rule='centered_clip'"),
    (dict(aggregation_rule="foolsgold", gm_iters=2), "needs aggregation_rule='geometric_median'"),
    (dict(aggregation_rule="foolsgold", aggregation_mode="fma"), "aggregation_rule='mean' only"),
    (dict(aggregation_rule="foolsgold", worker_number=65), "ROBUST_MAX_K=64"),
])
def test_fed_server_rejects(kw, what):
    """Every case raises before the GPU is needed (no doubles installed)."""
    args = dict(worker_number=10)
    args.update(kw)
    with pytest.raises(ValueError, match=what):
        _fed(**args)


@pytest.mark.parametrize("algo", ["fed_quant", "GTG_shapley_value", "multiround_shapley_value"])
def test_other_servers_reject_foolsgold(algo, doubles):
    from distributed_learning_simulator_amd import factory
    with pytest.raises(ValueError, match="does not support aggregation_rule='foolsgold'"
                                         ".*FedServer"):
        factory.get_server(algo, sharded=False, tester=None, worker_number=5, synchronous=True,
                           device=CPU, aggregation_rule="foolsgold", fg_kappa=2.0)
    with pytest.raises(ValueError, match="needs aggregation_rule='foolsgold'"):
        factory.get_server(algo, sharded=False, tester=None, worker_number=5, synchronous=True,
                           device=CPU, fg_kappa=2.0)


@pytest.mark.parametrize("algo", ["fed", "fed_quant", "GTG_shapley_value",
                                  "multiround_shapley_value"])
def test_sharded_servers_reject_foolsgold(algo, doubles):
    from distributed_learning_simulator_amd import factory
    with pytest.raises(ValueError, match="does not support aggregation_rule='foolsgold'"
                                         ".*FedServer"):
        factory.get_server(algo, sharded=True, tester=None, worker_number=5, synchronous=True,
                           device=CPU, aggregation_rule="foolsgold")


# ------------------------------------------------------------------ simulator
def test_simulator_flags():
    from distributed_learning_simulator_amd import simulator
    from distributed_learning_simulator_amd.simulator import get_config, server_kwargs
    base = ["--worker_number", "10", "--round", "1", "--distributed_algorithm"]
    cfg = get_config(base + ["fed", "--aggregation_rule", "foolsgold"])
    assert (cfg.aggregation_rule, cfg.fg_kappa) == ("foolsgold", 1.0)
    assert server_kwargs(cfg) == {"aggregation_mode": "exact", "aggregation_rule": "foolsgold",
                                  "trim": 0, "fg_kappa": 1.0}
    cfg = get_config(base + ["fed", "--aggregation_rule", "foolsgold", "--fg_kappa", "2.5",
                             "--attack", "alie", "--attackers", "3,7"])
    kw = server_kwargs(cfg)
    assert kw["fg_kappa"] == 2.5 and kw["attack"] == "alie" and kw["attackers"] == (3, 7)
    # the other rules' dicts do not hold the new key
    assert get_config(base + ["fed"]).fg_kappa == 1.0
    assert server_kwargs(get_config(base + ["fed"])) == {"aggregation_mode": "exact"}
    assert "fg_kappa" not in server_kwargs(get_config(base + ["fed", "--aggregation_rule",
                                                              "centered_clip"]))
    with pytest.raises(SystemExit):
        get_config(base + ["fed", "--aggregation_rule", "foolsgold", "--fg_kappa", "one"])
    with pytest.raises(SystemExit):  # the vote has no mean to replace
        get_config(base + ["sign_SGD", "--aggregation_rule", "foolsgold"])
    assert "--aggregation_rule foolsgold" in simulator.__doc__


# ------------------------------------------------------------ source plumbing
def test_source_plumbing():
    from distributed_learning_simulator_amd import _native
    with open(os.path.join(ROOT, "include", "dls_hip.h")) as fh:
        header = fh.read()
    assert "int64_t dls_rows_gram_workspace(int32_t K, int64_t P);" in header
    assert "int dls_rows_gram_f32(const float *U, int64_t ldu, const int32_t *rows, int32_t K, " \
        "int64_t P,\n                      const float *base, double *G, void *workspace" in header
    assert "int dls_history_gram_f32(const float *U, int64_t ldu, const int32_t *rows, float *H, " \
        "int64_t ldh," in header
    assert "(120 + 8) * 2^-24 * sum_p |h_a h_b| <= 2^-17 * |h_a| |h_b|" in header
    L = _native.lib()
    _i32, _i64, _p = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    assert _native.SIGNATURES["dls_rows_gram_workspace"] == ([_i32, _i64], _i64)
    assert _native.SIGNATURES["dls_rows_gram_f32"] == \
        ([_p, _i64, _p, _i32, _i64, _p, _p, _p, _p], _i32)
    assert _native.SIGNATURES["dls_history_gram_f32"] == \
        ([_p, _i64, _p, _p, _i64, _p, _i32, _i64, _p, _p, _p, _p], _i32)
    for name in ("dls_rows_gram_workspace", "dls_rows_gram_f32", "dls_history_gram_f32"):
        assert hasattr(L, name)
    assert L.dls_abi_version() == 2
    assert L.dls_source_hash().decode() == _native.source_hash()
    assert "gram.hip" in _native.CSRC_HASHED
    csrc = os.path.join(ROOT, "distributed_learning_simulator_amd", "csrc")
    with open(os.path.join(csrc, "Makefile")) as fh:
        assert "gram.hip" in fh.read()
    with open(os.path.join(csrc, "gram.hip")) as fh:
        src = fh.read()
    assert 'extern "C" int dls_history_gram_f32(' in src
    assert "getenv" not in src and "atomic" not in src.lower().replace("no atomics", "")
    assert "asm" not in src  # ordinary vector stores
