"""CPU checks of differentially private FedAvg: the reference generator of tests/dp_ref.py
against the Random123 known answers and the moments of its normals, the privacy accountant
``aggregation.dp_epsilon``, the argument validation of the four entry points and their
wrappers (all of it runs before any device call), the servers' constructor validation, a
two-round FedServer on the CPU stand-ins, the simulator flags and the build plumbing."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from tests import dp_ref as R

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF, NAN = float("inf"), float("nan")
KAT = [  # (counter, key, output): the Random123 known answers of Philox4x32-10
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]
MOMENT_SEEDS = ((1, 0), (0x9E3779B97F4A7C15, 3), (2 ** 64 - 1, 2 ** 32 + 7))  # (seed, stream id)


# ------------------------------------------------------------------ reference
@pytest.mark.parametrize("counter, key, want", KAT)
def test_reference_known_answers(counter, key, want):
    got = R.philox4x32(np.array(counter, np.uint32), np.array(key, np.uint32))
    assert got.dtype == np.uint32 and tuple(int(v) for v in got) == want


def test_reference_words_follow_the_counter_layout():
    # key = the seed's halves, counter = (block lo, block hi, stream lo, stream hi)
    seed, sid = 0x299f31d0a4093822, 0x0370734413198a2e
    block = 0x85a308d3243f6a88
    assert tuple(int(v) for v in R.words(4, seed, sid, 4 * block)) == KAT[2][2]
    assert tuple(int(v) for v in R.words(4, 0, 0, 0)) == KAT[0][2]
    # any window of the stream is the same words
    whole = R.words(64, 5, 7, 0)
    for first, n in ((1, 5), (3, 1), (4, 9), (7, 57), (63, 1)):
        assert np.array_equal(R.words(n, 5, 7, first), whole[first:first + n])
    assert R.words(0, 5, 7, 3).size == 0
    # the seed, the stream id and the coordinate each change the words
    assert not np.array_equal(R.words(8, 5, 7), R.words(8, 6, 7))
    assert not np.array_equal(R.words(8, 5, 7), R.words(8, 5, 8))
    assert not np.array_equal(R.words(8, 5, 7), R.words(8, 5 + (1 << 32), 7))
    assert not np.array_equal(R.words(8, 5, 7), R.words(8, 5, 7 + (1 << 32)))
    assert not np.array_equal(R.words(4, 5, 7, 0), R.words(4, 5, 7, 1 << 34))  # block hi word


def test_reference_uniforms_and_normals():
    u = R.uniforms(np.array([0, 0x1FF, 0x200, 0xFFFFFFFF], np.uint32))
    assert u.tolist() == [2.0 ** -24, 2.0 ** -24, 3 * 2.0 ** -24, 1.0 - 2.0 ** -24]
    assert np.array_equal(u.astype(np.float32).astype(np.float64), u)  # exact in fp32
    # the extreme radius: u_a = 2^-24 gives sqrt(48 ln 2); the pair is (r cos, r sin)
    top = (1 << 23) - 1
    g, r = R.normal_pairs64(np.array([0, 0, 0, top << 9, top << 9, 0], np.uint32))
    assert abs(r[0] - R.NORMAL_MAX) < 1e-12 and abs(R.NORMAL_MAX - 5.768) < 1e-3
    assert abs(math.hypot(g[0], g[1]) - r[0]) < 1e-12 and g[0] > 5.76 and 0 < g[1] < 1e-5
    assert g[2] > 5.76 and -1e-5 < g[3] < 0  # the angle just below 2 pi
    assert abs(r[4] - math.sqrt(-2 * math.log(1 - 2.0 ** -24))) < 1e-15
    # the pairing is by coordinate: an odd start shares its pair with the coordinate before
    whole = R.normals64(16, 3, 9, 0)
    assert np.array_equal(R.normals64(5, 3, 9, 3), whole[3:8])
    assert np.array_equal(R.normals64(1, 3, 9, 1), whole[1:2])


@pytest.mark.parametrize("seed, sid", MOMENT_SEEDS)
def test_reference_normals_have_the_moments(seed, sid):
    n = 1 << 20
    g = R.normals64(n, seed, sid)
    assert abs(g.mean()) <= 5.0 / math.sqrt(n)
    assert abs(g.var() - 1.0) <= 5.0 * math.sqrt(2.0 / n)
    assert np.abs(g).max() <= R.NORMAL_MAX


def test_reference_step_is_the_clip_step_plus_one_rounded_product():
    from tests import centered_clip_ref as CR
    rng = np.random.default_rng(0)
    X = rng.standard_normal((3, 8)).astype(np.float32)
    c = np.array([0.3, 0.2, 0.5], np.float32)
    z = rng.standard_normal(8).astype(np.float32)
    g = rng.standard_normal(8).astype(np.float32)
    y = CR.step_bits(X, c, z)
    assert np.array_equal(R.step_bits(X, c, z, 0.0, g), y)
    assert np.array_equal(R.step_bits(X, c, z, 0.25, None), y)
    want = (y.view(np.float32) + (np.float32(0.1) * g).astype(np.float32)).astype(np.float32)
    assert np.array_equal(R.step_bits(X, c, z, 0.1, g), want.view(np.uint32))


# ----------------------------------------------------------------- accountant
def _eps(*a):
    from distributed_learning_simulator_amd.aggregation import dp_epsilon
    return dp_epsilon(*a)


@pytest.mark.parametrize("z, T, delta", [(1.0, 1, 1e-5), (0.5, 100, 1e-6), (4.0, 1000, 1e-3)])
def test_epsilon_is_the_closed_form(z, T, delta):
    got = _eps(z, T, delta)
    assert got == pytest.approx(R.epsilon(z, T, delta), rel=1e-14)
    # the closed form is the minimum over the Renyi orders: a search never gets below it
    # and comes close
    search = R.epsilon_by_search(z, T, delta)
    assert got <= search * (1 + 1e-12) and search <= got * (1 + 1e-3)


def test_epsilon_is_monotone_and_handles_the_edges():
    assert _eps(1.0, 10, 1e-5) < _eps(1.0, 11, 1e-5)  # more rounds cost more
    assert _eps(1.0, 10, 1e-5) > _eps(1.1, 10, 1e-5)  # more noise costs less
    assert _eps(1.0, 10, 1e-5) > _eps(1.0, 10, 1e-4)  # a larger delta costs less
    assert _eps(0.0, 3, 1e-5) == INF and _eps(0, 0, 1e-5) == INF
    assert _eps(1.0, 0, 1e-5) == 0.0
    assert type(_eps(2, 5, 0.5)) is float
    for delta in (0.0, 1.0, -1e-5, 1.5, NAN, True, None, "1e-5"):
        with pytest.raises(ValueError, match=r"delta must be in \(0, 1\)"):
            _eps(1.0, 1, delta)
    for T in (-1, 1.0, True, None):
        with pytest.raises(ValueError, match="rounds must be a non-negative integer"):
            _eps(1.0, T, 1e-5)
    for z in (-1.0, INF, NAN, True, None):
        with pytest.raises(ValueError, match="noise_multiplier must be"):
            _eps(z, 1, 1e-5)


# ------------------------------------------------------------------------ ABI
def test_abi_rejects_bad_arguments_without_gpu():
    from distributed_learning_simulator_amd import _native
    L = _native.lib()
    d = ctypes.c_void_p(256)  # 16-byte aligned, never dereferenced
    odd2, odd4 = ctypes.c_void_p(258), ctypes.c_void_p(260)
    err = L.dls_last_error

    for name in (b"dls_philox_u32", b"dls_philox_normal_f32"):
        f = getattr(L, name.decode())

        def gen(out=d, n=8, seed=1, sid=2, first=0):
            return f(out, n, seed, sid, first, None)

        assert gen(out=None) == -1 and b"null pointer" in err() and name in err()
        assert gen(n=-1) == -1 and b"n=-1" in err() and name in err()
        assert gen(first=-1) == -1 and b"first=-1" in err() and name in err()
        assert gen(n=2, first=(1 << 63) - 2) == -1 and b"first + n" in err()
        assert gen(out=odd2) == -2 and b"alignment" in err() and name in err()
        assert gen(n=0) == 0 and gen(n=0, first=(1 << 63) - 1) == 0  # nothing launched
        assert gen(out=odd4, n=0) == 0

    name = b"dls_normal_from_bits_f32"
    assert L.dls_normal_from_bits_f32(None, 8, d, None) == -1 and b"null pointer" in err()
    assert L.dls_normal_from_bits_f32(d, 8, None, None) == -1 and name in err()
    assert L.dls_normal_from_bits_f32(d, -2, d, None) == -1 and b"n=-2" in err()
    assert L.dls_normal_from_bits_f32(d, 7, d, None) == -1 and b"even" in err() and name in err()
    assert L.dls_normal_from_bits_f32(odd2, 8, d, None) == -2 and b"alignment" in err()
    assert L.dls_normal_from_bits_f32(d, 8, odd2, None) == -2 and name in err()
    assert L.dls_normal_from_bits_f32(d, 0, d, None) == 0

    name = b"dls_dp_clip_noise_step_f32"

    def step(U=d, ldu=64, rows=d, K=3, c=d, P=64, z=d, sigma=0.5):
        return L.dls_dp_clip_noise_step_f32(U, ldu, rows, K, c, P, z, sigma, 1, 2, None)

    for arg in ("U", "rows", "c", "z"):
        assert step(**{arg: None}) == -1 and b"null pointer" in err() and name in err()
    assert step(K=0) == -1 and b"DLS_ROBUST_MAX_K=64" in err() and name in err()
    assert step(K=65) == -1 and b"DLS_ROBUST_MAX_K=64" in err() and name in err()
    for sigma in (-1.0, INF, -INF, NAN):
        assert step(sigma=sigma) == -1 and b"sigma" in err() and name in err()
    assert step(sigma=-1.0, P=62) == -1  # the scalar is checked before the layout
    assert step(K=0, sigma=-1.0) == -1 and b"DLS_ROBUST_MAX_K" in err()  # and after K
    assert step(P=-4) == -1 and name in err()
    assert step(P=62) == -2 and b"multiples of 4" in err() and name in err()
    assert step(ldu=60) == -2 and step(ldu=66) == -2 and name in err()
    for arg in ("U", "z"):
        assert step(**{arg: odd4}) == -2 and b"alignment" in err() and name in err()
        assert step(**{arg: ctypes.c_void_p(264)}) == -2
    assert step(c=odd2) == -2 and b"alignment" in err()
    # a 4-byte aligned c passes every check; P == 0 launches nothing
    assert step(P=0, c=odd4) == 0 and step(P=0, sigma=0.0) == 0


def test_wrappers_validate_before_the_library_call():
    from distributed_learning_simulator_amd import _native
    U = torch.zeros(8, 64)
    rows = torch.arange(5, dtype=torch.int32)
    z = torch.zeros(64)
    c = torch.full((5,), 0.2)
    cases = [
        (dict(U=U.double()), "U must be"),
        (dict(U=torch.zeros(64)), "U must be"),
        (dict(rows=rows.long()), "rows must be"),
        (dict(rows=torch.zeros(0, dtype=torch.int32)), "ROBUST_MAX_K=64"),
        (dict(rows=torch.zeros(65, dtype=torch.int32)), "ROBUST_MAX_K=64"),
        (dict(P=62), "multiple of 4"),
        (dict(P=68), "row length"),
        (dict(U=torch.zeros(8, 66)[:, :64]), "row pitch"),
        (dict(c=c.double()), "c must be"),
        (dict(c=torch.zeros(4)), "c must be"),
        (dict(c=torch.zeros(5, device="meta")), "c is on meta"),
        (dict(z=z.double()), "z must be"),
        (dict(z=torch.zeros(60)), "z must be"),
        (dict(z=torch.zeros(128)[::2]), "z must be"),
        (dict(z=torch.zeros(64, device="meta")), "z is on meta"),
        (dict(z=U[2]), "U and z overlap"),
        (dict(sigma=-0.5), "sigma=-0.5 must be finite in fp32 and >= 0"),
        (dict(sigma=INF), "sigma"), (dict(sigma=NAN), "sigma"), (dict(sigma=1e39), "sigma"),
        (dict(sigma=True), "sigma"), (dict(sigma=None), "sigma"),
        (dict(seed=-1), "seed=-1 must be an integer in 0..2\\^64 - 1"),
        (dict(seed=1 << 64), "seed="), (dict(seed=1.0), "seed="), (dict(seed=True), "seed="),
        (dict(stream_id=-1), "stream_id=-1"), (dict(stream_id=1 << 64), "stream_id="),
        (dict(U=torch.zeros(8 * 64 + 1)[1:].view(8, 64)), "16-byte aligned"),
        (dict(z=torch.zeros(65)[1:]), "16-byte aligned"),
    ]
    for change, what in cases:
        kw = dict(U=U, rows=rows, c=c, P=64, z=z, sigma=0.5, seed=1, stream_id=2)
        kw.update(change)
        with pytest.raises(RuntimeError, match="dp_clip_noise_step: .*" + what):
            _native.dp_clip_noise_step(**kw)
    # valid operands reach the library, which has no CPU path
    with pytest.raises(RuntimeError, match="not on the GPU"):
        _native.dp_clip_noise_step(U, rows, c, 64, z, 0.5, 1, 2)
    with pytest.raises(RuntimeError, match="not on the GPU"):
        _native.dp_clip_noise_step(U, rows, c, 64, z, 0.0, 2 ** 64 - 1, 2 ** 64 - 1)

    for fn, dtype in ((_native.philox_u32, torch.int32), (_native.philox_normal, torch.float32)):
        name = fn.__name__ + ("_f32" if fn is _native.philox_normal else "")
        for kw, what in ((dict(n=-1), "n=-1"), (dict(first=-1), "first=-1"),
                         (dict(n=2, first=(1 << 63) - 2), "first \\+ n"),
                         (dict(seed=-1), "seed=-1"), (dict(seed=1 << 64), "seed="),
                         (dict(stream_id=1.5), "stream_id=1.5"),
                         (dict(out=None), "out or device is needed"),
                         (dict(out=torch.zeros(8, dtype=torch.float64)), "out must be"),
                         (dict(out=torch.zeros(4, dtype=dtype)), "out must be"),
                         (dict(out=torch.zeros(16, dtype=dtype)[::2]), "out must be")):
            args = dict(n=8, seed=1, stream_id=2, first=0, out=torch.zeros(8, dtype=dtype))
            args.update(kw)
            with pytest.raises(RuntimeError, match=name + ": .*" + what):
                fn(**args)
        with pytest.raises(RuntimeError, match="not on the GPU"):
            fn(8, 1, 2, out=torch.zeros(8, dtype=dtype))
        with pytest.raises(RuntimeError, match="not on the GPU"):
            fn(8, 1, 2, device=CPU)

    bits = torch.zeros(8, dtype=torch.int32)
    for kw, what in ((dict(bits=bits.long()), "bits must be"),
                     (dict(bits=torch.zeros(16, dtype=torch.int32)[::2]), "bits must be"),
                     (dict(bits=bits[:7]), "n=7 words, not word pairs"),
                     (dict(out=torch.zeros(8, dtype=torch.float64)), "out must be"),
                     (dict(out=torch.zeros(6)), "out must be"),
                     (dict(out=torch.zeros(8, device="meta")), "out is on meta")):
        args = dict(bits=bits, out=torch.zeros(8))
        args.update(kw)
        with pytest.raises(RuntimeError, match="normal_from_bits: .*" + what):
            _native.normal_from_bits(**args)
    with pytest.raises(RuntimeError, match="not on the GPU"):
        _native.normal_from_bits(bits)
    assert abs(_native.NORMAL_MAX - R.NORMAL_MAX) < 1e-15


# -------------------------------------------------------------------- servers
@pytest.fixture
def doubles(monkeypatch):
    R.install(monkeypatch)


def _fed(**kw):
    from distributed_learning_simulator_amd.servers.fed_server import FedServer
    return FedServer(tester=None, device=CPU, synchronous=True, **kw)


def test_fed_server_accepts_the_options(doubles):
    from distributed_learning_simulator_amd.servers import fed_server as FS
    assert FS.DP_DEFAULTS == {"dp_clip": None, "dp_noise_multiplier": 1.0, "dp_seed": 0,
                              "dp_delta": 1e-5}
    assert all(FS.OPTIONS[name].feature == "dp" for name in FS.DP_DEFAULTS)
    s = _fed(worker_number=4)
    assert (s.dp_clip, s.dp_noise_multiplier, s.dp_seed, s.dp_delta) == (None, 1.0, 0, 1e-5)
    assert s.last_dp == {} and FS.FedServer._dp_unsupported is None
    s = _fed(worker_number=64, dp_clip=2, dp_noise_multiplier=0, dp_seed=2 ** 64 - 1,
             dp_delta=0.5)
    assert (s.dp_clip, s.dp_noise_multiplier, s.dp_seed, s.dp_delta) == (2.0, 0.0, 2 ** 64 - 1, 0.5)
    assert type(s.dp_clip) is float and type(s.dp_noise_multiplier) is float
    s = _fed(worker_number=4, dp_clip=1.0, server_optimizer="adam")  # post-processing
    assert s.server_optimizer == "adam"
    s = _fed(worker_number=4, dp_clip=1.0, attack="sign_flip", attackers=(1,))
    # the frozen name lists keep their contents
    assert list(FS.RULES) == ["mean", "median", "trimmed_mean", "multi_krum", "geometric_median",
                              "centered_clip", "mean_around_median", "bulyan", "foolsgold"]
    assert FS.ATTACKS == ("alie", "ipm", "sign_flip")
    assert FS.SERVER_OPTIMIZERS == ("sgd", "adagrad", "adam", "yogi")


@pytest.mark.parametrize("kw, what", [
    (dict(dp_noise_multiplier=0.5), "dp_noise_multiplier=0.5 needs dp_clip set.*not None"),
    (dict(dp_seed=7), "dp_seed=7 needs dp_clip set"),
    (dict(dp_delta=1e-6), "dp_delta=1e-06 needs dp_clip set"),
    (dict(dp_clip=0.0), "dp_clip must be a positive finite number"),
    (dict(dp_clip=-1.0), "dp_clip must be a positive finite number"),
    (dict(dp_clip=INF), "dp_clip must be a positive finite number"),
    (dict(dp_clip=NAN), "dp_clip must be a positive finite number"),
    (dict(dp_clip="1"), "dp_clip must be a positive finite number"),
    (dict(dp_clip=True), "dp_clip must be a positive finite number"),
    (dict(dp_clip=1.0, dp_noise_multiplier=-0.1), "dp_noise_multiplier must be non-negative"),
    (dict(dp_clip=1.0, dp_noise_multiplier=INF), "dp_noise_multiplier must be a finite number"),
    (dict(dp_clip=1.0, dp_noise_multiplier=None), "dp_noise_multiplier must be a finite number"),
    (dict(dp_clip=1.0, dp_seed=-1), "dp_seed must be a non-negative integer"),
    (dict(dp_clip=1.0, dp_seed=1.0), "dp_seed must be a non-negative integer"),
    (dict(dp_clip=1.0, dp_seed=True), "dp_seed must be a non-negative integer"),
    (dict(dp_clip=1.0, dp_seed=2 ** 64), r"dp_seed must be an integer in 0..2\^64 - 1"),
    (dict(dp_clip=1.0, dp_delta=0.0), r"dp_delta must be in \(0, 1\)"),
    (dict(dp_clip=1.0, dp_delta=1.0), r"dp_delta must be in \(0, 1\)"),
    (dict(dp_clip=1.0, dp_delta=NAN), "dp_delta must be a finite number"),
    (dict(dp_clip=1.0, aggregation_rule="median"),
     "dp_clip=1.0 needs aggregation_rule='mean' and aggregation_mode='exact'.*'median'"),
    (dict(dp_clip=1.0, aggregation_rule="centered_clip"), "needs aggregation_rule='mean'"),
    (dict(dp_clip=1.0, aggregation_mode="fma"), "aggregation_mode='exact'.*'fma'"),
    (dict(dp_clip=1.0, worker_number=65), "ROBUST_MAX_K=64 clients, not worker_number=65"),
    (dict(attack="gaussian", attackers=(1,)), "attack must be None or one of"),
])
def test_fed_server_rejects(kw, what):
    """Every case raises before the GPU is needed (no doubles installed)."""
    args = dict(worker_number=10)
    args.update(kw)
    with pytest.raises(ValueError, match=what):
        _fed(**args)


@pytest.mark.parametrize("algo, why", [
    ("fed_quant", "int payloads"), ("fed_topk", "sparse updates"),
    ("GTG_shapley_value", "release of its own"), ("multiround_shapley_value", "release of its own")])
def test_other_servers_refuse_dp(algo, why, doubles):
    from distributed_learning_simulator_amd import factory
    more = {"initial_model": {"w": torch.zeros(8)}} if algo == "fed_topk" else {}
    with pytest.raises(ValueError, match=r"does not support dp_clip=1.0 \(.*" + why
                                         + r".*FedServer .* runs differentially private FedAvg"):
        factory.get_server(algo, sharded=False, tester=None, worker_number=4, synchronous=True,
                           device=CPU, dp_clip=1.0, **more)
    with pytest.raises(ValueError, match="dp_seed=3 needs dp_clip set"):
        factory.get_server(algo, sharded=False, tester=None, worker_number=4, synchronous=True,
                           device=CPU, dp_seed=3, **more)


@pytest.mark.parametrize("algo", ["fed", "fed_quant", "GTG_shapley_value",
                                  "multiround_shapley_value"])
def test_sharded_servers_refuse_dp(algo, doubles):
    from distributed_learning_simulator_amd import factory
    with pytest.raises(ValueError, match="does not support dp_clip=0.5"):
        factory.get_server(algo, sharded=True, tester=None, worker_number=4, synchronous=True,
                           device=CPU, dp_clip=0.5)


# ------------------------------------------------------------- the round trip
SHAPES = {"a.weight": (5, 13), "a.bias": (5,), "b.weight": (3, 5)}  # padded to 64s: gaps


def _clients(K, seed):
    g = torch.Generator().manual_seed(seed)
    first = {n: torch.randn(s, generator=g) for n, s in SHAPES.items()}
    rounds = [[{n: first[n] + (3.0 if w == 0 else 0.05) * torch.randn(s, generator=g)
                for n, s in SHAPES.items()} for w in range(K)] for _ in range(2)]
    return first, rounds


def _two_rounds(K=5, **kw):
    """Two rounds of a FedServer that starts from a model; the aggregates and the server."""
    from distributed_learning_simulator_amd.servers.fed_server import FedServer
    first, rounds = _clients(K, 11)

    class Started(FedServer):
        def _initial_model(self):
            return {n: v.clone() for n, v in first.items()}

    server = Started(tester=None, device=CPU, synchronous=True, worker_number=K, **kw)
    q = server.worker_data_queue
    for w in range(K):
        q.get_result(consumer=w)  # the initial broadcast
    out, extra = [], []
    for clients in rounds:
        for w in (3, 1, 4, 0, 2):  # any arrival order: the clients are taken in id order
            q.add_task((w, 100 + 7 * w, clients[w]))
        agg = q.get_result(consumer=0)
        for w in range(1, K):
            q.get_result(consumer=w)
        out.append({n: v.clone() for n, v in agg.items()})
        extra.append(dict(server.last_dp))
    return out, extra, server


def _bits(model):
    return np.concatenate([v.numpy().ravel().view(np.uint32) for v in model.values()])


def test_two_rounds_are_reproducible_and_seeded(doubles):
    a, info, server = _two_rounds(dp_clip=1.0, dp_noise_multiplier=0.5, dp_seed=7)
    b, _, _ = _two_rounds(dp_clip=1.0, dp_noise_multiplier=0.5, dp_seed=7)
    c, _, _ = _two_rounds(dp_clip=1.0, dp_noise_multiplier=0.5, dp_seed=8)
    for r in range(2):
        assert np.array_equal(_bits(a[r]), _bits(b[r]))
        assert not np.array_equal(_bits(a[r]), _bits(c[r]))
    # the two rounds draw from different streams: the noise of round 2 is not round 1's
    plain, _, _ = _two_rounds(dp_clip=1.0, dp_noise_multiplier=0.0, dp_seed=7)
    n1 = torch.cat([(a[0][n] - plain[0][n]).ravel() for n in SHAPES])
    assert float(n1.abs().max()) > 0 and float(n1.abs().max()) <= 5.8 * 0.5 * 1.0 / 5 * 1.01
    # last_dp: the latest round's info and the composed epsilon
    assert server.round == 2
    for r, d in enumerate(info):
        assert sorted(d) == ["clipped_fraction", "delta", "epsilon", "norms", "rejected",
                             "releases", "round", "scales", "sigma"]
        assert d["round"] == d["releases"] == r + 1 and d["rejected"] == [] and d["delta"] == 1e-5
        assert d["sigma"] == float(np.float32(0.5 * 1.0 / 5))
        assert d["epsilon"] == pytest.approx(R.epsilon(0.5, r + 1, 1e-5), rel=1e-14)
        assert sorted(d["norms"]) == sorted(d["scales"]) == [0, 1, 2, 3, 4]
        # worker 0 sits far away and is clipped; its scale is clip / norm
        assert d["scales"][0] == pytest.approx(1.0 / d["norms"][0]) and d["norms"][0] > 1.0
        assert all(d["scales"][w] == (1.0 if d["norms"][w] <= 1.0 else 1.0 / d["norms"][w])
                   for w in range(5))
        assert d["clipped_fraction"] == sum(1 for s in d["scales"].values() if s < 1.0) / 5
    # round 1: the four clients near the start are inside the radius
    assert all(info[0]["scales"][w] == 1.0 for w in (1, 2, 3, 4))
    assert info[0]["clipped_fraction"] == 0.2
    assert info[1]["epsilon"] > info[0]["epsilon"]


def test_noise_multiplier_zero_is_centered_clip_with_one_step(doubles):
    a, info, _ = _two_rounds(dp_clip=0.75, dp_noise_multiplier=0.0)
    b, _, _ = _two_rounds(aggregation_rule="centered_clip", cc_iters=1, cc_tau=0.75)
    for r in range(2):
        assert np.array_equal(_bits(a[r]), _bits(b[r]))
    assert info[1]["sigma"] == 0.0 and info[1]["epsilon"] == INF


def test_subset_model_carries_no_noise_and_books_nothing(doubles):
    from distributed_learning_simulator_amd.servers.fed_server import FedServer
    first, rounds = _clients(5, 11)
    seen = []

    class Spy(FedServer):
        def _initial_model(self):
            return {n: v.clone() for n, v in first.items()}

        def _before_aggregate(self):
            for subset in ((0, 1, 2, 3, 4), (4, 2, 0), (0, 2, 4), ()):
                seen.append({n: v.clone() for n, v in self.get_subset_model(subset).items()})
            assert self.last_dp == {}

    server = Spy(tester=None, device=CPU, synchronous=True, worker_number=5, dp_clip=0.75,
                 dp_noise_multiplier=2.0, dp_seed=3)
    for w in range(5):
        server.worker_data_queue.add_task((w, 10, rounds[0][w]))
    noisy = server.worker_data_queue.get_result(consumer=0)
    plain, _, _ = _two_rounds(dp_clip=0.75, dp_noise_multiplier=0.0)
    assert np.array_equal(_bits(seen[0]), _bits(plain[0]))  # the whole round without noise
    assert not np.array_equal(_bits(noisy), _bits(plain[0]))
    assert np.array_equal(_bits(seen[1]), _bits(seen[2]))  # the clients in id order
    assert not np.array_equal(_bits(seen[1]), _bits(seen[0]))
    assert np.array_equal(_bits(seen[3]), _bits(first))  # the empty subset: the previous model
    assert server.last_dp["releases"] == 1


def test_a_round_without_a_previous_model_raises(doubles):
    _, rounds = _clients(3, 5)
    server = _fed(worker_number=3, dp_clip=1.0)
    server.worker_data_queue.add_task((0, 10, rounds[0][0]))
    server.worker_data_queue.add_task((1, 10, rounds[0][1]))
    with pytest.raises(ValueError, match="dp_clip=1.0: no previous global model in round 1"):
        server.worker_data_queue.add_task((2, 10, rounds[0][2]))


def test_a_server_optimizer_steps_on_the_noised_aggregate(doubles, monkeypatch):
    from distributed_learning_simulator_amd import _native
    from tests import server_opt_ref as SR
    calls = []

    def server_opt_step(kind, agg, x, m, v, out, P, lr, beta1, beta2, tau, stream=None):
        calls.append(agg.clone())
        o, _ = SR.sgd(agg.numpy(), x.numpy(), None, SR.coeffs(lr, beta1, beta2, tau))
        out.copy_(torch.from_numpy(o))
        return out

    monkeypatch.setattr(_native, "server_opt_step", server_opt_step)
    a, _, server = _two_rounds(dp_clip=1.0, dp_noise_multiplier=0.5, dp_seed=7,
                               server_optimizer="sgd", server_lr=0.5)
    b, _, _ = _two_rounds(dp_clip=1.0, dp_noise_multiplier=0.5, dp_seed=7)
    lay = server.parameters.store.layout
    assert len(calls) == 2
    assert np.array_equal(_bits(lay.views(calls[0])), _bits(b[0]))  # the noised aggregate
    # the padding between the tensors is zero again after the noise
    used = torch.zeros(lay.P, dtype=torch.bool)
    for o, n in zip(lay.offsets, lay.numels):
        used[o:o + n] = True
    assert not used.all() and bool((calls[0][~used] == 0).all())
    assert not np.array_equal(_bits(a[0]), _bits(b[0]))  # half the step


def test_store_dp_mean_rejects_a_non_finite_client(doubles):
    from distributed_learning_simulator_amd.aggregation import ClientUpdateStore
    from distributed_learning_simulator_amd.layout import ParameterLayout
    store = ClientUpdateStore(ParameterLayout([("w", (64,))]), CPU, capacity=4)
    rng = np.random.default_rng(1)
    store.U.copy_(torch.from_numpy(rng.standard_normal((4, 64)).astype(np.float32)))
    store.U[2, 5] = INF
    start = torch.zeros(64)
    flat, info = store.dp_mean([3, 2, 0], ["c", "b", "a"], start, 2.0, 1.5, 9, 4)
    assert info["rejected"] == ["b"] and sorted(info["norms"]) == ["a", "c"]
    assert info["sigma"] == float(np.float32(1.5 * 2.0 / 2))  # divided by the number kept
    X = store.U.numpy()[[0, 3]]
    from tests import centered_clip_ref as CR
    _, _, c = CR.scales(CR.sqdist_to(X, start.numpy()), 2.0)
    g = R.normals64(64, 9, 4).astype(np.float32)
    assert np.array_equal(flat.numpy().view(np.uint32), R.step_bits(X, c, start.numpy(), 1.5, g))
    assert bool((start == 0).all())  # the start is never modified
    for kw, what in ((dict(clip=0.0), "clip must be a positive finite"),
                     (dict(noise_multiplier=-1.0), "noise_multiplier must be >= 0"),
                     (dict(noise_multiplier=NAN), "noise_multiplier must be a finite"),
                     (dict(ids=["a", "a", "b"]), "one distinct id per row"),
                     (dict(start=torch.zeros(60)), "start must be an fp32 vector")):
        args = dict(rows=[3, 2, 0], ids=["c", "b", "a"], start=start, clip=2.0,
                    noise_multiplier=1.5, seed=9, stream_id=4)
        args.update(kw)
        with pytest.raises(ValueError, match=what):
            store.dp_mean(**args)
    store.U[:, 0] = NAN
    with pytest.raises(ValueError, match="no client has a finite distance"):
        store.dp_mean([0, 1], [0, 1], start, 2.0, 1.0, 9, 4)


# ------------------------------------------------------------------ simulator
def test_simulator_flags():
    from distributed_learning_simulator_amd.simulator import get_config, server_kwargs
    base = ["--worker_number", "4", "--round", "2", "--distributed_algorithm"]
    cfg = get_config(base + ["fed"])
    assert (cfg.dp_clip, cfg.dp_noise_multiplier, cfg.dp_seed, cfg.dp_delta) == (None,) * 4
    assert server_kwargs(cfg) == {"aggregation_mode": "exact"}
    cfg = get_config(base + ["fed", "--dp_clip", "1.0", "--dp_noise_multiplier", "0.5",
                             "--dp_seed", "7"])
    assert server_kwargs(cfg) == {"aggregation_mode": "exact", "dp_clip": 1.0,
                                  "dp_noise_multiplier": 0.5, "dp_seed": 7}
    cfg = get_config(base + ["fed", "--dp_clip", "2", "--dp_delta", "1e-6",
                             "--server_optimizer", "adam"])
    assert server_kwargs(cfg) == {"aggregation_mode": "exact", "server_optimizer": "adam",
                                  "dp_clip": 2.0, "dp_delta": 1e-6}
    for algo in ("sign_SGD", "fed_quant", "fed_topk", "GTG_shapley_value",
                 "multiround_shapley_value"):
        for flag, value in (("--dp_clip", "1.0"), ("--dp_noise_multiplier", "0.5"),
                            ("--dp_seed", "7"), ("--dp_delta", "1e-6")):
            with pytest.raises(SystemExit):
                get_config(base + [algo, flag, value])
    with pytest.raises(SystemExit):
        get_config(base + ["fed", "--dp_seed", "seven"])
    # a parameter without --dp_clip is the server's refusal
    cfg = get_config(base + ["fed", "--dp_seed", "7"])
    with pytest.raises(ValueError, match="dp_seed=7 needs dp_clip set"):
        _fed(worker_number=4, **{k: v for k, v in server_kwargs(cfg).items()
                                 if k != "aggregation_mode"})
    from distributed_learning_simulator_amd import simulator
    assert "[--dp_clip 1.0 [--dp_noise_multiplier 1.0] [--dp_seed 0] [--dp_delta 1e-5]]" \
        in simulator.__doc__
    with open(os.path.join(ROOT, "README.md")) as fh:
        assert "--dp_clip" in fh.read()


# ------------------------------------------------------------ source plumbing
def test_source_plumbing():
    from distributed_learning_simulator_amd import _native
    csrc = os.path.join(ROOT, "distributed_learning_simulator_amd", "csrc")
    with open(os.path.join(csrc, "Makefile")) as fh:
        srcs = next(line for line in fh if line.startswith("SRCS :=")).split()[2:]
    assert srcs[-1] == "dpnoise.hip" and srcs[-2] == "topk.hip"
    hashed = _native.CSRC_HASHED
    assert hashed[:len(srcs)] == srcs and hashed[len(srcs)] == "dls_common.h"
    with open(os.path.join(ROOT, "include", "dls_hip.h")) as fh:
        header = fh.read()
    assert "#define DLS_ABI_VERSION 2" in header
    assert "sqrt(48 ln 2)" in header  # the truncated tail is stated
    _p, _i32, _i64, _f32, _u64 = (ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float,
                                  ctypes.c_uint64)
    want = {
        "dls_philox_u32": ([_p, _i64, _u64, _u64, _i64, _p], _i32),
        "dls_philox_normal_f32": ([_p, _i64, _u64, _u64, _i64, _p], _i32),
        "dls_normal_from_bits_f32": ([_p, _i64, _p, _p], _i32),
        "dls_dp_clip_noise_step_f32": ([_p, _i64, _p, _i32, _p, _i64, _p, _f32, _u64, _u64, _p],
                                       _i32),
    }
    L = _native.lib()
    with open(os.path.join(csrc, "dpnoise.hip")) as fh:
        src = fh.read()
    for name, sig in want.items():
        assert "int " + name + "(" in header
        assert _native.SIGNATURES[name] == sig and hasattr(L, name)
        assert 'extern "C" int ' + name + "(" in src
    assert L.dls_abi_version() == 2
    assert L.dls_source_hash().decode() == _native.source_hash()
    assert "getenv" not in src and "atomic" not in src.lower().replace("no atomics", "")
    assert "asm" not in src  # plain C++ only
