"""GPU checks of the random stream and the fused DP-FedAvg step (csrc/dpnoise.hip) against
tests/dp_ref.py: the words exactly, the normals within the contract's bound of the fp64
transform, the step bit for bit in numpy float32 with the device's own normals, every
refusal of the four entry points, and one simulator round trip."""
import itertools

import numpy as np
import pytest
import torch

from tests import dp_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SEEDS = (0x9E3779B97F4A7C15, (7 << 32) | 3)  # both with a non-zero high half
STREAM_IDS = (0, 2 ** 32 + 7)
# 2^32 - 2 is the issue's; 2^34 - 2 is where the block index enters counter word 1
FIRSTS = (0, 1, 3, 4, 2 ** 32 - 2, 2 ** 34 - 2)
COUNTS = (1, 5, 1027)
BIG_P = 512 * 1024 + 260  # more than 2048 tiles of 256: a wave visits more than one tile


def _native():
    from distributed_learning_simulator_amd import _native
    return _native


def _words(n, seed, sid, first=0):
    return _native().philox_u32(n, seed, sid, first, device=DEV).cpu().numpy().view(np.uint32)


def _normals(n, seed, sid, first=0):
    return _native().philox_normal(n, seed, sid, first, device=DEV).cpu().numpy()


def _from_bits(bits):
    t = torch.from_numpy(np.asarray(bits, np.uint32).view(np.int32).copy()).to(DEV)
    return _native().normal_from_bits(t).cpu().numpy()


def _same(got, want):
    return np.array_equal(np.asarray(got, np.float32).view(np.uint32),
                          np.asarray(want, np.float32).view(np.uint32))


# ------------------------------------------------------------------ the words
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("sid", STREAM_IDS)
def test_words_equal_the_reference(seed, sid):
    for first, n in itertools.product(FIRSTS, COUNTS):
        assert np.array_equal(_words(n, seed, sid, first), R.words(n, seed, sid, first)), (first, n)
    assert _words(0, seed, sid, 3).size == 0


def test_words_do_not_depend_on_the_call():
    seed, sid = SEEDS[0], STREAM_IDS[1]
    whole = _words(1027, seed, sid, 3)
    for cut in (1, 513, 1025):  # odd split points
        parts = np.concatenate([_words(cut, seed, sid, 3), _words(1027 - cut, seed, sid, 3 + cut)])
        assert np.array_equal(parts, whole), cut
    # into a larger buffer: only n elements are written; another HIP stream: the same words
    out = torch.full((16,), -1, dtype=torch.int32, device=DEV)
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        _native().philox_u32(5, seed, sid, 3, out=out, stream=side)
    side.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(got[:5].view(np.uint32), whole[:5]) and (got[5:] == -1).all()


# ---------------------------------------------------------------- the normals
def _check_normals(bits, tag):
    got = _from_bits(bits).astype(np.float64)
    want, r = R.normal_pairs64(bits)
    err = np.abs(got - want)
    worst = float((err / (2.0 ** -23 * r)).max())
    print(f"{tag}: max |g_gpu - g_ref| / (2^-23 r) = {worst:.4f} "
          f"(bound {R.E_LOG / 2 + R.E_TRIG + 1.5:.4f})")
    assert (err <= R.normal_bound(r)).all(), (tag, worst)
    assert np.abs(got).max() <= R.NORMAL_MAX * (1 + 2.0 ** -22)


def test_normals_of_chosen_words_are_within_the_bound():
    kat = np.array([0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8,
                    0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd,
                    0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1], np.uint32)
    _check_normals(kat, "known-answer blocks")
    rng = np.random.default_rng(5)
    _check_normals(rng.integers(0, 2 ** 32, 2 << 16, dtype=np.uint64).astype(np.uint32),
                   "2^16 random pairs")
    top = ((1 << 23) - 1) << 9
    # all four pairings of the top-23-bit values 0 and 2^23 - 1
    ext = np.array([w for a, b in itertools.product((0, top), repeat=2) for w in (a, b)],
                   np.uint32)
    _check_normals(ext, "extreme uniforms")
    g = _from_bits(ext)
    # u_a = 2^-24: the largest radius there is, on the +x side for both extreme angles
    assert g[0] > 5.76 and g[2] > 5.76 and abs(g[1]) < 1e-5 and abs(g[3]) < 1e-5
    assert np.isfinite(g).all()
    # the low 9 bits of a word play no part
    assert _same(_from_bits(ext | np.uint32(0x1FF)), g)


@pytest.mark.parametrize("seed, sid", [(SEEDS[0], STREAM_IDS[1]), (SEEDS[1], STREAM_IDS[0])])
def test_stream_normals_are_the_transform_of_the_stream_words(seed, sid):
    for first, n in itertools.product(FIRSTS, COUNTS):
        lo, hi = first - first % 2, first + n + (first + n) % 2  # whole pairs
        want = _from_bits(_words(hi - lo, seed, sid, lo))[first - lo:first - lo + n]
        assert _same(_normals(n, seed, sid, first), want), (first, n)
    whole = _normals(1027, seed, sid, 3)
    parts = np.concatenate([_normals(513, seed, sid, 3), _normals(514, seed, sid, 516)])
    assert _same(parts, whole)


# ------------------------------------------------------------------- the step
def _step_case(K, P, pad, seed=0):
    """K listed rows (out of order, not from row 0) of a [K + 3, P + pad] matrix, c and z."""
    rng = np.random.default_rng(1000 * K + P % 1000 + seed)
    U = rng.standard_normal((K + 3, P + pad)).astype(np.float32)
    rows = (rng.permutation(K) + 2).astype(np.int32)
    c = (rng.random(K) / K).astype(np.float32)
    z = rng.standard_normal(P).astype(np.float32)
    U[rows[0], 0] = -0.0
    z[0] = -0.0  # a -0.0 coordinate: d = 0, and -0 + -0 keeps its sign only without noise
    if K == 1:
        c[0] = 1.0
    return U, rows, c, z


def _run_step(U, rows, c, z, P, sigma, seed, sid, stream=None):
    N = _native()
    zt = torch.from_numpy(z.copy()).to(DEV)
    N.dp_clip_noise_step(torch.from_numpy(U).to(DEV), torch.from_numpy(rows).to(DEV),
                         torch.from_numpy(c).to(DEV), P, zt, sigma, seed, sid, stream=stream)
    return zt


@pytest.mark.parametrize("K", [1, 2, 3, 32, 33, 64])
def test_step_equals_the_reference_bit_for_bit(K):
    N = _native()
    seed, sid, sigma = SEEDS[0], STREAM_IDS[1], 0.37
    for P, pad in itertools.product((4, 8, 252, 256, 260), (0, 4)):
        U, rows, c, z = _step_case(K, P, pad)
        g = _normals(P, seed, sid)
        got = _run_step(U, rows, c, z, P, sigma, seed, sid).cpu().numpy()
        want = R.step_bits(U[rows, :P], c, z, sigma, g)
        assert np.array_equal(got.view(np.uint32), want), (K, P, pad)
        # sigma = 0: the clip step's bits, the -0.0 coordinate included
        Ut, rt, ct = (torch.from_numpy(a).to(DEV) for a in (U, rows, c))
        zc = torch.from_numpy(z.copy()).to(DEV)
        N.centered_clip_step(Ut, rt, ct, P, zc)
        z0 = _run_step(U, rows, c, z, P, 0.0, seed, sid)
        assert torch.equal(z0.view(torch.int32), zc.view(torch.int32)), (K, P, pad)
        assert np.array_equal(z0.cpu().numpy().view(np.uint32), R.step_bits(U[rows, :P], c, z, 0, None))
        # c = 0 for every row: z' - z is fl(sigma * g) exactly
        zn = _run_step(U, rows, np.zeros_like(c), np.zeros_like(z), P, sigma, seed, sid)
        assert _same(zn.cpu().numpy(), (np.float32(sigma) * g).astype(np.float32)), (K, P, pad)


@pytest.mark.parametrize("K, pad", [(3, 0), (33, 4)])
def test_step_on_a_row_of_many_tiles(K, pad):
    P, seed, sid, sigma = BIG_P, SEEDS[1], 5, 0.01
    U, rows, c, z = _step_case(K, P, pad)
    g = _normals(P, seed, sid)
    got = _run_step(U, rows, c, z, P, sigma, seed, sid)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), R.step_bits(U[rows, :P], c, z, sigma, g))
    side = torch.cuda.Stream(DEV)  # another HIP stream: the same bits
    torch.cuda.synchronize(DEV)
    with torch.cuda.stream(side):
        again = _run_step(U, rows, c, z, P, sigma, seed, sid, stream=side)
    side.synchronize()
    assert torch.equal(again.view(torch.int32), got.view(torch.int32))
    # the moments of the device's normals at this length (n = 524,548)
    assert abs(float(g.mean(dtype=np.float64))) <= 5.0 / np.sqrt(P)
    assert abs(float(g.var(dtype=np.float64)) - 1.0) <= 5.0 * np.sqrt(2.0 / P)


def test_a_non_finite_row_poisons_its_coordinate_alone():
    U, rows, c, z = _step_case(5, 64, 0)
    U[rows[2], 7] = np.inf
    U[rows[4], 9] = np.nan
    c[2] = 0.0  # 0 * inf is NaN
    got = _run_step(U, rows, c, z, 64, 0.5, 1, 2).cpu().numpy()
    assert np.isnan(got[7]) and np.isnan(got[9])
    clean = np.ones(64, bool)
    clean[[7, 9]] = False
    want = R.step_bits(U[rows, :64], c, z, 0.5, _normals(64, 1, 2)).view(np.float32)
    assert _same(got[clean], want[clean])


# ------------------------------------------------------------------- refusals
def test_refusals_leave_z_untouched():
    N = _native()
    L = N.lib()
    U = torch.zeros(8, 64, device=DEV)
    rows = torch.arange(5, dtype=torch.int32, device=DEV)
    c = torch.full((5,), 0.2, device=DEV)
    z = torch.full((64,), 3.0, device=DEV)
    st = N._stream(None, U)

    def step(U_=U.data_ptr(), ldu=64, rows_=rows.data_ptr(), K=5, c_=c.data_ptr(), P=64,
             z_=z.data_ptr(), sigma=0.5):
        return L.dls_dp_clip_noise_step_f32(U_, ldu, rows_, K, c_, P, z_, sigma, 1, 2, st)

    for kw, rc in ((dict(U_=None), -1), (dict(rows_=None), -1), (dict(c_=None), -1),
                   (dict(z_=None), -1), (dict(K=0), -1), (dict(K=65), -1),
                   (dict(sigma=-1.0), -1), (dict(sigma=float("inf")), -1),
                   (dict(sigma=float("nan")), -1), (dict(P=-4), -1), (dict(P=62), -2),
                   (dict(ldu=60), -2), (dict(ldu=66), -2), (dict(U_=U.data_ptr() + 4), -2),
                   (dict(z_=z.data_ptr() + 4, P=60), -2), (dict(c_=c.data_ptr() + 2), -2)):
        assert step(**kw) == rc, kw
        assert b"dls_dp_clip_noise_step_f32" in L.dls_last_error()
    for kw, what in ((dict(P=62), "multiple of 4"), (dict(sigma=-0.5), "sigma"),
                     (dict(sigma=float("nan")), "sigma"), (dict(seed=-1), "seed"),
                     (dict(stream_id=1 << 64), "stream_id"), (dict(z=torch.zeros(65, device=DEV)[1:]), "16-byte aligned"),
                     (dict(z=z.cpu()), "z is on cpu"), (dict(c=c[:4]), "c must be"),
                     (dict(z=U[1]), "overlap")):
        args = dict(U=U, rows=rows, c=c, P=64, z=z, sigma=0.5, seed=1, stream_id=2)
        args.update(kw)
        with pytest.raises(RuntimeError, match="dp_clip_noise_step: .*" + what):
            N.dp_clip_noise_step(**args)
    torch.cuda.synchronize(DEV)
    assert bool((z == 3.0).all()) and bool((U == 0).all())
    assert step(P=0) == 0 and bool((z == 3.0).all())  # P == 0 launches nothing

    out = torch.full((8,), 7, dtype=torch.int32, device=DEV)
    fout = torch.full((8,), 7.0, device=DEV)
    for f, o in ((L.dls_philox_u32, out), (L.dls_philox_normal_f32, fout)):
        p = o.data_ptr()
        for args, rc in (((None, 8, 1, 2, 0), -1), ((p, -1, 1, 2, 0), -1), ((p, 8, 1, 2, -1), -1),
                         ((p, 2, 1, 2, (1 << 63) - 2), -1), ((p + 2, 4, 1, 2, 0), -2)):
            assert f(*args, st) == rc, args
        assert f(p, 0, 1, 2, 0, st) == 0
    bits = torch.zeros(8, dtype=torch.int32, device=DEV)
    f = L.dls_normal_from_bits_f32
    for args, rc in (((None, 8, fout.data_ptr()), -1), ((bits.data_ptr(), 8, None), -1),
                     ((bits.data_ptr(), 7, fout.data_ptr()), -1),
                     ((bits.data_ptr(), -2, fout.data_ptr()), -1),
                     ((bits.data_ptr() + 2, 4, fout.data_ptr()), -2),
                     ((bits.data_ptr(), 4, fout.data_ptr() + 2), -2)):
        assert f(*args, st) == rc, args
    assert f(bits.data_ptr(), 0, fout.data_ptr(), st) == 0
    with pytest.raises(RuntimeError, match="philox_u32: .*n=-1"):
        N.philox_u32(-1, 1, 2, device=DEV)
    with pytest.raises(RuntimeError, match="philox_normal_f32: .*seed"):
        N.philox_normal(8, -1, 2, device=DEV)
    with pytest.raises(RuntimeError, match="normal_from_bits: .*word pairs"):
        N.normal_from_bits(bits[:7])
    with pytest.raises(RuntimeError, match="not on the GPU"):
        N.normal_from_bits(bits.cpu())
    torch.cuda.synchronize(DEV)
    assert bool((out == 7).all()) and bool((fout == 7.0).all())


# ------------------------------------------------------------------ end to end
def test_store_dp_mean_matches_the_reference():
    from distributed_learning_simulator_amd.aggregation import ClientUpdateStore
    from distributed_learning_simulator_amd.layout import ParameterLayout
    from tests import centered_clip_ref as CR
    P = 320
    store = ClientUpdateStore(ParameterLayout([("w", (P,))]), DEV, capacity=6)
    rng = np.random.default_rng(2)
    X = (0.1 * rng.standard_normal((6, P))).astype(np.float32)
    X[4] *= 40.0  # far outside the radius
    store.U.copy_(torch.from_numpy(X))
    start = torch.zeros(P, device=DEV)
    flat, info = store.dp_mean([5, 4, 1, 0], [9, 8, 3, 2], start, 2.0, 0.5, 11, 3)
    order = [0, 1, 4, 5]  # the rows in id order
    d2 = [float((X[r].astype(np.float64) ** 2).sum()) for r in order]
    _, s, c = CR.scales(d2, 2.0)
    assert info["rejected"] == [] and info["clipped_fraction"] == 0.25
    assert info["scales"][8] < 1.0 and info["scales"][2] == 1.0
    assert info["sigma"] == float(np.float32(0.5 * 2.0 / 4))
    # the device's distances are within 2^-17 of the exact ones: the coefficients may differ
    # in the last bit for the clipped client, so the reference takes the device's own scales
    c = np.array([info["scales"][i] / 4.0 for i in (2, 3, 8, 9)]).astype(np.float32)
    want = R.step_bits(X[order], c, np.zeros(P, np.float32), info["sigma"], _normals(P, 11, 3))
    assert np.array_equal(flat.cpu().numpy().view(np.uint32), want)
    assert bool((start == 0).all())


def test_simulator_round_trip_is_reproducible(tmp_path, monkeypatch):
    """Two runs of one DP configuration end in the same bits.  The workers' training is
    torch's: its convolution backward is only reproducible with MIOpen's deterministic
    solutions, which the Trainer does not ask for itself (the tester does, for the
    duration of an inference), so the test holds the flags for both runs."""
    from distributed_learning_simulator_amd import simulator
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(torch.backends.cudnn, "benchmark", False)

    def run(tag):
        cfg = simulator.get_config(
            ["--distributed_algorithm", "fed", "--worker_number", "4", "--round", "2",
             "--dp_clip", "1.0", "--dp_noise_multiplier", "0.5", "--dp_seed", "7",
             "--train_size", "512", "--test_size", "128", "--log_dir", str(tmp_path / tag)])
        return simulator.run(cfg)

    a, b = run("a"), run("b")
    assert a.round == b.round == 2
    for name, v in a.prev_model.items():
        assert torch.equal(v.view(torch.int32), b.prev_model[name].view(torch.int32)), name
        assert bool(torch.isfinite(v).all())
    assert a.last_dp["releases"] == 2 and np.isfinite(a.last_dp["epsilon"])
    assert a.last_dp["epsilon"] == pytest.approx(R.epsilon(0.5, 2, 1e-5), rel=1e-12)
    assert a.last_dp == b.last_dp
