"""Host checks behind tests/test_gpu_division.py (no GPU): the numpy reference of
tests/division_ref.py against fp64 and the C oracle, and the division ALGORITHMS
(Markstein, two-constant) for every divisor of the shared table, so that a
mismatch on the device can be blamed on device code."""
import numpy as np
import pytest
import torch

from oracle import _c
from tests import division_ref as R

DIVISORS = R.DIVISORS
FAST = [b for b in DIVISORS if R.in_fast_divisor_range(b)]


@pytest.fixture(scope="module")
def sweep():
    return R.binade_sweep(4096)


def test_denormals_are_not_flushed():
    """The reference is only a reference while the CPU keeps denormals."""
    assert np.float32(1e-40) * np.float32(1) != 0
    # torch has set_flush_denormal but (in the builds this project runs on) no
    # getter: ask for the mode where a getter exists, and observe it either way
    get = getattr(torch, "get_flush_denormal", None)
    assert get is None or not get()
    t = torch.tensor([1e-40, -1e-45], dtype=torch.float32)
    assert bool(((t * 1.0) != 0).all()) and bool(((t + 0.0) != 0).all())
    assert float(np.float32(1e-45)) > 0 and np.float32(1e-38) / np.float32(1000) != 0


def test_sweeps_cover_what_they_claim():
    """mantissa_sweep: every fp32 of [1, 2) once; binade_sweep: every binade's first
    and last mantissa for both signs, denormals, and the values one ulp either
    side of the kernels' 2^-60 / 2^61 guard."""
    m = R.mantissa_sweep()
    assert m.shape == (1 << 23,) and m[0] == 1 and m[-1] == np.nextafter(np.float32(2), np.float32(0))
    assert np.array_equal(np.diff(m.view(np.uint32)), np.ones((1 << 23) - 1, np.uint32))
    s = R.binade_sweep(4096)
    bits = set(s.view(np.uint32).tolist())
    for e in range(255):
        for sign in (0, 0x80000000):
            assert (sign | e << 23) in bits and (sign | e << 23 | 0x7FFFFF) in bits
    for v in (2.0 ** -60, 2.0 ** 61):
        f = np.float32(v)
        for x in (f, np.nextafter(f, np.float32(0)), -f, -np.nextafter(f, np.float32(0))):
            assert int(np.float32(x).view(np.uint32)) in bits
    assert {0x0, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x007FFFFF, 0x807FFFFF} <= bits
    d = R.device_sweep(4096)
    assert len(d) % 4 == 0 and np.array_equal(d[:len(s)].view(np.uint32), s.view(np.uint32))
    edges = set(R.guard_edges().view(np.uint32).tolist())
    for v in (2.0 ** -60, 2.0 ** 61):
        b = int(np.float32(v).view(np.uint32))
        assert {b - 1, b, b + 1, 0x80000000 | b - 1, 0x80000000 | b + 1} <= edges
    assert 1 in edges


@pytest.mark.parametrize("N", DIVISORS, ids=R.div_id)
def test_weighted_terms_fp32_matches_fp64_quotient(sweep, N):
    """weighted_terms' fp32 division equals the fp64 quotient rounded to fp32 on the
    whole binade sweep.  A correctly rounded fp64 quotient of two fp32 numbers
    rounds to the correctly rounded fp32 quotient (53 >= 2 * 24 + 2: the double
    rounding is innocuous, also for denormal results, which keep fewer bits), so
    this pins numpy's float32 division as IEEE division with denormals."""
    for w in (1.0, 3.0, 1000.0, 0.5):
        with np.errstate(all="ignore"):
            t = sweep * np.float32(w)  # fl(x * w): the dividend
            want = (t.astype(np.float64) / np.float64(np.float32(N))).astype(np.float32)
        got = R.weighted_terms(sweep, w, N)
        assert R.same_bits(got, want), (w, R.first_mismatch(got, want, t))


@pytest.mark.parametrize("N", [b for b in DIVISORS if float(b).is_integer() and b < 2 ** 62],
                         ids=R.div_id)
def test_fold_matches_oracle_on_integer_cases(sweep, N):
    """fold(weighted_terms) equals the C oracle's orc_fedavg_ref wherever the
    oracle applies: integer sample counts whose sum is the divisor (K = 2, or
    K = 1 for N = 1), rows of the binade sweep so that signed zeros, denormal
    partial sums and inf - inf are summed."""
    N = int(N)
    n = [1] if N == 1 else [N // 3 + 1, N - (N // 3 + 1)]
    U = np.stack([sweep, np.roll(-sweep, 12345)][:len(n)])
    order = list(range(len(n)))[::-1]
    want = _c.fedavg_ref(U, n, order)
    got = R.fold([R.weighted_terms(U[i], n[i], N) for i in order])
    assert R.same_bits(got, want), R.first_mismatch(got, want)


@pytest.mark.parametrize("N", FAST, ids=R.div_id)
def test_markstein_exact_for_table_divisor(N):
    """The C restatement of the kernels' Markstein quotient equals IEEE a / N for
    every fp32 mantissa of a, for each table divisor in the fast range [1, 2^31]."""
    assert _c.fastdiv_check(N) == 0


def _two_constant_expected(b):
    """numpy restatement of the host prover: fma(a, yh, RN(a * yl)) == RN(a / b)
    for every mantissa, b in the fast range and a * yl normal over it."""
    if not R.in_fast_divisor_range(b):
        return 0
    b32 = np.float32(b)
    yh = np.float32(1.0 / float(b32))
    yl = np.float32(1.0 / float(b32) - float(yh))
    if yl != 0 and abs(float(yl)) < 2.0 ** -66:
        return 0
    a = R.mantissa_sweep()
    lo = a * yl
    # a * yh has <= 48 significant bits: the float64 sum is the exact fma input
    q = (a.astype(np.float64) * np.float64(yh) + np.float64(lo)).astype(np.float32)
    return int(np.array_equal(q, a / b32))


def test_two_constant_classes_of_table_divisors():
    """Which table divisors dls_two_constant_division accepts (the kernels then
    take the 2-op quotient) and which it rejects (Markstein, or IEEE outside the
    fast range): both classes occur, 11735695 is rejected, 55123 and the powers
    of two are accepted, nothing outside [1, 2^31] is accepted, and every verdict
    equals an independent numpy restatement of the proof."""
    from distributed_learning_simulator_amd import _native
    verdict = {b: _native.two_constant_division(b) for b in DIVISORS}
    accepted = [b for b in DIVISORS if verdict[b]]
    rejected = [b for b in DIVISORS if not verdict[b]]
    print("two-constant accepted:", accepted)
    print("two-constant rejected:", rejected)
    assert accepted and rejected
    assert 11735695.0 in rejected and 55123.0 in accepted
    # the record: accepted 1, 3, 7, 550, 55123, 16777215, 16777216, 2147483520,
    # 2147483648 and 1.5; rejected inside the fast range (Markstein) 11735695,
    # 16777218 and 8388607; rejected outside it 2147483904, 2^40, 0.5, 1 - 2^-24, 3e38
    assert set(accepted) == {1.0, 3.0, 7.0, 550.0, 55123.0, 16777215.0, 16777216.0,
                             2147483520.0, 2147483648.0, 1.5}
    assert {b for b in rejected if R.in_fast_divisor_range(b)} == {11735695.0, 16777218.0,
                                                                   8388607.0}
    assert all(R.in_fast_divisor_range(b) for b in accepted)
    # rejected AND in the fast range: the kernels' Markstein branch is reached
    assert any(R.in_fast_divisor_range(b) for b in rejected)
    for b in DIVISORS:
        assert verdict[b] == _two_constant_expected(b), b
