"""Host tests of tests/bn_ref.py, the CPU reference the eval batch-norm kernels are
pinned against (tests/test_gpu_bn_exact.py): every function against exact rational
arithmetic (fractions.Fraction, one rounding per step), the fused multiply-add where
a double rounding through fp64 would differ, and the coverage tie: the shape lists
of the GPU file reach every launch form of csrc/infer.hip."""
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import bn_ref as R
from tests.attack_ref import fmaf

F = np.float32
TWO = Fraction(2)


# ------------------------------------------------- exact fp32 arithmetic, scalar
def fl(q):
    """Fraction (non-zero) -> the nearest fp32, ties to even, gradual underflow,
    overflow to inf; a result that rounds to zero keeps q's sign."""
    s, a = (-1.0, -q) if q < 0 else (1.0, q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    while TWO ** e > a:
        e -= 1
    while TWO ** (e + 1) <= a:
        e += 1
    quantum = TWO ** (max(e, -126) - 23)
    n = a / quantum
    k = n.numerator // n.denominator
    rem = n - k
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and k & 1):
        k += 1
    v = k * quantum
    if v >= TWO ** 128:
        return F(s * math.inf)
    return F(s * float(v))  # exact: v has at most 24 significant bits


def _exact(op, *args):
    """One correctly rounded fp32 operation on fp32 scalars.  Finite operands with a
    non-zero exact result go through Fraction; infinities, NaNs and exact zeros (whose
    sign IEEE fixes) through fp64, where products of fp32 values are exact and the
    special-value rules are the same."""
    a = [float(x) for x in args]
    with np.errstate(all="ignore"):
        d = [np.float64(x) for x in a]
        wide = {"mul": lambda: d[0] * d[1], "add": lambda: d[0] + d[1], "sub": lambda: d[0] - d[1],
                "fma": lambda: d[0] * d[1] + d[2]}[op]()
    if not all(math.isfinite(x) for x in a):
        return F(wide)  # inf or NaN by the IEEE rules; no finite result is possible
    q = [Fraction(x) for x in a]
    r = {"mul": lambda: q[0] * q[1], "add": lambda: q[0] + q[1], "sub": lambda: q[0] - q[1],
         "fma": lambda: q[0] * q[1] + q[2]}[op]()
    if r == 0:
        return F(wide)  # the fp64 result is zero exactly when r is, with IEEE's sign
    return fl(r)


def exact_sqrt(x):
    x = float(x)
    if not math.isfinite(x) or x <= 0:
        with np.errstate(all="ignore"):
            return F(np.sqrt(np.float64(x)))
    q = Fraction(x)
    N = q.numerator * q.denominator  # sqrt(n / d) = sqrt(n * d) / d
    K = 64
    r = math.isqrt(N << (2 * K))
    den = q.denominator << K
    if r * r == N << (2 * K):
        return fl(Fraction(r, den))
    # irrational: strictly between r and r + 1; no fp32 rounding boundary lies there
    return fl(Fraction(2 * r + 1, 2 * den))


def exact_recip(x):
    x = float(x)
    if not math.isfinite(x) or x == 0:
        with np.errstate(all="ignore"):
            return F(np.float64(1.0) / np.float64(x))
    return fl(1 / Fraction(x))


def relu_scalar(t, keeps):
    if math.isnan(t):
        return t
    if keeps:
        return F(0) if t < 0 else t
    return t if t > 0 else F(0)


def same(a, b):
    a, b = F(a), F(b)
    if np.isnan(a) or np.isnan(b):
        return bool(np.isnan(a) and np.isnan(b))
    return a.view(np.uint32) == b.view(np.uint32)


# ----------------------------------------------------------------- the pool
def edge_pool():
    b = [0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00800000,
         0x80800000, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000,
         0x3F800000, 0xBF800000, 0x3F800001, 0x3F7FFFFF, 0x7E800000, 0x5F800000, 0x1F800000,
         0x00400000, 0x33800000, 0x4B800001]
    return R.from_bits(b)


def scalars(n, seed):
    rng = np.random.default_rng(seed)
    pool = edge_pool()
    out = np.empty((n, 6), np.float32)
    for j in range(6):
        rnd = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)).astype(np.float32)
        pick = rng.random(n) < 0.4
        out[:, j] = np.where(pick, pool[rng.integers(0, pool.size, n)], rnd)
    return out


N_SCALARS = 400


@pytest.mark.parametrize("keeps", [False, True])
def test_act_matches_rational_arithmetic(keeps):
    S = scalars(N_SCALARS, 1)
    x, a, b, r = S[:, 0], S[:, 1], S[:, 2], S[:, 3]
    for res in (False, True):
        for relu in (False, True):
            got = R.act(x, a, b, r if res else None, relu, keeps_neg_zero=keeps)
            for i in range(N_SCALARS):
                t = _exact("add", _exact("mul", x[i], a[i]), b[i])
                if res:
                    t = _exact("add", t, r[i])
                if relu:
                    t = relu_scalar(t, keeps)
                assert same(got[i], t), (i, x[i], a[i], b[i], r[i], got[i], t)


@pytest.mark.parametrize("keeps", [False, True])
def test_act_exact_matches_rational_arithmetic(keeps):
    S = scalars(N_SCALARS, 2)
    x, m, iv, w, b, r = (S[:, j].copy() for j in range(6))
    x[::7] = m[::7]  # the cancellation x == mean
    consts = np.concatenate([m, iv, w, b])
    ch = np.arange(N_SCALARS)
    for res in (False, True):
        for relu in (False, True):
            got = R.act_exact(x, consts, r if res else None, relu, ch=ch, keeps_neg_zero=keeps)
            for i in range(N_SCALARS):
                h = _exact("mul", _exact("sub", x[i], m[i]), iv[i])
                t = _exact("fma", w[i], h, b[i])
                if res:
                    t = _exact("add", t, r[i])
                if relu:
                    t = relu_scalar(t, keeps)
                assert same(got[i], t), (i, x[i], m[i], iv[i], w[i], b[i], r[i], got[i], t)


def test_fold_matches_rational_arithmetic():
    S = scalars(N_SCALARS, 3)
    w, b, mean, var = S[:, 0], S[:, 1], S[:, 2], np.abs(S[:, 3])
    var[::5] = S[::5, 3]  # negative and -0 sums too
    for eps in (1e-5, 0.0, 1e-3):
        for affine in (True, False):
            alpha, beta = R.fold(w if affine else None, b if affine else None, mean, var, eps)
            for i in range(N_SCALARS):
                s = _exact("add", var[i], F(eps))
                inv = exact_recip(exact_sqrt(s))
                a = _exact("mul", inv, w[i]) if affine else inv
                bb = _exact("sub", b[i] if affine else F(0), _exact("mul", mean[i], a))
                assert same(alpha[i], a), (i, var[i], eps, w[i], alpha[i], a)
                assert same(beta[i], bb), (i, mean[i], b[i], beta[i], bb)
            mp, iv, wp, bp = R.fold_exact_parts(w if affine else None, b if affine else None, mean,
                                                var, eps)
            assert np.array_equal(R.bits(mp), R.bits(mean))
            assert np.array_equal(R.bits(wp), R.bits(w if affine else np.ones_like(w)))
            assert np.array_equal(R.bits(bp), R.bits(b if affine else np.zeros_like(b)))
            for i in range(0, N_SCALARS, 3):
                s = abs(float(_exact("add", var[i], F(eps))))
                if math.isnan(s):
                    assert math.isnan(iv[i])
                elif s == 0 or math.isinf(s):
                    assert iv[i] == (math.inf if s == 0 else 0.0)
                else:  # an fp64 1/sqrt: within 2 fp64 roundings of the true value
                    true = 1 / Fraction(exact_sqrt_wide(s))
                    assert abs(Fraction(float(iv[i])) - true) <= true * Fraction(1, 1 << 50)


def exact_sqrt_wide(s):
    """sqrt of a positive float as a Fraction good to 2^-100 relative."""
    q = Fraction(s)
    N, K = q.numerator * q.denominator, 128
    return Fraction(math.isqrt(N << (2 * K)), q.denominator << K)


def test_exact_arithmetic_helpers_on_known_values():
    """The rational rounding itself, on values whose fp32 result is known."""
    assert same(fl(Fraction(1, 3)), F(1) / F(3))
    assert same(fl(Fraction(1) + Fraction(1, 1 << 24)), F(1))               # tie to even
    assert same(fl(Fraction(1) + Fraction(3, 1 << 24)), R.from_bits([0x3F800002])[0])
    assert same(fl(TWO ** -150), F(0)) and same(fl(-(TWO ** -150)), F(-0.0))  # tie to even: 0
    assert same(fl(TWO ** -149), R.from_bits([1])[0])
    assert same(fl(TWO ** 128 - TWO ** 103), F(np.inf))                       # rounds up to 2^128
    assert same(fl(TWO ** 128 - TWO ** 103 - 1), R.from_bits([0x7F7FFFFF])[0])
    assert same(exact_sqrt(F(2)), np.sqrt(F(2))) and same(exact_sqrt(F(4)), F(2))
    assert same(_exact("sub", F(-0.0), F(0.0)), F(-0.0)) and same(_exact("add", F(-0.0), F(0.0)), F(0))
    assert same(_exact("fma", F(1), F(-0.0), F(-0.0)), F(-0.0))
    assert same(_exact("mul", F(np.inf), F(0)), F(np.nan))


def test_relu_keeps_nan_and_treats_negative_zero_as_told():
    t = R.from_bits([0x80000000, 0x00000000, 0x7FC00001, 0xFFC00000, 0xBF800000, 0x3F800000,
                     0x80000001, 0xFF800000, 0x7F800000])
    plus = R.bits(R.relu(t, False))
    keep = R.bits(R.relu(t, True))
    assert list(plus) == [0, 0, 0x7FC00001, 0xFFC00000, 0, 0x3F800000, 0, 0, 0x7F800000]
    assert list(keep) == [0x80000000, 0, 0x7FC00001, 0xFFC00000, 0, 0x3F800000, 0, 0, 0x7F800000]
    assert np.array_equal(R.bits(R.relu(t)), keep if R.RELU_KEEPS_NEG_ZERO else plus)


def test_fmaf_where_a_double_rounding_differs():
    """x * y lands exactly on an fp32 tie and z, far below fp64's last bit of the
    product, decides the side: fl32(fl64(x * y + z)) rounds the tie to even, the fused
    result follows z."""
    cases = []
    for k, (xa, ya) in enumerate([(2 ** 12 + 1, 2 ** 12 + 1), (2 ** 12 + 1, 2 ** 12 + 3),
                                  (2 ** 11 + 1, 2 ** 13 + 7), (2 ** 12 + 5, 2 ** 12 + 9)]):
        for zs in (1.0, -1.0):
            for ze in (-40, -80, -126, -149):
                for scale in (0, -60, 40):
                    cases.append((F(xa) * F(2.0 ** scale), F(ya), F(zs * 2.0 ** (ze + scale // 2))))
    differ = 0
    for x, y, z in cases:
        p = Fraction(float(x)) * Fraction(float(y))
        true = fl(p + Fraction(float(z)))
        got = fmaf(x, y, z)
        assert same(got, true), (x, y, z, got, true)
        with np.errstate(all="ignore"):
            twice = F(np.float64(x) * np.float64(y) + np.float64(z))
        differ += not same(twice, true)
    assert differ >= len(cases) // 4, (differ, len(cases))  # the cases do what they are for
    # and special values, zeros' signs, overflow, underflow
    for x, y, z in [(np.inf, 0.0, 1.0), (np.inf, 1.0, -np.inf), (1.0, -0.0, -0.0), (1.0, -0.0, 0.0),
                    (3e38, 2.0, -3e38), (3e38, 2.0, -np.inf), (1e-30, 1e-30, 0.0), (1e-30, -1e-30, 0.0),
                    (1e-20, 1e-20, 1e-45), (2.0, 3.0, -6.0), (-2.0, 3.0, 6.0)]:
        assert same(fmaf(F(x), F(y), F(z)), _exact("fma", F(x), F(y), F(z))), (x, y, z)


def test_layout_helpers():
    N, C, H, W = 2, 3, 2, 2
    idx = np.arange(N * C * H * W)
    nchw = np.broadcast_to(np.arange(C)[None, :, None, None], (N, C, H, W)).reshape(-1)
    nhwc = np.broadcast_to(np.arange(C)[None, None, None, :], (N, H, W, C)).reshape(-1)
    assert np.array_equal(R.nchw_channel(idx, C, H * W), nchw)
    assert np.array_equal(R.nhwc_channel(idx, C), nhwc)
    big = np.array([2 ** 31 + 5, 2 ** 33 + 7])
    assert list(R.nhwc_channel(big, 12)) == [(2 ** 31 + 5) % 12, (2 ** 33 + 7) % 12]
    assert list(R.nchw_channel(big, 12, 49)) == [(2 ** 31 + 5) // 49 % 12, (2 ** 33 + 7) // 49 % 12]


def test_mismatches_rule():
    ref = R.from_bits([0x3F800000, 0x7FC00000, 0x80000000, 0xFFC00001])
    assert R.mismatches(ref, ref).size == 0
    got = R.from_bits([0x3F800001, 0xFFC12345, 0x00000000, 0x3F800000])
    assert list(R.mismatches(got, ref)) == [0, 2, 3]  # a NaN of any payload passes; -0 != +0


# --------------------------------------------------------- the launch forms
BLOCK, UNROLL = 256, 4


def _loops(n4):
    """(blocks, unrolled loop used, tail loop used) of the grid-stride walk below
    the grid cap: blocks = ceil(n4 / 1024), thread i runs unrolled rounds while
    i + 3 * stride < n4 and the tail loop over what is left."""
    blocks = max(1, -(-n4 // (BLOCK * UNROLL)))
    stride = BLOCK * blocks
    unrolled = n4 > (UNROLL - 1) * stride
    tail = False
    for i in range(min(stride, n4)):
        k = i
        while k + (UNROLL - 1) * stride < n4:
            k += UNROLL * stride
        if k < n4:
            tail = True
            break
    return blocks, unrolled, tail


def nhwc_form(N, C, H, W):
    C4 = C // 4
    n4 = N * H * W * C4
    blocks, unrolled, tail = _loops(n4)
    fixed = (BLOCK * blocks) % C4 == 0
    return {"fixed": fixed, "c4": C4, "c4_pow2": C4 & (C4 - 1) == 0, "unrolled": unrolled,
            "tail": tail, "blocks": blocks}


def nchw_form(N, C, H, W):
    HW = H * W
    if HW % 4:
        return {"element": True}
    HW4 = HW // 4
    blocks, unrolled, tail = _loops(N * C * HW4)
    hp, cp = HW4 & (HW4 - 1) == 0, C & (C - 1) == 0
    return {"element": False, "pow2": hp and cp, "hw4_pow2": hp, "c_pow2": cp, "hw4": HW4,
            "unrolled": unrolled, "tail": tail, "blocks": blocks}


def test_loop_arithmetic_on_the_issue_s_examples():
    assert nhwc_form(1, 12, 25, 10) == {"fixed": False, "c4": 3, "c4_pow2": False, "unrolled": False,
                                        "tail": True, "blocks": 1}            # n4 = 750
    assert nhwc_form(1, 12, 40, 25) == {"fixed": True, "c4": 3, "c4_pow2": False, "unrolled": True,
                                        "tail": True, "blocks": 3}            # n4 = 3000
    assert _loops(3072) == (3, True, False) and _loops(1) == (1, False, True)


def test_gpu_shape_lists_reach_every_launch_form():
    from tests.test_gpu_bn_exact import NCHW_SHAPES, NHWC_SHAPES
    nhwc = [nhwc_form(*s) for s in NHWC_SHAPES]
    want_nhwc = {
        "FIXED, C4 not a power of two": lambda f: f["fixed"] and not f["c4_pow2"],
        "not FIXED, C4 not a power of two": lambda f: not f["fixed"] and not f["c4_pow2"],
        "FIXED, C4 a power of two": lambda f: f["fixed"] and f["c4_pow2"],
        "FIXED, unrolled and tail loop in one launch":
            lambda f: f["fixed"] and f["unrolled"] and f["tail"],
        "not FIXED, unrolled and tail loop in one launch":
            lambda f: not f["fixed"] and f["unrolled"] and f["tail"],
        "tail loop only": lambda f: not f["unrolled"] and f["tail"],
        "more than one block": lambda f: f["blocks"] > 1,
        "C4 == 1": lambda f: f["c4"] == 1,
    }
    for name, pred in want_nhwc.items():
        assert any(pred(f) for f in nhwc), "no NHWC shape reaches: " + name
    nchw = [nchw_form(*s) for s in NCHW_SHAPES]
    vec = [f for f in nchw if not f["element"]]
    want_nchw = {
        "HW % 4 != 0 (element kernel)": lambda f: f["element"],
        "POW2": lambda f: not f["element"] and f["pow2"],
        "not POW2": lambda f: not f["element"] and not f["pow2"],
        "HW4 == 1, POW2": lambda f: not f["element"] and f["hw4"] == 1 and f["pow2"],
        "HW4 == 1, not POW2": lambda f: not f["element"] and f["hw4"] == 1 and not f["pow2"],
        "HW4 a power of two, C not": lambda f: not f["element"] and f["hw4_pow2"] and not f["c_pow2"]
            and f["hw4"] > 1,
        "C a power of two, HW4 not": lambda f: not f["element"] and f["c_pow2"] and not f["hw4_pow2"],
        "neither a power of two": lambda f: not f["element"] and not f["c_pow2"] and not f["hw4_pow2"],
        "POW2, unrolled and tail loop in one launch":
            lambda f: not f["element"] and f["pow2"] and f["unrolled"] and f["tail"],
        "not POW2, unrolled and tail loop in one launch":
            lambda f: not f["element"] and not f["pow2"] and f["unrolled"] and f["tail"],
    }
    for name, pred in want_nchw.items():
        assert any(pred(f) for f in nchw), "no NCHW shape reaches: " + name
    assert vec and all(s[1] % 4 == 0 for s in NHWC_SHAPES)
    assert any(s[1] % 4 for s in NCHW_SHAPES)  # NCHW takes any channel count
    # small: a case is milliseconds
    assert all(N * C * H * W <= 1 << 16 for N, C, H, W in NHWC_SHAPES + NCHW_SHAPES)
