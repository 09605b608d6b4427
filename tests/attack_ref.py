"""CPU reference of the crafted Byzantine rows (include/dls_hip.h, dls_craft_rows_f32)
and of the sign flip — TEST INFRASTRUCTURE ONLY (the package has no CPU path).

Restates the contract's steps literally, per column, on the order-preserving keys of
tests/robust_ref.py: sort, sum ascending in ``np.float32`` and divide by
``np.float32(Kh)``; when b != 0 the deviations d = fl(v[i] - mu) and s = fmaf(d, d, s);
then the population variance, ``np.sqrt`` on float32 (correctly rounded, denormals
included), and multiply, then add: out = base + (a * (mu - base) + b * sigma); a NaN
result is 0x7fc00000.  The divisions are those of tests/division_ref.py.

The fused multiply-add is evaluated in fp64: d * d is exact there (48 significant
bits), and the sum with s is rounded to odd (the error of the fp64 addition, from
TwoSum, decides the last bit), so the final rounding to fp32 is the fmaf's single
rounding in every case, not only where the fp64 sum happens to be exact.
"""
import numpy as np

from tests import division_ref as D
from tests.robust_ref import QNAN, keys, unkeys


def sorted_values(X):
    X = np.ascontiguousarray(X)
    bits = X.view(np.uint32) if X.dtype != np.uint32 else X
    return unkeys(np.sort(keys(bits), axis=0)).view(np.float32)


def _div(x, n):
    """fl32(x / fl32(n)), one IEEE rounding (x * 1 is x)."""
    return D.weighted_terms(x, 1.0, n)


def mean_of_sorted(v):
    """fp32 [P]: the ascending sum divided by fl32(K) (K == 1: v[0]'s own bits)."""
    K = v.shape[0]
    with np.errstate(all="ignore"):
        acc = v[0].copy()
        for i in range(1, K):
            acc = (acc + v[i]).astype(np.float32)
    return _div(acc, K) if K > 1 else acc


def fmaf(x, y, z):
    """fl32(x * y + z) with one rounding (see the module docstring)."""
    x, y, z = (np.asarray(t, np.float32).astype(np.float64) for t in (x, y, z))
    with np.errstate(all="ignore"):
        p = x * y  # exact
        t = p + z
        bb = t - p
        err = (p - (t - bb)) + (z - bb)  # TwoSum: p + z == t + err exactly
        odd = (t.view(np.int64) & 1).astype(bool)
        fix = np.isfinite(t) & np.isfinite(err) & (err != 0) & ~odd
        toward = np.where(err > 0, np.inf, -np.inf)
        t = np.where(fix, np.nextafter(t, toward), t)
        return t.astype(np.float32)


def sigma_of_sorted(v, mu):
    """fp32 [P]: sqrt of the population variance of step 2."""
    K = v.shape[0]
    s = np.zeros(v.shape[1], np.float32)
    with np.errstate(all="ignore"):
        for i in range(K):
            d = (v[i] - mu).astype(np.float32)
            s = fmaf(d, d, s)
        var = _div(s, K) if K > 1 else s
        return np.sqrt(var).astype(np.float32)


def craft_bits(X, a, b, base=None):
    """X: [Kh, P] fp32 (or uint32 bit patterns) of the honest rows, base: None or fp32
    [P] -> uint32 [P], the bits every attacker row gets."""
    v = sorted_values(X)
    a, b = np.float32(a), np.float32(b)
    mu = mean_of_sorted(v)
    with np.errstate(all="ignore"):
        if base is not None:
            base = np.ascontiguousarray(base)
            base = base.view(np.float32) if base.dtype == np.uint32 else base.astype(np.float32)
            t = (mu - base).astype(np.float32)
        else:
            t = mu
        r = (a * t).astype(np.float32)
        if b != 0:
            e = (b * sigma_of_sorted(v, mu)).astype(np.float32)
            r = (r + e).astype(np.float32)
        out = (base + r).astype(np.float32) if base is not None else r
    ob = out.view(np.uint32).copy()
    ob[np.isnan(out)] = QNAN
    return ob


def sign_flip_bits(x, scale, base=None):
    """One row x (fp32 [P]) -> uint32 [P]: d = x - base; d *= fl32(scale); base - d
    (without base: -(fl32(scale) * x))."""
    x = np.asarray(x, np.float32)
    s = np.float32(scale)
    with np.errstate(all="ignore"):
        if base is None:
            return (-(x * s).astype(np.float32)).view(np.uint32)
        base = np.asarray(base, np.float32)
        d = (x - base).astype(np.float32)
        d = (d * s).astype(np.float32)
        return (base - d).astype(np.float32).view(np.uint32)


def column(values, a, b, base=None):
    """One column given as Python floats -> the result's bits."""
    x = np.array(values, dtype=np.float32).reshape(-1, 1)
    bs = None if base is None else np.array([base], np.float32)
    return int(craft_bits(x, a, b, bs)[0])
