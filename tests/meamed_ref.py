"""CPU reference of the coordinate-wise mean around the median (include/dls_hip.h,
dls_mean_around_median_f32) — TEST INFRASTRUCTURE ONLY (the package has no CPU path).

Restates the contract's four steps literally, per column, on the order-preserving
keys of tests/robust_ref.py: sort, take the median, find the window start as the
FIRST index whose comparison is false (not the count of true ones, which is the
kernel's shortcut), sum the kept values ascending in ``np.float32`` and divide by
``np.float32(keep)``; a NaN result is 0x7fc00000; keep == 1 returns the kept value's
own bits.
"""
import numpy as np

from tests.robust_ref import QNAN, keys, unkeys


def sorted_values(X):
    """X: [K, P] fp32 (or uint32 bit patterns) -> fp32 [K, P], every column ascending in
    the contract's total order."""
    X = np.ascontiguousarray(X)
    bits = X.view(np.uint32) if X.dtype != np.uint32 else X
    return unkeys(np.sort(keys(bits), axis=0)).view(np.float32)


def median_of_sorted(v):
    """fp32 [P]: v[(K-1)/2]'s own bits (odd K) or fl32(fl32(lo + hi) / 2) (even K)."""
    K = v.shape[0]
    if K % 2:
        return v[(K - 1) // 2].copy()
    with np.errstate(all="ignore"):
        return ((v[K // 2 - 1] + v[K // 2]).astype(np.float32) / np.float32(2)).astype(np.float32)


def comparisons(v, med, keep):
    """bool [K - keep, P]: fl32(med - v[i]) > fl32(v[i + keep] - med); False with a NaN."""
    K = v.shape[0]
    with np.errstate(all="ignore"):
        return np.array([(med - v[i]).astype(np.float32) > (v[i + keep] - med).astype(np.float32)
                         for i in range(K - keep)], dtype=bool).reshape(K - keep, v.shape[1])


def window_start(v, med, keep):
    """int [P]: the first i in 0 .. K-keep-1 whose comparison is false, else K - keep."""
    K = v.shape[0]
    c = comparisons(v, med, keep)
    s = np.full(v.shape[1], K - keep, dtype=np.int64)
    for i in range(K - keep - 1, -1, -1):  # the lowest false index wins
        s[~c[i]] = i
    return s


def mean_around_median_bits(X, keep):
    """X: [K, P] fp32 (or uint32 bit patterns) -> uint32 [P], the result's bits."""
    v = sorted_values(X)
    K, P = v.shape
    keep = int(keep)
    assert 1 <= keep <= K
    s = window_start(v, median_of_sorted(v), keep)
    cols = np.arange(P)
    with np.errstate(all="ignore"):
        acc = v[s, cols].copy()
        for t in range(1, keep):
            acc = (acc + v[s + t, cols]).astype(np.float32)  # one fp32 rounding per addition
        out = acc if keep == 1 else (acc / np.float32(keep)).astype(np.float32)
    ob = out.view(np.uint32).copy()
    ob[np.isnan(out)] = QNAN
    return ob


def column(values, keep):
    """One column given as Python floats / np.float32 scalars -> the result's bits."""
    x = np.array(values, dtype=np.float32).reshape(-1, 1)
    return int(mean_around_median_bits(x, keep)[0])


def column_bits(bit_patterns, keep):
    x = np.array(bit_patterns, dtype=np.uint32).reshape(-1, 1)
    return int(mean_around_median_bits(x, keep)[0])
