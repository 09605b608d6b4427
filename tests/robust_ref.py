"""CPU reference of the coordinate-wise trimmed mean / median (include/dls_hip.h,
dls_trimmed_mean_f32) — TEST INFRASTRUCTURE ONLY (the package has no CPU path).

Per column: sort order-preserving integer keys (-0 below +0, every NaN on the
top key), drop ``trim`` at each end, sum the kept values ascending in
``np.float32`` (one rounding per addition), divide by ``np.float32(m)``; a NaN
result is the canonical quiet NaN 0x7fc00000; m == 1 returns the kept value's
own bits.
"""
import numpy as np

QNAN = np.uint32(0x7FC00000)
TOP = np.uint32(0xFFFFFFFF)


def keys(bits):
    """uint32 fp32 bit patterns -> uint32 keys whose unsigned order is the rule's."""
    u = np.asarray(bits, dtype=np.uint32)
    neg = (u >> np.uint32(31)).astype(bool)
    k = np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    return np.where(nan, TOP, k).astype(np.uint32)


def unkeys(k):
    k = np.asarray(k, dtype=np.uint32)
    pos = (k >> np.uint32(31)).astype(bool)
    return np.where(pos, k ^ np.uint32(0x80000000), ~k).astype(np.uint32)


def trimmed_mean_bits(X, trim):
    """X: [K, P] fp32 (or uint32 bit patterns) -> uint32 [P], the result's bits."""
    X = np.ascontiguousarray(X)
    bits = X.view(np.uint32) if X.dtype != np.uint32 else X
    K = bits.shape[0]
    trim = int(trim)
    assert 0 <= 2 * trim < K
    srt = unkeys(np.sort(keys(bits), axis=0)).view(np.float32)
    kept = srt[trim:K - trim]
    m = kept.shape[0]
    with np.errstate(all="ignore"):
        acc = kept[0].copy()
        for i in range(1, m):
            acc = (acc + kept[i]).astype(np.float32)  # one fp32 rounding per addition
        out = acc if m == 1 else (acc / np.float32(m)).astype(np.float32)
    ob = out.view(np.uint32).copy()
    ob[np.isnan(out)] = QNAN
    return ob


def median_bits(X):
    return trimmed_mean_bits(X, (np.asarray(X).shape[0] - 1) // 2)


def column(values, trim):
    """One column given as Python floats / np.float32 scalars -> the result's bits."""
    x = np.array(values, dtype=np.float32).reshape(-1, 1)
    return int(trimmed_mean_bits(x, trim)[0])


def column_bits(bit_patterns, trim):
    x = np.array(bit_patterns, dtype=np.uint32).reshape(-1, 1)
    return int(trimmed_mean_bits(x, trim)[0])
