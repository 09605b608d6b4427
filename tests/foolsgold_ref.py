"""numpy reference of the Gram / history-fold kernel (dls_rows_gram_f32,
dls_history_gram_f32) and of the FoolsGold rule built on it (tests only).

``fold_bits`` is the fold's bit-level contract (float32, one rounding per operation);
``gram_exact`` and ``abs_products`` are exact sums of the fp64 products (a product of
two fp32 values is exact in fp64), which the kernel's G is compared with at the
contract's bound ``TOL * abs_products``; ``weights`` restates the weight steps
independently of ``aggregation.foolsgold_weights``."""
import math

import numpy as np

TOL = (120 + 8) * 2.0 ** -24  # chains of <= 120 fp32 fmas + the fp64 sums: 2^-17


def updates(X, base=None):
    """h_k = fl32(x_k - base) (the rows themselves without a base), float32 [K, P]."""
    X = np.asarray(X, dtype=np.float32)
    return X if base is None else (X - np.asarray(base, np.float32)[None, :]).astype(np.float32)


def fold_bits(H, X, base=None):
    """fl32(H + fl32(X - base)) as uint32 bit patterns [K, P]: the subtraction and the
    addition each rounded once."""
    H = np.asarray(H, dtype=np.float32)
    with np.errstate(all="ignore"):
        return (H + updates(X, base)).astype(np.float32).view(np.uint32)


def _sum2(p):
    """The sum of the fp64 values p[..., :] as if computed in twice the working
    precision (Ogita, Rump & Oishi's Sum2 on a pairwise tree: every addition's rounding
    error is recovered exactly by TwoSum and added back at the end), the equivalent of
    math.fsum up to the final rounding; vectorised over the leading axes."""
    p = np.array(p, dtype=np.float64)
    err = np.zeros(p.shape[:-1], np.float64)
    while p.shape[-1] > 1:
        if p.shape[-1] % 2:
            p = np.concatenate([p, np.zeros(p.shape[:-1] + (1,), np.float64)], axis=-1)
        a, b = p[..., 0::2], p[..., 1::2]
        s = a + b
        bb = s - a
        err += ((a - (s - bb)) + (b - bb)).sum(axis=-1)
        p = s
    return p[..., 0] + err if p.shape[-1] else err


def _integers(X, e=-9):
    """I with X == I * 2^e exactly, an integer matrix (float64), or None when the fp32
    rows are not all integers times 2^e (``grid_rows`` and what folds make of them are)."""
    Xi = np.ldexp(np.asarray(X, np.float32), -e)
    if not np.array_equal(Xi, np.rint(Xi)):  # false for inf and NaN, too
        return None
    return Xi.astype(np.float64)


def gram_and_abs(Hh):
    """(sum_p h_a h_b, sum_p |h_a h_b|) for every pair, exactly, each fp64 [K, K].  Rows
    that are small integers times one power of two (``grid_rows``) whose sums of products
    stay below 2^53 are added exactly by a plain fp64 matrix product in any order;
    otherwise the exact fp64 products are added by ``_sum2``, pair by pair."""
    Hh = np.asarray(Hh, np.float32)
    K, P = Hh.shape
    e = -9  # grid_rows' default
    I = _integers(Hh, e)
    if I is not None:
        A = np.abs(I)
        if P * A.max(initial=0.0) ** 2 < 2.0 ** 53:
            return np.ldexp(I @ I.T, 2 * e), np.ldexp(A @ A.T, 2 * e)
    Hh = Hh.astype(np.float64)
    out, mag = np.empty((K, K), np.float64), np.empty((K, K), np.float64)
    for a in range(K):
        with np.errstate(all="ignore"):
            prod = Hh[a][None, :] * Hh[a:]
            out[a, a:], mag[a, a:] = _sum2(prod), _sum2(np.abs(prod))
        out[a:, a], mag[a:, a] = out[a, a:], mag[a, a:]
    return out, mag


def gram_exact(Hh):
    """The exact Gram matrix of the fp32 rows, rounded once to fp64."""
    return gram_and_abs(Hh)[0]


def abs_products(Hh):
    """sum_p |h_a h_b| in fp64: what the kernel's error bound is relative to."""
    return gram_and_abs(Hh)[1]


def gram_exact_fsum(Hh):
    """``gram_exact`` by math.fsum (slow: for checking the reference on small cases)."""
    Hh = np.asarray(Hh, np.float32).astype(np.float64)
    K = Hh.shape[0]
    return np.array([[math.fsum((Hh[a] * Hh[b]).tolist()) for b in range(K)] for a in range(K)])


def grid_rows(K, P, seed, bits=9, corr=0.0):
    """float32 [K, P] rows of integers of about ``bits`` bits times 2^-bits (a shared
    component of weight about ``corr`` makes the rows point alike): ``gram_exact`` adds
    their products exactly with a matrix product, however long the rows, while a chain of
    120 fp32 fmas of such 2*bits-bit products still rounds."""
    rng = np.random.default_rng(seed)
    X = rng.integers(-2 ** bits, 2 ** bits + 1, (K, P), dtype=np.int32)
    if corr:
        X += int(round(4 * corr)) * rng.integers(-2 ** bits, 2 ** bits + 1, P, dtype=np.int32)
    return np.ldexp(X.astype(np.float32), -bits)


def weights(G, kappa=1.0):
    """The FoolsGold weights from a [K, K] Gram matrix in fp64 with numpy, steps 1-5 of
    ``aggregation.foolsgold_weights`` restated on whole matrices: (alpha, similarity,
    rejected)."""
    G = np.array(G, dtype=np.float64)
    K = G.shape[0]
    d = np.diag(G)
    ok = np.isfinite(d) & (d >= 0)
    live = np.flatnonzero(ok)
    alpha = np.zeros(K)
    sim = np.full(K, np.nan)
    rejected = [int(i) for i in np.flatnonzero(~ok)]
    if live.size <= 1:
        alpha[live] = 1.0
        return alpha, sim, rejected
    Gl = G[np.ix_(live, live)]
    n = np.sqrt(np.diag(Gl))
    with np.errstate(all="ignore"):
        cs = Gl / np.sqrt(np.outer(np.diag(Gl), np.diag(Gl)))  # n_i n_j; 1 for equal rows
    cs[(n == 0)[:, None] | (n == 0)[None, :]] = 0.0
    off = ~np.eye(live.size, dtype=bool)
    v = np.where(off, cs, -np.inf).max(axis=1)
    with np.errstate(all="ignore"):
        ratio = v[:, None] / v[None, :]
    pardon = (v[None, :] > v[:, None]) & (v[None, :] != 0)
    with np.errstate(all="ignore"):
        cs = np.where(pardon, cs * ratio, cs)
    m = np.where(off, cs, -np.inf).max(axis=1)
    m = np.where(np.isnan(np.where(off, cs, 0.0)).any(axis=1), np.nan, m)
    a = np.where(np.isnan(m), 0.0, np.clip(1.0 - m, 0.0, 1.0))
    sim[live] = m
    if a.max() > 0:
        a = a / a.max()
        a[a == 1.0] = 0.99
        with np.errstate(all="ignore"):
            a = np.where(a == 0, 0.0, np.clip(kappa * (np.log(a / (1.0 - a)) + 0.5), 0.0, 1.0))
    alpha[live] = a
    return alpha, sim, rejected


def combine_bits(X, base, c):
    """fl32(base + sum_k fl32(c_k * fl32(x_k - base))) as uint32 [P]: subtract, multiply,
    add in the order given, then add to base, every operation rounded once (the
    arithmetic of dls_centered_clip_step_f32)."""
    X = np.asarray(X, np.float32)
    base = np.asarray(base, np.float32)
    c = np.asarray(c, np.float32)
    acc = None
    for k in range(X.shape[0]):
        t = ((X[k] - base).astype(np.float32) * c[k]).astype(np.float32)
        acc = t if acc is None else (acc + t).astype(np.float32)
    return (base + acc).astype(np.float32).view(np.uint32)


def coefficients(alpha):
    """fl32(alpha_k / sum alpha) over the clients with alpha > 0, the sum taken in the
    order given in fp64: (kept indices, float32 coefficients)."""
    kept = [k for k, a in enumerate(alpha) if a > 0]
    total = 0.0
    for k in kept:
        total += float(alpha[k])
    return kept, np.array([float(alpha[k]) / total for k in kept], np.float64).astype(np.float32)


def median_bits(X):
    """The coordinate-wise median of float32 rows as dls_trimmed_mean_f32 defines it for
    finite values: the middle value, or fl32(fl32(lo + hi) / 2) for an even count."""
    S = np.sort(np.asarray(X, np.float32), axis=0)
    K = S.shape[0]
    if K % 2:
        return S[K // 2].copy()
    return ((S[K // 2 - 1] + S[K // 2]).astype(np.float32) / np.float32(2)).astype(np.float32)
