"""CPU reference of the fused Weiszfeld step, the row-to-point squared distances
(include/dls_hip.h, dls_weiszfeld_step_f32 / dls_rows_sqdist_to_f32) and the
geometric-median rule on them - TEST INFRASTRUCTURE ONLY (the package has no CPU
path).  Written independently of ``aggregation.weiszfeld_weights`` and
``ClientUpdateStore.geometric_median``.
"""
import numpy as np

TOL = 2.0 ** -17  # the contract's bound: (120 + 8) * 2^-24 relative


def step_bits(X, w):
    """uint32 [P]: z = sum_k fl32(w[k] * X[k]) - multiply, then add in row order, one
    fp32 rounding per operation, no fma."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    w = np.asarray(w, dtype=np.float32)
    assert X.shape[0] == w.shape[0] >= 1
    with np.errstate(all="ignore"):
        acc = (w[0] * X[0]).astype(np.float32)
        for k in range(1, X.shape[0]):
            t = (w[k] * X[k]).astype(np.float32)
            acc = (acc + t).astype(np.float32)
    return acc.view(np.uint32).copy()


def sqdist_to(X, z):
    """fp64 [K]: the squared distances of the fp32 rows of X to the fp32 point z, every
    term from the difference; a row with inf / NaN gives inf / NaN."""
    X = np.asarray(X, dtype=np.float32).astype(np.float64)
    z = np.asarray(z, dtype=np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        d = X - z[None, :]
        return (d * d).sum(axis=1)


def weights(dist2, nu):
    """(kept indices, float32 weights): entries of dist2 that are not finite or are
    negative are dropped; beta = 1 / max(nu, sqrt(dist2)); the weights are
    float32(beta / sum(beta)), the sum taken in ascending index order in fp64."""
    d2 = np.asarray(dist2, dtype=np.float64)
    nu = float(nu)
    assert np.isfinite(nu) and nu > 0
    with np.errstate(all="ignore"):
        kept = [int(i) for i in np.flatnonzero(np.isfinite(d2) & (d2 >= 0))]
    if not kept:
        raise ValueError("nothing kept")
    beta = 1.0 / np.maximum(nu, np.sqrt(d2[kept]))
    total = np.float64(0.0)
    for b in beta:  # sequential: np.sum would add pairwise
        total = total + b
    return kept, (beta / total).astype(np.float32)


def median0(X):
    """The fp64 coordinate-wise median (an even K averages the two middle values)."""
    return np.median(np.asarray(X, dtype=np.float64), axis=0)


def weiszfeld64(X, iters, nu, z0=None):
    """fp64 smoothed Weiszfeld from z0 (default: the coordinate-wise median):
    (z, [objective after the start and after each step])."""
    X = np.asarray(X, dtype=np.float64)
    z = median0(X) if z0 is None else np.asarray(z0, dtype=np.float64)
    dist = np.sqrt(((X - z[None, :]) ** 2).sum(axis=1))
    objective = [float(dist.sum())]
    for _ in range(int(iters)):
        beta = 1.0 / np.maximum(float(nu), dist)
        z = (beta[:, None] * X).sum(axis=0) / beta.sum()
        dist = np.sqrt(((X - z[None, :]) ** 2).sum(axis=1))
        objective.append(float(dist.sum()))
    return z, objective
