"""CPU reference of the fused centered-clipping step (include/dls_hip.h,
dls_centered_clip_step_f32) and of the centered-clipping rule on it (Karimireddy, He &
Jaggi 2021) - TEST INFRASTRUCTURE ONLY (the package has no CPU path).  Written
independently of ``aggregation.clip_scales`` and ``ClientUpdateStore.centered_clip``.
"""
import numpy as np

from tests.geomedian_ref import TOL, sqdist_to  # noqa: F401  (the distances' contract)

assert TOL == 2.0 ** -17


def step_bits(X, c, z):
    """uint32 [P]: z' = fl32(z + sum_k fl32(c[k] * fl32(X[k] - z))) - subtract,
    multiply, add in row order, then add to z; one fp32 rounding per operation, no fma."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    c = np.asarray(c, dtype=np.float32)
    z = np.asarray(z, dtype=np.float32)
    assert X.shape[0] == c.shape[0] >= 1 and X.shape[1:] == z.shape
    with np.errstate(all="ignore"):
        acc = None
        for k in range(X.shape[0]):
            d = (X[k] - z).astype(np.float32)
            t = (c[k] * d).astype(np.float32)
            acc = t if acc is None else (acc + t).astype(np.float32)
        out = (z + acc).astype(np.float32)
    return out.view(np.uint32).copy()


def scales(dist2, tau):
    """(kept indices, fp64 scales, float32 coefficients): entries of dist2 that are not
    finite or are negative are dropped; s = 1 where sqrt(dist2) <= tau, else tau /
    sqrt(dist2); the coefficients are float32(s / number kept)."""
    d2 = np.asarray(dist2, dtype=np.float64)
    tau = float(tau)
    assert np.isfinite(tau) and tau > 0
    with np.errstate(all="ignore"):
        kept = [int(i) for i in np.flatnonzero(np.isfinite(d2) & (d2 >= 0))]
    if not kept:
        raise ValueError("nothing kept")
    dist = np.sqrt(d2[kept])
    with np.errstate(all="ignore"):
        s = np.where(dist <= tau, 1.0, tau / np.where(dist > 0, dist, 1.0))
    return kept, s, (s / np.float64(len(kept))).astype(np.float32)


def centered_clip64(X, v0, tau, iters):
    """fp64 centered clipping from v0: (v, [per step the scales], [per step the step's
    length])."""
    X = np.asarray(X, dtype=np.float64)
    v = np.asarray(v0, dtype=np.float64).copy()
    all_s, moved = [], []
    for _ in range(int(iters)):
        D = X - v[None, :]
        dist = np.sqrt((D * D).sum(axis=1))
        s = np.where(dist <= tau, 1.0, tau / np.where(dist > 0, dist, 1.0))
        step = (s[:, None] * D).sum(axis=0) / X.shape[0]
        v = v + step
        all_s.append(s)
        moved.append(float(np.sqrt((step * step).sum())))
    return v, all_s, moved
