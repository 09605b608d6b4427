"""The three fed_scaffold contracts of include/dls_hip.h restated in numpy float32 (every
operation rounded once), and the same formulas in fp64."""
import numpy as np

f32 = np.float32


def coeff(steps, lr, population=1):
    """fl32(1 / (steps * lr * population)), the quotient in fp64."""
    return f32(1.0 / (float(steps) * float(lr) * float(population)))


def local_step(p, g, x, corr, lr, wd, mu, control, dtype=f32):
    """One element-wise step; p, g, x, corr equally long (x, corr ignored where off)."""
    t = dtype
    p, g = p.astype(t), g.astype(t)
    d = g
    if wd != 0:
        d = d + t(wd) * p
    if mu != 0:
        d = d + t(mu) * (p - x.astype(t))
    if control:
        d = d + corr.astype(t)
    return p - t(lr) * d


def finish(y, x, c, ci, a, control, dtype=f32):
    """(delta, new c_i or None, number of non-finite deltas)."""
    t = dtype
    with np.errstate(all="ignore"):
        delta = y.astype(t) - x.astype(t)
        new = (ci.astype(t) - c.astype(t)) - t(a) * delta if control else None
    return delta, new, int((~np.isfinite(delta)).sum())


def server_step(U, n, b, eta_g, f, x, c, control, dtype=f32):
    """U: the K delta rows in the order they are walked; n: their sample counts; returns
    (x', c' or None)."""
    t = dtype
    total = t(sum(n))
    acc = s = None
    for k, row in enumerate(U):
        row = row.astype(t)
        term = (row * t(n[k])) / total
        acc = term if acc is None else acc + term
        if control:
            sk = t(b[k]) * row
            s = sk if s is None else s + sk
    xn = x.astype(t) + t(eta_g) * acc
    cn = (c.astype(t) - t(f) * c.astype(t)) - s if control else None
    return xn, cn
