"""numpy restatement of the dls_powersgd_* contract (include/dls_hip.h): u is formed in
float32 exactly as defined, everything after it in float64."""
import numpy as np

F32 = np.float32
U24 = 2.0 ** -24
CHUNK, TILE = 256, 64  # DLS_POWERSGD_CHUNK, DLS_POWERSGD_CLIENT_TILE


def g(L):
    """The header's factor for L roundings."""
    return L * U24 / (1 - L * U24)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def ru64(x):
    return (x + 63) // 64 * 64


def view(shape):
    numel = max(int(np.prod(shape)), 1)
    n = max(int(shape[0]), 1) if len(shape) else 1
    return n, numel // n


def compressed(n, m, r):
    return r <= min(n, m) and (n + m) * r < n * m


def plan(shapes, r, slack=()):
    """bounds, dims, kinds and payload blocks [(poff, qoff)] of a row of tensors (``slack``:
    tensors followed by one more word of padding), and the payload's length."""
    bounds, dims, kinds, blocks, off = [0], [], [], [], 0
    for t, shape in enumerate(shapes):
        n, m = view(shape)
        bounds.append(bounds[-1] + ru64(n * m) + (64 if t in slack else 0))
        dims.append((n, m))
        kinds.append(int(compressed(n, m, r)))
        blocks.append((off, off + ru64(n * r)) if kinds[-1] else (off, 0))
        off += ru64(n * r) + ru64(m * r) if kinds[-1] else ru64(n * m)
    return bounds, dims, kinds, blocks, off


def update(w, base, e=None):
    u = w.astype(F32) - base.astype(F32)
    return u if e is None else u + e.astype(F32)


def mgs(P):
    """Modified Gram-Schmidt, column order 0..r-1, a zero or non-finite norm -> a zero column."""
    P = P.astype(np.float64).copy()
    with np.errstate(all="ignore"):
        for q in range(P.shape[1]):
            n2 = float(np.sum(P[:, q] * P[:, q]))
            if not (n2 > 0 and np.isfinite(n2)):
                P[:, q] = 0.0
                continue
            P[:, q] /= np.sqrt(n2)
            P[:, q + 1:] -= np.outer(P[:, q], P[:, q] @ P[:, q + 1:])
    return P


def compress_tensor(U, Q0):
    """One compressed tensor: U float32 [n, m], Q0 float32 [m, r] -> P (fp64), P^ rounded to
    float32, Q = U^T P^ (fp64, from the rounded P^), e = U - P^ Q^T (fp64)."""
    U64 = U.astype(np.float64)
    with np.errstate(all="ignore"):
        P = U64 @ Q0.astype(np.float64)
        Ph = mgs(P).astype(F32)
        Q = U64.T @ Ph.astype(np.float64)
        return P, Ph, Q, U64 - Ph.astype(np.float64) @ Q.T


def server_tensor(base, Phs, Qs, ns):
    """base [n, m] + sum_i fl(c_i P^_i) Q_i^T in fp64, and the sum of the terms' magnitudes."""
    N = F32(sum(ns))
    out, mag = base.astype(np.float64), np.abs(base.astype(np.float64))
    for Ph, Q, n in zip(Phs, Qs, ns):
        A = ((F32(n) / N) * Ph.astype(F32)).astype(np.float64)
        out = out + A @ Q.astype(np.float64).T
        mag = mag + np.abs(A) @ np.abs(Q.astype(np.float64)).T
    return out, mag
