"""numpy reference of the rotated one-bit compressor (include/dls_hip.h:
dls_hadamard_rotate_f32, dls_drive_compress_f32, dls_drive_fedavg_f32) - TEST INFRASTRUCTURE
ONLY.  Every fp32 step is a numpy float32 operation (one rounding each); the sums are fp64.
sigma comes in as the dls_philox_u32 words of the coordinates 0 .. Pd / 32 - 1, which
tests/test_gpu_dpnoise.py pins: the reference has no Philox of its own."""
import numpy as np

from tests.efsign_ref import pack, unpack
from tests.topk_ref import bits  # noqa: F401

F32 = np.float32
D = 4096


def blocks(P):
    return -(-P // D)


def flip(x, neg):
    """sigma * x: the sign bit flipped where ``neg``."""
    return (x.view(np.uint32) ^ (neg.astype(np.uint32) << np.uint32(31))).view(F32)


def hadamard(x):
    """2^-6 H per block of 4096: the stages h = 1 .. 2048 ascending, (a, b) -> (a + b, a - b)
    on every pair (i, i + h) with i & h == 0."""
    x = np.asarray(x, F32).reshape(-1, D)
    h = 1
    with np.errstate(all="ignore"):
        while h < D:
            p = x.reshape(x.shape[0], -1, 2, h)
            a, b = p[:, :, 0, :], p[:, :, 1, :]
            x = np.stack([(a + b).astype(F32), (a - b).astype(F32)], axis=2).reshape(-1, D)
            h *= 2
        return (x * F32(2.0 ** -6)).astype(F32).reshape(-1)


def rotate(x, P, words, inverse=False):
    """Forward: x[:P] -> y[:Pd]; inverse: y[:Pd] -> x[:P]."""
    Pd = D * blocks(P)
    neg = unpack(words, Pd)
    if inverse:
        return flip(hadamard(x[:Pd]), neg)[:P]
    return hadamard(flip(np.concatenate([np.asarray(x[:P], F32), np.zeros(Pd - P, F32)]), neg))


def compress(w, base, P, words, mode):
    """(bits uint64 [Pd / 64], scales fp32 [NB], nonfinite); mode 0 unbiased, 1 min-MSE."""
    with np.errstate(all="ignore"):
        u = (w[:P] - base[:P]).astype(F32)
        y = rotate(u, P, words).astype(np.float64).reshape(-1, D)
        sq, l1 = (y * y).sum(axis=1), np.abs(y).sum(axis=1)
        s = np.where(l1 == 0, 0.0, (sq / l1) if mode == 0 else l1 / float(D)).astype(F32)
    return pack(y.reshape(-1) < 0), s, int((~np.isfinite(u)).sum())


def fedavg(base, rows, ns, P, words):
    """fl(base + v), v the inverse rotation of the chain of +-fl(fl(s[B] * n_i) / N) over
    ``rows`` (a list of (bits, scales)) in order, the first assigning."""
    N = F32(sum(int(n) for n in ns))
    Pd = D * blocks(P)
    z = None
    for (client, s), n_i in zip(rows, ns):
        c = np.repeat(((np.asarray(s, F32)[:blocks(P)] * F32(int(n_i))).astype(F32) / N).astype(F32), D)
        term = flip(c, unpack(client, Pd))
        z = term if z is None else (z + term).astype(F32)
    return (np.asarray(base[:P], F32) + rotate(z, P, words, inverse=True)).astype(F32)
