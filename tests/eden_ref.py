"""numpy reference of the multi-bit rotated compressor (include/dls_hip.h:
dls_eden_compress_f32, dls_eden_fedavg_f32) on top of tests/drive_ref.py's rotation - TEST
INFRASTRUCTURE ONLY.  Every fp32 step is a numpy float32 operation (one rounding each); the
sums sq, dot and qq are fp64 in the contract's order, so random inputs are bit-exact too.  The
codebooks are the binding's constants, which tests/test_eden_host.py checks against the
Lloyd-Max conditions and the header."""
import numpy as np

from distributed_learning_simulator_amd._native import EDEN_BOUNDS, EDEN_CENTROIDS
from tests.drive_ref import D, F32, bits, blocks, rotate  # noqa: F401

F64 = np.float64


def ordered_sum(t):
    """Per block the fp64 sum of t [NB, 4096] in the kernels' order: coordinate 1024 v + 64 r + l
    belongs to thread (v, l), which adds r = 0..15 ascending; the xor butterfly 32..1 over l;
    the four v in order."""
    t = t.reshape(-1, 4, 16, 64)
    acc = t[:, :, 0]
    for r in range(1, 16):
        acc = acc + t[:, :, r]
    for dist in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, :, np.arange(64) ^ dist]
    w = acc[:, :, 0]
    return ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]


def quantize(y, b):
    """(fields [NB, 4096], scales-to-be (sq, dot, qq), thr [NB, M - 1]) of the rotated y."""
    cent, bound = np.array(EDEN_CENTROIDS[b], F32), np.array(EDEN_BOUNDS[b], F32)
    y = np.asarray(y, F32).reshape(-1, D)
    with np.errstate(all="ignore"):
        sq = ordered_sum(y.astype(F64) ** 2)
        rms = np.sqrt(sq / float(D)).astype(F32)
        thr = (bound[None, :] * rms[:, None]).astype(F32)
        m = (np.abs(y)[:, :, None] > thr[:, None, :]).sum(axis=2)
        c = cent[m].astype(F64)
        dot, qq = ordered_sum(np.abs(y).astype(F64) * c), ordered_sum(c * c)
    return m | ((y < 0).astype(np.int64) << (b - 1)), (sq, dot, qq), thr


def pack(f, b):
    """uint32 [NB * 128 * b]: field (v, r, l) at bit (r % fpw) * b of word (v * (b / 2) + r / fpw)
    * 64 + l of its block, fpw = 32 / b."""
    fpw = 32 // b
    f = f.reshape(-1, 4, b // 2, fpw, 64).astype(np.uint64)
    return (f << (np.arange(fpw, dtype=np.uint64) * np.uint64(b))[:, None]).sum(axis=3).astype(
        np.uint32).reshape(-1)


def unpack(codes, b):
    """The fields [NB, 4096] of the uint32 words."""
    fpw = 32 // b
    w = np.asarray(codes, np.uint32).astype(np.int64).reshape(-1, 4, b // 2, 1, 64)
    return ((w >> (np.arange(fpw) * b)[:, None]) & ((1 << b) - 1)).reshape(-1, D)


def compress(w, base, P, b, words, mode):
    """(codes uint32 [NB * 128 * b], scales fp32 [NB], nonfinite); mode 0 unbiased, 1 min-MSE."""
    with np.errstate(all="ignore"):
        u = (w[:P] - base[:P]).astype(F32)
        f, (sq, dot, qq), _ = quantize(rotate(u, P, words), b)
        s = np.where(dot == 0, 0.0, (sq / dot) if mode == 0 else dot / qq).astype(F32)
    return pack(f, b), s, int((~np.isfinite(u)).sum())


def decode(codes, scales, b):
    """fp64 scale * (+-cent) of every rotated coordinate."""
    f = unpack(codes, b)
    q = np.array(EDEN_CENTROIDS[b], F64)[f & ((1 << (b - 1)) - 1)] * np.where(f >> (b - 1), -1.0, 1.0)
    return (q * np.asarray(scales, F64)[:, None]).reshape(-1)


def fedavg(base, rows, ns, P, b, words):
    """fl(base + v), v the inverse rotation of the chain of t[i][f] = +-fl(c_i * cent[m]), c_i =
    fl(fl(s[B] * n_i) / N), over ``rows`` (a list of (codes, scales)) in order, the first
    assigning; the sign bit is set, not flipped."""
    N, NB, M = F32(sum(int(n) for n in ns)), blocks(P), 1 << (b - 1)
    cent, z = np.array(EDEN_CENTROIDS[b], F32), None
    for (codes, s), n_i in zip(rows, ns):
        c = ((np.asarray(s, F32)[:NB] * F32(int(n_i))).astype(F32) / N).astype(F32)
        f = unpack(codes[:NB * 128 * b], b)
        t = (c[:, None] * cent[f & (M - 1)]).astype(F32)
        term = (t.view(np.uint32) | ((f >> (b - 1)).astype(np.uint32) << np.uint32(31))).view(F32)
        term = term.reshape(-1)
        z = term if z is None else (z + term).astype(F32)
    return (np.asarray(base[:P], F32) + rotate(z, P, words, inverse=True)).astype(F32)
