"""numpy reference of the stochastic quantizer (include/dls_hip.h: dls_qsgd_compress_f32,
dls_qsgd_fedavg_f32) - TEST INFRASTRUCTURE ONLY.  Every fp32 step is a numpy float32 operation
(one rounding each); the L2 norm's sum is fp64 in the contract's order.  The Philox words of
the coordinates 0 .. 512 NB - 1 come in as an argument (tests/dp_ref.words makes them)."""
import numpy as np

F32, F64 = np.float32, np.float64
BUCKET = 512


def buckets(P):
    return -(-P // BUCKET)


def levels(bits):
    return (1 << (bits - 1)) - 1


def quantize(u, P, bits, norm, words):
    """(q int32 [512 NB], d fp32 [NB], nonfinite) of the update u[:P]; norm 0 max, 1 l2."""
    NB, s = buckets(P), F32(levels(bits))
    u = np.concatenate([np.asarray(u[:P], F32), np.zeros(BUCKET * NB - P, F32)]).reshape(NB, BUCKET)
    a = np.abs(u)
    with np.errstate(all="ignore"):
        if norm == 0:
            n = a.view(np.uint32).max(axis=1).view(F32)
        else:
            v = (u.astype(F64) ** 2).reshape(NB, 64, 8)
            lane = v[:, :, 0]
            for k in range(1, 8):
                lane = lane + v[:, :, k]
            for dist in (32, 16, 8, 4, 2, 1):
                lane = lane + lane[:, np.arange(64) ^ dist]
            n = np.sqrt(lane[:, 0]).astype(F32)
        r, d = (s / n).astype(F32), (n / s).astype(F32)
        t = (a * r[:, None]).astype(F32)
        l0 = np.floor(t)
        f = (t - l0).astype(F32)
        xi = (np.asarray(words, np.uint32)[:BUCKET * NB] >> np.uint32(8)).astype(F32) * F32(2.0 ** -24)
        l = (l0 + (xi.reshape(NB, BUCKET) < f).astype(F32)).astype(F32)
        l = np.where(l < s, l, s).astype(np.int32)
    q = np.where(u < 0, -l, l) * ((n > 0) & np.isfinite(n))[:, None]
    return q.reshape(-1).astype(np.int32), d, int((~np.isfinite(u)).sum())


def pack(q, bits):
    """uint32 [NB * 16 * bits]: field j at bit (j % (32 / bits)) * bits of word j / (32 / bits)."""
    per = 32 // bits
    fields = (q.astype(np.int64) & ((1 << bits) - 1)).reshape(-1, per)
    return (fields << (np.arange(per) * bits)).sum(axis=1).astype(np.uint32)


def unpack(codes, bits):
    """int32 levels of every field of the uint32 words."""
    per = 32 // bits
    f = (np.asarray(codes, np.uint32).astype(np.int64)[:, None] >> (np.arange(per) * bits)) & ((1 << bits) - 1)
    return np.where(f >= 1 << (bits - 1), f - (1 << bits), f).reshape(-1).astype(np.int32)


def compress(w, base, P, bits, norm, words):
    """(codes, scales, nonfinite)."""
    with np.errstate(all="ignore"):
        q, d, bad = quantize((w[:P] - base[:P]).astype(F32), P, bits, norm, words)
    return pack(q, bits), d, bad


def decode(codes, scales, P, bits):
    """fp64 q * d of the first P coordinates."""
    return (unpack(codes, bits).astype(F64) * np.repeat(scales.astype(F64), BUCKET))[:P]


def fedavg(base, rows, ns, P, bits):
    """fl(base + acc), acc the chain of fl(q_i * fl(fl(d_i[B] * n_i) / N)) over ``rows`` (a list
    of (codes, scales)) in order, the first assigning."""
    N, NB, acc = F32(sum(int(n) for n in ns)), buckets(P), None
    for (codes, d), n_i in zip(rows, ns):
        c = ((np.asarray(d, F32)[:NB] * F32(int(n_i))).astype(F32) / N).astype(F32)
        p = (unpack(codes[:NB * 16 * bits], bits).astype(F32) * np.repeat(c, BUCKET)).astype(F32)
        acc = p if acc is None else (acc + p).astype(F32)
    return (np.asarray(base[:P], F32) + acc[:P]).astype(F32)
