"""numpy reference of the scaled-sign compressor and the FedAvg over bit rows
(include/dls_hip.h: dls_efsign_compress_f32, dls_efsign_fedavg_f32) - TEST INFRASTRUCTURE
ONLY.  Every fp32 step is a numpy float32 operation (one rounding each); L1_t is math.fsum."""
import math

import numpy as np

from tests.topk_ref import bits, update  # noqa: F401  (u = fl(fl(w - base) + e))

F32 = np.float32


def segments(sizes, slack=()):
    """(bounds, count) of tensors of ``sizes`` real elements, each padded to whole 64-slot
    words; the tensors listed in ``slack`` get one more word of padding."""
    bounds = [0]
    for t, n in enumerate(sizes):
        bounds.append(bounds[-1] + -(-n // 64) * 64 + (64 if t in slack else 0))
    return bounds, list(sizes)


def pack(neg):
    """bool [P] -> uint64 [P / 64]: bit j % 64 of word j / 64."""
    return np.packbits(neg.reshape(-1, 64), axis=1, bitorder="little").view("<u8").reshape(-1)


def unpack(words, P):
    return np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little")[:P] != 0


def compress(w, base, e, bounds, count, scales=None):
    """(bits uint64 [P / 64], scales fp32 [T], e_new fp32 [P], nonfinite); ``scales`` given:
    those instead of the reference's own."""
    u = update(w, base, e)
    neg, e_new = np.zeros(u.size, bool), np.zeros(u.size, F32)
    s = np.zeros(len(count), F32) if scales is None else np.asarray(scales, F32)
    bad = 0
    with np.errstate(all="ignore"):
        for t, (a, n) in enumerate(zip(bounds, count)):
            ut = u[a:a + n]
            bad += int((~np.isfinite(ut)).sum())
            if scales is None:
                s[t] = F32(math.fsum(np.abs(ut.astype(np.float64))) / n)
            neg[a:a + n] = ut < 0
            e_new[a:a + n] = np.where(ut < 0, (ut + s[t]).astype(F32), (ut - s[t]).astype(F32))
    return pack(neg), s, e_new, bad


def fedavg(base, rows, bounds, count, ns):
    """out = base on padding and fl(base + acc) on real slots, acc the chain of +-fl(fl(s *
    n_i) / N) over ``rows`` (a list of (bits, scales)) in order, the first assigning."""
    base = np.asarray(base, F32)
    N = F32(sum(int(n) for n in ns))
    out = base.copy()
    for t, (a, n) in enumerate(zip(bounds, count)):
        acc = None
        for (words, s), n_i in zip(rows, ns):
            c = F32(F32(F32(s[t]) * F32(int(n_i))) / N)
            term = np.where(unpack(words, base.size)[a:a + n], -c, c).astype(F32)
            acc = term if acc is None else (acc + term).astype(F32)
        out[a:a + n] = (base[a:a + n] + acc).astype(F32)
    return out
