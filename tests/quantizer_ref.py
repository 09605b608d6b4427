"""CPU reference of the quantizer chain (include/dls_hip.h: dls_segment_minmax_f32,
dls_qparams_minmax, dls_quantize_affine) — TEST INFRASTRUCTURE ONLY (the package
has no CPU path).

numpy only.  Where the header fixes the arithmetic every operation is one
``np.float32`` operation (one rounding each); min / max are ``np.fmin`` /
``np.fmax`` (fminf / fmaxf: a NaN operand is dropped), so every special value
has a defined result:

* an empty or all-NaN segment has (min, max) = (+inf, -inf);
* zeros compare by value (the sign of a zero minimum / maximum is open);
* a NaN quantizes to qmin, +inf to qmax, -inf to qmin.
"""
import numpy as np

F32 = np.float32
EPS = F32(2.0 ** -23)  # torch.finfo(torch.float32).eps


def _f32(a):
    return np.atleast_1d(np.asarray(a, dtype=np.float32))


def segment_minmax(x, seg_off):
    """fp32 [nseg] minima and maxima of x[seg_off[s]:seg_off[s+1]], NaNs ignored."""
    x = _f32(x).reshape(-1)
    off = np.asarray(seg_off, dtype=np.int64)
    nseg = len(off) - 1
    mins = np.full(nseg, np.inf, F32)
    maxs = np.full(nseg, -np.inf, F32)
    for s in range(nseg):
        part = x[off[s]:off[s + 1]]
        part = part[~np.isnan(part)]
        if part.size:
            mins[s] = part.min()
            maxs[s] = part.max()
    return mins, maxs


def qparams(lo, hi, qmin, qmax, symmetric=False):
    """(scale fp32 [n], zero point int32 [n]) of the header's two formulas."""
    with np.errstate(all="ignore"):
        lo = np.fmin(_f32(lo), F32(0))
        hi = np.fmax(_f32(hi), F32(0))
        if symmetric:
            half = F32(qmax - qmin) / F32(2)
            scale = np.fmax(np.fmax(-lo, hi) / half, EPS)
            zp = 0 if qmin < 0 else (qmin + qmax + 1) // 2
            return scale.astype(F32), np.full(scale.shape, zp, np.int32)
        scale = np.fmax((hi - lo) / F32(qmax - qmin), EPS).astype(F32)
        z = F32(qmin) - np.rint(lo / scale)  # NaN for lo = -inf: dropped by the fmax below
        z = np.fmin(np.fmax(z, F32(qmin)), F32(qmax))
        return scale, z.astype(np.int32)


def segment_of(seg_off, total):
    """int64 [total]: the segment of each element (empty segments own nothing)."""
    off = np.asarray(seg_off, dtype=np.int64)
    assert off[0] == 0 and off[-1] == total and np.all(np.diff(off) >= 0)
    return np.searchsorted(off[:-1], np.arange(total, dtype=np.int64), side="right") - 1


def _scaled(x, seg_off, scale, zp):
    x = _f32(x).reshape(-1)
    s = segment_of(seg_off, x.size)
    sc = _f32(scale)[s]
    z = np.atleast_1d(np.asarray(zp, dtype=np.int32))[s].astype(F32)
    inv = F32(1) / sc
    return x * inv, sc, z


def _clamp(r, z, qmin, qmax):
    # fmax drops a NaN: NaN -> qmin; +-inf -> the clamps
    return np.fmin(np.fmax(r + z, F32(qmin)), F32(qmax))


def quantize(x, seg_off, scale, zp, qmin, qmax):
    """(q int32 [total], deq fp32 [total]): q = clamp(rne(fl(x * fl(1/scale))) + zp),
    deq = fl(fl(q - zp) * scale)."""
    with np.errstate(all="ignore"):
        v, sc, z = _scaled(x, seg_off, scale, zp)
        qf = _clamp(np.rint(v), z, qmin, qmax)
        deq = ((qf - z) * sc).astype(F32)
    return qf.astype(np.int32), deq


def stochastic_bracket(x, seg_off, scale, zp, qmin, qmax):
    """The two admissible q of stochastic rounding, int32 [total] each:
    clamp(floor(v) + zp) and clamp(floor(v) + 1 + zp)."""
    with np.errstate(all="ignore"):
        v, _, z = _scaled(x, seg_off, scale, zp)
        f = np.floor(v)
        lo = _clamp(f, z, qmin, qmax)
        hi = _clamp(f + F32(1), z, qmin, qmax)
    return lo.astype(np.int32), hi.astype(np.int32)


def as_bytes(q, qmin):
    """The stored byte of each q: int8 for a signed range, else uint8."""
    return np.asarray(q).astype(np.int8 if qmin < 0 else np.uint8)
