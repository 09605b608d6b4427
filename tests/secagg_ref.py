"""CPU reference of the two secure-aggregation entry points (include/dls_hip.h:
dls_secagg_mask_f32, dls_secagg_unmask_f32) - TEST INFRASTRUCTURE ONLY (the package has no
CPU path).

* the mask words from ``tests.dp_ref.words`` (Philox4x32-10 in numpy);
* the encode in numpy float32, the ring in uint32 / uint64 arithmetic, the decode in float64;
* CPU stand-ins for the two wrappers (``install``).
Every contract is exact: the tests compare bits.
"""
import functools

import numpy as np
import torch

from tests import dp_ref

F32 = np.float32
U32 = np.uint32


@functools.lru_cache(maxsize=256)
def words(P, seed, stream_id):
    """uint32 [P], read-only: ``dp_ref.words(P, seed, stream_id)``, with the counters built as
    one array (the tests draw up to 64 streams of half a million coordinates)."""
    P, seed, stream_id = int(P), int(seed), int(stream_id)
    b = np.arange((P + 3) // 4, dtype=np.uint64)
    ctr = np.stack([b & dp_ref.MASK, b >> np.uint64(32),
                    np.full_like(b, stream_id & 0xFFFFFFFF), np.full_like(b, stream_id >> 32)],
                   axis=-1)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    out = dp_ref.philox4x32(ctr, key).reshape(-1)[:P].copy()
    out.setflags(write=False)
    return out


def mask_words(P, seed, streams):
    """uint32 [P]: the sum mod 2^32 of the words of coordinates 0..P-1 under every stream."""
    acc = np.zeros(int(P), np.uint64)
    for t in streams:
        acc += words(P, seed, t)
    return (acc & np.uint64(0xFFFFFFFF)).astype(U32)


def quantise(w, base, frac_bits, bits):
    """(q int64 [P], saturated bool [P], nonfinite bool [P]) of the encode: d = fl32(w - base),
    r = rint(fl32(d * 2^frac_bits)) (ties to even), q = clamp(r, -L, L), 0 where d is not
    finite; saturated: d finite and |r| > L."""
    L = (1 << (bits - 1)) - 1
    with np.errstate(all="ignore"):
        d = (np.asarray(w, F32) - np.asarray(base, F32)).astype(F32)
        x = (d * np.ldexp(F32(1.0), int(frac_bits))).astype(F32)
        r = np.rint(x).astype(np.float64)  # an integer or an infinity: exact in fp64
    bad = ~np.isfinite(d)
    sat = ~bad & (np.abs(r) > L)
    q = np.clip(np.where(bad, 0.0, r), -L, L).astype(np.int64)
    return q, sat, bad


def encode(w, base, frac_bits, bits, weight):
    """(e uint32 [P] = q * weight mod 2^32, #saturated, #nonfinite)."""
    q, sat, bad = quantise(w, base, frac_bits, bits)
    e = ((q.astype(np.uint64) * np.uint64(weight)) & np.uint64(0xFFFFFFFF)).astype(U32)  # wraps
    return e, int(sat.sum()), int(bad.sum())


def mask(w, base, frac_bits, bits, weight, add, sub, seed):
    """(y uint32 [P], #saturated, #nonfinite): dls_secagg_mask_f32."""
    e, n_sat, n_bad = encode(w, base, frac_bits, bits, weight)
    P = e.size
    with np.errstate(over="ignore"):
        y = e + mask_words(P, seed, add) - mask_words(P, seed, sub)
    return y.astype(U32), n_sat, n_bad


def ring_sum(rows):
    """uint32 [P]: the sum mod 2^32 of uint32 rows [K, P]."""
    return (np.asarray(rows, U32).astype(np.uint64).sum(axis=0) & np.uint64(0xFFFFFFFF)).astype(U32)


def decode(S, base, frac_bits, total):
    """uint32 bits of out = fl32(base + (float)((double)(int32)S * 2^-frac_bits / total))."""
    v = np.asarray(S, U32).view(np.int32).astype(np.float64)
    delta = ((v * 2.0 ** -int(frac_bits)) / np.float64(total)).astype(F32)
    return (np.asarray(base, F32) + delta).astype(F32).view(U32).copy()


def unmask(Y, rows, add, sub, seed, base, frac_bits, total, P):
    """(out bits uint32 [P], S uint32 [P]): dls_secagg_unmask_f32."""
    X = np.asarray(Y, U32)[np.asarray(rows, np.int64), :P]
    with np.errstate(over="ignore"):
        S = (ring_sum(X) + mask_words(P, seed, add) - mask_words(P, seed, sub)).astype(U32)
    return decode(S, np.asarray(base, F32)[:P], frac_bits, total), S


def stream_table(ids):
    """The int64 tensor (uint64 bit patterns) the wrappers take, or None for no stream."""
    if not len(ids):
        return None
    return torch.from_numpy(np.array([int(i) for i in ids], dtype=np.uint64).view(np.int64).copy())


# ----------------------------------------------------------- CPU stand-ins
def _np(t):
    return t.detach().cpu().numpy()


def _ids(t):
    return [] if t is None else [int(i) for i in _np(t).view(np.uint64)]


def secagg_mask(w, base, P, frac_bits, bits, weight, add_streams, sub_streams, seed, y, stats,
                stream=None):
    yb, n_sat, n_bad = mask(_np(w)[:P], _np(base)[:P], frac_bits, bits, weight, _ids(add_streams),
                            _ids(sub_streams), seed)
    y[:P].copy_(torch.from_numpy(yb.view(np.int32).copy()))
    stats += torch.tensor([n_sat, n_bad], dtype=torch.int32)
    return y


def secagg_unmask(Y, rows, add_streams, sub_streams, seed, base, frac_bits, total, P, out,
                  sum_out=None, stream=None):
    ob, S = unmask(_np(Y).view(U32), _np(rows), _ids(add_streams), _ids(sub_streams), seed,
                   _np(base), frac_bits, total, P)
    out[:P].copy_(torch.from_numpy(ob.view(F32).copy()))
    if sum_out is not None:
        sum_out[:P].copy_(torch.from_numpy(S.view(np.int32).copy()))
    return out


_DOUBLES = ("secagg_mask", "secagg_unmask")


def install(monkeypatch):
    """cpu_doubles.install, then the stand-ins above."""
    from distributed_learning_simulator_amd import _native
    from tests import cpu_doubles
    cpu_doubles.install(monkeypatch)
    for name in _DOUBLES:
        monkeypatch.setattr(_native, name, globals()[name])
