"""numpy reference of the microscaling compressor (include/dls_hip.h: dls_mx_compress_f32,
dls_mx_fedavg_f32) - TEST INFRASTRUCTURE ONLY.  Codes are integers; t = |u| 2^-e, the grid step
and the fraction f are fp64 values that hold them exactly (24-bit significands times powers of
two), so every comparison is the contract's comparison of real numbers.  The Philox words of the
coordinates 0 .. 512 NG - 1 come in as an argument (tests/dp_ref.words makes them)."""
import numpy as np

F32, F64 = np.float32, np.float64
GROUP, BLOCK = 512, 32
# name -> (mantissa bits M, emax, emin, code bits, fmax)
FORMATS = {"e4m3": (3, 8, -6, 8, 448.0), "e5m2": (2, 15, -14, 8, 57344.0), "e2m1": (1, 2, 0, 4, 6.0)}


def groups(P):
    return -(-P // GROUP)


def step(t, fmt):
    """The grid step at t >= 0 (fp64, elementwise)."""
    M, _, emin = FORMATS[fmt][:3]
    return np.ldexp(1.0, np.where(t > 0, np.maximum(np.frexp(t)[1] - 1, emin), emin) - M)


def value(mag, fmt):
    """fp64 value of the magnitude codes (sign bit stripped)."""
    M, _, emin = FORMATS[fmt][:3]
    ef, m = mag >> M, (mag & ((1 << M) - 1)).astype(F64)
    return np.where(ef > 0, np.ldexp(1.0 + m / (1 << M), ef - 1 + emin), np.ldexp(m, emin - M))


def quantize(u, P, fmt, rounding, words):
    """(codes int64 [512 NG], scale bytes uint8 [16 NG], dec fp32 [512 NG], nonfinite) of u[:P];
    rounding 0 nearest, 1 stochastic."""
    M, emax, emin, bits, fmax = FORMATS[fmt]
    n = GROUP * groups(P)
    u = np.concatenate([np.asarray(u[:P], F32), np.zeros(n - P, F32)])
    a = u.view(np.uint32) & np.uint32(0x7FFFFFFF)
    m = a.reshape(-1, BLOCK).max(axis=1).astype(np.int64)
    fm = int(F32(fmax).view(np.uint32)) & 0x7FFFFF
    e = np.maximum((m >> 23) - 127 - emax + ((m & 0x7FFFFF) > fm), -127)
    finite = m < 0x7F800000
    with np.errstate(all="ignore"):
        t = np.ldexp(np.where(np.repeat(finite, BLOCK), np.abs(u.astype(F64)), 0.0), -np.repeat(e, BLOCK))
        q = step(t, fmt)
        l0 = np.floor(t / q)
        f = t / q - l0
        if rounding == 0:
            up = (f > 0.5) | ((f == 0.5) & (l0 % 2 == 1))
        else:
            up = (np.asarray(words, np.uint32)[:n] >> np.uint32(8)).astype(F64) * 2.0 ** -24 < f
        v = (l0 + up) * q  # a grid point, at most fmax
        sub = v < 2.0 ** emin
        mant, ex = np.frexp(np.where(sub, 1.0, v))
        mag = np.where(sub, v * 2.0 ** (M - emin), ((ex - emin) << M) + (2 * mant - 1) * (1 << M)).astype(np.int64)
        code = np.where(np.repeat(finite, BLOCK), (np.signbit(u).astype(np.int64) << (bits - 1)) | mag, 0)
        dec = np.where(np.repeat(finite, BLOCK), np.copysign(np.ldexp(v, np.repeat(e, BLOCK)), u), 0.0).astype(F32)
    return code, np.where(finite, e + 127, 255).astype(np.uint8), dec, int((a[:P] >= 0x7F800000).sum())


def pack(code, fmt):
    """uint32 words: code j is byte j at 8 bits, nibble j & 1 of byte j >> 1 at 4."""
    if FORMATS[fmt][3] == 4:
        code = code[0::2] | (code[1::2] << 4)
    return np.ascontiguousarray(code.astype(np.uint8)).view(np.uint32)


def unpack(codes, fmt):
    b = np.ascontiguousarray(codes, np.uint32).view(np.uint8).astype(np.int64)
    return b if FORMATS[fmt][3] == 8 else np.stack([b & 15, b >> 4], axis=1).reshape(-1)


def compress(w, base, r, P, fmt, rounding, words):
    """(codes, scale bytes, r' or None, nonfinite); r None: no residual."""
    with np.errstate(all="ignore"):
        u = (w[:P] - base[:P]).astype(F32)
        if r is not None:
            u = (u + r[:P]).astype(F32)
        code, sb, dec, bad = quantize(u, P, fmt, rounding, words)
        rn = None if r is None else (u - dec[:P]).astype(F32)
    return pack(code, fmt), sb, rn, bad


def decode(codes, sb, P, fmt):
    """fp64 code * 2^e of the first P coordinates (exact; every one is an fp32 value)."""
    c, bits = unpack(codes, fmt), FORMATS[fmt][3]
    x = np.ldexp(value(c & ((1 << (bits - 1)) - 1), fmt), np.repeat(sb.astype(np.int64) - 127, BLOCK))
    return np.where(c >> (bits - 1) == 1, -x, x)[:P]


def fedavg(base, rows, ns, P, fmt):
    """fl(base + acc), acc the chain of fl(x_i * fl(n_i / N)) over ``rows`` (a list of (codes,
    scale bytes)) in order, the first assigning."""
    N, acc = F32(sum(int(n) for n in ns)), None
    for (codes, sb), n_i in zip(rows, ns):
        p = (decode(codes, sb, P, fmt).astype(F32) * (F32(int(n_i)) / N).astype(F32)).astype(F32)
        acc = p if acc is None else (acc + p).astype(F32)
    return (np.asarray(base[:P], F32) + acc).astype(F32)
