"""Plain numpy reference of the exact aggregation arithmetic and the fp32 sweeps
that drive the division kernels (TEST INFRASTRUCTURE; imports neither the
package nor the oracle).

The reference divides ``fl(x * fl32(n_i))`` by ``fl32(N)`` with one IEEE
rounding per operation (servers/fed_server.py:57-65); numpy's float32 ufuncs do
exactly that, denormals included, as long as nothing switched the CPU to
flush-to-zero (tests/test_division_host.py asserts it has not).
"""
import numpy as np

F32_BELOW_ONE = float(np.nextafter(np.float32(1), np.float32(0)))

# The divisors fl32(N) every sweep uses (tests/test_division_host.py proves the
# algorithm for those in [1, 2^31]; tests/test_gpu_division.py runs the device code).
DIVISORS = (
    1.0, 3.0, 7.0, 550.0,
    55123.0,        # two-constant quotient proven exact
    11735695.0,     # two-constant quotient NOT exact: Markstein
    16777215.0, 16777216.0, 16777218.0,
    8388607.0,      # all-ones mantissa
    2147483520.0,   # the largest fp32 below 2^31
    2147483648.0,   # last fast divisor
    2147483904.0,   # first slow divisor
    float(2 ** 40),
    0.5, 1.5,
    F32_BELOW_ONE,  # just below the fast range
    3e38,           # quotients go denormal or zero
)
assert all(float(np.float32(b)) == b for b in DIVISORS[:-1])  # fp32 values (3e38 rounds)

FAST_LO, FAST_HI = 1.0, 2147483648.0  # the kernels' Markstein range of divisors


def in_fast_divisor_range(b):
    return FAST_LO <= float(np.float32(b)) <= FAST_HI


def div_id(b):
    """A readable pytest id of a divisor."""
    return f"N={float(b):.9g}"


def mantissa_sweep():
    """All 2^23 fp32 values in [1, 2), ascending."""
    return (np.arange(1 << 23, dtype=np.uint32) | np.uint32(0x3F800000)).view(np.float32)


def binade_sweep(stride):
    """For every biased exponent 0..254 (denormals included) and both signs the
    mantissas 0, stride, 2 stride, ... and the binade's last mantissa; then
    +-0, +-inf and nan."""
    m = np.arange(0, 1 << 23, stride, dtype=np.uint32)
    if m[-1] != (1 << 23) - 1:
        m = np.append(m, np.uint32((1 << 23) - 1))
    e = np.arange(255, dtype=np.uint32)[:, None] << np.uint32(23)
    pos = (e | m[None, :]).reshape(-1)
    bits = np.concatenate([pos, pos | np.uint32(0x80000000),
                           np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000],
                                    np.uint32)])
    return bits.view(np.float32)


def guard_edges():
    """Both signs of the values one ulp either side of (and at) the kernels'
    exponent guard, 2^-60 and 2^61, the same around 2^60 (the bound the header
    used to state), and the smallest denormal: the neighbours binade_sweep's
    stride skips."""
    out = []
    for v in (2.0 ** -60, 2.0 ** 60, 2.0 ** 61):
        b = int(np.float32(v).view(np.uint32))
        out += [b - 1, b, b + 1]
    out.append(1)
    pos = np.array(out, np.uint32)
    return np.concatenate([pos, pos | np.uint32(0x80000000)]).view(np.float32)


def device_sweep(stride):
    """binade_sweep + guard_edges, padded with 1.0 to a multiple of 4 elements (the
    kernels' row granularity)."""
    return pad4(np.concatenate([binade_sweep(stride), guard_edges()]))


def weighted_terms(x, w, N):
    """fl(fl(x * fl32(w)) / fl32(N)): one fp32 rounding per operation."""
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        t = x * np.float32(w)
        assert t.dtype == np.float32
        return t / np.float32(N)


def fold(terms):
    """The in-order fp32 sum, the first term assigned (servers/fed_server.py:62-65)."""
    acc = None
    with np.errstate(all="ignore"):
        for t in terms:
            t = np.asarray(t, np.float32)
            acc = t if acc is None else acc + t
    return acc


def dequant_terms(q, zp, s, w, N):
    """fl(fl(fl(fl(q - zp) * s) * n) / N) written out in numpy fp32 (q, zp: integer
    valued; s per element or broadcastable)."""
    with np.errstate(all="ignore"):
        d = np.asarray(q, np.float32) - np.asarray(zp, np.float32)
        return ((d * np.asarray(s, np.float32)) * np.float32(w)) / np.float32(N)


def pad4(x, fill=1.0):
    """x padded to a multiple of 4 elements (the kernels' row granularity)."""
    x = np.asarray(x, np.float32)
    n = -len(x) % 4
    return np.concatenate([x, np.full(n, fill, np.float32)]) if n else x


def same_bits(a, b):
    """NaN positions equal, every other bit pattern equal (signed zeros differ)."""
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(
        a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


def first_mismatch(got, ref, x=None):
    """(index, got bits, ref bits[, dividend]) of the first differing element, for
    assertion messages; None when same_bits."""
    got = np.asarray(got, np.float32)
    ref = np.asarray(ref, np.float32)
    bad = (got.view(np.uint32) != ref.view(np.uint32)) & ~(np.isnan(got) & np.isnan(ref))
    if not bad.any():
        return None
    i = int(np.argmax(bad))
    r = (i, int(np.count_nonzero(bad)), hex(int(got.view(np.uint32)[i])),
         hex(int(ref.view(np.uint32)[i])))
    return r + (float(x[i]),) if x is not None else r
