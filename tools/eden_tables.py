"""The Lloyd-Max codebooks of N(0, 1) that dls_eden_compress_f32 and dls_eden_fedavg_f32 carry
(include/dls_hip.h: DLS_EDEN_CENT2 / _BOUND2 / _CENT4 / _BOUND4; _native.EDEN_CENTROIDS /
EDEN_BOUNDS).

For b bits the quantizer has 2^b levels, symmetric, so M = 2^(b-1) magnitudes on |N(0, 1)|:
centroids c[0] < .. < c[M-1], boundaries t[m] = (c[m] + c[m+1]) / 2, and every centroid the
conditional mean of |x| over its cell [t[m-1], t[m]) (t[-1] = 0, t[M-1] = inf):
    E[x | a <= x < b] = (phi(a) - phi(b)) / (Phi(b) - Phi(a)).
The Lloyd iteration alternates the two in fp64 (math.erf / math.exp) until nothing moves, and
the tables are printed rounded to fp32 as C hex floats.  This output is authoritative: the
header's and the binding's constants are pasted from it, and tests/test_eden_host.py checks the
fixed-point conditions on what is committed.

    python tools/eden_tables.py
"""
import math
import struct


def phi(x):
    return 0.0 if math.isinf(x) else math.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def Phi(x):
    return 1.0 if math.isinf(x) else 0.5 * (1.0 + math.erf(x / math.sqrt(2.0)))


def cell_mean(a, b):
    """E[x | a <= x < b] of the standard normal."""
    return (phi(a) - phi(b)) / (Phi(b) - Phi(a))


def lloyd_max(bits, sweeps=100000):
    """(centroids, boundaries) of the 2^(bits-1) magnitudes, fp64, at the fixed point."""
    M = 1 << (bits - 1)
    cent = [(m + 0.5) * 3.0 / M for m in range(M)]
    for _ in range(sweeps):
        bound = [0.5 * (cent[m] + cent[m + 1]) for m in range(M - 1)]
        edges = [0.0] + bound + [math.inf]
        new = [cell_mean(edges[m], edges[m + 1]) for m in range(M)]
        moved = max(abs(a - b) for a, b in zip(new, cent))
        cent = new
        if moved == 0.0:
            break
    return cent, [0.5 * (cent[m] + cent[m + 1]) for m in range(M - 1)]


def fl32(x):
    return struct.unpack("f", struct.pack("f", x))[0]


def c_hex(x):
    mantissa, exponent = fl32(x).hex().split("p")
    return f"{mantissa.rstrip('0')}p{exponent}f"


def main():
    for bits in (2, 4):
        cent, bound = lloyd_max(bits)
        print(f"#define DLS_EDEN_CENT{bits} {{{', '.join(c_hex(c) for c in cent)}}}")
        print(f"#define DLS_EDEN_BOUND{bits} {{{', '.join(c_hex(t) for t in bound)}}}")
    for name, k in (("EDEN_CENTROIDS", 0), ("EDEN_BOUNDS", 1)):
        rows = ", ".join(f"{bits}: {tuple(fl32(x) for x in lloyd_max(bits)[k])!r}" for bits in (2, 4))
        print(f"{name} = {{{rows}}}")


if __name__ == "__main__":
    main()
