"""Edge values of the quantizer chain (csrc/quant.hip: dls_segment_minmax_f32,
dls_qparams_minmax, dls_quantize_affine) through _native, against
tests/quantizer_ref.py.  Everything is equality of bits or integers (minima and
maxima by value: the sign of a zero is open); the one tolerance is the binomial
bound of the stochastic share."""
import math

import numpy as np
import pytest
import torch

from tests import quantizer_ref as R

pytestmark = pytest.mark.gpu

dev = torch.device("cuda")

CHUNK = 8192  # elements per block of the min / max kernel
INF = np.float32("inf")
NAN = np.float32("nan")
FMAX = np.float32(3.4028235e38)
DEN = np.float32(2.0 ** -149)  # the smallest denormal
RANGES = [(0, 255), (-128, 127), (0, 127), (0, 15), (0, 1)]


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def cycle_sizes(pattern, total):
    """Segment sizes cycling through ``pattern`` (the last one cut) up to ``total``."""
    sizes, left, i = [], total, 0
    while left > 0:
        sizes.append(min(pattern[i % len(pattern)], left))
        left -= sizes[-1]
        i += 1
    return sizes


# --------------------------------------------------------------------- min / max
def gpu_minmax(xd, off, shift):
    """Minima / maxima of the device values ``xd`` read through a view that starts
    ``shift`` floats into its buffer (shift % 4 != 0: the scalar-load branch)."""
    from distributed_learning_simulator_amd import _native
    total = xd.numel()
    buf = torch.full((total + shift,), 1e30, device=dev)
    view = buf[shift:]
    view.copy_(xd)
    assert view.data_ptr() % 16 == 4 * (shift % 4)
    nseg = len(off) - 1
    mins = torch.full((nseg,), 777.0, device=dev)
    maxs = torch.full((nseg,), 777.0, device=dev)
    _native.segment_minmax(view, torch.from_numpy(off).to(dev), total, mins, maxs)
    return mins.cpu().numpy(), maxs.cpu().numpy()


MINMAX_LAYOUTS = {
    "one_1": [1], "one_3": [3], "one_4": [4], "one_5": [5], "one_8191": [8191],
    "one_8192": [8192], "one_8193": [8193], "one_3chunks": [3 * CHUNK],
    "many_1_to_7": list(range(1, 8)) * 40,
    "many_1_to_7_across_a_border": [CHUNK - 12] + list(range(1, 8)) * 3,
    "boundary_at_8192": [CHUNK, 5000],
    "empty_segments": [0, 5, 0, 0, 8300, 0],
    "middle_chunk_interior": [100, 3 * CHUNK - 200, 100],
}


def _uniform(a, b):
    return lambda r, n: r.uniform(a, b, n).astype(np.float32)


# name -> (background, the value placed as the minimum, as the maximum)
MINMAX_CLASSES = {
    "negative": (_uniform(-2, -1), -3.0, -0.5),
    "positive": (_uniform(1, 2), 0.5, 3.0),
    "mixed": (_uniform(-1, 1), -3.0, 3.0),
    "negzero_among_negatives": (_uniform(-2, -1), -3.0, -0.0),
    "zeros_of_both_signs": (lambda r, n: np.where(r.random(n) < 0.5, -0.0, 0.0).astype(np.float32),
                            -0.0, 0.0),
    "all_negzero": (lambda r, n: np.full(n, -0.0, np.float32), -0.0, -0.0),
    "infinities": (_uniform(-1, 1), -INF, INF),
    "all_posinf": (lambda r, n: np.full(n, INF, np.float32), INF, INF),
    "all_neginf": (lambda r, n: np.full(n, -INF, np.float32), -INF, -INF),
    "flt_max": (_uniform(-1, 1), -FMAX, FMAX),
    "denormals": (lambda r, n: np.zeros(n, np.float32), -DEN, DEN),
    "nan_neighbours": (_uniform(-1, 1), -3.0, 3.0),
    "all_nan": (lambda r, n: np.full(n, NAN, np.float32), NAN, NAN),
}
PLACEMENTS = ["first", "last", "middle", "border_left", "border_right"]


def extreme_positions(off, placement):
    """Per non-empty segment the element that holds its minimum and its maximum.
    border_*: the two elements on either side of a chunk border inside the segment
    (a segment without one takes the middle pair, in the same order)."""
    out = []
    for a, b in zip(off[:-1].tolist(), off[1:].tolist()):
        n = b - a
        if n == 0:
            continue
        g = next((g for g in range(CHUNK, int(off[-1]), CHUNK) if a < g < b), None)
        if placement.startswith("border") and g is None:
            lo, hi = a + n // 2, a + (n // 2 + 1) % n
        elif placement.startswith("border"):
            lo, hi = g - 1, g
        elif placement == "first":
            lo, hi = a, b - 1
        elif placement == "last":
            lo, hi = b - 1, a
        else:
            lo, hi = a + (n // 2 + 1) % n, a + n // 2
        if placement == "border_right":
            lo, hi = hi, lo
        out.append((a, b, lo, hi))
    return out


def minmax_input(off, cls, placement, seed):
    bg, vmin, vmax = MINMAX_CLASSES[cls]
    x = bg(np.random.default_rng(seed), int(off[-1]))
    for a, b, lo, hi in extreme_positions(off, placement):
        x[hi] = vmax
        x[lo] = vmin  # a one-element segment holds the minimum
        if cls == "nan_neighbours":
            for p in (lo - 1, lo + 1, hi - 1, hi + 1):
                if a <= p < b and p not in (lo, hi):
                    x[p] = NAN
    return x


@pytest.mark.parametrize("layout", list(MINMAX_LAYOUTS))
def test_segment_minmax_edge_values(layout):
    """Every value class x placement of the extremes x base-pointer shift on one
    segment layout.  A chunk inside one segment takes the bulk path, a chunk that
    touches a boundary the per-element atomics."""
    off = offsets(MINMAX_LAYOUTS[layout])
    assert off[-1] <= 3 * CHUNK
    for ci, cls in enumerate(MINMAX_CLASSES):
        for pi, placement in enumerate(PLACEMENTS):
            x = minmax_input(off, cls, placement, 100 * ci + pi)
            want_lo, want_hi = R.segment_minmax(x, off)
            xd = torch.from_numpy(x).to(dev)
            for shift in range(4):
                lo, hi = gpu_minmax(xd, off, shift)
                assert np.array_equal(lo, want_lo), (cls, placement, shift, "min")
                assert np.array_equal(hi, want_hi), (cls, placement, shift, "max")


def test_segment_minmax_negzero_arrives_after_the_minimum():
    """Cases whose outcome does not hang on the arrival order.  On the per-element
    path a thread takes the elements e, e + 256, e + 512 of its chunk in this order,
    so the -0.0 at +256 and +512 reach the atomics after the segment's minimum, and
    nothing negative follows.  On the bulk path a chunk whose only non-negative
    elements are -0.0 has the partial maximum -0.0, every other chunk a negative one."""
    sizes = [700, 900, 3 * CHUNK - 1600]
    off = offsets(sizes)
    x = np.random.default_rng(1).uniform(0.5, 1.0, int(off[-1])).astype(np.float32)
    for a in off[:2]:
        x[a] = -3.0
        x[a + 256] = x[a + 512] = -0.0
    a = int(off[2])  # the rest of chunk 0 (per-element path) and chunks 1, 2 (bulk path)
    x[a:] = -np.abs(x[a:])
    x[CHUNK + 5] = -7.0  # the minimum
    x[2 * CHUNK - 1] = -0.0  # the only non-negative elements of the segment
    x[2 * CHUNK + 256] = -0.0
    want_lo, want_hi = R.segment_minmax(x, off)
    assert want_lo.tolist() == [-3.0, -3.0, -7.0] and want_hi[2] == 0.0
    xd = torch.from_numpy(x).to(dev)
    for shift in range(4):
        lo, hi = gpu_minmax(xd, off, shift)
        assert np.array_equal(lo, want_lo) and np.array_equal(hi, want_hi), (shift, lo, hi)
    # a segment of three chunks, all negative but one -0.0 in the bulk chunk
    off1 = offsets([3 * CHUNK])
    y = -np.random.default_rng(2).uniform(0.5, 1.0, 3 * CHUNK).astype(np.float32)
    y[CHUNK + 4097] = -0.0
    lo, hi = gpu_minmax(torch.from_numpy(y).to(dev), off1, 0)
    assert lo[0] == y.min() and hi[0] == 0.0, (lo, hi)
    # ... and a chunk of -0.0 and positives only, next to a chunk that holds the minimum
    y = np.random.default_rng(3).uniform(0.5, 1.0, 2 * CHUNK).astype(np.float32)
    y[17] = -5.0
    y[CHUNK + 300::7] = -0.0
    lo, hi = gpu_minmax(torch.from_numpy(y).to(dev), offsets([2 * CHUNK]), 0)
    assert lo[0] == -5.0 and hi[0] == y.max(), (lo, hi)


def test_segment_minmax_repeats():
    """The atomics' arrival order varies from launch to launch; the result does not."""
    off = offsets([0] + list(range(1, 8)) * 30 + [CHUNK + 77, 0, 900, 3])
    rng = np.random.default_rng(8)
    x = rng.standard_normal(int(off[-1])).astype(np.float32)
    x[rng.random(x.size) < 0.2] = -0.0
    x[rng.random(x.size) < 0.1] = 0.0
    x[rng.random(x.size) < 0.05] = NAN
    want = R.segment_minmax(x, off)
    xd = torch.from_numpy(x).to(dev)
    for rep in range(8):
        lo, hi = gpu_minmax(xd, off, rep % 4)
        assert np.array_equal(lo, want[0]) and np.array_equal(hi, want[1]), rep


# ----------------------------------------------------------------------- qparams
def qparams_table():
    t = [(1.0, 5.0), (-5.0, -1.0), (0.25, 0.25), (-0.25, -0.25),  # clamped to include 0
         (0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0), (INF, -INF),
         (0.0, DEN), (-DEN, DEN), (-DEN, 0.0), (-8 * DEN, 100 * DEN),  # scale becomes eps
         (-FMAX, FMAX), (-FMAX, 1.0), (-1.0, FMAX),  # hi - lo overflows
         (-INF, 1.0), (-INF, -1.0), (-1.0, INF), (1.0, INF), (-INF, INF), (-FMAX, 0.0),
         (-1.0, 1.0), (-0.1, 0.3), (-1e-3, 7.0), (-7.0, 1e-3), (-1e30, 1e-30), (-3.0, 1e20)]
    for span in (255, 127, 15, 1):  # lo / scale an exact .5 tie at scale 1 (and 2^-5)
        for k in range(4):
            t.append((-(k + 0.5), span - (k + 0.5)))
            t.append((-(k + 0.5) / 32, (span - (k + 0.5)) / 32))
        t.append((-(span + 0.5), 0.0))  # the zero point pushed to qmax and one beyond
        t.append((-float(span), 1e-3))
    rng = np.random.default_rng(4)
    for _ in range(40):
        a, b = np.sort(rng.standard_normal(2) * 10.0 ** rng.integers(-6, 6))
        t.append((a, b))
    lo, hi = np.array(t, dtype=np.float32).T
    return np.ascontiguousarray(lo), np.ascontiguousarray(hi)


@pytest.mark.parametrize("symmetric", [False, True], ids=["affine", "symmetric"])
@pytest.mark.parametrize("qmin,qmax", RANGES)
def test_qparams_table(qmin, qmax, symmetric):
    """No pair of the table is left out: with fminf / fmaxf every pair, the
    non-finite ones included, has a defined scale and zero point (dls_hip.h)."""
    from distributed_learning_simulator_amd import _native
    lo, hi = qparams_table()
    want_sc, want_zp = R.qparams(lo, hi, qmin, qmax, symmetric)
    if not symmetric:  # the table does hold ties and reaches both clamps
        sc = want_sc
        with np.errstate(all="ignore"):
            frac = np.abs(np.fmin(lo, 0) / sc) % 1
        assert np.any((frac == 0.5) & np.isfinite(sc))
        assert np.any(want_zp == qmin) and np.any(want_zp == qmax)
        assert np.any(sc == R.EPS) and np.any(np.isposinf(sc))
    scale = torch.full((lo.size,), 777.0, device=dev)
    zp = torch.full((lo.size,), 777, dtype=torch.int32, device=dev)
    _native.qparams_minmax(torch.from_numpy(lo).to(dev), torch.from_numpy(hi).to(dev), scale, zp,
                           qmin, qmax, symmetric)
    got_sc, got_zp = scale.cpu().numpy(), zp.cpu().numpy()
    bad = np.flatnonzero((bits(got_sc) != bits(want_sc)) | (got_zp != want_zp))
    assert bad.size == 0, [(lo[i], hi[i], got_sc[i], want_sc[i], got_zp[i], want_zp[i]) for i in bad]


# ---------------------------------------------------------------------- quantize
Q_CANARY = 0xA5
DEQ_CANARY = 1234.5


def gpu_quantize(x, off, scale, zp, qmin, qmax, qshift=0, stochastic=False, seed=0):
    """(q bytes, deq) with q a view starting ``qshift`` bytes into its buffer; asserts
    that nothing outside [0, total) of either output was written."""
    from distributed_learning_simulator_amd import _native
    total = x.size
    qbuf = torch.full((total + 24,), Q_CANARY, dtype=torch.uint8, device=dev)
    dbuf = torch.full((total + 16,), DEQ_CANARY, device=dev)
    q = qbuf[8 + qshift:8 + qshift + total]
    deq = dbuf[8:8 + total]
    assert q.data_ptr() % 4 == qshift % 4
    if qmin < 0:
        q = q.view(torch.int8)
    _native.quantize(torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev),
                     torch.from_numpy(off).to(dev), total,
                     torch.from_numpy(np.asarray(scale, np.float32)).to(dev),
                     torch.from_numpy(np.asarray(zp, np.int32)).to(dev), q, deq, qmin, qmax,
                     stochastic=stochastic, seed=seed)
    qh, dh = qbuf.cpu().numpy(), dbuf.cpu().numpy()
    assert np.all(qh[:8 + qshift] == Q_CANARY) and np.all(qh[8 + qshift + total:] == Q_CANARY)
    assert np.all(dh[:8] == np.float32(DEQ_CANARY)) and np.all(dh[8 + total:] == np.float32(DEQ_CANARY))
    return q.cpu().numpy(), dh[8:8 + total]


def check_quantize(x, off, scale, zp, qmin, qmax, qshift=0, tag=None):
    want_q, want_deq = R.quantize(x, off, scale, zp, qmin, qmax)
    q, deq = gpu_quantize(x, off, scale, zp, qmin, qmax, qshift)
    bad = np.flatnonzero(q != R.as_bytes(want_q, qmin))
    assert bad.size == 0, (tag, qshift, [(i, x[i], q[i], want_q[i]) for i in bad[:8]])
    nan = np.isnan(want_deq)  # only from a non-finite scale (not used here)
    assert not nan.any()
    bad = np.flatnonzero(bits(deq) != bits(want_deq))
    assert bad.size == 0, (tag, qshift, [(i, x[i], deq[i], want_deq[i]) for i in bad[:8]])


QUANT_LAYOUTS = {
    "total_1": [1], "total_3": cycle_sizes([1, 2, 3, 5], 3),
    "total_1023": cycle_sizes([1, 2, 3, 5], 1023), "total_1025": cycle_sizes([1, 2, 3, 5], 1025),
    "total_4099": cycle_sizes([1, 2, 3, 5], 4099),
    "empty_segments": [0, 0, 1, 2, 0, 3, 5, 0, 0, 1, 1, 1, 1, 2, 0] * 30 + [0, 0],
    "segment_at_1024": [1000, 24, 50], "segment_at_1025": [1000, 25, 50],
    "segment_at_1024_after_empty": [1024, 0, 0, 3, 1021, 1, 0],
}


@pytest.mark.parametrize("qmin,qmax", [(0, 255), (-128, 127)])
@pytest.mark.parametrize("layout", list(QUANT_LAYOUTS))
def test_quantize_segment_layouts(layout, qmin, qmax):
    """One thread's four elements over up to four segments, empty segments, segment
    starts at and next to a block's first element, totals around the block size,
    q at every byte alignment; per-segment scales and non-zero zero points."""
    off = offsets(QUANT_LAYOUTS[layout])
    nseg = len(off) - 1
    rng = np.random.default_rng(nseg + qmax)
    scale = (rng.uniform(0.01, 2.0, nseg) * 10.0 ** rng.integers(-3, 3, nseg)).astype(np.float32)
    zp = rng.integers(qmin, qmax + 1, nseg).astype(np.int32)
    seg = R.segment_of(off, int(off[-1]))
    v = rng.uniform(qmin - 4, qmax + 4, seg.size) - zp[seg]
    ties = rng.random(seg.size) < 0.3
    v[ties] = np.rint(v[ties]) + 0.5
    x = (v * scale[seg]).astype(np.float32)
    for qshift in range(4):
        check_quantize(x, off, scale, zp, qmin, qmax, qshift, layout)


def edge_values(scale, zp, qmin, qmax):
    """x of one segment: ties, both clamps' neighbourhoods and the special values."""
    s = np.float32(scale)
    v = [0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 3.5, -3.5, 0.25, -0.75]
    for c in (qmin - zp, qmax - zp):
        for d in (-1.5, -1.0, -0.5, 0.0, 0.5, 1.0, 1.5):
            w = np.float32(c + d)
            v += [w, np.nextafter(w, -INF), np.nextafter(w, INF)]
    x = (np.array(v, np.float32) * s).astype(np.float32)
    special = np.array([-0.0, 0.0, NAN, INF, -INF, FMAX, -FMAX, DEN, -DEN, 3 * DEN, -5 * DEN,
                        2.0 ** -127, -(2.0 ** -126)], np.float32)
    return np.concatenate([x, special])


QUANT_RANGES = {
    (0, 255): [0, 10, 128, 255], (-128, 127): [0, -128, 127, 5], (0, 15): [0, 3, 15],
    (0, 127): [0, 64, 127],
}


@pytest.mark.parametrize("qmin,qmax", list(QUANT_RANGES))
def test_quantize_edge_values(qmin, qmax):
    """Ties round to even, the clamps hold on both sides, NaN -> qmin, +-inf and
    +-FLT_MAX -> the clamps, -0.0 like +0.0, denormal x and a denormal scale (for
    which x * fl(1 / scale) is a small integer only if denormals are kept)."""
    scales = [0.0625, 1.0, 3.0, 0.1, 2.0 ** -23, 2.0 ** -127, 1e30]
    xs, sc, zps = [], [], []
    for zp in QUANT_RANGES[(qmin, qmax)]:
        for s in scales:
            xs.append(edge_values(s, zp, qmin, qmax))
            sc.append(s)
            zps.append(zp)
    off = offsets([len(a) for a in xs])
    x = np.concatenate(xs)
    want_q, _ = R.quantize(x, off, sc, zps, qmin, qmax)
    seg = R.segment_of(off, x.size)
    for i, (s, zp) in enumerate(zip(sc, zps)):  # what the header states, on the reference
        mine, xi = want_q[seg == i], x[seg == i]
        assert np.all(mine[np.isnan(xi)] == qmin) and np.all(mine[xi == INF] == qmax)
        assert np.all(mine[xi == -INF] == qmin) and np.all(mine[xi == 0] == zp)
        if s == np.float32(2.0 ** -127):
            assert np.any((mine != zp) & (np.abs(xi) < 2.0 ** -126))  # denormals count
    assert set(np.unique(want_q)) >= {qmin, qmin + 1, qmax - 1, qmax}
    for qshift in (0, 1):
        check_quantize(x, off, sc, zps, qmin, qmax, qshift)


def test_quantize_multiplies_by_the_reciprocal():
    """scale = 3: x * fl(1/3) and x / 3 round to different integers for some x next
    to the ties; the kernel must follow the reciprocal (torch's quantize_val)."""
    base = (np.arange(0, 120, dtype=np.float32) + np.float32(0.5)) * np.float32(3)
    x = base.copy()
    for _ in range(4):
        x = np.concatenate([np.nextafter(x, -INF), x, np.nextafter(x, INF)])
    x = np.unique(x)
    off = offsets([x.size])
    want_q, _ = R.quantize(x, off, [3.0], [0], 0, 255)
    by_division = np.clip(np.rint(x / np.float32(3)), 0, 255).astype(np.int32)
    assert np.any(want_q != by_division)  # the case is not vacuous
    check_quantize(x, off, [3.0], [0], 0, 255)
    xs = np.concatenate([-x[::-1], x])
    check_quantize(xs, offsets([xs.size]), [3.0], [5], -128, 127)


# -------------------------------------------------------------------- stochastic
@pytest.mark.parametrize("qmin,qmax,zp0", [(0, 255, 7), (-128, 127, 5), (0, 15, 3)])
def test_stochastic_bracket_and_seeds(qmin, qmax, zp0):
    off = offsets([0, 3, 1, 1021, 0, 2, 5, 4099 - 1032])
    nseg = len(off) - 1
    rng = np.random.default_rng(qmax)
    scale = rng.uniform(0.05, 1.0, nseg).astype(np.float32)
    zp = np.clip(zp0 + rng.integers(-3, 4, nseg), qmin, qmax).astype(np.int32)
    seg = R.segment_of(off, int(off[-1]))
    x = ((rng.uniform(qmin - 3, qmax + 3, seg.size) - zp[seg]) * scale[seg]).astype(np.float32)
    x[:8] = [NAN, INF, -INF, -0.0, FMAX, -FMAX, DEN, 0.0]
    lo, hi = R.stochastic_bracket(x, off, scale, zp, qmin, qmax)
    lo, hi = R.as_bytes(lo, qmin), R.as_bytes(hi, qmin)
    q1, _ = gpu_quantize(x, off, scale, zp, qmin, qmax, 1, stochastic=True, seed=42)
    assert np.all((q1 == lo) | (q1 == hi)), np.flatnonzero((q1 != lo) & (q1 != hi))[:8]
    assert np.any(q1 == lo) and np.any((q1 == hi) & (hi != lo))
    q2, _ = gpu_quantize(x, off, scale, zp, qmin, qmax, 0, stochastic=True, seed=42)
    assert np.array_equal(q1, q2)  # the same seed, whatever the alignment of q
    q3, deq3 = gpu_quantize(x, off, scale, zp, qmin, qmax, 0, stochastic=True, seed=43)
    assert np.all((q3 == lo) | (q3 == hi)) and not np.array_equal(q1, q3)
    z = zp[seg].astype(np.float32)
    want_deq = (q3.astype(np.float32) - z) * scale[seg]
    assert np.array_equal(bits(deq3), bits(want_deq))


def test_stochastic_independent_of_segmentation():
    """The uniform of an element is a function of (seed, element index): the same
    scale and zero point everywhere give the same bytes however the elements are cut."""
    total = 4099
    rng = np.random.default_rng(6)
    x = rng.uniform(-5, 20, total).astype(np.float32)
    cuts = [offsets([total]), offsets(cycle_sizes([1, 2, 3, 5], total)),
            offsets([0, 1024, 0, 1, 3074, 0])]
    got = []
    for off in cuts:
        nseg = len(off) - 1
        q, _ = gpu_quantize(x, off, np.full(nseg, 0.25, np.float32), np.full(nseg, 9, np.int32), 0, 255,
                            stochastic=True, seed=2024)
        got.append(q)
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])


def test_stochastic_share_rounded_up():
    """v = k + 0.25 exactly: each element rounds up with probability 1/4.  Over
    n = 65,536 independent elements the share is within 6 standard deviations,
    6 * sqrt(0.25 * 0.75 / n) ~ 0.0102, of 0.25."""
    n = 65536
    k = (np.arange(n) % 201).astype(np.float32)
    x = (k + np.float32(0.25)) * np.float32(0.5)
    off = offsets([n])
    q, _ = gpu_quantize(x, off, [0.5], [0], 0, 255, stochastic=True, seed=7)
    up = q.astype(np.int64) - k.astype(np.int64)
    assert set(np.unique(up)) <= {0, 1}
    share = float(up.mean())
    print("share rounded up:", share)
    assert abs(share - 0.25) <= 6 * math.sqrt(0.25 * 0.75 / n), share


# ------------------------------------------------------------ through the callers
def worker_weights(shape):
    """Channel 0 all zeros; 1: small positives, the most negative value in the
    middle and a -0.0 after it, last (and one before it, first: a short row is one
    wave's single atomic instruction, whose lanes arrive in no stated order); 2:
    the same with negatives only; 3: one huge outlier; the rest random."""
    rng = np.random.default_rng(shape[0])
    w = rng.standard_normal(shape).astype(np.float32)
    r = w.reshape(shape[0], -1)
    mid = r.shape[1] // 2
    r[0] = 0.0
    r[1] = np.abs(r[1]) * 0.1
    r[1, mid] = -3.0
    r[1, 0] = r[1, -1] = -0.0
    r[2] = -np.abs(r[2]) - 0.5
    r[2, mid] = -5.0
    r[2, 0] = r[2, -1] = -0.0
    r[3, mid] = 1e30
    return torch.from_numpy(w)


@pytest.mark.parametrize("shape", [(8, 3, 3, 3), (4, 16)], ids=["conv_8x3x3x3", "linear_4x16"])
def test_worker_per_channel_symmetric_edge_channels(shape):
    from torch.ao.quantization.observer import PerChannelMinMaxObserver
    from distributed_learning_simulator_amd.workers.fed_quant_worker import \
        quantize_per_channel_symmetric
    w = worker_weights(shape)
    obs = PerChannelMinMaxObserver(ch_axis=0, dtype=torch.qint8, qscheme=torch.per_channel_symmetric)
    obs(w)
    sc_ref, zp_ref = obs.calculate_qparams()
    assert float(sc_ref[0]) == float(R.EPS) and float(sc_ref[1]) == float(np.float32(3.0) / np.float32(127.5))
    q, sc, zp = quantize_per_channel_symmetric(w.to(dev))
    assert np.array_equal(bits(sc.cpu().numpy()), bits(sc_ref.float().numpy()))
    assert np.array_equal(zp.cpu().numpy(), zp_ref.numpy().astype(np.int32))
    qt = torch.quantize_per_channel(w, sc_ref.double(), zp_ref, 0, torch.qint8)
    assert np.array_equal(q.cpu().numpy(), qt.int_repr().numpy())
    C = shape[0]
    want_q, _ = R.quantize(w.numpy(), np.arange(C + 1) * (w.numel() // C), sc_ref.float().numpy(),
                           np.zeros(C, np.int32), -128, 127)
    assert np.array_equal(q.cpu().numpy().reshape(-1), R.as_bytes(want_q, -128))


def server_aggregate():
    """Three small tensors (one shorter than the 64-element row padding), each with
    a -0.0 after its minimum.  "fc" holds the model's minimum -3.5 at its first
    element, a -0.0 256 elements later in the flat row (the same thread's next
    element), only positives after that, and the maximum 11.5: at 16 levels the scale
    is 1 and rne(11.5) - rne(-3.5) = 16, one beyond qmax."""
    rng = np.random.default_rng(12)
    conv = -rng.uniform(0.5, 3.0, (5, 27)).astype(np.float32)
    conv[0, 0] = -3.25
    conv[-1, -1] = -0.0
    bias = -rng.uniform(0.5, 3.0, 37).astype(np.float32)
    bias[0] = -3.0
    bias[-1] = -0.0
    fc = rng.uniform(0.0, 11.0, (3, 100)).astype(np.float32)
    fc.reshape(-1)[:256] = rng.uniform(-3.4, 11.0, 256)
    fc[0, 0] = -3.5
    fc[0, 7] = 11.5
    fc.reshape(-1)[256] = -0.0
    fc[-1, -1] = -0.0
    return {"conv.weight": conv, "conv.bias": bias, "fc.weight": fc}


@pytest.mark.parametrize("level", [256, 16])
@pytest.mark.parametrize("granularity", ["model", "tensor"])
def test_fed_quant_server_requantizes_edge_aggregate(granularity, level):
    from distributed_learning_simulator_amd.servers.fed_quant_server import FedQuantServer
    agg = server_aggregate()
    names = list(agg)
    payload = {
        "conv.weight": (torch.zeros((5, 27), dtype=torch.int8), torch.ones(5, dtype=torch.float64),
                        torch.zeros(5, dtype=torch.int64)),
        "conv.bias": torch.zeros(37),
        "fc.weight": (torch.zeros((3, 100), dtype=torch.int8), torch.ones(3, dtype=torch.float64),
                      torch.zeros(3, dtype=torch.int64)),
    }
    server = FedQuantServer(tester=None, worker_number=1, synchronous=True, granularity=granularity,
                            quantization_level=level)
    server.parameters.store = server._make_store(payload)
    layout = server.parameters.store.layout
    assert layout.P == 192 + 64 + 320
    flat = torch.zeros(layout.P, device=dev)  # the store's flat row: zero padding
    views = layout.views(flat)
    for n in names:
        views[n].copy_(torch.from_numpy(agg[n]))
    out = server._process_aggregated_parameter(views)
    q, sc, zp = server.quantized_parameter
    q, sc, zp = q.cpu().numpy(), sc.cpu().numpy(), zp.cpu().numpy()
    qmax = level - 1
    parts = [agg[n].reshape(-1) for n in names]
    if granularity == "tensor":
        off = offsets([p.size for p in parts])
        lo, hi = R.segment_minmax(np.concatenate(parts), off)
        want_sc, want_zp = R.qparams(lo, hi, 0, qmax)
        want_q, want_deq = R.quantize(np.concatenate(parts), off, want_sc, want_zp, 0, qmax)
        got_q = np.concatenate([q[o:o + m] for o, m in zip(layout.offsets, layout.numels)])
    else:
        cat = np.concatenate(parts)
        lo, hi = R.segment_minmax(cat, [0, cat.size])
        want_sc, want_zp = R.qparams(lo, hi, 0, qmax)
        want_q, want_deq = R.quantize(cat, [0, cat.size], want_sc, want_zp, 0, qmax)
        got_q = q
    assert want_q.max() <= qmax
    if level == 16:
        assert float(want_sc[-1]) == 1.0 and int(want_zp[-1]) == 4  # the tie of the docstring
    assert np.array_equal(bits(sc), bits(want_sc)) and np.array_equal(zp, want_zp)
    assert np.array_equal(got_q, R.as_bytes(want_q, 0))
    got_deq = np.concatenate([out[n].reshape(-1).cpu().numpy() for n in names])
    assert np.array_equal(bits(got_deq), bits(want_deq))
    assert [tuple(out[n].shape) for n in names] == [agg[n].shape for n in names]
