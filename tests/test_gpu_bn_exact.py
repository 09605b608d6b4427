"""GPU: the fused eval batch-norm passes of csrc/infer.hip against tests/bn_ref.py, a
numpy reference with one rounding per fp32 step (itself checked against rational
arithmetic, tests/test_bn_ref_host.py), element by element.

The comparison rule everywhere: the same uint32 bits on every element, except where
the reference is NaN, where the kernel must give some NaN (bn_ref.mismatches).

* The act kernels (dls_bn_act_nhwc_f32, dls_bn_act_exact_nhwc_f32,
  dls_bn_act_exact_nchw_f32) get constants the test uploads, so they are pinned
  apart from the fold kernels: every launch form (the shape lists below;
  tests/test_bn_ref_host.py proves they reach each one), residual x ReLU, channel
  parameters that differ per channel (zero, negative, infinite, overflowing), data
  with +-0, denormals, FLT_MIN, FLT_MAX, inf, NaN, x == mean; in place, out =
  residual, out inside a canary buffer, a non-default stream, 4-byte aligned NCHW
  views, and the capped grid.
* The fold kernels: dls_bn_fold_f32 bit for bit; dls_bn_fold_exact_f32's copied
  planes bit for bit and its v_rsq_f32 within 1 ulp of 1 / sqrt in fp64.
* ReLU(-0): the kernels and torch.relu on the device agree (+0).
"""
import time
import zlib

import numpy as np
import pytest
import torch

from tests import bn_ref as R

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)

# (N, C, H, W).  NHWC: n4 = N*H*W*C/4 float4s, blocks = ceil(n4 / 1024), FIXED when
# (256 * blocks) % (C/4) == 0.
NHWC_SHAPES = [
    (1, 12, 25, 10),   # n4 = 750: one block, not FIXED, tail loop only
    (1, 12, 40, 25),   # n4 = 3000: three blocks, FIXED, unrolled and tail loop
    (2, 12, 35, 20),   # n4 = 4200: five blocks, not FIXED, unrolled and tail loop
    (3, 64, 7, 5),     # C4 = 16: FIXED, two blocks
    (1, 4, 1, 1),      # one float4, C4 = 1
    (5, 20, 3, 3),     # C4 = 5, not FIXED
]
# NCHW: HW % 4 != 0 runs the element kernel; else n4 = N*C*HW/4, POW2 when HW/4 and C
# both are powers of two.
NCHW_SHAPES = [
    (2, 8, 4, 4),      # POW2
    (3, 8, 2, 2),      # HW4 == 1, POW2
    (3, 12, 2, 2),     # HW4 == 1, C not a power of two
    (2, 12, 4, 4),     # HW4 a power of two, C not
    (2, 8, 4, 3),      # C a power of two, HW4 = 3 not
    (2, 5, 2, 6),      # neither; C not a multiple of 4
    (11, 16, 8, 8),    # POW2, n4 = 2816: unrolled and tail loop
    (5, 12, 10, 20),   # not POW2, n4 = 3000: unrolled and tail loop
    (3, 24, 7, 5),     # HW = 35: element kernel
    (2, 6, 3, 3),      # HW = 9: element kernel
]
FLAGS = [(False, False), (False, True), (True, False), (True, True)]  # residual, relu

FLT_MAX, FLT_MIN = 0x7F7FFFFF, 0x00800000
POOL = R.from_bits([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF,
                    FLT_MIN, FLT_MIN | 0x80000000, FLT_MAX, FLT_MAX | 0x80000000,
                    0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFA00000,
                    0x7E967699, 0xFE967699, 0x71000000, 0x0D000000])  # .. 1e38, 2^99, 2^-101
CANARY = 0x7FA5A5A5
PAD = 64  # floats: keeps the 16-byte alignment of what follows


def _values(n, rng, scale=3.0):
    v = (rng.standard_normal(n) * scale).astype(np.float32)
    k = np.flatnonzero(rng.random(n) < 0.25)
    v[k] = POOL[rng.integers(0, POOL.size, k.size)]
    return v


def _put(a, k, value):
    """Every 12th channel from k on gets `value`: whatever C is, the first channels
    carry the edge parameters."""
    a[k::12] = np.float32(value)


def exact_consts(C, rng):
    """[mean | iv | w | b], every channel different."""
    mean = (rng.standard_normal(C) * 0.5).astype(np.float32)
    iv = (rng.random(C) * 3 + 0.1).astype(np.float32)
    w = rng.standard_normal(C).astype(np.float32)
    b = (rng.standard_normal(C) * 0.3).astype(np.float32)
    _put(w, 0, 0.0), _put(w, 1, -0.0), _put(iv, 2, 0.0), _put(iv, 3, np.inf), _put(w, 4, -1.5)
    _put(mean, 5, 0.0), _put(b, 5, -0.0), _put(w, 5, 1.0)      # a pre-activation of -0
    _put(iv, 6, 1e12), _put(mean, 7, -0.0), _put(iv, 8, 1e-41)  # overflow; a denormal iv
    _put(b, 9, np.inf), _put(mean, 10, 3e38), _put(w, 11, np.nan)
    return np.concatenate([mean, iv, w, b])


def plain_consts(C, rng):
    alpha = (rng.standard_normal(C) * 2).astype(np.float32)
    beta = (rng.standard_normal(C) * 0.3).astype(np.float32)
    _put(alpha, 0, 0.0), _put(alpha, 1, -0.0), _put(beta, 1, -0.0), _put(alpha, 2, np.inf)
    _put(alpha, 3, -1.7), _put(alpha, 4, 1e30), _put(alpha, 5, 1e-41), _put(beta, 6, np.inf)
    _put(beta, 7, -1e38), _put(alpha, 8, 1.0), _put(beta, 8, -0.0), _put(alpha, 9, np.nan)
    return alpha, beta


class Entry:
    """One act entry point: how to call it and what it must compute."""

    def __init__(self, name, nhwc, exact):
        self.name, self.nhwc, self.exact = name, nhwc, exact

    def __repr__(self):
        return self.name

    def params(self, C, rng):
        return exact_consts(C, rng) if self.exact else plain_consts(C, rng)

    def upload(self, params):
        if self.exact:
            return (torch.from_numpy(params).to(dev),)
        return tuple(torch.from_numpy(p).to(dev) for p in params)

    def run(self, x, dparams, **kw):
        from distributed_learning_simulator_amd import _native
        fn = {"bn_act_nhwc": _native.bn_act_nhwc, "bn_act_exact_nhwc": _native.bn_act_exact_nhwc,
              "bn_act_exact_nchw": _native.bn_act_exact_nchw}[self.name]
        return fn(x, *dparams, **kw)

    def channels(self, lo, hi, C, HW):
        idx = np.arange(lo, hi, dtype=np.int64)
        return R.nhwc_channel(idx, C) if self.nhwc else R.nchw_channel(idx, C, HW)

    def ref(self, x, params, r, relu, ch):
        if self.exact:
            return R.act_exact(x, params, r, relu, ch=ch)
        return R.act(x, params[0], params[1], r, relu, ch=ch)

    # a flat array in memory order <-> the [N, C, H, W] tensor the wrappers take
    def tensor(self, flat, shape):
        N, C, H, W = shape
        if self.nhwc:
            return flat.view(N, H, W, C).permute(0, 3, 1, 2)
        return flat.view(N, C, H, W)

    def flat(self, t):
        return (t.permute(0, 2, 3, 1) if self.nhwc else t).reshape(-1)


ACT = Entry("bn_act_nhwc", True, False)
EXACT_NHWC = Entry("bn_act_exact_nhwc", True, True)
EXACT_NCHW = Entry("bn_act_exact_nchw", False, True)
ENTRIES = [ACT, EXACT_NHWC, EXACT_NCHW]
CASES = [(e, s) for e in ENTRIES for s in (NHWC_SHAPES if e.nhwc else NCHW_SHAPES)]


def _check(got, ref, what):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    bad = R.mismatches(got, ref)
    if bad.size:
        i = int(bad[0])
        g, w = R.bits(got.reshape(-1)[i:i + 1])[0], R.bits(np.asarray(ref).reshape(-1)[i:i + 1])[0]
        pytest.fail(f"{what}: {bad.size} of {ref.size} elements differ, the first at flat index "
                    f"{i}: got {g:#010x}, want {w:#010x}")


def _case(entry, shape, seed):
    """Host data of one case, in memory order, and the four references."""
    N, C, H, W = shape
    n = N * C * H * W
    rng = np.random.default_rng(seed)
    params = entry.params(C, rng)
    ch = entry.channels(0, n, C, H * W)
    x, r = _values(n, rng), _values(n, rng, 1.0)
    if entry.exact:  # the cancellation x == mean, exactly
        k = np.flatnonzero(rng.random(n) < 0.05)
        x[k] = params[:C][ch[k]]
    r[::17] = np.float32(-0.0)
    refs = {(res, relu): entry.ref(x, params, r if res else None, relu, ch) for res, relu in FLAGS}
    return params, x, r, refs


_cache = {}


def case(entry, shape):
    key = (entry.name, shape)
    if key not in _cache:
        _cache[key] = _case(entry, shape, zlib.crc32(repr(key).encode()))
    return _cache[key]


def dev_flat(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.parametrize("res,relu", FLAGS)
@pytest.mark.parametrize("entry,shape", CASES, ids=[f"{e}-{'x'.join(map(str, s))}" for e, s in CASES])
def test_act_kernels_match_reference(entry, shape, res, relu):
    """A fresh output and the in-place call, every launch form, bit for bit."""
    params, x, r, refs = case(entry, shape)
    dp = entry.upload(params)
    xt, rt = entry.tensor(dev_flat(x), shape), entry.tensor(dev_flat(r), shape) if res else None
    y = entry.run(xt, dp, residual=rt, relu=relu)
    assert y.data_ptr() != xt.data_ptr() and y.shape == xt.shape
    _check(entry.flat(y), refs[res, relu], f"{entry} {shape} res={res} relu={relu}")
    _check(entry.flat(xt), x, "the input of an out-of-place call")  # unchanged (NaN payloads aside)
    y2 = entry.run(xt, dp, residual=rt, relu=relu, inplace=True)
    assert y2.data_ptr() == xt.data_ptr()
    _check(entry.flat(y2), refs[res, relu], f"{entry} {shape} res={res} relu={relu} in place")


# both loops in one launch for the float4 kernels, and the element kernel
ALIAS_CASES = [(ACT, (1, 12, 40, 25)), (EXACT_NHWC, (2, 12, 35, 20)), (EXACT_NCHW, (5, 12, 10, 20)),
               (EXACT_NCHW, (3, 24, 7, 5))]


@pytest.mark.parametrize("entry,shape", ALIAS_CASES,
                         ids=[f"{e}-{'x'.join(map(str, s))}" for e, s in ALIAS_CASES])
def test_out_may_alias_and_writes_nothing_else(entry, shape):
    """out = x, out = residual (the kernel's comment allows both), and out a slice
    of a larger buffer whose neighbours keep their canary bits."""
    params, x, r, refs = case(entry, shape)
    dp = entry.upload(params)
    n = x.size
    for res, relu in FLAGS:
        what = f"{entry} {shape} res={res} relu={relu}"
        xt = entry.tensor(dev_flat(x), shape)
        rt = entry.tensor(dev_flat(r), shape) if res else None
        y = entry.run(xt, dp, residual=rt, relu=relu, out=xt)
        assert y is xt
        _check(entry.flat(y), refs[res, relu], what + " out = x")
        if res:
            xt = entry.tensor(dev_flat(x), shape)
            y = entry.run(xt, dp, residual=rt, relu=relu, out=rt)
            assert y is rt
            _check(entry.flat(y), refs[res, relu], what + " out = residual")
            _check(entry.flat(xt), x, what + " out = residual: x")
            rt = entry.tensor(dev_flat(r), shape)
        buf = torch.full((n + 2 * PAD,), CANARY, dtype=torch.int32, device=dev).view(torch.float32)
        out = entry.tensor(buf[PAD:PAD + n], shape)
        y = entry.run(entry.tensor(dev_flat(x), shape), dp, residual=rt, relu=relu, out=out)
        assert y is out
        _check(buf[PAD:PAD + n], refs[res, relu], what + " out in a canary buffer")
        edge = torch.cat([buf[:PAD], buf[PAD + n:]]).view(torch.int32)
        assert bool((edge == CANARY).all()), what + ": wrote outside out"


@pytest.mark.parametrize("entry,shape", ALIAS_CASES[:3], ids=[str(e) for e, _ in ALIAS_CASES[:3]])
def test_non_default_stream(entry, shape):
    params, x, r, refs = case(entry, shape)
    dp = entry.upload(params)
    xt, rt = entry.tensor(dev_flat(x), shape), entry.tensor(dev_flat(r), shape)
    out = torch.empty_like(xt)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=dev)
    y = entry.run(xt, dp, residual=rt, relu=True, out=out, stream=s)
    s.synchronize()
    _check(entry.flat(y), refs[True, True], f"{entry} on a side stream")


@pytest.mark.parametrize("shape", [(5, 12, 10, 20), (11, 16, 8, 8)], ids=["div", "pow2"])
@pytest.mark.parametrize("which", ["x", "residual", "out"])
def test_unaligned_nchw_view_runs_the_element_kernel(shape, which):
    """A contiguous [N, C, H, W] view one float into a buffer (4-byte aligned, HW % 4
    == 0) as x, as the residual, as out: the element kernel's bits are the float4
    kernel's and the reference's (a NaN for a NaN: which operand's payload a NaN
    result carries is the compiler's choice per kernel)."""
    entry = EXACT_NCHW
    params, x, r, refs = case(entry, shape)
    dp = entry.upload(params)
    n = x.size

    def off(a=None):
        buf = torch.full((n + 8,), CANARY, dtype=torch.int32, device=dev).view(torch.float32)
        v = buf[1:1 + n]
        if a is not None:
            v.copy_(torch.from_numpy(a))
        assert v.data_ptr() % 16 == 4
        return buf, entry.tensor(v, shape)

    xt = off(x)[1] if which == "x" else entry.tensor(dev_flat(x), shape)
    rt = off(r)[1] if which == "residual" else entry.tensor(dev_flat(r), shape)
    buf, out = off() if which == "out" else (None, torch.empty_like(xt))
    aligned = entry.run(entry.tensor(dev_flat(x), shape), dp, residual=entry.tensor(dev_flat(r), shape),
                        relu=True)
    y = entry.run(xt, dp, residual=rt, relu=True, out=out)
    _check(entry.flat(y), refs[True, True], f"unaligned {which}")
    _check(entry.flat(y), aligned.cpu().numpy(), f"unaligned {which} against the aligned run")
    if buf is not None:
        edge = torch.cat([buf[:1], buf[1 + n:]]).view(torch.int32)
        assert bool((edge == CANARY).all())


@pytest.mark.parametrize("entry", [ACT, EXACT_NHWC], ids=str)
@pytest.mark.parametrize("which", ["x", "residual", "out"])
def test_nhwc_entries_refuse_an_unaligned_view(entry, which):
    shape = (1, 12, 40, 25)
    n = 12 * 40 * 25
    dp = entry.upload(entry.params(12, np.random.default_rng(0)))
    good = lambda: entry.tensor(torch.zeros(n, device=dev), shape)  # noqa: E731
    odd = entry.tensor(torch.zeros(n + 8, device=dev)[1:1 + n], shape)
    kw = {"x": good(), "residual": good(), "out": good()}
    kw[which] = odd
    with pytest.raises(RuntimeError, match=r"status -2.*alignment"):  # DLS_ELAYOUT
        entry.run(kw["x"], dp, residual=kw["residual"], relu=True, out=kw["out"])


# --------------------------------------------------------------- the grid cap
SLAB = 4096  # floats on each side of a boundary


def _slabs(n, marks):
    """Merged [lo, hi) ranges: the first and last SLAB elements and SLAB on each side
    of every mark."""
    r = sorted((max(0, m - SLAB), min(n, m + SLAB)) for m in [0, n] + [m for m in marks if 0 < m < n])
    out = [list(r[0])]
    for lo, hi in r[1:]:
        if lo <= out[-1][1]:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    return out


def _device_values(n, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    v = torch.randn(n, device=dev, generator=g) * 3
    pool = torch.from_numpy(POOL).to(dev)
    for k in range(POOL.size):  # edge values at odd strides, in every slab
        v[k * 37 + 5::977] = pool[k]
    return v


def _capped(entry, shape, marks, seed):
    N, C, H, W = shape
    n = N * C * H * W
    params = entry.params(C, np.random.default_rng(seed))
    dp = entry.upload(params)
    xf, rf = _device_values(n, seed), _device_values(n, seed + 1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    y = entry.run(entry.tensor(xf, shape), dp, residual=entry.tensor(rf, shape), relu=True)
    yf = entry.flat(y)
    assert yf.data_ptr() == y.data_ptr()  # a view: memory order
    for lo, hi in _slabs(n, marks):
        ch = entry.channels(lo, hi, C, H * W)
        ref = entry.ref(xf[lo:hi].cpu().numpy(), params, rf[lo:hi].cpu().numpy(), True, ch)
        _check(yf[lo:hi], ref, f"{entry} capped grid, elements {lo}..{hi}")
    return time.perf_counter() - t0


def _round_marks(n):
    """Every multiple, below n floats, of grid_threads * kBnUnroll float4s, for each
    grid the cap can give: resident blocks per CU o = 1..8, grid = o * CUs * 4 blocks
    of 256 threads (the occupancy the runtime reports is not visible from here; with
    all eight, the marks of the true one are among them)."""
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    marks = set()
    for o in range(1, 9):
        step = o * cus * 4 * 256 * 4 * 4  # floats per unrolled round
        marks.update(range(step, n, step))
        marks.update(range(step // 4, n, step // 4))  # and per grid stride, where u changes
    return sorted(marks)


def _min_n4():
    return 8 * torch.cuda.get_device_properties(dev).multi_processor_count * 4 * 1024


@pytest.mark.parametrize("entry", ENTRIES, ids=str)
def test_capped_grid_walks_more_than_one_round(entry):
    """More float4s than the largest grid the cap allows covers in one unrolled round
    (at most 8 resident blocks of 256 threads per CU, x 4 generations, x 4 float4s per
    thread), plus a ragged remainder: threads come back for a second round.  Inputs
    are generated on the device; the reference is computed for the first and last
    4096 elements and 4096 on each side of every round and stride boundary.
    Measured on an MI355X (256 CUs, 33.6 M elements, 32 boundaries): 4.3 ms for
    dls_bn_act_nhwc_f32 and 7.2 ms for each exact entry from the launch to the last
    compared slab; the slowest whole case, inputs included, 0.13 s."""
    C = 12
    if entry.nhwc:
        rows = _min_n4() // (C // 4) + 1501
        shape = (1, C, rows, 1)
    else:
        shape = (_min_n4() // (C * 2) + 61, C, 2, 4)  # HW4 = 2, C = 12: the division path
    n = shape[0] * shape[1] * shape[2] * shape[3]
    assert n // 4 > _min_n4() and (n // 4) % 1024
    dt = _capped(entry, shape, _round_marks(n), 7)
    print(f"{entry}: capped grid, {n} elements, {dt * 1e3:.1f} ms")


def test_element_kernel_grid_clamp():
    """The NCHW element kernel above 65,536 blocks x 256 threads: a thread walks its
    grid-stride loop twice.  HW = 9.  Measured on an MI355X: 0.7 ms from the launch
    to the last compared slab (16.8 M elements), the whole case 0.01 s."""
    stride = 65536 * 256
    shape = (stride // (6 * 9) + 50, 6, 3, 3)
    n = shape[0] * 6 * 9
    assert stride < n < 2 * stride
    dt = _capped(EXACT_NCHW, shape, [stride], 9)
    print(f"element kernel: clamped grid, {n} elements, {dt * 1e3:.1f} ms")


# ------------------------------------------------------------------ the folds
class Stats:
    """What the fold wrappers read of a BatchNorm module."""

    def __init__(self, w, b, mean, var, eps):
        up = lambda a: None if a is None else torch.from_numpy(a).to(dev)  # noqa: E731
        self.weight, self.bias, self.running_mean, self.running_var = up(w), up(b), up(mean), up(var)
        self.eps, self.num_features = eps, mean.size


def _fold_inputs(C, eps, rng):
    """var such that fl(var + eps) is 0, denormal, 1e-38 (denormal), FLT_MIN, 1e38,
    FLT_MAX, inf, NaN, negative, and ordinary; w with 0, -0, negative, inf."""
    e = np.float32(eps)
    var = (rng.random(C) * 2 + 0.01).astype(np.float32)
    want = np.array([0.0, 1e-45, 1e-41, 1e-38, 1.17549435e-38, 1e38, 3.4028235e38, np.inf, np.nan,
                     -1.0, -4.0, -1e-41, 1e-30, 1e30], np.float32)
    with np.errstate(all="ignore"):
        v = (want - e).astype(np.float32)  # fl(v + eps) is want, or next to it
    var[:want.size] = v
    var[want.size] = -e  # fl(var + eps) == 0 exactly
    var[want.size + 1] = np.float32(-0.0)
    mean = (rng.standard_normal(C) * 0.5).astype(np.float32)
    mean[20:26] = R.from_bits([0, 0x80000000, 1, FLT_MAX, 0x7F800000, 0x7FC00000])
    w = (rng.random(C) + 0.5).astype(np.float32)
    w[26:32] = R.from_bits([0, 0x80000000, 0xBFC00000, 0x7F800000, FLT_MAX, 0x7FC00000])
    w[:8:2] = np.float32(-1.25)
    b = (rng.standard_normal(C) * 0.1).astype(np.float32)
    b[32:36] = R.from_bits([0x80000000, 0x7F800000, 1, 0xFFC00000])
    return w, b, mean, var


@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("eps", [0.0, 1e-5, 1e-3])
def test_bn_fold_matches_reference(eps, affine):
    from distributed_learning_simulator_amd import _native
    C = 301  # two blocks, ragged
    w, b, mean, var = _fold_inputs(C, eps, np.random.default_rng(5))
    if not affine:
        w = b = None
    alpha = torch.full((C + 2 * PAD,), CANARY, dtype=torch.int32, device=dev).view(torch.float32)
    beta = alpha.clone()
    _native.bn_fold(Stats(w, b, mean, var, eps), alpha[PAD:PAD + C], beta[PAD:PAD + C])
    ra, rb = R.fold(w, b, mean, var, eps)
    _check(alpha[PAD:PAD + C], ra, f"alpha eps={eps}")
    _check(beta[PAD:PAD + C], rb, f"beta eps={eps}")
    for t in (alpha, beta):
        edge = torch.cat([t[:PAD], t[PAD + C:]]).view(torch.int32)
        assert bool((edge == CANARY).all())


@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("eps", [0.0, 1e-5, 1e-3])
def test_bn_fold_exact_planes_and_iv(eps, affine):
    """mean, w (or 1) and b (or 0) are copies, bit for bit, NaN payloads included; iv =
    v_rsq_f32(|fl(var + eps)|): +inf at 0, +0 at inf, NaN at NaN, within 1 ulp of the
    fp64 value at a normal argument, +inf at a denormal one (see
    test_rsq_distance_from_fp64)."""
    from distributed_learning_simulator_amd import _native
    C = 301
    w, b, mean, var = _fold_inputs(C, eps, np.random.default_rng(6))
    if not affine:
        w = b = None
    buf = torch.full((4 * C + 2 * PAD,), CANARY, dtype=torch.int32, device=dev).view(torch.float32)
    _native.bn_fold_exact(Stats(w, b, mean, var, eps), buf[PAD:PAD + 4 * C])
    got = buf[PAD:PAD + 4 * C].cpu().numpy().reshape(4, C)
    edge = torch.cat([buf[:PAD], buf[PAD + 4 * C:]]).view(torch.int32)
    assert bool((edge == CANARY).all())
    mp, iv64, wp, bp = R.fold_exact_parts(w, b, mean, var, eps)
    for name, g, want in (("mean", got[0], mp), ("w", got[2], wp), ("b", got[3], bp)):
        assert np.array_equal(R.bits(g), R.bits(want)), name
    with np.errstate(all="ignore"):
        s = np.abs(var + np.float32(eps))
    _check_iv(got[1], iv64, s)


def _check_iv(iv, iv64, s):
    nan, zero, inf = np.isnan(s), s == 0, np.isinf(s)
    denormal = (s > 0) & (s < R.from_bits([FLT_MIN])[0])
    normal = ~(nan | zero | inf | denormal)
    assert nan.sum() == np.isnan(iv64).sum() and np.isnan(iv[nan]).all()
    assert np.array_equal(R.bits(iv[zero | denormal]), np.full((zero | denormal).sum(), 0x7F800000, np.uint32))
    assert np.array_equal(R.bits(iv[inf]), np.zeros(inf.sum(), np.uint32))
    d = R.ulps_from(iv[normal], iv64[normal])
    assert d.size and d.max() <= 1.0, (d.max(), s[normal][d.argmax()])
    return d


def test_rsq_distance_from_fp64():
    """v_rsq_f32 against 1 / sqrt(x) in fp64 (whose own error, 2^-52 relative, is
    2^-29 ulp of fp32): every binade of the normal range, 4,104 mantissas each (the
    binade's ends, its middle, 4,096 random ones), through dls_bn_fold_exact_f32.
    The bound asserted is 1 ulp, the figure of the vendor's ISA manual.
    Measured on an MI355X: 0.7934 ulp at most over these 1.04 M arguments (0.8636 over
    every mantissa of [1, 2), 0.8243 over [2, 4)); 89.1 % of the results are the
    correctly rounded value.
    A denormal argument is read as zero (the instruction does not handle denormal
    inputs, whatever the kernel's denormal mode: LLVM's AMDGPU backend scales the
    argument of its own rsq expansions for that reason): +inf, measured for every
    one of 4,100 denormal arguments, where 1 / sqrt is 9.2e18 .. 2.7e22.  A running
    variance + eps below FLT_MIN therefore gives iv = +inf, as it does in the GPU
    library's own kernel, which uses the same instruction."""
    from distributed_learning_simulator_amd import _native
    rng = np.random.default_rng(0)
    man = np.unique(np.concatenate([rng.integers(0, 1 << 23, 4096),
                                    [0, 1, 2, (1 << 23) - 1, (1 << 23) - 2, 1 << 22, (1 << 22) - 1,
                                     (1 << 22) + 1]])).astype(np.uint32)
    exps = np.arange(1, 255, dtype=np.uint32)
    var = R.from_bits((exps[:, None] << 23 | man[None, :]).reshape(-1))
    den = R.from_bits(np.unique(np.concatenate([rng.integers(1, 1 << 23, 4096), [1, 2, 3, (1 << 23) - 1],
                                                1 << np.arange(23)])).astype(np.uint32))
    var = np.concatenate([var, den])
    C = var.size
    consts = torch.empty(4 * C, device=dev)
    _native.bn_fold_exact(Stats(None, None, np.zeros(C, np.float32), var, 0.0), consts)
    iv = consts[C:2 * C].cpu().numpy()
    _, iv64, _, _ = R.fold_exact_parts(None, None, np.zeros(C, np.float32), var, 0.0)
    d = _check_iv(iv, iv64, var)
    print(f"v_rsq_f32: at most {d.max():.4f} ulp from fp64 over {d.size} normal arguments; "
          f"{den.size} denormal arguments give +inf")


# ------------------------------------------------------------------- ReLU(-0)
@pytest.mark.parametrize("shape", [(2, 8, 2, 2), (2, 8, 3, 1)], ids=["float4", "element"])
@pytest.mark.parametrize("fmt", ["nchw", "nhwc"])
def test_relu_of_negative_zero_is_torchs(fmt, shape):
    """A pre-activation of -0 (x = -0, mean = +0, w = 1, b = -0, and again with a -0
    residual): the three act kernels and torch.relu(bn(x) [+ r]) on the device give
    the same bits.  Measured on an MI355X: torch's relu gives +0 (0x00000000), so do
    the kernels (t > 0 ? t : 0), and bn_ref.RELU_KEEPS_NEG_ZERO is False."""
    from distributed_learning_simulator_amd import _native
    C = shape[1]
    mf = torch.channels_last if fmt == "nhwc" else torch.contiguous_format
    bn = torch.nn.BatchNorm2d(C).to(dev).eval()
    with torch.no_grad():
        bn.weight.fill_(1.0), bn.bias.fill_(-0.0), bn.running_mean.fill_(0.0), bn.running_var.fill_(1.0)
    x = torch.full(shape, -0.0, device=dev).contiguous(memory_format=mf)
    r = torch.full(shape, -0.0, device=dev).contiguous(memory_format=mf)
    consts = torch.empty(4 * C, device=dev)
    _native.bn_fold_exact(bn, consts)
    alpha, beta = torch.ones(C, device=dev), torch.full((C,), -0.0, device=dev)
    c = consts.cpu().numpy()
    for rr in (None, r):
        with torch.no_grad():
            pre = bn(x) if rr is None else bn(x) + rr
            want = torch.relu(pre)
        assert bool((pre.view(torch.int32) == -2 ** 31).all())  # the pre-activation is -0
        wb = want.view(torch.int32)
        assert bool((wb == wb.flatten()[0]).all())
        keeps = int(wb.flatten()[0]) != 0
        assert keeps == R.RELU_KEEPS_NEG_ZERO, hex(int(wb.flatten()[0]) & 0xFFFFFFFF)
        got = [_native.bn_act_exact(x, consts, residual=rr, relu=True)]
        if fmt == "nhwc":
            got.append(_native.bn_act_nhwc(x, alpha, beta, residual=rr, relu=True))
        for y in got:
            assert torch.equal(y.view(torch.int32), wb)
        rn = None if rr is None else np.full(x.numel(), -0.0, np.float32)
        ref = R.act_exact(np.full(x.numel(), -0.0, np.float32), c, rn, True,
                          ch=np.arange(x.numel()) % C)
        assert np.array_equal(R.bits(ref), np.full(x.numel(), int(wb.flatten()[0]) & 0xFFFFFFFF, np.uint32))
        nor = _native.bn_act_exact(x, consts, residual=rr, relu=False)  # without ReLU: -0 stays
        assert bool((nor.view(torch.int32) == -2 ** 31).all())
