"""CPU reference of the fused eval batch-norm passes (csrc/infer.hip; include/dls_hip.h,
dls_bn_fold_f32 .. dls_bn_act_exact_nchw_f32) — TEST INFRASTRUCTURE ONLY (the package
has no CPU path).

numpy on float32 arrays, no torch in the arithmetic: every fp32 operation is one numpy
float32 operation (IEEE: one rounding, denormals kept, inf and NaN propagated), so every
step is rounded on its own.  The fused multiply-add of the exact pass is
tests/attack_ref.py's fmaf (fp64 TwoSum, rounded to odd, then to fp32: one rounding).
tests/test_bn_ref_host.py checks these functions against exact rational arithmetic.

    fold        alpha = fl(fl(1 / fl(sqrt(fl(var + eps)))) * w),  beta = fl(b - fl(mean * alpha))
    act         y = relu(fl(fl(x * alpha) + beta) [+ r])
    act_exact   y = relu(fma(w, fl(fl(x - mean) * iv), b) [+ r]),  consts = [mean | iv | w | b]

ReLU keeps NaN, and sends a pre-activation of -0 to +0 or keeps it, by
RELU_KEEPS_NEG_ZERO: what torch.relu does on the device the module's forward runs on
(tests/test_gpu_bn_exact.py::test_relu_of_negative_zero_is_torchs measures it).
"""
import numpy as np

from tests.attack_ref import fmaf

RELU_KEEPS_NEG_ZERO = False

_F = np.float32


def _f32(a):
    a = np.asarray(a)
    assert a.dtype == np.float32, a.dtype  # no silent conversion: the callers pass fp32
    return a


def bits(a):
    """fp32 array -> its uint32 bit patterns (a copy, C order)."""
    return np.ascontiguousarray(_f32(a)).view(np.uint32).copy()


def from_bits(b):
    return np.ascontiguousarray(np.asarray(b, dtype=np.uint32)).view(np.float32)


def relu(t, keeps_neg_zero=None):
    """max(t, 0) that keeps NaN; -0 stays -0 (t < 0 ? 0 : t) or becomes +0
    (t > 0 ? t : 0), by `keeps_neg_zero` (default: RELU_KEEPS_NEG_ZERO)."""
    t = _f32(t)
    if keeps_neg_zero is None:
        keeps_neg_zero = RELU_KEEPS_NEG_ZERO
    with np.errstate(invalid="ignore"):
        if keeps_neg_zero:
            return np.where(t < 0, _F(0), t)
        return np.where(t > 0, t, np.where(np.isnan(t), t, _F(0)))


# ------------------------------------------------------------------ layouts
def nhwc_channel(index, C):
    """Channel of the element at flat index `index` of a [N, H, W, C] tensor."""
    return np.asarray(index, np.int64) % C


def nchw_channel(index, C, HW):
    """Channel of the element at flat index `index` of a [N, C, H*W] tensor."""
    return (np.asarray(index, np.int64) // HW) % C


# ------------------------------------------------------------------- folds
def fold(w, b, mean, var, eps):
    """(alpha, beta) of dls_bn_fold_f32; w / b may be None (affine=False)."""
    mean, var = _f32(mean), _f32(var)
    with np.errstate(all="ignore"):
        s = var + _F(eps)
        invstd = _F(1) / np.sqrt(s)  # numpy's float32 sqrt and divide: correctly rounded
        alpha = invstd * _f32(w) if w is not None else invstd
        t = mean * alpha
        beta = (_f32(b) if b is not None else np.zeros_like(mean)) - t
    assert alpha.dtype == beta.dtype == np.float32
    return alpha, beta


def fold_exact_parts(w, b, mean, var, eps):
    """(mean, iv64, w, b) of dls_bn_fold_exact_f32: the three copied planes as fp32
    (w -> 1 and b -> 0 when None), and what iv approximates, 1 / sqrt(|fl(var + eps)|),
    in fp64 (+inf at 0, 0 at inf, NaN at NaN)."""
    mean, var = _f32(mean), _f32(var)
    with np.errstate(all="ignore"):
        s = np.abs(var + _F(eps)).astype(np.float64)
        iv = 1.0 / np.sqrt(s)
    wp = _f32(w).copy() if w is not None else np.ones_like(mean)
    bp = _f32(b).copy() if b is not None else np.zeros_like(mean)
    return mean.copy(), iv, wp, bp


def ulps_from(got, exact):
    """|got - exact| in units of the fp32 spacing of exact's binade (exact: fp64, finite,
    positive and in the fp32 normal range)."""
    _, e = np.frexp(exact)
    return np.abs(_f32(got).astype(np.float64) - exact) / np.ldexp(1.0, e - 24)


# ------------------------------------------------------------------ passes
def act(x, alpha, beta, r=None, relu_on=False, ch=None, keeps_neg_zero=None):
    """dls_bn_act_nhwc_f32.  alpha / beta are [C]; `ch` gives each element's channel
    (default: x's last axis is the channel axis)."""
    x, alpha, beta = _f32(x), _f32(alpha), _f32(beta)
    if ch is not None:
        alpha, beta = alpha[ch], beta[ch]
    with np.errstate(all="ignore"):
        t = x * alpha
        t = t + beta
        if r is not None:
            t = t + _f32(r)
    assert t.dtype == np.float32
    return relu(t, keeps_neg_zero) if relu_on else t


def act_exact(x, consts, r=None, relu_on=False, ch=None, keeps_neg_zero=None):
    """dls_bn_act_exact_{nhwc,nchw}_f32.  consts is [4 * C] = [mean | iv | w | b]; `ch`
    gives each element's channel (default: x's last axis is the channel axis)."""
    x = _f32(x)
    m, iv, w, b = _f32(consts).reshape(4, -1)
    if ch is not None:
        m, iv, w, b = m[ch], iv[ch], w[ch], b[ch]
    with np.errstate(all="ignore"):
        h = x - m
        h = h * iv
        t = fmaf(np.broadcast_to(w, h.shape), h, np.broadcast_to(b, h.shape))
        if r is not None:
            t = t + _f32(r)
    assert t.dtype == np.float32
    return relu(t, keeps_neg_zero) if relu_on else t


def mismatches(got, ref):
    """Flat indices where `got` differs from `ref`: bit for bit as uint32, except
    where ref is NaN, where got must be some NaN (payloads are not compared)."""
    got = np.ascontiguousarray(_f32(got)).reshape(-1)
    ref = np.ascontiguousarray(_f32(ref)).reshape(-1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    nan = np.isnan(ref)
    bad = np.where(nan, ~np.isnan(got), got.view(np.uint32) != ref.view(np.uint32))
    return np.flatnonzero(bad)
