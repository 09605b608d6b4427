"""numpy float32 restatement of dls_server_opt_step_f32 (include/dls_hip.h): every
operation on float32 arrays, so each is rounded once and nothing is fused.  One function
per kind, ``step`` to pick one by its number, ``run`` to chain steps, and ``coeffs``, the
fp32 coefficients as the binding forms them (restated here, not imported)."""
import numpy as np

SGD, ADAGRAD, ADAM, YOGI = range(4)
KINDS = {"sgd": SGD, "adagrad": ADAGRAD, "adam": ADAM, "yogi": YOGI}
F = np.float32


def coeffs(lr, beta1, beta2, tau):
    """(lr, beta1, omb1, beta2, omb2, tau) as numpy float32: each of the four rounded to
    fp32 once, omb = float32(1.0 - float64(float32(beta)))."""
    lr, beta1, beta2, tau = F(lr), F(beta1), F(beta2), F(tau)
    return lr, beta1, F(1.0 - float(beta1)), beta2, F(1.0 - float(beta2)), tau


def v_start(tau):
    """fl32(tau * tau) of the fp32 tau: where the store starts v on tensor elements."""
    return F(float(F(tau)) * float(F(tau)))


def _f(a):
    a = np.asarray(a)
    assert a.dtype == np.float32, a.dtype
    return a


def sgd(agg, x, m, c):
    """(out, m'): m may be None with beta1 == 0 (then m' = d)."""
    lr, beta1 = c[0], c[1]
    with np.errstate(all="ignore"):
        d = _f(agg) - _f(x)
        if m is None:
            assert beta1 == 0
            m1 = d
        else:
            m1 = beta1 * _f(m) + d
        out = x + lr * m1
    return out, m1


def _adaptive(agg, x, m, v, c, second):
    lr, beta1, omb1, beta2, omb2, tau = c
    with np.errstate(all="ignore"):
        d = _f(agg) - _f(x)
        m1 = beta1 * _f(m) + omb1 * d
        d2 = d * d
        v1 = second(_f(v), d2, beta2, omb2)
        out = x + (lr * m1) / (np.sqrt(v1) + tau)
    assert out.dtype == m1.dtype == v1.dtype == np.float32
    return out, m1, v1


def adagrad(agg, x, m, v, c):
    return _adaptive(agg, x, m, v, c, lambda v, d2, b2, o2: v + d2)


def adam(agg, x, m, v, c):
    return _adaptive(agg, x, m, v, c, lambda v, d2, b2, o2: b2 * v + o2 * d2)


def _yogi_v(v, d2, b2, o2):
    t = v - d2
    s = (t > 0).astype(np.float32) - (t < 0).astype(np.float32)  # 0 for a NaN t
    return v - (o2 * d2) * s


def yogi(agg, x, m, v, c):
    return _adaptive(agg, x, m, v, c, _yogi_v)


def step(kind, agg, x, m, v, c):
    """(out, m', v') of one step of ``kind``; v' is None for SGD."""
    if kind == SGD:
        assert v is None
        out, m1 = sgd(agg, x, m, c)
        return out, m1, None
    return {ADAGRAD: adagrad, ADAM: adam, YOGI: yogi}[kind](agg, x, m, v, c)


def run(kind, aggs, x, m, v, c):
    """Chain one step per aggregate in ``aggs`` from (x, m, v): the list of (out, m', v')
    after each step; each step starts from the previous step's out."""
    trail = []
    for agg in aggs:
        x, m1, v = step(kind, agg, x, m, v, c)
        m = m1 if m is not None or kind != SGD else None
        trail.append((x, m1, v))
    return trail


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def same_bits(got, want):
    """Equal bits wherever ``want`` is not NaN, NaN wherever it is."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and bool(np.array_equal(bits(got)[~nan], bits(want)[~nan])) \
        and bool(np.isnan(got[nan]).all())
