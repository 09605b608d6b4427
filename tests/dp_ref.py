"""CPU reference of the library's random stream and of the DP-FedAvg step on it
(include/dls_hip.h: dls_philox_u32, dls_philox_normal_f32, dls_normal_from_bits_f32,
dls_dp_clip_noise_step_f32) - TEST INFRASTRUCTURE ONLY (the package has no CPU path).

* Philox4x32-10 in numpy uint64 arithmetic (the Random123 known answers pin it);
* the uniforms, exact; the normals in fp64 (``np.log``, ``np.cos(2 pi u)``), which the
  device's fp32 normals match within ``normal_bound``;
* the step in numpy float32, with the normals handed in;
* CPU stand-ins for the four wrappers and for the two calls ``dp_mean`` and
  ``centered_clip`` share with them (``install``);
* the closed-form epsilon, restated.
"""
import math

import numpy as np
import torch

from tests import centered_clip_ref as CR

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
NORMAL_MAX = math.sqrt(48.0 * math.log(2.0))

# The error of the device's logf and cospif / sinpif in ulp, as far as the entry point
# shows it, measured on an MI355X (ROCm 7; DESIGN.md "Differentially private FedAvg" has
# the sweep): with every one of the 2^23 uniforms in one word and the other word fixed,
# the largest |g_gpu - g_ref| / (2^-23 r) was MEASURED_LOG_SWEEP when the radius word
# varied and MEASURED_TRIG_SWEEP when the angle word varied.  Read as if the whole error
# of a sweep came from the function it varies (the most the function can be blamed for),
# that is e_log <= 2 * MEASURED_LOG_SWEEP ulp and e_trig <= MEASURED_TRIG_SWEEP ulp; the
# bound uses twice those, so that another point release of the math library passes.
MEASURED_LOG_SWEEP = 1.40   # 1.3996 at radius word 0x21a38200 beside angle word 0x41c83b0e
MEASURED_TRIG_SWEEP = 1.20  # 1.1991 at angle word 0x64742000 beside radius word 0x6627e8d5
E_LOG = 2.0 * (2.0 * MEASURED_LOG_SWEEP)
E_TRIG = 2.0 * MEASURED_TRIG_SWEEP


def philox4x32(counter, key):
    """Philox4x32-10 of uint32 counters [..., 4] under uint32 keys [..., 2] (broadcast):
    uint32 [..., 4]."""
    c = [np.asarray(counter)[..., i].astype(np.uint64) for i in range(4)]
    k = [np.asarray(key)[..., i].astype(np.uint64) for i in range(2)]
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK,
             (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return np.stack(np.broadcast_arrays(*c), axis=-1).astype(np.uint32)


def words(n, seed, stream_id, first=0):
    """uint32 [n]: the words of coordinates first .. first + n - 1 under (seed, stream_id)."""
    n, first, seed, stream_id = int(n), int(first), int(seed), int(stream_id)
    if n == 0:
        return np.zeros(0, np.uint32)
    b0, b1 = first // 4, (first + n - 1) // 4
    blocks = [b0 + i for i in range(b1 - b0 + 1)]  # Python ints: past 2^63 is fine
    ctr = np.array([[b & 0xFFFFFFFF, b >> 32, stream_id & 0xFFFFFFFF, stream_id >> 32]
                    for b in blocks], dtype=np.uint64)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)
    out = philox4x32(ctr, key).reshape(-1)
    o = first - 4 * b0
    return out[o:o + n].copy()


def uniforms(w):
    """fp64 (and exactly fp32) u = ((w >> 9) + 0.5) * 2^-23 of uint32 words."""
    return ((np.asarray(w, np.uint32) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def normal_pairs64(bits):
    """fp64 (g [n], r [n]) of uint32 word pairs bits [n] (n even): out[2j], out[2j+1] =
    r cos(2 pi u_b), r sin(2 pi u_b) with r = sqrt(-2 ln u_a); r is repeated per pair."""
    bits = np.asarray(bits, np.uint32)
    assert bits.ndim == 1 and bits.size % 2 == 0
    ua, ub = uniforms(bits[0::2]), uniforms(bits[1::2])
    r = np.sqrt(-2.0 * np.log(ua))
    g = np.empty(bits.size, np.float64)
    g[0::2] = r * np.cos(2.0 * np.pi * ub)
    g[1::2] = r * np.sin(2.0 * np.pi * ub)
    return g, np.repeat(r, 2)


def normals64(n, seed, stream_id, first=0):
    """fp64 [n]: the reference normals of coordinates first .. first + n - 1."""
    n, first = int(n), int(first)
    lo = first - first % 2  # whole pairs
    hi = first + n + (first + n) % 2
    g, _ = normal_pairs64(words(hi - lo, seed, stream_id, lo))
    return g[first - lo:first - lo + n]


def normal_bound(r):
    """The largest |g_gpu - g_ref| the contract allows at radius r (fp64 array)."""
    return (E_LOG / 2.0 + E_TRIG + 1.5) * 2.0 ** -23 * np.asarray(r, np.float64)


def step_bits(X, c, z, sigma, g):
    """uint32 [P]: z' = fl32(y + fl32(sigma * g)) with y the clip step's new z
    (centered_clip_ref.step_bits); sigma == 0 (or g None) returns y itself."""
    y = CR.step_bits(X, c, z).view(np.float32)
    if g is None or float(sigma) == 0.0:
        return y.view(np.uint32).copy()
    with np.errstate(all="ignore"):
        n = (np.float32(sigma) * np.asarray(g, np.float32)).astype(np.float32)
        out = (y + n).astype(np.float32)
    return out.view(np.uint32).copy()


def epsilon(z, T, delta):
    """T / (2 z^2) + sqrt(2 T ln(1 / delta)) / z: the optimum over the Renyi order alpha of
    alpha T / (2 z^2) + ln(1 / delta) / (alpha - 1) (Mironov 2017, Prop. 3)."""
    return T / (2.0 * z * z) + math.sqrt(2.0 * T * math.log(1.0 / delta)) / z


def epsilon_by_search(z, T, delta, steps=200000):
    """The same minimum found numerically over a grid of orders alpha: never below the
    closed form, and close to it."""
    best = math.inf
    for i in range(1, steps):
        a = 1.0 + i * 1e-3
        best = min(best, a * T / (2.0 * z * z) + math.log(1.0 / delta) / (a - 1.0))
    return best


# ----------------------------------------------------------- CPU stand-ins
def _np(t):
    return t.detach().cpu().numpy()


def philox_u32(n, seed, stream_id, first=0, out=None, device=None, stream=None):
    w = torch.from_numpy(words(n, seed, stream_id, first).view(np.int32).copy())
    if out is None:
        return w
    out[:int(n)].copy_(w)
    return out


def philox_normal(n, seed, stream_id, first=0, out=None, device=None, stream=None):
    g = torch.from_numpy(normals64(n, seed, stream_id, first).astype(np.float32))
    if out is None:
        return g
    out[:int(n)].copy_(g)
    return out


def normal_from_bits(bits, out=None, stream=None):
    g = torch.from_numpy(normal_pairs64(_np(bits).view(np.uint32))[0].astype(np.float32))
    if out is None:
        return g
    out[:g.numel()].copy_(g)
    return out


def dp_clip_noise_step(U, rows, c, P, z, sigma, seed, stream_id, stream=None):
    X = _np(U)[_np(rows).astype(np.int64), :P]
    g = normals64(P, seed, stream_id).astype(np.float32) if float(sigma) != 0.0 else None
    z[:P].copy_(torch.from_numpy(step_bits(X, _np(c), _np(z)[:P], sigma, g).view(np.float32)))
    return z


def rows_sqdist_to(U, rows, P, z, out=None, stream=None):
    X = _np(U)[_np(rows).astype(np.int64), :P]
    d2 = torch.from_numpy(np.asarray(CR.sqdist_to(X, _np(z)[:P]), np.float64))
    if out is None:
        return d2
    out.copy_(d2)
    return out


def centered_clip_step(U, rows, c, P, z, dist2=None, stream=None):
    X = _np(U)[_np(rows).astype(np.int64), :P]
    z[:P].copy_(torch.from_numpy(CR.step_bits(X, _np(c), _np(z)[:P]).view(np.float32)))
    return z, rows_sqdist_to(U, rows, P, z, out=dist2)


_DOUBLES = ("philox_u32", "philox_normal", "normal_from_bits", "dp_clip_noise_step",
            "rows_sqdist_to", "centered_clip_step")


def install(monkeypatch):
    """cpu_doubles.install, then the stand-ins above."""
    from distributed_learning_simulator_amd import _native
    from tests import cpu_doubles
    cpu_doubles.install(monkeypatch)
    for name in _DOUBLES:
        monkeypatch.setattr(_native, name, globals()[name])
