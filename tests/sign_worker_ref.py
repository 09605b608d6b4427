"""Inputs and oracle trajectories of the signSGD worker tests — TEST INFRASTRUCTURE ONLY.

Shared by tests/test_sign_worker_host.py (the oracle against torch's CPU ops at
these inputs) and tests/test_gpu_sign_worker.py (the kernels against the oracle).
Every reference value comes from oracle.sign (C oracle / numpy); nothing here
restates a kernel.
"""
import functools

import numpy as np

from oracle import sign as osign

# 1025 is the first size with a second block of the direction kernel (4 tiles of
# 256 per block); 70003 has a tail in the last lane group and a last tile of 4 words
SIZES = (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4100, 70003)

# the four configurations of tests/golden/make_golden.py: gen_sign_worker; the
# last one has no momentum and runs with buf=None
CONFIGS = (
    dict(momentum=0.9, dampening=0.0, nesterov=False, weight_decay=0.0, lr=0.01),
    dict(momentum=0.9, dampening=0.0, nesterov=True, weight_decay=1e-4, lr=0.05),
    dict(momentum=0.5, dampening=0.1, nesterov=False, weight_decay=5e-4, lr=0.1),
    dict(momentum=0.0, dampening=0.0, nesterov=False, weight_decay=1e-3, lr=0.01),
)
STEPS = 3

FLT_MAX = np.finfo(np.float32).max
EDGES = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, FLT_MAX, -FLT_MAX, np.inf, -np.inf,
                  np.nan], np.float32)

FILL = int(np.array([0xABABABABABABABAB], np.uint64).view(np.int64)[0])


def same_bits(a, b):
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(
        a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


def edge_positions(P):
    """The first and last element and both sides of every 64 (hence 256) boundary."""
    pos = {0, P - 1}
    for b in range(64, P, 64):
        pos.update((b - 1, b))
    return np.array(sorted(pos), np.int64)


def fma_slots(P):
    """Up to 16 positions that are never edge positions (index % 64 in {7, 37})."""
    idx = np.arange(P)
    idx = idx[((idx % 64 == 7) | (idx % 64 == 37)) & (idx != P - 1)]
    return idx[:16]


def edge_vector(P, seed, shift=0):
    """randn * 0.1 with 2 % exact zeros, then EDGES cycled over edge_positions(P)."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(P) * 0.1).astype(np.float32)
    x[rng.random(P) < 0.02] = 0.0
    pos = edge_positions(P)
    x[pos] = EDGES[(np.arange(pos.size) + shift) % EDGES.size]
    return x


def unfused_direction(g, buf, first, momentum, dampening, nesterov):
    """The worker's transform with every product rounded on its own (no fma):
    what the kernel would compute if it did not contract.  Only used to prove
    that the inputs tell the two apart."""
    g = np.asarray(g, np.float32)
    m, a = np.float32(momentum), np.float32(1.0 - dampening)
    with np.errstate(all="ignore"):
        b = g.copy() if first else (g * a + np.asarray(buf, np.float32) * m).astype(np.float32)
        d = (b * m + g).astype(np.float32) if nesterov else b
    return d, b


def fma_sensitive(buf, cfg, rng):
    """Per element of ``buf`` (the momentum buffer before a non-first step) a
    gradient for which fused and unfused arithmetic give another result, where
    one is found: another buffer when 1 - dampening != 1 (the product g * a is
    inexact), another *sign* of the nesterov direction (g cancels momentum * buf
    up to the rounding of the product, so the unfused sum is 0 and the fused one
    is not).  With dampening 0 and no nesterov no such gradient exists:
    fma(g, 1, x) == g + x.  Returns (g, found)."""
    m, damp, nest = cfg["momentum"], cfg["dampening"], cfg["nesterov"]
    buf = np.asarray(buf, np.float32)
    n = buf.size
    ncand = 513
    a = 1.0 - damp
    if nest:
        # d = g + m * (a g + m buf) = 0  <=>  g = -m^2 buf / (1 + m a); walk its ulps
        g0 = (-(m * m) * buf.astype(np.float64) / (1.0 + m * a)).astype(np.float32)
        cand = (g0.view(np.int32)[:, None] + (np.arange(ncand, dtype=np.int32) - ncand // 2))
        cand = cand.astype(np.int32).view(np.float32)
    else:
        cand = (rng.standard_normal((n, ncand)) * 0.1).astype(np.float32)
    bb = np.repeat(buf, ncand)
    df, bf = osign.worker_direction(cand.reshape(-1), bb, False, m, damp, nest)
    du, bu = unfused_direction(cand.reshape(-1), bb, False, m, damp, nest)
    if nest:
        differs = osign.worker_sign(df) != osign.worker_sign(du)
    else:
        differs = bf.view(np.uint32) != bu.view(np.uint32)
    differs = differs.reshape(n, ncand) & np.isfinite(cand)
    found = differs.any(1)
    pick = differs.argmax(1)
    return cand[np.arange(n), pick], found


@functools.lru_cache(maxsize=None)
def trajectory(P, ci):
    """STEPS steps of configuration ``ci`` at size P: per step a dict of
    grad, first, buf_in (None on the first step or without momentum), d, buf
    (None without momentum), sign, and nsens, the number of elements whose result
    depends on the fused multiply-add.  Read-only: shared between tests."""
    cfg = CONFIGS[ci]
    m = cfg["momentum"]
    rng = np.random.default_rng(1000 * P + ci)
    buf, out = None, []
    for s in range(STEPS):
        first = s == 0 and m != 0
        g = edge_vector(P, seed=(P, ci, s), shift=3 * s)
        slots, found = fma_slots(P), np.zeros(0, bool)
        if m != 0 and not first and slots.size:
            gs, found = fma_sensitive(buf[slots], cfg, rng)
            g[slots[found]] = gs[found]
            pos = edge_positions(P)  # the edges win (fma_slots avoids them anyway)
            assert not np.intersect1d(pos, slots).size
        d, nb = osign.worker_direction(g, buf, first, m, cfg["dampening"], cfg["nesterov"])
        step = dict(grad=g, first=first, buf_in=buf, d=d, buf=nb if m != 0 else None,
                    sign=osign.worker_sign(d), nsens=0)
        if m != 0 and not first:
            du, bu = unfused_direction(g, buf, False, m, cfg["dampening"], cfg["nesterov"])
            nan = np.isnan(nb)
            step["nsens"] = int(((nb.view(np.uint32) != bu.view(np.uint32)) & ~nan).sum()
                                + (osign.worker_sign(du) != step["sign"]).sum())
        for v in step.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        out.append(step)
        buf = nb if m != 0 else None
    return tuple(out)


def fma_matters(cfg):
    """Whether fused and unfused arithmetic can differ in what the worker keeps
    (the buffer) or sends (the sign); see fma_sensitive."""
    return cfg["momentum"] != 0 and (cfg["dampening"] != 0 or cfg["nesterov"])


def ternary_vote(P, seed, nan_code_at=()):
    """A random vote in {-1, 0, +1}; returns (vote as applied, packed planes uint64).
    Positions in ``nan_code_at`` carry the NaN code (both bits) on the wire and
    count as vote 0."""
    rng = np.random.default_rng(seed)
    v = rng.integers(-1, 2, P).astype(np.float32)
    planes = osign.pack_planes(v).copy()
    v = v.copy()
    for e in nan_code_at:
        planes[2 * (e // 64)] |= np.uint64(1) << np.uint64(e % 64)
        planes[2 * (e // 64) + 1] |= np.uint64(1) << np.uint64(e % 64)
        v[e] = 0.0
    return v, planes


def layout_row(layout, tensors):
    """Flat fp32 row of ``layout`` (ParameterLayout) holding ``tensors`` at its
    offsets, the padding zero."""
    row = np.zeros(layout.P, np.float32)
    for o, n, t in zip(layout.offsets, layout.numels, tensors):
        row[o:o + n] = np.asarray(t, np.float32).reshape(-1)
    return row
