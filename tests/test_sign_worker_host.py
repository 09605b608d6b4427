"""CPU: the signSGD worker oracle against torch's own CPU ops at the inputs of
tests/test_gpu_sign_worker.py (edge values, fma-sensitive pairs, every size), so that
the GPU tests may trust the oracle there.  Bit-exact, NaN positions included."""
import numpy as np
import pytest
import torch

from oracle import sign as osign
from tests import sign_worker_ref as R


def test_edge_vector_holds_every_edge_at_the_boundaries():
    for P in R.SIZES:
        x = R.edge_vector(P, seed=P)
        pos = R.edge_positions(P)
        assert pos[0] == 0 and pos[-1] == P - 1
        for b in range(64, P, 64):
            assert b - 1 in pos and b in pos
        if P >= 1023:  # enough boundaries for the whole cycle
            bits = set(x[pos].view(np.uint32).tolist())
            assert set(R.EDGES[:-1].view(np.uint32).tolist()) <= bits and np.isnan(x[pos]).any()
    assert np.float32(1e-45) > 0 and np.float32(1e-39) > 0  # denormals, not flushed by numpy


@pytest.mark.parametrize("ci", range(len(R.CONFIGS)))
def test_direction_oracle_equals_torch_cpu_ops(ci):
    """workers/sign_sgd_worker.py:32-44 with torch's ops on the CPU: clone on the first
    step, buf.mul_(m).add_(g, alpha=1 - dampening), nesterov g.add(buf, alpha=m), sign."""
    cfg = R.CONFIGS[ci]
    m = cfg["momentum"]
    for P in R.SIZES:
        buf = None
        for s, st in enumerate(R.trajectory(P, ci)):
            g = torch.from_numpy(st["grad"].copy())
            d = g
            if m != 0:
                if buf is None:
                    assert st["first"]
                    buf = torch.clone(g).detach()
                else:
                    buf.mul_(m).add_(g, alpha=1 - cfg["dampening"])
                d = g.add(buf, alpha=m) if cfg["nesterov"] else buf
                assert R.same_bits(st["buf"], buf.numpy()), (P, s)
            else:
                assert st["buf"] is None and not st["first"]
            assert R.same_bits(st["d"], d.numpy()), (P, s)
            assert R.same_bits(st["sign"], torch.sign(d).numpy()), (P, s)
            assert not np.isnan(st["sign"]).any()


def test_inputs_tell_fused_from_unfused_arithmetic():
    """Where the fused multiply-add can matter (dampening != 0: the buffer; nesterov:
    the sign sent), every non-first step of every size with a free slot holds
    elements whose result differs from the separately rounded one, so a kernel
    that did not fuse (or fused elsewhere) could not pass."""
    for ci, cfg in enumerate(R.CONFIGS):
        for P in R.SIZES:
            for s, st in enumerate(R.trajectory(P, ci)):
                if R.fma_matters(cfg) and not st["first"] and R.fma_slots(P).size:
                    assert st["nsens"] > 0, (ci, P, s)
                if not R.fma_matters(cfg):
                    assert st["nsens"] == 0, (ci, P, s)  # fma(g, 1, x) == g + x


@pytest.mark.parametrize("wd", [0.0, 1e-4, 5e-4])
@pytest.mark.parametrize("lr", [0.01, 0.1])
def test_apply_oracle_equals_torch_cpu_ops(wd, lr):
    """workers/sign_sgd_worker.py:48-57: d = vote.add(p, alpha=wd) when wd != 0;
    p.add_(d, alpha=-lr)."""
    for P in R.SIZES:
        p0 = R.edge_vector(P, seed=(P, 77))
        vote, _ = R.ternary_vote(P, seed=P, nan_code_at=(0, P // 2, P - 1))
        p = torch.from_numpy(p0.copy())
        d = torch.from_numpy(vote.copy())
        if wd != 0:
            d = d.add(p, alpha=wd)
        p.add_(d, alpha=-lr)
        assert R.same_bits(osign.worker_apply(p0, vote, lr, wd), p.numpy()), P


def test_planes_roundtrip_is_the_worker_sign():
    P = 1000 + 37  # ragged: no multiple of 64
    x = R.edge_vector(P, seed=5)
    x[[1, 70, P - 2]] = np.nan
    x[[2, 71]] = [0.0, -0.0]
    s = osign.worker_sign(x)
    nan = np.isnan(x)
    assert nan.sum() >= 4
    # what the worker sends: the sign first (NaN -> 0, neither bit), then the pack
    sent = osign.pack_planes(s)
    assert sent.size == (P + 255) // 256 * 8
    assert R.same_bits(osign.unpack_planes(sent, P), s)
    # the pack of the raw values differs only by the NaN code (both bits)
    back = osign.unpack_planes(osign.pack_planes(x), P)
    assert np.array_equal(np.isnan(back), nan)
    assert R.same_bits(back[~nan], s[~nan]) and np.all(s[nan] == 0)
    w = sent.reshape(-1, 2)
    for e in np.flatnonzero(nan).tolist():
        assert (int(w[e // 64, 0]) >> (e % 64)) & 1 == 0 and (int(w[e // 64, 1]) >> (e % 64)) & 1 == 0
    # bits past P are zero
    assert np.all(osign.unpack_planes(sent, sent.size * 32)[P:] == 0)


def test_ternary_vote_nan_code():
    v, planes = R.ternary_vote(130, seed=1, nan_code_at=(0, 64, 129))
    back = osign.unpack_planes(planes, 130)
    assert np.isnan(back[[0, 64, 129]]).all() and np.all(v[[0, 64, 129]] == 0)
    keep = ~np.isnan(back)
    assert R.same_bits(back[keep], v[keep])
