"""GPU: dls_topk_compress_f32 past its launch caps, bit for bit against tests/topk_ref.py
through test_gpu_topk's check().  The rows come from topk_ref's scale shapes (which
tests/test_topk_host.py holds to the paths they are named for): P_SCAN2, where a scan thread
owns two chunks and the upper threads none; P_STRIDE, where blocks 0 and 1 of the histogram
passes take a second trip (the ragged chunk in it) and a scan thread owns three chunks;
P_RESNET, the workload's own size.  Every input puts what decides the output into the chunks
only those paths reach.  No tolerances anywhere."""
import math

import numpy as np
import pytest
import torch

from distributed_learning_simulator_amd import _native
from tests import test_gpu_topk as T
from tests import topk_ref
from tests.topk_ref import P_RESNET, P_SCAN2, P_STRIDE, bits

pytestmark = pytest.mark.gpu

F32 = np.float32
C, H, S = _native.TOPK_CHUNK, _native.TOPK_HIST_BLOCKS, _native.TOPK_SCAN_BLOCK
SCALE = [P_SCAN2, P_STRIDE]
PAD = 256  # sentinel elements on either side of a guarded operand (keeps 16-byte alignment)


def late_start(P):
    """The first coordinate of the chunks that only the path past the cap reaches: those of
    the second histogram trip, or (no second trip) those past the first SCAN_BLOCK chunks,
    which a one-chunk-per-thread scan would never add."""
    return (H if topk_ref.hist_trips(P) >= 2 else S) * C


def small(P, rng):
    """|u| < 0.1 everywhere, all three operands in play."""
    w, base, e = ((rng.standard_normal(P) * s).astype(F32) for s in (1e-3, 1e-3, 1e-4))
    assert np.abs(topk_ref.update(w, base, e)).max() < 0.1
    return w, base, e


# ------------------------------------------------------------------ what is selected
@pytest.mark.parametrize("P", SCALE)
def test_winners_only_in_the_late_chunks(P):
    """Every large |u| lies at or past late_start(P), the ragged tail included; k = their
    number and one less.  A histogram without the late chunks' keys picks another threshold."""
    rng = np.random.default_rng(P % 1009)
    late = late_start(P)
    w, base, e = small(P, rng)
    where = np.unique(np.concatenate([[late, late + C - 1, late + C, P - 3, P - 1],
                                      late + rng.choice(P - late, 40, replace=False)]))
    n = where.size
    w[where] = (1.0 + rng.permutation(n)).astype(F32) * rng.choice(np.array([-1.0, 1.0], F32), n)
    got = T.check(w, base, e, n)
    assert np.array_equal(got[0], where) and where[0] == late and (where >= late + C).sum() >= 3
    got = T.check(w, base, e, n - 1)  # all but the smallest of them (|u| ~ 1.0)
    smallest = where[np.argmin(np.abs(w[where]))]
    assert np.array_equal(got[0], where[where != smallest])


@pytest.mark.parametrize("P", [4100] + SCALE)
def test_last_chunk_alone_holds_the_winners(P):
    """The k largest |u| all lie in the ragged last chunk, so no earlier chunk counts a key
    above or equal to the threshold and both of the chunk's prefixes are 0; the workspace
    holds zeros on entry.  The chunk is written only if the scan stored the totals behind
    the prefixes: a stale 0 there reads as "nothing of this chunk is selected"."""
    rng = np.random.default_rng(P % 1019)
    w, base, e = small(P, rng)
    where = np.array([P - P % C, P - 3, P - 1])
    w[where] = np.array([3.0, -2.0, 4.0], F32)
    for k in (3, 2):
        got = T.run_compress(w, base, e, k, ws_fill=0)
        assert np.array_equal(got[0], where if k == 3 else where[[0, 2]])
        T.check(w, base, e, k, got=got)


@pytest.mark.parametrize("P", SCALE)
def test_threshold_group_cut_inside_a_late_chunk(P):
    """Eight magnitudes, the threshold group (about P / 8 entries) spread over every chunk;
    k puts the cut (the last equal key that is sent) inside the second chunk of a scan
    thread, then inside the ragged last chunk, whose prefix sums every other chunk: more
    than HIST_BLOCKS of them at P_STRIDE, more than SCAN_BLOCK at P_SCAN2."""
    rng = np.random.default_rng(8)
    mags = np.array([0.5, 0.75, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0], F32)
    pick = rng.integers(0, 8, P)
    pick[-4:] = 4  # the ragged chunk holds members whatever its length
    w = mags[pick] * rng.choice(np.array([-1.0, 1.0], F32), P)
    above = int((pick > 4).sum())
    members = np.flatnonzero(pick == 4)
    per, n = topk_ref.scan_per(P), topk_ref.nchunks(P)
    second_of_a_thread, ragged = per * (S // 3) + 1, n - 1
    assert per >= 2 and second_of_a_thread % per == 1 and ragged * C >= late_start(P) + C
    for chunk, cut in ((second_of_a_thread, second_of_a_thread * C + C // 2), (ragged, P - 2)):
        r = int(np.searchsorted(members, cut))  # the members before the cut
        assert members[r - 1] // C == chunk == members[r] // C
        got = T.check(w, T.zeros(P), T.zeros(P), above + r)
        # the group's members that were sent are its lowest indices
        sent = np.zeros(P, bool)
        sent[got[0]] = True
        assert sent[members[:r]].all() and not sent[members[r:]].any()


@pytest.mark.parametrize("P", SCALE)
def test_nonfinite_only_in_the_late_chunks(P):
    """NaNs and infinities at or past late_start(P) alone, two of them in the ragged chunk:
    counted, and they take the selected slots first (the NaNs before the infinities)."""
    rng = np.random.default_rng(5)
    w, base, e = T.gaussian(P, rng)
    late = late_start(P)
    nans, infs = [late + 2049, late + C, P - 1], [late, late + C - 1]
    assert late + C == P - P % C and len(set(nans + infs)) == 5
    w[nans] = np.nan
    w[infs] = [np.inf, -np.inf]
    k = 8
    got = T.check(w, base, e, k)
    assert got[3].tolist() == [k, 5] and set(nans + infs) <= set(got[0].tolist())
    got = T.check(w, base, e, 4)  # fewer slots than non-finite values: the NaNs, then index order
    assert got[3].tolist() == [4, 5] and set(got[0].tolist()) == set(nans) | {late}


@pytest.mark.parametrize("k", [1, P_STRIDE])
def test_one_and_every_coordinate(k):
    """k = P: every chunk writes, each at the offset its prefix gives: idx is 0 .. P-1."""
    P = P_STRIDE
    w, base, e = T.gaussian(P, np.random.default_rng(4))
    got = T.check(w, base, e, k)
    if k == P:
        assert np.array_equal(got[0], np.arange(P, dtype=np.int32))


# ------------------------------------------------------------------ what is written
def run_compress_guarded(w, base, e, k):
    """run_compress with the workspace a slice of exactly the queried size, and e, idx and
    val slices of exactly P, k and k elements, each inside a sentinel-filled buffer: asserts
    that no byte outside the slices changed."""
    dev = T._dev()
    P = w.size
    need = int(_native.lib().dls_topk_workspace(P))
    assert need == topk_ref.workspace_bytes(P)

    def guarded(n, dtype, fill):
        buf = torch.full((n + 2 * PAD,), fill, dtype=dtype, device=dev)
        return buf, buf[PAD:PAD + n]

    ws_buf, ws = guarded(need, torch.uint8, 0xA5)
    idx_buf, idx = guarded(k, torch.int32, -7)
    val_buf, val = guarded(k, torch.float32, 123.0)
    e_buf, te = guarded(P, torch.float32, 321.0)
    te.copy_(torch.from_numpy(np.ascontiguousarray(e, dtype=F32)))
    tw, tb = (torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(dev) for a in (w, base))
    stats = torch.full((2,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    _native.topk_compress(tw, tb, te, k, P, idx, val, stats, ws)
    torch.cuda.synchronize()
    for name, buf, n, fill in (("workspace", ws_buf, need, 0xA5), ("idx", idx_buf, k, -7),
                               ("val", val_buf, k, 123.0), ("e", e_buf, P, 321.0)):
        assert bool((buf[:PAD] == fill).all()), f"{name}: written before its first element"
        assert bool((buf[PAD + n:] == fill).all()), f"{name}: written past its last element"
    return idx.cpu().numpy(), val.cpu().numpy(), te.cpu().numpy(), stats.cpu().numpy()


@pytest.mark.parametrize("P", [4100] + SCALE)
def test_nothing_is_written_outside_the_operands(P):
    w, base, e = T.gaussian(P, np.random.default_rng(P % 1013))
    k = math.ceil(0.01 * P)
    T.check(w, base, e, k, got=run_compress_guarded(w, base, e, k))


# ------------------------------------------------------------------ the workload's size
K_RESNET = math.ceil(0.01 * P_RESNET)


def test_resnet_size_compress():
    w, base, e = T.gaussian(P_RESNET, np.random.default_rng(18))
    T.check(w, base, e, K_RESNET)


def test_resnet_size_sparse_fedavg_round():
    """Three clients' device-made payloads (each held to the exact-split invariant) through
    the server kernel: the reference's bits."""
    rng = np.random.default_rng(19)
    _, base, _ = T.gaussian(P_RESNET, rng)
    pay = []
    for _ in range(3):
        w, _, e = T.gaussian(P_RESNET, rng)
        got = T.run_compress(w, base, e, K_RESNET)
        T.check_split(w, base, e, K_RESNET, got)
        pay.append((got[0], got[1]))
    ns = [300, 120, 777]
    out = T.run_sparse(base, pay, ns)
    assert np.array_equal(bits(out), bits(topk_ref.sparse_fedavg(base, pay, ns)))
