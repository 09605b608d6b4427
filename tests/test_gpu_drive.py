"""GPU: dls_hadamard_rotate_f32, dls_drive_compress_f32 and dls_drive_fedavg_f32 against
tests/drive_ref.py, bit for bit but for the scales of random inputs (1 ulp, derived below);
FedDriveWorker and FedDriveServer on the device."""
import ctypes

import numpy as np
import pytest
import torch

from tests import drive_ref as ref
from tests.drive_ref import bits
from tests.test_topk_host import FakeTrainer, initial_model, make_model

pytestmark = pytest.mark.gpu

F32 = np.float32
D, TILE = 4096, 64  # mirrored from _native below
SHAPES = [64, D, D + 64, 3 * D - 64]  # a sliver, one block, a nearly empty 2nd, a ragged 3rd
SEED, ROUND = 0x1234567890ABCDEF, 3


def _dev():
    return torch.device("cuda", 0)


def _t(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(_dev())


def sigma(P, seed=SEED, stream_id=ROUND):
    """The Philox words sigma is read from: coordinates 0 .. Pd / 32 - 1."""
    from distributed_learning_simulator_amd import _native
    assert (_native.DRIVE_BLOCK, _native.DRIVE_CLIENT_TILE) == (D, TILE)
    return _native.philox_u32(D * ref.blocks(P) // 32, seed, stream_id,
                              device=_dev()).cpu().numpy().view(np.uint32)


def spread(rng, n):
    """fp32 with exponents over about +-30 decades: a wrong stage order changes bits."""
    return (rng.standard_normal(n) * 10.0 ** rng.uniform(-30, 30, n)).astype(F32)


def run_rotate(x, P, inverse, seed=SEED, stream_id=ROUND):
    from distributed_learning_simulator_amd import _native
    n = P if inverse else D * ref.blocks(P)
    out = torch.full((n + 64,), 7.0, device=_dev())
    _native.hadamard_rotate(_t(x), P, seed, stream_id, inverse=inverse, out=out)
    out = out.cpu().numpy()
    assert np.all(out[n:] == 7.0)  # the canary
    return out[:n]


@pytest.mark.parametrize("P", SHAPES)
def test_rotation(P):
    rng = np.random.default_rng(P)
    x, words = spread(rng, P), sigma(P)
    y = run_rotate(x, P, False)
    assert np.array_equal(bits(y), bits(ref.rotate(x, P, words)))
    assert np.array_equal(bits(run_rotate(y, P, True)), bits(ref.rotate(y, P, words, inverse=True)))
    assert not np.array_equal(y, run_rotate(x, P, False, stream_id=ROUND + 1))
    assert not np.array_equal(y, run_rotate(x, P, False, seed=SEED + 1))
    k = rng.integers(-128, 129, P).astype(F32)  # every butterfly exact: H H = 4096
    assert np.array_equal(run_rotate(run_rotate(k, P, False), P, True), k)  # a zero: either sign


def run_compress(w, base, P, mode, stream=None):
    from distributed_learning_simulator_amd import _native
    NB = ref.blocks(P)
    words = torch.full((NB * D // 64 + 2,), -1, dtype=torch.int64, device=_dev())
    scales = torch.full((NB + 4,), -1.0, device=_dev())
    stats = torch.full((4,), -1, dtype=torch.int32, device=_dev())
    tw, tb = _t(w), _t(base)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream or torch.cuda.current_stream()):
        _native.drive_compress(tw, tb, P, SEED, ROUND, ("unbiased", "mse")[mode], words, scales,
                               stats, stream=stream)
    torch.cuda.synchronize()
    assert words[-2:].tolist() == [-1, -1] and scales[NB:].tolist() == [-1.0] * 4
    assert stats[1:].tolist() == [-1] * 3
    return words[:-2].cpu().numpy().view(np.uint64), scales[:NB].cpu().numpy(), int(stats[0])


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("P", SHAPES)
def test_compress_exact_sums(P, mode):
    """Integer updates |u| <= 128: every butterfly is exact, |y| <= 2^13 in multiples of 2^-6,
    so sq < 2^38 in multiples of 2^-12 and l1 are exact in any order: everything bit for bit.
    Zeros of both signs among the inputs; where the row has one, an all-zero last block."""
    rng = np.random.default_rng(10 * P + mode)
    base = rng.integers(-1000, 1001, P).astype(F32)
    w = base + rng.integers(-128, 129, P).astype(F32)
    z = rng.random(P) < 0.1
    w[z], base[z] = rng.choice(np.array([0.0, -0.0], F32), (2, int(z.sum())))
    w[1], base[1] = -0.0, 0.0  # u = -0.0
    if P > D:
        a = D * (ref.blocks(P) - 1)
        w[a:] = base[a:] = rng.choice(np.array([0.0, -0.0], F32), P - a)
    want = ref.compress(w, base, P, sigma(P), mode)
    got = run_compress(w, base, P, mode)
    assert (bits((w - base).astype(F32)) == 0x80000000).any()
    if P > D:
        assert bits(want[1])[-1] == 0 and not want[0][-D // 64:].any()
    assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))
    assert got[2] == want[2] == 0


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("P", SHAPES)
def test_compress_random(P, mode):
    """y is exact by contract, so the bits are the reference's.  Scales within 1 ulp: at most
    4096 non-negative fp64 terms in any order are within 4096 * 2^-53 of the exact sum and
    the fp64 quotient is rounded once to fp32: the same or an adjacent fp32.  A second HIP
    stream gives the same outputs; two non-finite inputs are counted."""
    rng = np.random.default_rng(20 * P + mode)
    w, base = spread(rng, P), spread(rng, P)
    want = ref.compress(w, base, P, sigma(P), mode)
    got = run_compress(w, base, P, mode)
    assert np.array_equal(got[0], want[0]) and got[2] == 0 and np.all(got[1] > 0)
    assert np.abs(bits(got[1]).astype(np.int64) - bits(want[1]).astype(np.int64)).max() <= 1
    again = run_compress(w, base, P, mode, stream=torch.cuda.Stream(_dev()))
    assert np.array_equal(again[0], got[0]) and np.array_equal(bits(again[1]), bits(got[1]))
    w[0], base[P - 1] = np.inf, np.nan
    assert run_compress(w, base, P, mode)[2] == 2


@pytest.mark.parametrize("K", [1, 2, TILE + 1])
@pytest.mark.parametrize("P", SHAPES)
def test_fedavg(P, K):
    """Pitches above Pd / 64 and NB, unequal weights with an odd total, a client whose
    scales are all zero, random bit words; then the reversed order."""
    from distributed_learning_simulator_amd import _native
    rng = np.random.default_rng(100 * P + K)
    NB, nw = ref.blocks(P), ref.blocks(P) * D // 64
    base = (rng.standard_normal(P) * 0.1).astype(F32)
    rows = rng.integers(0, 2 ** 64, (K, nw + 3), dtype=np.uint64)
    scales = (rng.random((K, NB + 5)) * 10.0 ** rng.uniform(-6, 0, (K, NB + 5))).astype(F32)
    scales[K // 2] = 0.0
    ns = [int(n) for n in rng.integers(100, 1001, K)]
    ns[0] += sum(ns) % 2 == 0 and 1  # an odd total
    words = sigma(P)
    for order in (list(range(K)), list(range(K))[::-1]):
        tb, ts = _t(rows.view(np.int64))[order], _t(scales)[order]
        out = torch.full((P + 64,), 7.0, device=_dev())
        _native.drive_fedavg(_t(base), tb[:, :nw + 1], ts[:, :NB + 1],
                             torch.tensor([float(ns[i]) for i in order], device=_dev()),
                             float(sum(ns)), P, SEED, ROUND, out)
        want = ref.fedavg(base, [(rows[i, :nw], scales[i]) for i in order], [ns[i] for i in order],
                          P, words)
        out = out.cpu().numpy()
        assert np.array_equal(bits(out[:P]), bits(want)) and np.all(out[P:] == 7.0)


def test_refusals():
    """Each with the documented status, and nothing written."""
    from distributed_learning_simulator_amd import _native
    dev = _dev()
    buf = torch.zeros(2 * 128 + D + 4, device=dev)
    w, base, off, wide = buf[:128], buf[128:256], buf[1:129], buf[256:256 + D]
    words = torch.full((64,), 5, dtype=torch.int64, device=dev)
    scales, stats = torch.full((4,), 5.0, device=dev), torch.full((4,), 5, dtype=torch.int32, device=dev)
    out, wt = torch.full((D,), 5.0, device=dev), torch.ones(4, device=dev)
    for args in ((off, base), (w, buf[129:257])):
        with pytest.raises(RuntimeError, match="aligned"):
            _native.drive_compress(*args, 128, 0, 1, "mse", words, scales, stats)
    for b, o in ((w, w), (w, buf[129:257])):
        with pytest.raises(RuntimeError, match="overlap|aligned"):
            _native.drive_fedavg(b, words[None], scales[None], wt[:1], 1.0, 128, 0, 1, o)
    L, p = _native.lib(), lambda t: ctypes.c_void_p(t.data_ptr())
    u64 = ctypes.c_uint64
    cases = [(L.dls_drive_compress_f32(p(w), p(base), P, u64(0), u64(1), 0, p(words), p(scales),
                                       p(stats), None), rc) for P, rc in ((96, -2), (0, -1))]
    cases += [(L.dls_drive_compress_f32(p(off), p(base), 128, u64(0), u64(1), 0, p(words),
                                        p(scales), p(stats), None), -2),
              (L.dls_drive_compress_f32(p(w), p(base), 128, u64(0), u64(1), 2, p(words),
                                        p(scales), p(stats), None), -1),
              (L.dls_drive_compress_f32(p(w), p(base), 128, u64(0), u64(1), 0, p(words),
                                        p(base), p(stats), None), -1),
              (L.dls_hadamard_rotate_f32(p(wide), 128, u64(0), u64(1), 1, p(wide), None), -1),
              (L.dls_hadamard_rotate_f32(p(w), 96, u64(0), u64(1), 0, p(out), None), -2),
              (L.dls_hadamard_rotate_f32(p(off), 128, u64(0), u64(1), 0, p(out), None), -2),
              (L.dls_drive_fedavg_f32(p(base), p(words), 64, p(scales), 1, p(wt), 1.0, 1, 128, u64(0),
                                      u64(1), p(base), None), -1),
              (L.dls_drive_fedavg_f32(p(base), p(words), 63, p(scales), 1, p(wt), 1.0, 1, 128, u64(0),
                                      u64(1), p(out), None), -2),
              (L.dls_drive_fedavg_f32(p(base), p(words), 64, p(scales), 0, p(wt), 1.0, 1, 128, u64(0),
                                      u64(1), p(out), None), -2),
              (L.dls_drive_fedavg_f32(p(base), p(words), 64, p(scales), 1, p(wt), 1.0, 0, 128, u64(0),
                                      u64(1), p(out), None), -1)]
    assert [got for got, _ in cases] == [rc for _, rc in cases]
    torch.cuda.synchronize()
    assert bool((words == 5).all()) and scales.tolist() == [5.0] * 4 and stats.tolist() == [5] * 4
    assert not buf.any() and bool((out == 5.0).all())


@pytest.mark.parametrize("scale", ["unbiased", "mse"])
def test_three_workers_two_rounds(scale):
    """Through FedDriveWorker / FedDriveServer on the device: every payload and both broadcast
    models are the reference's; a round's rotation is its own; a payload of another round is
    refused; a diverged worker sends nothing."""
    from distributed_learning_simulator_amd.servers.fed_drive_server import FedDriveServer
    from distributed_learning_simulator_amd.workers.fed_drive_worker import FedDriveWorker
    dev, ns, mode = _dev(), {0: 300, 1: 120, 2: 777}, ("unbiased", "mse").index(scale)
    server = FedDriveServer(seed=SEED, initial_model=initial_model(), tester=None, worker_number=3,
                            synchronous=True, device=dev)
    workers = {i: FedDriveWorker(seed=SEED, scale=scale, worker_id=i,
                                 trainer=FakeTrainer(make_model(10 + i).to(dev), ns[i]),
                                 worker_data_queue=server.worker_data_queue, round=2)
               for i in range(3)}
    for i, wk in workers.items():
        wk.load_model(server.worker_data_queue.get_result(consumer=i))
    lay = server.layout
    P = lay.P
    real = np.zeros(P, bool)  # the layout's padding slots are decoded too, and dropped
    for a, n in zip(lay.offsets, lay.numels):
        real[a:a + n] = True
    g = torch.Generator().manual_seed(4)
    for rnd, order in ((1, [2, 0, 1]), (2, [1, 2, 0])):
        prev = lay.flatten(server.prev_model, device=dev).cpu().numpy()
        words, sent = sigma(P, stream_id=rnd), {}
        for i in order:
            with torch.no_grad():
                for p in workers[i].trainer.model.parameters():
                    p += (0.05 * torch.randn(p.shape, generator=g)).to(dev)
            w = lay.flatten(dict(workers[i].trainer.model.named_parameters()), device=dev).cpu().numpy()
            sent[i] = ref.compress(w, prev, P, words, mode)[:2]
            up = workers[i].drive_update(rnd)
            assert np.array_equal(up.bits.cpu().numpy().view(np.uint64), sent[i][0])
            assert np.array_equal(bits(up.scales.cpu().numpy()), bits(sent[i][1]))
            if i == order[0]:
                other = workers[i].drive_update(rnd + 1)
                assert not torch.equal(other.bits, up.bits)
                with pytest.raises(ValueError, match="rotation of round"):
                    server.worker_data_queue.add_task((i, ns[i], other))
            server.worker_data_queue.add_task((i, ns[i], up))
        want = ref.fedavg(prev, [sent[i] for i in order], [ns[i] for i in order], P, words)
        for i in order:
            model = server.worker_data_queue.get_result(consumer=i)
            got = lay.flatten(model, device=dev).cpu().numpy()
            assert np.array_equal(bits(got)[real], bits(want)[real]) and not got[~real].any()
            workers[i].load_model(model)
    nbytes = D * ref.blocks(P) // 8 + 4 * ref.blocks(P)
    assert server.round == 2 and server.payload_bytes[0] == {i: nbytes for i in order}
    with torch.no_grad():
        next(workers[0].trainer.model.parameters())[0, 0] = float("inf")
    with pytest.raises(ValueError, match="not finite"):
        workers[0].drive_update(3)
    assert not server._payloads
