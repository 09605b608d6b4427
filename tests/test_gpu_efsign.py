"""GPU: dls_efsign_compress_f32 and dls_efsign_fedavg_f32 against tests/efsign_ref.py, bit for
bit but for the scales of random inputs (1 ulp, derived below); FedEFSignWorker and
FedEFSignServer on the device."""
import ctypes

import numpy as np
import pytest
import torch

from tests import efsign_ref as ref
from tests.efsign_ref import bits
from tests.test_topk_host import FakeTrainer, initial_model, make_model

pytestmark = pytest.mark.gpu

F32 = np.float32
CHUNK, TILE = 4096, 64  # mirrored from _native below
# tiny tensors between large ones; both sides of a word, of a chunk and of the 64 chunks
# one pass of the per-tensor combine takes; segment 2 carries a whole word of padding
SIZES_A = [CHUNK + 1, 1, 63, 65 * CHUNK + 17, 64, 65, CHUNK - 1, 1, CHUNK, 3 * CHUNK + 5]
PERM_B = [3, 0, 9, 7, 2, 8, 5]  # layout B: these tensors of A in this order, one new first
LAYOUTS = {"A": (SIZES_A, (2,)), "B": ([200] + [SIZES_A[t] for t in PERM_B], (0, 3))}


def _dev():
    return torch.device("cuda", 0)


def _t(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(_dev())


def contents(kind, t, n):
    """(w, base, e) of tensor t of layout A, the same whichever layout holds it."""
    rng = np.random.default_rng(1000 * t + n + len(kind))
    if kind == "exact":  # multiples of 2^-20 below 2^8 each: every fp64 partial sum is exact
        w, base, e = (np.ldexp(rng.integers(-2 ** 27, 2 ** 27, n) >> rng.integers(0, 27, n), -20)
                      .astype(F32) for _ in range(3))
        z = rng.random(n) < 0.1
        w[z], base[z], e[z] = rng.choice(np.array([0.0, -0.0], F32), (3, int(z.sum())))
        if t == 2:
            w, base, e = np.zeros((3, n), F32)
        return w, base, e
    scale = 10.0 ** rng.uniform(-30, 30)
    return tuple((rng.standard_normal(n) * scale * f).astype(F32) for f in (1.0, 1.0, 0.01))


def make_inputs(kind, layout):
    sizes, slack = LAYOUTS[layout]
    src = list(range(len(SIZES_A))) if layout == "A" else [len(SIZES_A)] + PERM_B
    bounds, count = ref.segments(sizes, slack)
    w = np.full(bounds[-1], np.nan, F32)   # padding of w and base holds NaN, of e garbage
    base, e = w.copy(), np.full(bounds[-1], 7.0, F32)
    for a, n, t in zip(bounds, count, src):
        w[a:a + n], base[a:a + n], e[a:a + n] = contents(kind, t, n)
    return w, base, e, bounds, count


def run_compress(w, base, e, bounds, count, stream=None):
    from distributed_learning_simulator_amd import _native
    assert (_native.EFSIGN_CHUNK, _native.EFSIGN_CLIENT_TILE) == (CHUNK, TILE)
    seg = _native.efsign_segments(bounds, count, _dev())
    tw, tb, te = _t(w), _t(base), _t(e)
    words = torch.full((seg.P // 64,), -1, dtype=torch.int64, device=_dev())
    scales = torch.full((seg.T,), -1.0, device=_dev())
    stats = torch.full((1,), -1, dtype=torch.int32, device=_dev())
    ws = _native.efsign_workspace(seg.P, seg.T, _dev()).fill_(0xFF)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream or torch.cuda.current_stream()):
        _native.efsign_compress(tw, tb, te, seg, words, scales, stats, ws, stream=stream)
    torch.cuda.synchronize()
    return (words.cpu().numpy().view(np.uint64), scales.cpu().numpy(), te.cpu().numpy(),
            int(stats[0]))


def same(got, want):
    return (np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1]))
            and np.array_equal(bits(got[2]), bits(want[2])) and got[3] == want[3])


@pytest.mark.parametrize("layout", ["A", "B"])
def test_compress_exact_sums(layout):
    """Inputs whose fp64 sums are exact in any order: everything bit for bit, -0.0 and an
    all-zero tensor included; padding of bits and e is zero (the reference's)."""
    w, base, e, bounds, count = make_inputs("exact", layout)
    want = ref.compress(w, base, e, bounds, count)
    assert (bits(ref.update(w, base, e)) == 0x80000000).any() and 0.0 in want[1]
    assert same(run_compress(w, base, e, bounds, count), want)


def test_compress_random_order_contract_and_streams():
    """Scales within 1 ulp: the terms are non-negative, so an fp64 sum of n <= 2^24 of them
    in any order is within n * 2^-53 < 2^-29 relative of the exact one, and one rounding to
    fp32 gives the same or an adjacent value.  With the kernel's scales the rest is exact.
    A tensor's scale has the same bits at another offset among another T; another stream
    gives the same outputs."""
    got = {}
    for layout in ("A", "B"):
        w, base, e, bounds, count = make_inputs("random", layout)
        got[layout] = g = run_compress(w, base, e, bounds, count)
        s_ref = ref.compress(w, base, e, bounds, count)[1]
        assert np.all(g[1] > 0) and float(g[1].max()) / float(g[1].min()) > 1e20
        assert np.abs(bits(g[1]).astype(np.int64) - bits(s_ref).astype(np.int64)).max() <= 1
        assert same(g, ref.compress(w, base, e, bounds, count, scales=g[1]))
    assert np.array_equal(bits(got["B"][1][1:]), bits(got["A"][1][PERM_B]))
    assert same(run_compress(w, base, e, bounds, count, stream=torch.cuda.Stream(_dev())), g)


def test_compress_counts_nonfinite():
    w, base, e, bounds, count = make_inputs("exact", "A")
    w[bounds[3] + 70000], w[bounds[9] + 5] = np.inf, np.nan
    assert run_compress(w, base, e, bounds, count)[3] == 2


@pytest.mark.parametrize("K", [1, 2, 3, TILE + 1])
def test_fedavg(K):
    """Pitches above P / 64 and T, unequal weights with a total that is no power of two, a
    client whose scales are all zero, -0.0 in base's padding; then the reversed order."""
    from distributed_learning_simulator_amd import _native
    rng = np.random.default_rng(K)
    sizes, slack = LAYOUTS["B"]
    bounds, count = ref.segments(sizes, slack)
    P, T = bounds[-1], len(count)
    real = np.zeros(P, bool)
    for a, n in zip(bounds, count):
        real[a:a + n] = True
    base = (rng.standard_normal(P) * 0.1).astype(F32)
    base[~real] = F32(-0.0)
    words = rng.integers(0, 2 ** 64, (K, P // 64 + 3), dtype=np.uint64)
    scales = (rng.random((K, T + 5)) * 10.0 ** rng.uniform(-6, 0, (K, T + 5))).astype(F32)
    scales[K // 2] = 0.0
    ns = [int(n) for n in rng.integers(100, 1001, K)]
    ns[0] += sum(ns) % 2 == 0 and 1  # an odd total
    seg = _native.efsign_segments(bounds, count, _dev())
    for order in (list(range(K)), list(range(K))[::-1]):
        tb, ts = _t(words.view(np.int64))[order], _t(scales)[order]
        out = torch.full((P,), 7.0, device=_dev())
        _native.efsign_fedavg(_t(base), tb[:, :P // 64 + 1], ts[:, :T + 1], seg,
                              torch.tensor([float(ns[i]) for i in order], device=_dev()),
                              float(sum(ns)), out)
        want = ref.fedavg(base, [(words[i, :P // 64], scales[i]) for i in order], bounds, count,
                          [ns[i] for i in order])
        assert np.array_equal(bits(out.cpu().numpy()), bits(want))
        assert np.all(bits(want)[~real] == 0x80000000) and (~real).sum() > 64


def test_refusals():
    """Each with the documented status, and nothing written."""
    from distributed_learning_simulator_amd import _native
    dev = _dev()
    for bounds, count in (([0, 32, 128], [1, 1]), ([0, 64, 128], [65, 1]), ([0, 64, 96], [1, 1])):
        with pytest.raises(RuntimeError, match="DLS_EINVAL"):
            _native.efsign_segments(bounds, count, dev)
    seg = _native.efsign_segments([0, 64, 128], [3, 64], dev)
    buf = torch.zeros(3 * 128 + 4, device=dev)
    w, base, e, off = buf[:128], buf[128:256], buf[256:384], buf[1:129]
    words = torch.full((2,), 5, dtype=torch.int64, device=dev)
    scales, stats = torch.full((2,), 5.0, device=dev), torch.full((1,), 5, dtype=torch.int32, device=dev)
    ws = _native.efsign_workspace(128, 2, dev)
    out, wt = torch.full((128,), 5.0, device=dev), torch.ones(1, device=dev)
    for args in ((w, base, w), (w, base, base[:128]), (off, base, e), (w, base, buf[257:385])):
        with pytest.raises(RuntimeError, match="overlap|aligned"):
            _native.efsign_compress(*args, seg, words, scales, stats, ws)
    for b, o in ((w, w), (w, buf[129:257])):
        with pytest.raises(RuntimeError, match="overlap|aligned"):
            _native.efsign_fedavg(b, words[None], scales[None], seg, wt, 1.0, o)
    L, p = _native.lib(), lambda t: ctypes.c_void_p(t.data_ptr())
    cases = [(L.dls_efsign_compress_f32(p(w), p(base), p(e), P, p(seg.bounds), p(seg.count), 2,
                                        p(words), p(scales), p(stats), p(ws), None), rc)
             for P, rc in ((96, -2), (0, -1))]
    cases += [(L.dls_efsign_compress_f32(p(w), p(base), p(w), 128, p(seg.bounds), p(seg.count), 2,
                                         p(words), p(scales), p(stats), p(ws), None), -1),
              (L.dls_efsign_compress_f32(p(off), p(base), p(e), 128, p(seg.bounds), p(seg.count),
                                         2, p(words), p(scales), p(stats), p(ws), None), -2),
              (L.dls_efsign_fedavg_f32(p(base), p(words), 2, p(scales), 2, p(seg.bounds),
                                       p(seg.count), 2, p(wt), 1.0, 1, 128, p(base), None), -1),
              (L.dls_efsign_fedavg_f32(p(base), p(words), 1, p(scales), 2, p(seg.bounds),
                                       p(seg.count), 2, p(wt), 1.0, 1, 128, p(out), None), -2)]
    assert [got for got, _ in cases] == [rc for _, rc in cases]
    torch.cuda.synchronize()
    assert words.tolist() == [5, 5] and scales.tolist() == [5.0, 5.0] and stats.tolist() == [5]
    assert not buf.any() and bool((out == 5.0).all())


@pytest.mark.parametrize("error_feedback", [True, False])
def test_three_workers_two_rounds(error_feedback):
    """Through FedEFSignWorker / FedEFSignServer on the device: the reference run, its
    residual carried over (or dropped) between the rounds; a diverged worker sends nothing."""
    from distributed_learning_simulator_amd.servers.fed_efsign_server import FedEFSignServer
    from distributed_learning_simulator_amd.workers.fed_efsign_worker import FedEFSignWorker
    dev, ns = _dev(), {0: 300, 1: 120, 2: 777}
    server = FedEFSignServer(initial_model=initial_model(), tester=None, worker_number=3,
                             synchronous=True, device=dev)
    workers = {i: FedEFSignWorker(worker_id=i, trainer=FakeTrainer(make_model(10 + i).to(dev), ns[i]),
                                  worker_data_queue=server.worker_data_queue, round=2,
                                  error_feedback=error_feedback) for i in range(3)}
    for i, wk in workers.items():
        wk.load_model(server.worker_data_queue.get_result(consumer=i))
    lay = server.layout
    bounds, count = list(lay.offsets) + [lay.P], lay.numels
    resid = {i: np.zeros(lay.P, F32) for i in workers}
    g = torch.Generator().manual_seed(4)
    for order in ([2, 0, 1], [1, 2, 0]):
        prev = lay.flatten(server.prev_model, device=dev).cpu().numpy()
        sent = {}
        for i in order:
            with torch.no_grad():
                for p in workers[i].trainer.model.parameters():
                    p += (0.05 * torch.randn(p.shape, generator=g)).to(dev)
            w = lay.flatten(dict(workers[i].trainer.model.named_parameters()), device=dev).cpu().numpy()
            e = resid[i] if error_feedback else np.zeros(lay.P, F32)
            words, s, resid[i], _ = ref.compress(w, prev, e, bounds, count)
            up = workers[i].sign_update()
            assert np.array_equal(up.bits.cpu().numpy().view(np.uint64), words)
            assert np.array_equal(bits(up.scales.cpu().numpy()), bits(s))
            assert np.array_equal(bits(workers[i].residual.cpu().numpy()), bits(resid[i]))
            sent[i] = (words, s)
            server.worker_data_queue.add_task((i, ns[i], up))
        want = ref.fedavg(prev, [sent[i] for i in order], bounds, count, [ns[i] for i in order])
        for i in order:
            model = server.worker_data_queue.get_result(consumer=i)
            assert np.array_equal(bits(lay.flatten(model, device=dev).cpu().numpy()), bits(want))
            workers[i].load_model(model)
    assert server.round == 2 and server.payload_bytes[0] == {i: lay.P // 8 + 8 for i in order}
    with torch.no_grad():
        next(workers[0].trainer.model.parameters())[0, 0] = float("inf")
    with pytest.raises(ValueError, match="not finite"):
        workers[0].sign_update()
    assert not server._payloads
