"""GPU: dls_eden_compress_f32 and dls_eden_fedavg_f32 against tests/eden_ref.py, bit for bit
(the reference restates the order of the fp64 sums); FedEDENWorker and FedEDENServer on the
device."""
import numpy as np
import pytest
import torch

from tests import eden_ref as ref
from tests.eden_ref import bits
from tests.test_gpu_drive import ROUND, SEED, SHAPES, _dev, _t, sigma, spread
from tests.test_topk_host import FakeTrainer, initial_model, make_model

pytestmark = pytest.mark.gpu

F32 = np.float32
D, TILE = 4096, 64
MODES = ("unbiased", "mse")
# u = A e_0 + B e_1 rotates to |y| in {(A + B) / 64, (A - B) / 64}, exactly; for these pairs one
# of the two equals a threshold of the reference (bits 2: thr[0]; bits 4: thr[2]) to the bit
TIES = {2: (12163481.0, 221837.0, 0), 4: (12163481.0, 2270229.0, 2)}


def words_of(P, b):
    from distributed_learning_simulator_amd import _native
    assert _native.EDEN_CLIENT_TILE == TILE and _native.eden_code_words(P, b) == ref.blocks(P) * 128 * b
    return ref.blocks(P) * 128 * b


def run_compress(w, base, P, b, mode, stream=None):
    """(codes, scales, stats[0]) of the device, the canaries past every output checked."""
    from distributed_learning_simulator_amd import _native
    NB, nw = ref.blocks(P), words_of(P, b)
    codes = torch.full((nw + 4,), -1, dtype=torch.int32, device=_dev())
    scales = torch.full((NB + 4,), -1.0, device=_dev())
    stats = torch.full((4,), -1, dtype=torch.int32, device=_dev())
    tw, tb = _t(w), _t(base)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream or torch.cuda.current_stream()):
        _native.eden_compress(tw, tb, P, b, SEED, ROUND, MODES[mode], codes, scales, stats, stream=stream)
    torch.cuda.synchronize()
    assert codes[nw:].tolist() == [-1] * 4 and scales[NB:].tolist() == [-1.0] * 4
    assert stats[1:].tolist() == [-1] * 3
    return codes[:nw].cpu().numpy().view(np.uint32), scales[:NB].cpu().numpy(), int(stats[0])


def same(got, want):
    return np.array_equal(got[0], want[0]) and got[2] == want[2] and (
        np.array_equal(bits(got[1]), bits(want[1])) or
        (np.isnan(want[1]).any() and np.array_equal(got[1], want[1], equal_nan=True)))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("b", [2, 4])
@pytest.mark.parametrize("P", SHAPES)
def test_compress_structured(P, b, mode):
    """Block 0: the two spikes of TIES among zeros of both signs, so a rotated value lies on a
    threshold (a tie takes the lower cell).  Block 1, where the row has one: integers, zeros
    and u = -0.0.  Block 2: all zeros (every threshold is 0 and ties; the scale is +0.0).
    Then one inf and one NaN."""
    rng = np.random.default_rng(10 * P + b)
    w = rng.choice(np.array([0.0, -0.0], F32), P)
    base = rng.choice(np.array([0.0, -0.0], F32), P)
    A, Bv, m = TIES[b]
    w[:2], base[:2] = (A, Bv), 0.0
    if P > D:
        n = min(P, 2 * D) - D
        base[D:D + n] = rng.integers(-1000, 1001, n)
        w[D:D + n] = base[D:D + n] + rng.integers(-128, 129, n) * (rng.random(n) < 0.9)
        w[D + 1], base[D + 1] = -0.0, 0.0  # u = -0.0
    words = sigma(P)
    y = ref.rotate((w - base).astype(F32), P, words).reshape(-1, D)
    assert (np.abs(y[0]) == ref.quantize(y, b)[2][0, m]).any()
    want = ref.compress(w, base, P, b, words, mode)
    assert want[2] == 0 and (P <= 2 * D or bits(want[1])[2] == 0)
    assert same(run_compress(w, base, P, b, mode), want)
    w[P - 1], base[P // 2] = np.inf, np.nan
    want = ref.compress(w, base, P, b, words, mode)
    assert want[2] == 2 and same(run_compress(w, base, P, b, mode), want)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("b", [2, 4])
@pytest.mark.parametrize("P", SHAPES)
def test_compress_random(P, b, mode):
    """Exponents over +-30 decades; a second HIP stream gives the same outputs."""
    rng = np.random.default_rng(20 * P + b)
    w, base = spread(rng, P), spread(rng, P)
    want = ref.compress(w, base, P, b, sigma(P), mode)
    got = run_compress(w, base, P, b, mode)
    assert same(got, want) and got[2] == 0 and np.all(got[1] > 0)
    assert same(run_compress(w, base, P, b, mode, stream=torch.cuda.Stream(_dev())), got)


@pytest.mark.parametrize("K", [1, 2, TILE + 1])
@pytest.mark.parametrize("b", [2, 4])
@pytest.mark.parametrize("P", SHAPES)
def test_fedavg(P, b, K):
    """Random code words (every field is a level), pitches above the rows, unequal weights with
    an odd total, a client whose scales are all zero; then a larger ldc on a second stream."""
    from distributed_learning_simulator_amd import _native
    rng = np.random.default_rng(100 * P + 10 * b + K)
    NB, nw = ref.blocks(P), words_of(P, b)
    base = (rng.standard_normal(P) * 0.1).astype(F32)
    rows = rng.integers(0, 2 ** 32, (K, nw + 7), dtype=np.uint64).astype(np.uint32)
    scales = (rng.random((K, NB + 5)) * 10.0 ** rng.uniform(-6, 0, (K, NB + 5))).astype(F32)
    scales[K // 2] = 0.0
    ns = [int(n) for n in rng.integers(100, 1001, K)]
    ns[0] += sum(ns) % 2 == 0 and 1  # an odd total
    want = ref.fedavg(base, [(rows[i, :nw], scales[i]) for i in range(K)], ns, P, b, sigma(P))
    ts, tn = _t(scales), torch.tensor([float(n) for n in ns], device=_dev())
    for pad, stream in ((0, None), (9, torch.cuda.Stream(_dev()))):
        tc = _t(np.pad(rows, ((0, 0), (0, pad))).view(np.int32))
        out = torch.full((P + 64,), 7.0, device=_dev())
        torch.cuda.synchronize()
        with torch.cuda.stream(stream or torch.cuda.current_stream()):
            _native.eden_fedavg(_t(base), tc[:, :nw + 1], ts[:, :NB + 1], tn, float(sum(ns)), P, b,
                                SEED, ROUND, out, stream=stream)
        torch.cuda.synchronize()
        out = out.cpu().numpy()
        assert np.array_equal(bits(out[:P]), bits(want)) and np.all(out[P:] == 7.0)


@pytest.mark.parametrize("b", [2, 4])
@pytest.mark.parametrize("scale", MODES)
def test_three_workers_two_rounds(scale, b):
    """Through FedEDENWorker / FedEDENServer on the device: every payload and both broadcast
    models are the reference's; a payload of another width is refused."""
    from distributed_learning_simulator_amd.servers.fed_eden_server import FedEDENServer
    from distributed_learning_simulator_amd.workers.fed_eden_worker import FedEDENWorker
    dev, ns, mode = _dev(), {0: 300, 1: 120, 2: 777}, MODES.index(scale)
    server = FedEDENServer(bits=b, seed=SEED, initial_model=initial_model(), tester=None,
                           worker_number=3, synchronous=True, device=dev)
    workers = {i: FedEDENWorker(bits=b, seed=SEED, scale=scale, worker_id=i,
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
            sent[i] = ref.compress(w, prev, P, b, words, mode)[:2]
            up = workers[i].eden_update(rnd)
            assert np.array_equal(up.codes.cpu().numpy().view(np.uint32), sent[i][0])
            assert np.array_equal(bits(up.scales.cpu().numpy()), bits(sent[i][1]))
            server.worker_data_queue.add_task((i, ns[i], up))
        want = ref.fedavg(prev, [sent[i] for i in order], [ns[i] for i in order], P, b, words)
        for i in order:
            model = server.worker_data_queue.get_result(consumer=i)
            got = lay.flatten(model, device=dev).cpu().numpy()
            assert np.array_equal(bits(got)[real], bits(want)[real]) and not got[~real].any()
            workers[i].load_model(model)
    nbytes = 4 * words_of(P, b) + 4 * ref.blocks(P)
    assert server.round == 2 and server.payload_bytes[0] == {i: nbytes for i in order}
    workers[0].bits = 6 - b
    with pytest.raises(ValueError, match="the server decodes"):
        server.worker_data_queue.add_task((0, ns[0], workers[0].eden_update(3)))
    assert not server._payloads
