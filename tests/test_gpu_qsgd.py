"""GPU: dls_qsgd_compress_f32 and dls_qsgd_fedavg_f32 against tests/qsgd_ref.py bit for bit
and against fp64; FedQSGDWorker and FedQSGDServer on the device.

The decode bound |q d - u| <= d (1 + 2^-20).  With a = |u| <= n, r = (s / n)(1 + e1), d = (n /
s)(1 + e2), t = a r (1 + e3), |e| <= 2^-24: l is floor(t) or floor(t) + 1 (or s where t >= s,
and then t - s < 1), so q d - u = +-((l - t) d + (t d - a)), |l - t| <= 1 and |t d - a| <= 3.01 s
2^-24 d.  That term, r against 1 / d, is the slack: below 2^-20 d at s = 1; at s = 7 and 127 it
can reach 2^-19.6 d and 2^-15.4 d, but only beside |l - t| > 1 - 2^-15, i.e. f within 2^-15 of
an integer and xi on its far side (about 10^-9 per coordinate).  The seeds are fixed and the
tests first require the bound of the reference's own codes: a condition on the inputs."""
import numpy as np
import pytest
import torch

from tests import dp_ref, qsgd_ref as ref
from tests.test_gpu_drive import bits as u32, spread
from tests.test_topk_host import FakeTrainer, initial_model, make_model

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SHAPES = [64, 512, 576, 3 * 512 - 64]  # a sliver, one bucket, a nearly empty 2nd, a ragged 3rd
SEED, SID = 0x1234567890ABCDEF, (3 << 32) + 5
NORMS = ["max", "l2"]


def _dev():
    return torch.device("cuda", 0)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def words(P, seed=SEED, sid=SID):
    return dp_ref.words(512 * ref.buckets(P), seed, sid)


def run_compress(w, base, P, bits, norm, seed=SEED, sid=SID, stream=None):
    """(codes uint32, scales, stats[0]) with canaries past every output."""
    from distributed_learning_simulator_amd import _native
    assert (_native.QSGD_BUCKET, _native.QSGD_CLIENT_TILE) == (ref.BUCKET, 64)
    NB, nw = ref.buckets(P), _native.qsgd_code_words(P, bits)
    codes = torch.full((nw + 4,), -3, dtype=torch.int32, device=_dev())
    scales = torch.full((NB + 4,), -1.0, device=_dev())
    stats = torch.full((4,), -1, dtype=torch.int32, device=_dev())
    tw, tb = _t(w), _t(base)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream or torch.cuda.current_stream()):
        _native.qsgd_compress(tw, tb, P, bits, norm, seed, sid, codes, scales, stats, stream=stream)
    torch.cuda.synchronize()
    assert codes[nw:].tolist() == [-3] * 4 and scales[NB:].tolist() == [-1.0] * 4
    assert stats[1:].tolist() == [-1] * 3
    return codes[:nw].cpu().numpy().view(np.uint32), scales[:NB].cpu().numpy(), int(stats[0])


def within_decode_bound(codes, d, u, P, bits):
    err = np.abs(ref.decode(codes, d, P, bits) - u.astype(F64))
    return bool(np.all(err <= np.repeat(d.astype(F64), 512)[:P] * (1 + 2.0 ** -20)))


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("bits", [2, 4, 8])
@pytest.mark.parametrize("P", SHAPES)
def test_compress(P, bits, norm):
    """Codes, scales and stats are the reference's bits: inputs over +-30 decades, zeros of both
    signs, u = -0.0, an all-zero last bucket where there is a second one; every decode within
    the bound; another seed or stream id gives other codes; a NaN and an inf are counted."""
    rng = np.random.default_rng(1000 * P + 10 * bits + NORMS.index(norm))
    w, base = spread(rng, P), spread(rng, P)
    z = rng.random(P) < 0.1
    w[z], base[z] = rng.choice(np.array([0.0, -0.0], F32), (2, int(z.sum())))
    w[1], base[1] = -0.0, 0.0  # u = -0.0
    if P > 512:
        w[512 * (ref.buckets(P) - 1):] = base[512 * (ref.buckets(P) - 1):]
    u = (w - base).astype(F32)
    want = ref.compress(w, base, P, bits, NORMS.index(norm), words(P))
    got = run_compress(w, base, P, bits, norm)
    assert u32(u)[1] == 0x80000000 and (P <= 512 or (want[1][-1] == 0 and not want[0][-16 * bits:].any()))
    assert np.array_equal(got[0], want[0]) and np.array_equal(u32(got[1]), u32(want[1]))
    assert got[2] == want[2] == 0 and want[0].any()
    assert within_decode_bound(want[0], want[1], u, P, bits)  # the inputs' condition
    assert within_decode_bound(got[0], got[1], u, P, bits)
    m, zero = rng.standard_normal(P).astype(F32), np.zeros(P, F32)  # one decade: every f matters
    codes = run_compress(m, zero, P, bits, norm)[0]
    assert np.array_equal(codes, ref.compress(m, zero, P, bits, NORMS.index(norm), words(P))[0])
    assert not np.array_equal(codes, run_compress(m, zero, P, bits, norm, seed=SEED + 1)[0])
    assert not np.array_equal(codes, run_compress(m, zero, P, bits, norm, sid=SID + 1)[0])
    w[0], base[P - 1] = np.inf, np.nan
    want = ref.compress(w, base, P, bits, NORMS.index(norm), words(P))
    got = run_compress(w, base, P, bits, norm, stream=torch.cuda.Stream(_dev()))
    assert got[2] == want[2] == 2 and np.array_equal(got[0], want[0])
    assert np.array_equal(got[1], want[1], equal_nan=True) and not np.isfinite(got[1]).all()


@pytest.mark.parametrize("norm", NORMS)
@pytest.mark.parametrize("bits", [2, 4, 8])
def test_unbiased(bits, norm):
    """Over R = 256 stream ids the mean decode is within 6 d / (2 sqrt(R)) of u per coordinate:
    one decode is l0 d or (l0 + 1) d, a two-point law of standard deviation <= d / 2, so the
    mean's is <= d / (2 sqrt(R)) and the bound is six of them (tests/qsgd_ref.py on the same
    seeds stays inside it; the grid of xi moves the mean by less than 2^-24 d)."""
    P, R = 512, 256
    rng = np.random.default_rng(7)
    base = rng.standard_normal(P).astype(F32)
    w = (base + 0.01 * rng.standard_normal(P)).astype(F32)
    u, mean = (w - base).astype(F32).astype(F64), np.zeros(P)
    for sid in range(R):
        codes, d, _ = run_compress(w, base, P, bits, norm, seed=11, sid=sid)
        mean += ref.decode(codes, d, P, bits) / R
    assert np.all(np.abs(mean - u) <= 6.0 * float(d[0]) / (2.0 * np.sqrt(R)))


@pytest.mark.parametrize("bits", [2, 4, 8])
def test_on_grid(bits):
    """u = q 2^e with max |q| = s under the max norm: d = 2^e, every f == 0, so the codes hold
    q whatever the seed, the decode is u, and with K = 4 equal weights c = 2^(e-2), every
    product and sum is exact and out is the fp64 base + mean rounded once."""
    from distributed_learning_simulator_amd import _native
    P, s, rng = 576, ref.levels(bits), np.random.default_rng(bits)
    e = np.repeat(np.array([2.0 ** -10, 2.0 ** 3], F32), 512)[:P]
    base = rng.standard_normal(P).astype(F32)
    rows, qs = [], []
    for i in range(4):
        q = rng.integers(-s, s + 1, P)
        q[[0, 520]] = s, -s
        w = (q * e).astype(F32)  # against a zero base: u = w
        got = run_compress(w, np.zeros(P, F32), P, bits, "max", seed=i)
        assert np.array_equal(got[0], run_compress(w, np.zeros(P, F32), P, bits, "max", seed=i + 9)[0])
        assert np.array_equal(ref.unpack(got[0], bits)[:P], q) and got[1].tolist() == [2.0 ** -10, 8.0]
        assert np.array_equal(u32(ref.decode(got[0], got[1], P, bits).astype(F32)), u32(w))
        rows.append(got)
        qs.append(q * e.astype(F64))
    out = torch.empty(P, device=_dev())
    _native.qsgd_fedavg(_t(base), _t(np.stack([r[0] for r in rows]).view(np.int32)),
                        _t(np.stack([r[1] for r in rows])), torch.full((4,), 300.0, device=_dev()),
                        1200.0, P, bits, out)
    assert np.array_equal(u32(out.cpu().numpy()), u32((base.astype(F64) + sum(qs) / 4).astype(F32)))


def fedavg_bound(base, rows, ns, P, bits):
    """sum_i (n_i / N) d_i[B] (1 + 2^-20) + K 2^-23 (|base| + sum_i |p_i|): the clients' decode
    bounds through the weighted mean, and one rounding of at most 2^-24 relative per operation
    of the chain (two per client: the product's factor c carries two more)."""
    N = float(sum(ns))
    dec = [n / N * ref.decode(c, d, P, bits) for (c, d), n in zip(rows, ns)]
    quant = sum(n / N * np.repeat(d.astype(F64), 512)[:P] for (_, d), n in zip(rows, ns))
    return quant * (1 + 2.0 ** -20) + len(ns) * 2.0 ** -23 * (np.abs(base) + sum(np.abs(x) for x in dec))


@pytest.mark.parametrize("K", [1, 3, 65])
@pytest.mark.parametrize("bits", [2, 4, 8])
@pytest.mark.parametrize("P", SHAPES)
def test_fedavg(P, bits, K):
    """The device's own payloads of K true updates (test_compress pins them), pitches above the
    rows' lengths, unequal weights: out is the reference chain's bits, out[P:] is untouched, the
    result is within fedavg_bound of the fp64 mean of the true updates and has the same bits on
    a second HIP stream."""
    from distributed_learning_simulator_amd import _native
    rng = np.random.default_rng(100 * P + 10 * bits + K)
    NB, nw = ref.buckets(P), ref.buckets(P) * 16 * bits
    base = (0.1 * rng.standard_normal(P)).astype(F32)
    ws = [(base + 0.01 * rng.standard_normal(P)).astype(F32) for _ in range(K)]
    ns = [int(n) for n in rng.integers(100, 1001, K)]
    rows = [run_compress(w, base, P, bits, "l2", sid=i)[:2] for i, w in enumerate(ws)]
    codes = torch.full((K, nw + 8), -3, dtype=torch.int32, device=_dev())
    scales = torch.full((K, NB + 5), -1.0, device=_dev())
    codes[:, :nw], scales[:, :NB] = _t(np.stack([r[0] for r in rows]).view(np.int32)), _t(np.stack([r[1] for r in rows]))
    want = ref.fedavg(base, rows, ns, P, bits)
    outs = []
    for stream in (None, torch.cuda.Stream(_dev())):
        out = torch.full((P + 64,), 7.0, device=_dev())
        torch.cuda.synchronize()
        with torch.cuda.stream(stream or torch.cuda.current_stream()):
            _native.qsgd_fedavg(_t(base), codes[:, :nw + 4], scales[:, :NB + 1],
                                torch.tensor([float(n) for n in ns], device=_dev()), float(sum(ns)),
                                P, bits, out, stream=stream)
        torch.cuda.synchronize()
        outs.append(out.cpu().numpy())
        assert np.array_equal(u32(outs[-1][:P]), u32(want)) and np.all(outs[-1][P:] == 7.0)
    true = base.astype(F64) + sum(n / sum(ns) * (w - base).astype(F32).astype(F64) for w, n in zip(ws, ns))
    assert np.all(np.abs(outs[0][:P] - true) <= fedavg_bound(base, rows, ns, P, bits))


@pytest.mark.parametrize("bits", [2, 4, 8])
def test_one_round(bits):
    """Through factory.get_worker / get_server("fed_qsgd") on the device: the payload sizes, the
    new model within fedavg_bound of the dense FedAvg of the same updates, the empty subset."""
    from distributed_learning_simulator_amd import factory
    dev, ns = _dev(), {0: 300, 1: 120, 2: 777}
    server = factory.get_server("fed_qsgd", sharded=False, bits=bits, initial_model=initial_model(),
                                tester=None, worker_number=3, synchronous=True, device=dev)
    workers = {i: factory.get_worker("fed_qsgd", bits=bits, norm="l2", seed=SEED, worker_id=i,
                                     trainer=FakeTrainer(make_model(10 + i).to(dev), ns[i]),
                                     worker_data_queue=server.worker_data_queue, round=1)
               for i in range(3)}
    for i, wk in workers.items():
        wk.load_model(server.worker_data_queue.get_result(consumer=i))
    lay = server.layout
    P, NB = lay.P, ref.buckets(lay.P)
    prev = lay.flatten(server.prev_model, device=dev).cpu().numpy()
    assert server.get_subset_model([]) is server.prev_model
    g, order, rows, us = torch.Generator().manual_seed(4), [2, 0, 1], [], []
    for i in order:
        with torch.no_grad():
            for p in workers[i].trainer.model.parameters():
                p += (0.05 * torch.randn(p.shape, generator=g)).to(dev)
        w = lay.flatten(dict(workers[i].trainer.model.named_parameters()), device=dev).cpu().numpy()
        up = workers[i].qsgd_update(1)
        rows.append((up.codes.cpu().numpy().view(np.uint32), up.scales.cpu().numpy()))
        us.append((w - prev).astype(F32).astype(F64))
        server.worker_data_queue.add_task((i, ns[i], up))
    got = lay.flatten(server.worker_data_queue.get_result(consumer=0), device=dev).cpu().numpy()
    weights = [ns[i] for i in order]
    dense = prev.astype(F64) + sum(n / sum(weights) * u for n, u in zip(weights, us))
    real = np.zeros(P, bool)  # the layout's padding slots are decoded too, and dropped
    for a, n in zip(lay.offsets, lay.numels):
        real[a:a + n] = True
    assert np.all((np.abs(got - dense) <= fedavg_bound(prev, rows, weights, P, bits))[real])
    assert server.round == 1 and server.payload_bytes[0] == {i: NB * 64 * bits + 4 * NB for i in order}
