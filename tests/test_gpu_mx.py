"""GPU: dls_mx_compress_f32 and dls_mx_fedavg_f32 against tests/mx_ref.py bit for bit and
against fp64; FedMXWorker and FedMXServer on the device.

The decode bounds are the formats' own and exact: with q the grid step at t = |u| 2^-e the
decode is one of the two grid points around t, so |dec - u| <= q 2^e / 2 under nearest and < q
2^e under stochastic rounding; no measured tolerance enters."""
import numpy as np
import pytest
import torch

from tests import dp_ref, mx_ref as ref
from tests.test_gpu_drive import bits as u32, spread
from tests.test_topk_host import FakeTrainer, initial_model, make_model

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
SHAPES = [64, 512, 576, 3 * 512 - 64]  # two blocks, one group, a nearly empty 2nd, a ragged 3rd
SEED, SID = 0x1234567890ABCDEF, (3 << 32) + 5
FORMATS, ROUNDINGS = list(ref.FORMATS), ["nearest", "stochastic"]


def _dev():
    return torch.device("cuda", 0)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def words(P, seed=SEED, sid=SID):
    return dp_ref.words(512 * ref.groups(P), seed, sid)


def run_compress(w, base, r, P, fmt, rounding, seed=SEED, sid=SID, stream=None):
    """(codes uint32, scale bytes, r' or None, stats[0]) with canaries past every output."""
    from distributed_learning_simulator_amd import _native
    nw, ns = _native.mx_code_words(P, fmt), _native.mx_scale_bytes(P)
    assert (nw, ns) == (ref.groups(P) * 16 * ref.FORMATS[fmt][3], 16 * ref.groups(P))
    codes = torch.full((nw + 4,), -3, dtype=torch.int32, device=_dev())
    scales = torch.full((ns + 16,), 77, dtype=torch.uint8, device=_dev())
    stats = torch.full((4,), -1, dtype=torch.int32, device=_dev())
    res = None if r is None else torch.cat([_t(r[:P]), torch.full((4,), 7.0, device=_dev())])
    tw, tb = _t(w), _t(base)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream or torch.cuda.current_stream()):
        _native.mx_compress(tw, tb, res, P, fmt, rounding, seed, sid, codes, scales, stats, stream=stream)
    torch.cuda.synchronize()
    assert codes[nw:].tolist() == [-3] * 4 and scales[ns:].tolist() == [77] * 16
    assert stats[1:].tolist() == [-1] * 3 and (res is None or res[P:].tolist() == [7.0] * 4)
    return (codes[:nw].cpu().numpy().view(np.uint32), scales[:ns].cpu().numpy(),
            None if res is None else res[:P].cpu().numpy(), int(stats[0]))


def real_step(u, sb, P, fmt):
    """fp64 q 2^e per coordinate: the grid step at t = |u| 2^-e in the units of u."""
    e = np.repeat(sb.astype(np.int64) - 127, 32)[:P]
    return np.ldexp(ref.step(np.ldexp(np.abs(u.astype(F64)), -e), fmt), e)


def within_bound(codes, sb, u, P, fmt, rounding):
    err, q = np.abs(ref.decode(codes, sb, P, fmt) - u.astype(F64)), real_step(u, sb, P, fmt)
    return bool(np.all(err <= q / 2) if rounding == "nearest" else np.all(err < q))


def edge_inputs(rng, P, fmt):
    """(w, base, r): +-30 decades and zeros of both signs; block 0 has a maximum of exactly fmax
    2^5, u = -0.0, every tie between neighbouring codes and values below half the least step;
    block 1 is denormal; from P = 512 on block 2 is all zero and block 3 has its maximum one ulp
    above fmax 2^-3."""
    M, _, emin, _, fmax = ref.FORMATS[fmt]
    w, base, r = spread(rng, P), spread(rng, P), spread(rng, P)
    z = rng.random(P) < 0.1
    w[z], base[z] = rng.choice(np.array([0.0, -0.0], F32), (2, int(z.sum())))
    grid = ref.value(np.arange(2 ** (ref.FORMATS[fmt][3] - 1) - (1 if fmt == "e4m3" else 4 if fmt == "e5m2" else 0)), fmt)
    ties = rng.choice((grid[:-1] + grid[1:]) / 2, 24)
    b0 = np.concatenate([[fmax, -0.0], ties, 2.0 ** (emin - M) * np.array([0.49, -0.3, 0.5, 2.0 ** -30, -0.51, 0.75])])
    w[:32], w[32:64] = 32.0 * b0, rng.integers(-2 ** 23, 2 ** 23, 32) * 2.0 ** -149
    w[1] = -0.0
    base[:64], r[:64] = 0.0, -0.0
    if P >= 512:
        w[64:96] = base[64:96]
        r[64:96] = 0.0
        w[96:128], base[96:128], r[96:128] = rng.standard_normal(32) / 64, 0.0, -0.0
        w[100] = np.nextafter(F32(fmax / 8), F32(np.inf))
    return w, base, r


@pytest.mark.parametrize("feedback", [False, True])
@pytest.mark.parametrize("rounding", ROUNDINGS)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("P", SHAPES)
def test_compress(P, fmt, rounding, feedback):
    """Codes, scale bytes, r' and stats are the reference's bits on edge_inputs; every decode is
    within the format's bound; stochastic: another seed or stream id gives other codes, nearest:
    the seed is ignored; a NaN and an infinity are counted, their blocks carry byte 255 and zero
    codes."""
    rng = np.random.default_rng(1000 * P + 10 * FORMATS.index(fmt) + 2 * ROUNDINGS.index(rounding) + feedback)
    w, base, r = edge_inputs(rng, P, fmt)
    r = r if feedback else None
    rd = ROUNDINGS.index(rounding)
    u = (w - base).astype(F32) if r is None else ((w - base).astype(F32) + r).astype(F32)
    want = ref.compress(w, base, r, P, fmt, rd, words(P))
    got = run_compress(w, base, r, P, fmt, rounding)
    assert u32(u)[1] == 0x80000000 and want[1][0] == 127 + 5 and want[1][1] == 0
    assert P < 512 or (want[1][2] == 0 and want[1][3] == 127 - 2 and not ref.unpack(want[0], fmt)[64:96].any())
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert got[3] == want[3] == 0 and (r is None or np.array_equal(u32(got[2]), u32(want[2])))
    assert within_bound(want[0], want[1], u, P, fmt, rounding)  # the inputs' condition
    assert within_bound(got[0], got[1], u, P, fmt, rounding)
    m, zero = rng.standard_normal(P).astype(F32), np.zeros(P, F32)  # one decade: every f matters
    codes = run_compress(m, zero, None, P, fmt, rounding)[0]
    assert np.array_equal(codes, ref.compress(m, zero, None, P, fmt, rd, words(P))[0])
    other = [run_compress(m, zero, None, P, fmt, rounding, seed=SEED + 1)[0],
             run_compress(m, zero, None, P, fmt, rounding, sid=SID + 1)[0]]
    assert all(np.array_equal(codes, o) == (rounding == "nearest") for o in other)
    w[0], base[P - 1] = np.inf, np.nan
    want = ref.compress(w, base, r, P, fmt, rd, words(P))
    got = run_compress(w, base, r, P, fmt, rounding, stream=torch.cuda.Stream(_dev()))
    assert got[3] == want[3] == 2 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert got[1][0] == 255 == got[1][P // 32 - 1] and not ref.unpack(got[0], fmt)[:32].any()
    assert r is None or np.array_equal(u32(got[2])[32:P - 32], u32(want[2])[32:P - 32])


def run_fedavg(base, rows, ns, P, fmt, stream=None):
    """out [P + 64] (canary 7.0) over pitches above the rows' lengths."""
    from distributed_learning_simulator_amd import _native
    K, nw, nsb = len(rows), rows[0][0].size, rows[0][1].size
    codes = torch.full((K, nw + 8), -3, dtype=torch.int32, device=_dev())
    scales = torch.full((K, nsb + 32), 200, dtype=torch.uint8, device=_dev())
    codes[:, :nw], scales[:, :nsb] = _t(np.stack([r[0] for r in rows]).view(np.int32)), _t(np.stack([r[1] for r in rows]))
    out = torch.full((P + 64,), 7.0, device=_dev())
    torch.cuda.synchronize()
    with torch.cuda.stream(stream or torch.cuda.current_stream()):
        _native.mx_fedavg(_t(base), codes[:, :nw + 4], scales[:, :nsb + 16],
                          torch.tensor([float(n) for n in ns], device=_dev()), float(sum(ns)), P, fmt,
                          out, stream=stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("fmt", FORMATS)
def test_on_grid(fmt):
    """Inputs on the element grid decode to themselves under both roundings and any seed, with r'
    == 0; K = 4 equal weights: every product and sum is exact, out is the fp64 base + mean
    rounded once."""
    P, rng, bits = 576, np.random.default_rng(FORMATS.index(fmt)), ref.FORMATS[fmt][3]
    top = 2 ** (bits - 1) - (1 if fmt == "e4m3" else 4 if fmt == "e5m2" else 0)  # codes 0 .. fmax's
    scale = np.repeat(np.array([2.0 ** -10, 2.0 ** 3], F64), 512)[:P]
    base, rows, us = rng.standard_normal(P).astype(F32), [], []
    for i in range(4):
        mag = rng.integers(max(0, top - (16 << ref.FORMATS[fmt][0])), top, P)  # 16 binades: sums stay exact
        mag[[0, 520]] = top - 1  # fmax in a block of either group: e is the scale's
        w = (ref.value(mag, fmt) * scale * np.where(mag % 2, -1.0, 1.0)).astype(F32)  # no -0.0: u = w + 0.0 loses it
        got = run_compress(w, np.zeros(P, F32), np.zeros(P, F32), P, fmt, ROUNDINGS[i % 2], seed=i)
        assert np.array_equal(u32(ref.decode(got[0], got[1], P, fmt).astype(F32)), u32(w)) and not got[2].any()
        rows.append(got[:2])
        us.append(w.astype(F64))
    out = run_fedavg(base, rows, [300] * 4, P, fmt)
    assert np.array_equal(u32(out[:P]), u32((base.astype(F64) + sum(us) / 4).astype(F32)))


@pytest.mark.parametrize("fmt", FORMATS)
def test_unbiased(fmt):
    """Over R = 256 stream ids the mean decode is within 6 q / (2 sqrt(R)) of u per coordinate, q
    that coordinate's step: one decode follows a two-point law of standard deviation <= q / 2.
    tests/mx_ref.py on the same seeds stays inside the bound first."""
    P, R = 512, 256
    rng = np.random.default_rng(7)
    base = rng.standard_normal(P).astype(F32)
    w = (base + 0.01 * rng.standard_normal(P)).astype(F32)
    u, mean, rmean = (w - base).astype(F32), np.zeros(P), np.zeros(P)
    for sid in range(R):
        codes, sb, _, _ = run_compress(w, base, None, P, fmt, "stochastic", seed=11, sid=sid)
        mean += ref.decode(codes, sb, P, fmt) / R
        rmean += ref.decode(*ref.compress(w, base, None, P, fmt, 1, words(P, 11, sid))[:2], P, fmt) / R
    bound = 6.0 * real_step(u, sb, P, fmt) / (2.0 * np.sqrt(R))
    assert np.all(np.abs(rmean - u.astype(F64)) <= bound) and np.all(np.abs(mean - u.astype(F64)) <= bound)


def fedavg_bound(base, rows, us, ns, P, fmt):
    """sum_i (n_i / N) step_i + K 2^-23 (|base| + sum_i |p_i|): the clients' decode bounds through
    the weighted mean, and the roundings of the chain."""
    N = float(sum(ns))
    quant = sum(n / N * real_step(u, sb, P, fmt) for (_, sb), u, n in zip(rows, us, ns))
    p = sum(n / N * np.abs(ref.decode(c, sb, P, fmt)) for (c, sb), n in zip(rows, ns))
    return quant + len(ns) * 2.0 ** -23 * (np.abs(base) + p)


@pytest.mark.parametrize("K", [1, 3, 65])
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("P", SHAPES)
def test_fedavg(P, fmt, K):
    """The device's own payloads of K true updates (test_compress pins them), pitches above the
    rows' lengths, unequal weights: out is the reference chain's bits, out[P:] is untouched, the
    bits are the same on a second HIP stream, and the result is within fedavg_bound of the fp64
    mean of the true updates."""
    rng = np.random.default_rng(100 * P + 10 * FORMATS.index(fmt) + K)
    base = (0.1 * rng.standard_normal(P)).astype(F32)
    ws = [(base + 0.01 * rng.standard_normal(P) * 10.0 ** rng.uniform(-3, 0, P)).astype(F32) for _ in range(K)]
    ns = [int(n) for n in rng.integers(100, 1001, K)]
    rows = [run_compress(w, base, None, P, fmt, ROUNDINGS[i % 2], sid=i)[:2] for i, w in enumerate(ws)]
    want = ref.fedavg(base, rows, ns, P, fmt)
    for stream in (None, torch.cuda.Stream(_dev())):
        out = run_fedavg(base, rows, ns, P, fmt, stream)
        assert np.array_equal(u32(out[:P]), u32(want)) and np.all(out[P:] == 7.0)
    us = [(w - base).astype(F32) for w in ws]
    true = base.astype(F64) + sum(n / sum(ns) * u.astype(F64) for u, n in zip(us, ns))
    assert np.all(np.abs(out[:P] - true) <= fedavg_bound(base, rows, us, ns, P, fmt))


@pytest.mark.parametrize("fmt", FORMATS)
def test_error_feedback(fmt):
    """Nearest rounding, 4 rounds of a fixed update: after every round the codes and the residual
    are the reference's bits, so the decodes sent so far plus the residual are the reference's;
    without a residual operand a buffer beside the inputs is never touched (run_compress's
    canaries) and the codes are those of r = 0."""
    P, rng = 576, np.random.default_rng(5)
    base = rng.standard_normal(P).astype(F32)
    w = (base + 0.01 * rng.standard_normal(P)).astype(F32)
    r, rr, sent, sum_ref = np.zeros(P, F32), np.zeros(P, F32), np.zeros(P), np.zeros(P)
    for _ in range(4):
        codes, sb, r, _ = run_compress(w, base, r, P, fmt, "nearest")
        wc, wsb, rr, _ = ref.compress(w, base, rr, P, fmt, 0, None)
        assert np.array_equal(codes, wc) and np.array_equal(sb, wsb) and np.array_equal(u32(r), u32(rr))
        sent += ref.decode(codes, sb, P, fmt)
        sum_ref += ref.decode(wc, wsb, P, fmt)
    assert r.any() and np.array_equal(sent + r, sum_ref + rr)
    assert np.array_equal(run_compress(w, base, None, P, fmt, "nearest")[0], ref.compress(w, base, None, P, fmt, 0, None)[0])


@pytest.mark.parametrize("fmt", FORMATS)
def test_one_round(fmt):
    """Through factory.get_worker / get_server("fed_mx") on the device: the payload sizes, the
    new model within fedavg_bound of the dense FedAvg of the same updates, the empty subset."""
    from distributed_learning_simulator_amd import factory
    dev, ns = _dev(), {0: 300, 1: 120, 2: 777}
    server = factory.get_server("fed_mx", sharded=False, format=fmt, initial_model=initial_model(),
                                tester=None, worker_number=3, synchronous=True, device=dev)
    workers = {i: factory.get_worker("fed_mx", format=fmt, rounding=ROUNDINGS[i % 2], seed=SEED, worker_id=i,
                                     trainer=FakeTrainer(make_model(10 + i).to(dev), ns[i]),
                                     worker_data_queue=server.worker_data_queue, round=1)
               for i in range(3)}
    for i, wk in workers.items():
        wk.load_model(server.worker_data_queue.get_result(consumer=i))
    lay = server.layout
    P = lay.P
    prev = lay.flatten(server.prev_model, device=dev).cpu().numpy()
    assert server.get_subset_model([]) is server.prev_model
    g, order, rows, us = torch.Generator().manual_seed(4), [2, 0, 1], [], []
    for i in order:
        with torch.no_grad():
            for p in workers[i].trainer.model.parameters():
                p += (0.05 * torch.randn(p.shape, generator=g)).to(dev)
        w = lay.flatten(dict(workers[i].trainer.model.named_parameters()), device=dev).cpu().numpy()
        up = workers[i].mx_update(1)
        rows.append((up.codes.cpu().numpy().view(np.uint32), up.scales.cpu().numpy()))
        us.append((w - prev).astype(F32))
        server.worker_data_queue.add_task((i, ns[i], up))
    got = lay.flatten(server.worker_data_queue.get_result(consumer=0), device=dev).cpu().numpy()
    weights = [ns[i] for i in order]
    dense = prev.astype(F64) + sum(n / sum(weights) * u.astype(F64) for n, u in zip(weights, us))
    real = np.zeros(P, bool)  # the layout's padding slots are decoded too, and dropped
    for a, n in zip(lay.offsets, lay.numels):
        real[a:a + n] = True
    assert np.all((np.abs(got - dense) <= fedavg_bound(prev, rows, us, weights, P, fmt))[real])
    padded = ref.groups(P) * (64 * ref.FORMATS[fmt][3] + 16)  # P b / 8 + P / 32 before padding
    assert server.round == 1 and server.payload_bytes[0] == {i: padded for i in order}
    assert padded >= P * ref.FORMATS[fmt][3] // 8 + P // 32 > padded - (64 * ref.FORMATS[fmt][3] + 16)
