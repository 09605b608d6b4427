"""GPU: dls_powersgd_compress_f32 and dls_powersgd_fedavg_f32 against tests/powersgd_ref.py with
the header's bounds, evaluated from the reference's fp64 |a||b| sums; exact inputs bit for bit;
FedPowerSGDWorker / FedPowerSGDServer and the simulator on the device."""
import math

import numpy as np
import pytest
import torch

from tests import powersgd_ref as ref
from tests.powersgd_ref import F32, U24, bits, g

pytestmark = pytest.mark.gpu

# not multiples of any tile; one full strip; (128, 1152): five 256-column chunks in the first
# pass and 72 strips of 16 columns in the last; (4, 4) is dense at every rank; vectors between
SHAPES = [(6, 25), (10,), (16, 150), (64,), (10, 512), (4, 4), (64, 576), (128, 1152)]
KAPPA_CAP = 10.0  # on the reference's P; a condition on the inputs (seeds checked on the CPU)
RANKS = [1, 4, 16]


def _dev():
    return torch.device("cuda", 0)


def _t(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(_dev())


def make_row(shapes, r, seed, slack=(2,)):
    """Gaussian w, base, e and Q0 over a row of ``shapes``: NaN in the padding of w and base,
    garbage in e's and in the parts of q0 that are no Q block."""
    rng = np.random.default_rng(seed)
    bounds, dims, kinds, blocks, L = ref.plan(shapes, r, slack)
    w = np.full(bounds[-1], np.nan, F32)
    base, e, q0 = w.copy(), np.full(bounds[-1], 7.0, F32), np.full(L, np.nan, F32)
    for a, (n, m), kind, (_, qoff) in zip(bounds, dims, kinds, blocks):
        w[a:a + n * m], base[a:a + n * m] = rng.standard_normal((2, n * m)).astype(F32)
        e[a:a + n * m] = (0.1 * rng.standard_normal(n * m)).astype(F32)
        if kind:
            q0[qoff:qoff + m * r] = rng.standard_normal(m * r).astype(F32)
    return w, base, e, q0, (bounds, dims, kinds, blocks, L)


def run_compress(w, base, e, q0, layout, r, stream=None):
    from distributed_learning_simulator_amd import _native
    assert (_native.POWERSGD_CHUNK, _native.POWERSGD_CLIENT_TILE) == (ref.CHUNK, ref.TILE)
    bounds, dims, kinds, blocks, L = layout
    plan = _native.powersgd_plan(bounds, dims, r, _dev())
    assert plan.L == L and [plan.kind(t) for t in range(plan.T)] == kinds
    assert [plan.blocks(t) for t in range(plan.T)] == blocks
    te = None if e is None else _t(e)
    payload = torch.full((L,), 5.0, device=_dev())
    stats = torch.full((1,), -1, dtype=torch.int32, device=_dev())
    ws = _native.powersgd_workspace(plan, _dev()).fill_(0xFF)
    _native.powersgd_compress(_t(w), _t(base), te, plan, _t(q0), payload, stats, ws, stream=stream)
    torch.cuda.synchronize()
    return payload.cpu().numpy(), None if e is None else te.cpu().numpy(), int(stats[0])


def factors(payload, layout, r, t):
    (n, m), (poff, qoff) = layout[1][t], layout[3][t]
    return payload[poff:poff + n * r].reshape(n, r), payload[qoff:qoff + m * r].reshape(m, r)


def check_invariants(U, Ph, Q, e_new, r):
    """What needs no conditioning: P^T P^ = I within 3u (each entry of P^ is rounded once,
    2u sum |p_i||p_j| <= 2u, the rest fp64 slack); Q against U^T P^ of the SAME P^ within
    g(n) |U|^T |P^|; e against u - P^ Q^T within g(r + 1) (|u| + |P^||Q|^T)."""
    n = U.shape[0]
    U64, P64, Q64 = U.astype(np.float64), Ph.astype(np.float64), Q.astype(np.float64)
    gram = P64.T @ P64
    live = np.diag(gram) > 0.5
    assert np.abs(gram - np.diag(live.astype(np.float64))).max() <= 3 * U24
    assert np.all(np.abs(Q64 - U64.T @ P64) <= g(n) * (np.abs(U64).T @ np.abs(P64)))
    if e_new is not None:
        bound = g(r + 1) * (np.abs(U64) + np.abs(P64) @ np.abs(Q64).T)
        assert np.all(np.abs(e_new - (U64 - P64 @ Q64.T)) <= bound)


@pytest.mark.parametrize("r", RANKS)
def test_compress_gaussian(r):
    """Against the reference: P^ within 2 kappa ||E||_F / ||P||_2 + u, E = g(min(m, chunk) + 1)
    |U||Q0| the first product's bound (first-order perturbation of the QR factor, Stewart
    1977, doubled for the higher orders; u the final rounding); then the invariants."""
    w, base, e, q0, layout = make_row(SHAPES, r, seed=r)
    bounds, dims, kinds, blocks, L = layout
    payload, e_new, bad = run_compress(w, base, e, q0, layout, r)
    assert bad == 0 and kinds[5] == int(r == 1) and sum(kinds) == {1: 6, 4: 5, 16: 2}[r]
    u = ref.update(w, base, e)
    for t, (a, (n, m), kind, (poff, qoff)) in enumerate(zip(bounds, dims, kinds, blocks)):
        pad = slice(a + n * m, bounds[t + 1])
        assert not bits(e_new[pad]).any()
        if not kind:
            assert np.array_equal(bits(payload[poff:poff + n * m]), bits(w[a:a + n * m]))
            assert not bits(e_new[a:a + n * m]).any()
            assert not bits(payload[poff + n * m:poff + ref.ru64(n * m)]).any()
            continue
        U, Q0 = u[a:a + n * m].reshape(n, m), q0[qoff:qoff + m * r].reshape(m, r)
        P, Ph_ref, _, _ = ref.compress_tensor(U, Q0)
        sv = np.linalg.svd(P, compute_uv=False)
        kappa = sv[0] / sv[-1]
        assert kappa < KAPPA_CAP
        E = g(min(m, ref.CHUNK) + 1) * (np.abs(U.astype(np.float64)) @ np.abs(Q0.astype(np.float64)))
        Ph, Q = factors(payload, layout, r, t)
        assert np.abs(Ph.astype(np.float64) - Ph_ref).max() <= 2 * kappa * np.linalg.norm(E) / sv[0] + U24
        check_invariants(U, Ph, Q, e_new[a:a + n * m].reshape(n, m).astype(np.float64), r)
        assert not bits(payload[poff + n * r:qoff]).any()


def hadamard(n):
    H = np.ones((1, 1))
    while H.shape[0] < n:
        H = np.block([[H, H], [H, -H]])
    return H


def exact_row(r, scale):
    """U = 2^scale x the first columns of the 16 x 16 and 64 x 64 Sylvester matrices with
    small-integer columns appended, Q0 = the first r columns of the identity: P's columns are
    orthogonal with a power-of-two norm, so P^, Q and e are exactly representable."""
    rng = np.random.default_rng(r)
    shapes = [(16, 40), (10,), (64, 100)]
    layout = ref.plan(shapes, r)
    bounds, dims, kinds, blocks, L = layout
    w, base = np.zeros(bounds[-1], F32), np.zeros(bounds[-1], F32)
    e, q0 = np.zeros(bounds[-1], F32), np.zeros(L, F32)
    for a, (n, m), kind, (_, qoff) in zip(bounds, dims, kinds, blocks):
        U = rng.integers(-3, 4, (n, m)).astype(np.float64)
        if m > 1:
            U[:, :n] = hadamard(n)
        base[a:a + n * m] = rng.integers(-4, 5, n * m)
        e[a:a + n * m] = rng.integers(-2, 3, n * m)
        w[a:a + n * m] = np.ldexp(U, scale).ravel() + base[a:a + n * m] - e[a:a + n * m]
        if kind:
            q0[qoff:qoff + m * r] = np.eye(m, r).ravel()
    return w, base, e, q0, layout


@pytest.mark.parametrize("r", RANKS)
def test_compress_exact_bit_for_bit(r):
    w, base, e, q0, layout = exact_row(r, scale=3)
    bounds, dims, kinds, blocks, L = layout
    payload, e_new, bad = run_compress(w, base, e, q0, layout, r)
    assert bad == 0 and kinds == [int(r < 16), 0, 1]
    u = ref.update(w, base, e)
    for t, (a, (n, m), kind) in enumerate(zip(bounds, dims, kinds)):
        if kind:
            U = u[a:a + n * m].reshape(n, m)
            _, Ph_ref, Q_ref, e_ref = ref.compress_tensor(U, np.eye(m, r, dtype=F32))
            Ph, Q = factors(payload, layout, r, t)
            assert np.array_equal(bits(Ph), bits(Ph_ref)) and np.abs(Ph).max() == 1 / math.sqrt(n)
            assert np.array_equal(bits(Q), bits(Q_ref.astype(F32)))
            assert np.array_equal(bits(e_new[a:a + n * m]), bits(e_ref.astype(F32).ravel()))


def run_fedavg(base, payloads, layout, r, ns, pitch_extra=4):
    from distributed_learning_simulator_amd import _native
    bounds, dims, _, _, L = layout
    plan = _native.powersgd_plan(bounds, dims, r, _dev())
    wide = np.full((len(ns), L + pitch_extra), np.nan, F32)
    wide[:, :L] = payloads
    out = torch.full((bounds[-1],), 7.0, device=_dev())
    _native.powersgd_fedavg(_t(base), _t(wide)[:, :L], plan, _t(np.array(ns, F32)),
                            float(sum(ns)), out)
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("kind", ["gauss", "exact"])
@pytest.mark.parametrize("K", [1, 3, ref.TILE + 1])
@pytest.mark.parametrize("r", RANKS)
def test_fedavg(r, K, kind):
    """gauss: every real coordinate within g(K r + 1) (|base| + sum |A||Q|); exact: dyadic
    factors and power-of-two weights, every product and partial sum representable, bit for
    bit.  Dense tensors: the bits of dls_fedavg_f32 on the sent values; padding: base's bits."""
    from distributed_learning_simulator_amd import _native
    rng = np.random.default_rng(100 * r + K)
    layout = ref.plan(SHAPES, r, (2,))
    bounds, dims, kinds, blocks, L = layout
    if kind == "gauss":
        ns = [int(n) for n in rng.integers(100, 1001, K)]
        base = rng.standard_normal(bounds[-1]).astype(F32)
        payloads = rng.standard_normal((K, L)).astype(F32)
    else:
        ns = [4] if K == 1 else [1] * (K - 1) + [K - 1]  # the total is a power of two
        base = (rng.integers(-16, 17, bounds[-1]) / 4).astype(F32)
        payloads = np.where(rng.random((K, L)) < 0.5, rng.integers(-8, 9, (K, L)),
                            rng.choice([0.25, -0.125, 0.0], (K, L))).astype(F32)
        for (n, m), k, (poff, qoff) in zip(dims, kinds, blocks):
            if k:  # P^ blocks dyadic fractions, Q blocks small integers
                payloads[:, poff:qoff] = rng.choice([0.25, -0.25, 0.125, -0.125, 0.0], (K, qoff - poff))
                payloads[:, qoff:qoff + m * r] = rng.integers(-8, 9, (K, m * r))
    real = np.zeros(bounds[-1], bool)
    for a, (n, m) in zip(bounds, dims):
        real[a:a + n * m] = True
    base[~real] = F32(-0.0)
    out = run_fedavg(base, payloads, layout, r, ns)
    for t, (a, (n, m), k, (poff, qoff)) in enumerate(zip(bounds, dims, kinds, blocks)):
        got = out[a:a + n * m]
        if not k:
            sent = payloads[:, poff:poff + ref.ru64(n * m)]
            want = torch.empty(sent.shape[1], device=_dev())
            _native.fedavg(_t(sent), torch.arange(K, dtype=torch.int32, device=_dev()),
                           _t(np.array(ns, F32)), float(sum(ns)), sent.shape[1], want)
            assert np.array_equal(bits(got), bits(want.cpu().numpy()[:n * m]))
            continue
        Phs = [p[poff:poff + n * r].reshape(n, r) for p in payloads]
        Qs = [p[qoff:qoff + m * r].reshape(m, r) for p in payloads]
        want, mag = ref.server_tensor(base[a:a + n * m].reshape(n, m), Phs, Qs, ns)
        if kind == "exact":
            assert np.array_equal(bits(got), bits(want.astype(F32).ravel()))
        else:
            assert np.all(np.abs(got.reshape(n, m) - want) <= g(K * r + 1) * mag)
    assert np.array_equal(bits(out[~real]), bits(base[~real])) and (~real).sum() > 64


def test_edges():
    """An all-zero tensor: zero columns, no NaN, e = u; two equal columns of Q0: the second
    column of P^ (and of Q) is zero, exactly, on exactly representable inputs; one inf in w is
    counted and stays inside its tensor; e == NULL writes nothing back and Q is formed from
    fl(w - base)."""
    r = 4
    w, base, e, q0, layout = exact_row(r, scale=0)
    bounds, dims, kinds, blocks, L = layout
    (a0, a2), ((n0, m0), _, (n2, m2)) = (bounds[0], bounds[2]), dims
    w[a0:a0 + n0 * m0], base[a0:a0 + n0 * m0], e[a0:a0 + n0 * m0] = 0.0, 0.0, 0.0
    q2 = q0[blocks[2][1]:blocks[2][1] + m2 * r].reshape(m2, r)
    q2[:, 1] = q2[:, 0]
    payload, e_new, bad = run_compress(w, base, e, q0, layout, r)
    assert bad == 0 and not np.isnan(payload).any() and not np.isnan(e_new).any()
    Ph0, Q0_ = factors(payload, layout, r, 0)
    assert not bits(Ph0).any() and not bits(Q0_).any() and not e_new[a0:a0 + n0 * m0].any()
    Ph2, Q2 = factors(payload, layout, r, 2)
    assert not bits(Ph2[:, 1]).any() and not bits(Q2[:, 1]).any() and Ph2[:, [0, 2, 3]].all()
    u = ref.update(w, base, e)
    check_invariants(u[a2:a2 + n2 * m2].reshape(n2, m2), Ph2, Q2,
                     e_new[a2:a2 + n2 * m2].reshape(n2, m2).astype(np.float64), r)
    # one inf
    w, base, e, q0, layout = make_row(SHAPES, r, seed=9)
    clean = run_compress(w, base, e, q0, layout, r)
    w[layout[0][4] + 700] = np.inf
    payload, e_new, bad = run_compress(w, base, e, q0, layout, r)
    lo, hi = layout[0][4], layout[0][5]
    keep = np.r_[0:lo, hi:layout[0][-1]]
    assert bad == 1 and np.array_equal(bits(e_new[keep]), bits(clean[1][keep]))
    others = np.ones(layout[4], bool)
    others[layout[3][4][0]:layout[3][5][0]] = False
    assert np.array_equal(bits(payload[others]), bits(clean[0][others]))
    # e == NULL
    w[lo + 700] = 1.0
    payload, none, bad = run_compress(w, base, None, q0, layout, r)
    assert none is None and bad == 0
    n, m = layout[1][7]
    U = ref.update(w, base)[layout[0][7]:layout[0][7] + n * m].reshape(n, m)
    check_invariants(U, *factors(payload, layout, r, 7), None, r)


def test_launch_geometry_independence():
    """The same tensors at other offsets in a row of another T, and on another stream: the
    same bits of P^, Q and e."""
    r = 4
    perm = [7, 0, 4, 6]
    w, base, e, q0, A = make_row(SHAPES, r, seed=3)
    got_a = run_compress(w, base, e, q0, A, r)
    B = ref.plan([(3, 3)] + [SHAPES[t] for t in perm], r, ())
    wb, bb, eb = (np.zeros(B[0][-1], F32) for _ in range(3))
    qb = np.zeros(B[4], F32)
    for tb, ta in enumerate(perm, start=1):
        n, m = A[1][ta]
        for dst, src in ((wb, w), (bb, base), (eb, e)):
            dst[B[0][tb]:B[0][tb] + n * m] = src[A[0][ta]:A[0][ta] + n * m]
        qb[B[3][tb][1]:B[3][tb][1] + m * r] = q0[A[3][ta][1]:A[3][ta][1] + m * r]
    got_b = run_compress(wb, bb, eb, qb, B, r, stream=torch.cuda.Stream(_dev()))
    for tb, ta in enumerate(perm, start=1):
        n, m = A[1][ta]
        for fa, fb in zip(factors(got_a[0], A, r, ta), factors(got_b[0], B, r, tb)):
            assert np.array_equal(bits(fa), bits(fb))
        assert np.array_equal(bits(got_a[1][A[0][ta]:A[0][ta] + n * m]),
                              bits(got_b[1][B[0][tb]:B[0][tb] + n * m]))


def test_workers_and_server_dense_rank_equals_fedavg():
    """Through FedPowerSGDWorker / FedPowerSGDServer at a rank at which every tensor of the
    model falls to dense: the round's model has the bits of dls_fedavg_f32 on the workers'
    models (LeNet-5's 120 x 400 layer is compressed at every rank up to 16, so this runs on
    the host tests' small model)."""
    from distributed_learning_simulator_amd import _native
    from distributed_learning_simulator_amd.servers.fed_powersgd_server import FedPowerSGDServer
    from distributed_learning_simulator_amd.workers.fed_powersgd_worker import FedPowerSGDWorker
    from tests.test_topk_host import FakeTrainer, initial_model, make_model
    dev, ns = _dev(), {0: 300, 1: 120, 2: 777}
    server = FedPowerSGDServer(initial_model=initial_model(), tester=None, worker_number=3,
                               synchronous=True, device=dev, rank=16)
    workers = {i: FedPowerSGDWorker(worker_id=i, trainer=FakeTrainer(make_model(10 + i).to(dev), ns[i]),
                                    worker_data_queue=server.worker_data_queue, round=1, rank=16)
               for i in range(3)}
    lay = server.layout
    rows = []
    for i in (2, 0, 1):
        workers[i].load_model(server.worker_data_queue.get_result(consumer=i))
        with torch.no_grad():
            for p in workers[i].trainer.model.parameters():
                p += 0.05 * (i + 1)
        rows.append(lay.flatten(dict(workers[i].trainer.model.named_parameters()), device=dev))
        up = workers[i].lowrank_update()
        assert not any(workers[i].plan.kind(t) for t in range(len(lay))) and up.floats == lay.numel
        server.worker_data_queue.add_task((i, ns[i], up))
    want = torch.empty(lay.P, device=dev)
    _native.fedavg(torch.stack(rows), torch.arange(3, dtype=torch.int32, device=dev),
                   torch.tensor([777.0, 300.0, 120.0], device=dev), 1197.0, lay.P, want)
    got = lay.flatten(server.worker_data_queue.get_result(consumer=0), device=dev)
    real = torch.zeros(lay.P, dtype=torch.bool, device=dev)
    for o, k in zip(lay.offsets, lay.numels):
        real[o:o + k] = True
    assert torch.equal(got[real].view(torch.int32), want[real].view(torch.int32)) and server.round == 1


def test_fed_powersgd_simulation(tmp_path, caplog):
    import logging
    from distributed_learning_simulator_amd import simulator
    cfg = simulator.get_config(["--distributed_algorithm", "fed_powersgd", "--worker_number", "4",
                                "--round", "2", "--model_name", "LeNet5", "--train_size", "512",
                                "--test_size", "256", "--log_dir", str(tmp_path / "log")])
    with caplog.at_level(logging.INFO, logger="distributed_learning_simulator_amd"):
        server = simulator.run(cfg)
    assert server.round == 2 and [sorted(c) for c in server.payload_floats] == [[0, 1, 2, 3]] * 2
    assert math.isfinite(float(server.get_metric(server.prev_model)))
    assert any("payload floats" in r.getMessage() for r in caplog.records)
