"""fed_scaffold on the GPU: the three kernels bit for bit against tests/scaffold_ref.py, and
the control variates removing client drift on heterogeneous quadratics."""
import numpy as np
import pytest
import torch

from tests import scaffold_ref as ref

pytestmark = pytest.mark.gpu
GUARD = 8  # elements around every tensor that must stay as they were


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a, np.float32)
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def dev():
    from distributed_learning_simulator_amd import _native
    _native.require_gpu()
    return torch.device("cuda", 0)


LENGTHS = (1, 3, 4, 5, 255, 256, 257, 1027)
MODES = [(0.0, 0.0, True), (5e-4, 0.0, True), (0.0, 0.01, False), (5e-4, 0.01, True)]


@pytest.mark.parametrize("wd,mu,control", MODES)
@pytest.mark.parametrize("count", [8, 33, 65])
def test_local_step(dev, count, wd, mu, control):
    from distributed_learning_simulator_amd import _native
    rng = np.random.default_rng(count)
    lens = [LENGTHS[(3 * t + count) % len(LENGTHS)] for t in range(count)]
    offs, P = [], 0
    for t, n in enumerate(lens):  # every third flat offset is not a multiple of 4
        offs.append(P + (1 if t % 3 == 1 else 0))
        P = (offs[-1] + n + 63) // 64 * 64
    x, corr = (rng.normal(0, 1, P).astype(np.float32) for _ in range(2))
    params, grads, hosts = [], [], []
    for t, n in enumerate(lens):
        buf = rng.normal(0, 1, n + 2 * GUARD + 1).astype(np.float32)
        start = GUARD + (1 if t % 5 == 2 else 0)  # buf[1:]-style views: the unaligned path
        g = rng.normal(0, 1, n).astype(np.float32)
        dbuf = torch.from_numpy(buf).to(dev)
        params.append(dbuf[start:start + n])
        grads.append(torch.from_numpy(g).to(dev))
        hosts.append((buf, start, g, dbuf))
    _native.scaffold_local_step(params, grads, offs, torch.from_numpy(x).to(dev),
                                torch.from_numpy(corr).to(dev) if control else None, 0.1, wd, mu)
    for (buf, start, g, dbuf), n, o in zip(hosts, lens, offs):
        want = buf.copy()
        want[start:start + n] = ref.local_step(buf[start:start + n], g, x[o:o + n], corr[o:o + n],
                                               0.1, wd, mu, control)
        assert np.array_equal(bits(dbuf), bits(want))  # the guards too


def test_local_step_channels_last_copy(dev):
    """What the worker does with a parameter whose memory is not in logical order."""
    from distributed_learning_simulator_amd import _native
    w = torch.randn(8, 4, 3, 3, device=dev).contiguous(memory_format=torch.channels_last)
    g = torch.randn(8, 4, 3, 3, device=dev).contiguous(memory_format=torch.channels_last)
    corr = torch.randn(320, device=dev)
    with pytest.raises(RuntimeError, match="logical order"):
        _native.scaffold_local_step([w], [g], [0], None, corr, 0.1)
    stepped = w.contiguous()
    _native.scaffold_local_step([stepped], [g.contiguous()], [0], None, corr, 0.1)
    want = ref.local_step(w.cpu().numpy().ravel(), g.cpu().numpy().ravel(), None,
                          corr.cpu().numpy()[:288], 0.1, 0, 0, True)
    assert np.array_equal(bits(stepped).ravel(), bits(want))


@pytest.mark.parametrize("control", [True, False])
@pytest.mark.parametrize("P", [4, 252, 256, 260, 4100])
def test_finish(dev, P, control):
    from distributed_learning_simulator_amd import _native
    rng = np.random.default_rng(P)
    y, x, c, ci = (rng.normal(0, 1, P).astype(np.float32) for _ in range(4))
    if P == 260:
        y[7], y[259] = np.inf, np.nan
    a = _native.scaffold_coeff(5, 0.1)
    assert a == float(ref.coeff(5, 0.1))
    t = lambda v: torch.from_numpy(v).to(dev)
    dci, delta = t(ci), torch.empty(P + 4, device=dev).fill_(7.0)
    stats = torch.full((4,), -1, dtype=torch.int32, device=dev)
    for _ in range(2 if not control else 1):  # the stream's counter cell is left zero
        _native.scaffold_finish(t(y), t(x), t(c) if control else None, dci if control else None,
                                delta, P, a, stats)
    d, new, bad = ref.finish(y, x, c, ci, a, control)
    assert int(stats[0]) == bad == (2 if P == 260 else 0)
    # bit for bit wherever the result is not NaN; a NaN is some NaN
    same = lambda got, want: ((bits(got) == bits(want)) | (np.isnan(got.cpu().numpy()) & np.isnan(want))).all()
    assert same(delta[:P], d) and float(delta[P]) == 7.0
    assert same(dci, new if control else ci)


@pytest.fixture(scope="module")
def rows_case(dev):
    rng = np.random.default_rng(7)
    U = rng.normal(0, 0.05, (1024, 1028 + 12)).astype(np.float32)
    U[3, 5] = 0.0
    U[4, 5] = -0.0
    return U, torch.from_numpy(U).to(dev), rng.integers(1, 1000, 1024).tolist()


@pytest.mark.parametrize("P", [4, 256, 260, 1028])
@pytest.mark.parametrize("K", [1, 2, 5, 64, 65, 1024])
def test_server_step(dev, rows_case, K, P):
    from distributed_learning_simulator_amd import _native
    U, dU, n_all = rows_case
    rng = np.random.default_rng(K * 4099 + P)
    order = rng.permutation(1024)[:K]
    n = [n_all[r] for r in order]
    b = [float(ref.coeff(1 + k % 7, 0.1, 2048)) for k in range(K)]
    x, c = (rng.normal(0, 0.01, P).astype(np.float32) for _ in range(2))  # the chains' scale
    f = float(np.float32(K / 2048))
    t = lambda v, dt=torch.float32: torch.tensor(np.ascontiguousarray(v), dtype=dt).to(dev)

    def run(order, n, b, eta, x, control):
        dx, dc = t(x), t(c)
        xo, co = _native.scaffold_server_step(dU, t(order, torch.int32), t(n), t(b) if control else None,
                                              float(sum(n)), P, eta, f, dx, dc if control else None)
        assert xo is dx and (co is dc if control else co is None)
        return dx, dc

    dx, dc = run(order, n, b, 0.7, x, True)
    wx, wc = ref.server_step(U[order, :P], n, b, 0.7, f, x, c, True)
    assert np.array_equal(bits(dx), bits(wx)) and np.array_equal(bits(dc), bits(wc))
    if K >= 5:  # another row order: another chain, as the restatement says
        back = slice(None, None, -1)
        dx2, dc2 = run(order[back], n[back], b[back], 0.7, x, True)
        wx2, wc2 = ref.server_step(U[order[back], :P], n[back], b[back], 0.7, f, x, c, True)
        assert np.array_equal(bits(dx2), bits(wx2)) and np.array_equal(bits(dc2), bits(wc2))
        assert P < 256 or (bits(wx2) != bits(wx)).any()
    # eta_g = 1 from x = 0 without control: dls_fedavg_f32's bits, c untouched
    dx, dc = run(order, n, None, 1.0, np.zeros(P, np.float32), False)
    avg = _native.fedavg(dU, t(order, torch.int32), t(n), float(sum(n)), P, torch.empty(P, device=dev))
    plus = lambda v: bits(v + np.float32(0))  # x' = 0 + acc: a -0 of the average becomes +0
    assert np.array_equal(bits(dx), plus(avg.cpu().numpy())) and np.array_equal(bits(dc), bits(c))


def test_server_step_refuses_too_many_rows(dev, rows_case):
    from distributed_learning_simulator_amd import _native
    dU = rows_case[1]
    z = torch.zeros(1025, device=dev)
    with pytest.raises(RuntimeError, match=r"K=1025 rows \(1\.\.SCAFFOLD_MAX_K=1024\)"):
        _native.scaffold_server_step(dU, torch.zeros(1025, dtype=torch.int32, device=dev), z, None,
                                     1.0, 4, 1.0, 1.0, z, None)
    lib = _native.lib()
    d = dU.data_ptr()
    assert lib.dls_scaffold_server_step_f32(d, 1040, d, d, None, 1025, 1.0, 4, 1.0, 1.0, d, None, d,
                                            None, 0, None) == -1
    assert b"K=1025 (1..DLS_SCAFFOLD_MAX_K=1024)" in lib.dls_last_error()


def test_control_variates_remove_client_drift(dev):
    """Heterogeneous quadratics f_i(y) = 1/2 sum_j h_ij (y_j - b_ij)^2, 4 clients, 5 local steps
    of 0.1: local SGD stalls away from the optimum sum h_i b_i / sum h_i (0.0798 in fp64),
    SCAFFOLD reaches it (1.1e-8 in fp64 after 30 rounds)."""
    from distributed_learning_simulator_amd import _native
    K, P, tau, lr = 4, 8, 5, 0.1
    rng = np.random.default_rng(0)
    h = rng.uniform(0.5, 2, (K, P))
    bq = rng.normal(0, 1, (K, P))
    best = (h * bq).sum(0) / h.sum(0)
    dh, db = (torch.tensor(v, dtype=torch.float32, device=dev) for v in (h, bq))
    rows = torch.arange(K, dtype=torch.int32, device=dev)
    weight = torch.ones(K, device=dev)
    coef = torch.full((K,), _native.scaffold_coeff(tau, lr, K), device=dev)
    a = _native.scaffold_coeff(tau, lr)
    err = {}
    for control in (False, True):
        x, c = torch.zeros(P, device=dev), torch.zeros(P, device=dev)
        ci, U = torch.zeros(K, P, device=dev), torch.empty(K, P, device=dev)
        stats = torch.zeros(4, dtype=torch.int32, device=dev)
        for _ in range(30):
            for i in range(K):
                y, corr = x.clone(), (c - ci[i] if control else None)
                for _ in range(tau):
                    _native.scaffold_local_step([y], [dh[i] * (y - db[i])], [0], None, corr, lr)
                _native.scaffold_finish(y, x, c if control else None, ci[i] if control else None,
                                        U[i], P, a, stats)
            _native.scaffold_server_step(U, rows, weight, coef if control else None, float(K), P, 1.0,
                                         1.0, x, c if control else None)
        err[control] = float(np.linalg.norm(x.cpu().numpy().astype(np.float64) - best))
    print("drift", err)
    assert err[True] < err[False] / 100
