"""GPU tests of dls_mean_around_median_f32 (the coordinate-wise mean around the
median, stage 2 of Bulyan) and of the layers above it.  Every result is compared bit
for bit (as uint32) with the numpy reference tests/meamed_ref.py."""
import numpy as np
import pytest
import torch

from tests import meamed_ref as M
from tests import robust_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
FMAX = 0x7F7FFFFF


def gpu_bits(bits, keep, rows=None, ld=None, store_rows=None):
    """uint32 [K, P] bit patterns -> the kernel's uint32 [P].  rows: where client k
    lies in a store of store_rows rows at pitch ld (default: dense, in order)."""
    from distributed_learning_simulator_amd import _native
    bits = np.ascontiguousarray(bits, dtype=np.uint32)
    K, P = bits.shape
    ld = P if ld is None else ld
    rows = list(range(K)) if rows is None else list(rows)
    n = max(rows) + 1 if store_rows is None else store_rows
    U = np.full((n, ld), 0x7FC0BEEF, np.uint32)  # rows / columns not selected: NaNs
    U[rows, :P] = bits
    Ud = torch.from_numpy(U.view(np.float32)).to(DEV)
    out = torch.empty(P, dtype=torch.float32, device=DEV)
    _native.mean_around_median(Ud[:, :P] if ld != P else Ud,
                               torch.tensor(rows, dtype=torch.int32, device=DEV), keep, P, out)
    return out.cpu().numpy().view(np.uint32)


def check(bits, keep, **kw):
    got = gpu_bits(bits, keep, **kw)
    want = M.mean_around_median_bits(np.ascontiguousarray(bits, dtype=np.uint32), keep)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"K={bits.shape[0]} keep={keep}: {bad.size} columns differ, first "
                           f"{bad[0]}: got {got[bad[0]]:#x} want {want[bad[0]]:#x}")


def f32(x):
    return np.asarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize("K", range(1, 17))
def test_zero_one_sweep(K):
    """All 2^K zero/one columns in one launch: every small network with its padding
    wires, and the tie rule (0/1 columns tie constantly)."""
    P = max(4, 1 << K)
    p = np.arange(P, dtype=np.uint32)
    X = np.stack([((p >> np.uint32(j)) & np.uint32(1)).astype(np.float32) for j in range(K)])
    for keep in sorted({1, (K + 1) // 2, max(1, K - 2), K}):
        check(f32(X), keep)


@pytest.mark.parametrize("K", [17, 31, 32, 33, 48, 63, 64])
def test_structured_columns(K):
    rng = np.random.default_rng(K)
    cols = [np.arange(K, dtype=np.float32) * 1.5 - 7.0,  # ascending rows
            np.arange(K, dtype=np.float32)[::-1] * 0.3 - 2.0,  # descending
            np.full(K, 3.25, np.float32)]  # all equal
    for pos in range(K):  # one outlier in each row position
        c = (1.0 + 0.001 * rng.standard_normal(K)).astype(np.float32)
        c[pos] = np.float32(1e30 if pos % 2 else -1e30)
        cols.append(c)
    for byz in (1, K // 4, (K - 1) // 2):  # a cluster off-centre: the window slides to an end
        for sign in (1.0, -1.0):
            c = (0.01 * rng.standard_normal(K)).astype(np.float32)
            c[rng.permutation(K)[:byz]] += np.float32(sign * 1e3)
            cols.append(c)
    X = np.stack(cols, axis=1)
    X = np.concatenate([X, rng.standard_normal((K, 256 - X.shape[1] % 4)).astype(np.float32)
                        * np.float32(10.0) ** rng.integers(-3, 4, (K, 1)).astype(np.float32)], axis=1)
    X = X[:, :X.shape[1] // 4 * 4]
    for keep in sorted({1, 2, K - 2 * (K // 4), K - 1, K}):
        check(f32(X), keep)


@pytest.mark.parametrize("K", [5, 8, 64])
def test_special_values(K):
    """+-0, +-inf, NaNs of both signs and odd payloads, denormals and +-FLT_MAX mixed
    at random into ordinary values (kept sums that overflow, inf - inf included)."""
    rng = np.random.default_rng(100 + K)
    pool = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000,
                     0x7F800001, 0xFFABCDEF, 0x7FFFFFFF, 0x00000001, 0x80000001, 0x007FFFFF,
                     0x807FFFFF, 0x00400000, FMAX, FMAX | 0x80000000, 0x7F000000, 0xFF000000],
                    np.uint32)
    P = 4096
    X = f32(rng.standard_normal((K, P)).astype(np.float32)).copy()
    for frac, lo in ((0.5, 0), (0.1, P // 2)):  # dense and sparse specials
        m = rng.random((K, P // 2)) < frac
        X[:, lo:lo + P // 2][m] = rng.choice(pool, int(m.sum()))
    X[:, :8] = FMAX  # sum overflows to +inf
    X[: K // 2, 8:16] = 0x80000000  # zeros only: -0 below +0
    X[K // 2:, 8:16] = 0
    for keep in sorted({1, (K + 1) // 2, K}):
        check(X, keep)


@pytest.mark.parametrize("P", [4, 64, 1088, 70004])
def test_layout(P):
    """ld > P, a scattered non-monotone row selection from a larger store, several
    blocks and a last wave that ends mid-wave."""
    rng = np.random.default_rng(P)
    K = 7
    X = f32(rng.standard_normal((K, P)).astype(np.float32))
    rows = [11, 2, 9, 0, 13, 5, 6]
    check(X, 3, rows=rows, ld=P + 12, store_rows=15)
    check(X, 6, rows=rows, ld=P + 4, store_rows=14)


@pytest.mark.parametrize("K", [1, 7, 16, 33, 64])
def test_consequences_on_the_device(K):
    """keep == K: the bits of dls_trimmed_mean_f32 with trim 0 on the same rows; keep ==
    1 with an odd K: the bits of the store's median (finite non-zero medians)."""
    from distributed_learning_simulator_amd import _native
    from distributed_learning_simulator_amd.aggregation import ClientUpdateStore
    from distributed_learning_simulator_amd.layout import ParameterLayout
    lay = ParameterLayout([("a", (2052,))])
    store = ClientUpdateStore(lay, DEV, capacity=K + 3)
    rng = np.random.default_rng(K)
    U = (rng.standard_normal((K + 3, lay.P)) * 10.0 ** rng.integers(-3, 4, (1, lay.P))) \
        .astype(np.float32)
    store.U.copy_(torch.from_numpy(U))
    rows = [int(r) for r in rng.permutation(K + 3)[:K]]
    r = torch.tensor(rows, dtype=torch.int32, device=DEV)
    mean = torch.empty(lay.P, device=DEV)
    _native.trimmed_mean(store.U, r, 0, lay.P, mean)
    full = store.mean_around_median(rows, K)
    assert np.array_equal(full.cpu().numpy().view(np.uint32), mean.cpu().numpy().view(np.uint32))
    if K % 2:
        one = store.mean_around_median(rows, 1)
        assert np.array_equal(one.cpu().numpy().view(np.uint32),
                              store.median(rows).cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("K, keep", [(10, 6), (33, 17), (64, 32)])
def test_permutation_invariance(K, keep):
    rng = np.random.default_rng(K)
    X = f32((rng.standard_normal((K, 2052)) * 1e3).astype(np.float32))
    first = gpu_bits(X, keep)
    assert np.array_equal(first, M.mean_around_median_bits(X, keep))
    for _ in range(5):
        perm = rng.permutation(K)
        assert np.array_equal(gpu_bits(X, keep, rows=perm, store_rows=K), first)


def test_store_methods_cols_and_out_slice():
    from distributed_learning_simulator_amd.aggregation import ClientUpdateStore
    from distributed_learning_simulator_amd.layout import ParameterLayout
    lay = ParameterLayout([("a", (1000,)), ("b", (37,)), ("c", (3, 50))])
    store = ClientUpdateStore(lay, DEV, capacity=12)
    rng = np.random.default_rng(3)
    U = rng.standard_normal((12, lay.P)).astype(np.float32)
    store.U.copy_(torch.from_numpy(U))
    rows = [7, 1, 10, 4, 3, 8]
    full = store.mean_around_median(rows, 4).cpu().numpy().view(np.uint32)
    assert np.array_equal(full, M.mean_around_median_bits(U[rows], 4))
    for c0, c1 in ((0, 64), (64, 1028), (1024, lay.P), (508, 512)):
        part = store.mean_around_median(rows, 3, cols=(c0, c1)).cpu().numpy().view(np.uint32)
        assert np.array_equal(part, M.mean_around_median_bits(U[rows][:, c0:c1], 3))
    # out: a slice of a larger buffer whose neighbours stay untouched
    buf = torch.full((lay.P + 128,), -123.0, device=DEV)
    store.mean_around_median(torch.tensor(rows, dtype=torch.int32, device=DEV), 2,
                             out=buf[64:64 + lay.P])
    b = buf.cpu().numpy()
    assert np.array_equal(b[64:64 + lay.P].view(np.uint32), M.mean_around_median_bits(U[rows], 2))
    assert (b[:64] == -123.0).all() and (b[64 + lay.P:] == -123.0).all()
    buf.fill_(-123.0)
    store.mean_around_median(rows, 5, out=buf[128:128 + 256], cols=(256, 512))
    b = buf.cpu().numpy()
    assert np.array_equal(b[128:384].view(np.uint32),
                          M.mean_around_median_bits(U[rows][:, 256:512], 5))
    assert (b[:128] == -123.0).all() and (b[384:] == -123.0).all()
    # Bulyan on the store: byzantine == 0 is the ascending mean of all rows
    flat, sel, scores = store.bulyan(rows, [60, 10, 50, 20, 40, 30], 0)
    assert sel == [10, 20, 30, 40, 50, 60] and scores == {}
    assert np.array_equal(flat.cpu().numpy().view(np.uint32), R.trimmed_mean_bits(U[rows], 0))


# ------------------------------------------------------------ server, end to end
def _clients(n, bad):
    from distributed_learning_simulator_amd.models import LeNet5
    torch.manual_seed(0)
    base = {k: v.detach().clone() for k, v in LeNet5().named_parameters()}
    g = torch.Generator().manual_seed(1)
    out = []
    for i in range(n):
        d = {k: v + 0.01 * torch.randn(v.shape, generator=g) for k, v in base.items()}
        if i in bad:  # inf, NaN or 1e30 in every coordinate
            hi = i == bad[0]
            for k, v in d.items():
                pick = torch.randint(0, 3, v.shape, generator=g)
                big = torch.full_like(v, 1e30 if hi else -1e30)
                big[pick == 1] = float("inf") if hi else float("-inf")
                big[pick == 2] = float("nan")
                d[k] = big
        out.append(d)
    return out


def _round(clients, order, **kw):
    from distributed_learning_simulator_amd.servers.fed_server import FedServer
    server = FedServer(tester=None, worker_number=len(clients), synchronous=True, device=DEV, **kw)
    q = server.worker_data_queue
    for w in order:
        q.add_task((w, 100 + 7 * w, clients[w]))
    for w in range(len(clients)):
        q.get_result(consumer=w)  # the initial broadcast
    agg = q.get_result(consumer=0)
    server.stop()
    return server, agg


def _flat_bits(lay, d):
    return lay.flatten(d, device=DEV).cpu().numpy().view(np.uint32)


def test_fed_server_bulyan_round_survives_two_bad_clients():
    from distributed_learning_simulator_amd.layout import ParameterLayout
    bad = (3, 7)
    clients = _clients(11, bad)
    lay = ParameterLayout.from_dict(clients[0])
    X = np.stack([lay.flatten(c).numpy() for c in clients])
    server, agg = _round(clients, [4, 0, 9, 2, 7, 10, 1, 3, 8, 6, 5], aggregation_rule="bulyan",
                         byzantine=2)
    sel = server.last_selection
    assert server.round == 1 and set(agg) == set(clients[0])
    assert isinstance(sel, tuple) and len(sel) == 7 == len(set(sel)) and not set(sel) & set(bad)
    assert set(server.last_scores) == set(sel)
    assert all(torch.isfinite(v).all() for v in agg.values())
    want = M.mean_around_median_bits(X[sorted(sel)], 3)
    assert np.array_equal(_flat_bits(lay, agg), want)
    assert np.array_equal(_flat_bits(lay, server.prev_model), want)
    server2, agg2 = _round(clients, [10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0], aggregation_rule="bulyan",
                           byzantine=2)
    assert server2.last_selection == sel
    assert np.array_equal(_flat_bits(lay, agg2), want)


def test_fed_server_mean_around_median_round_and_default_rule():
    from distributed_learning_simulator_amd.layout import ParameterLayout
    clients = _clients(10, (3, 7))
    lay = ParameterLayout.from_dict(clients[0])
    X = np.stack([lay.flatten(c).numpy() for c in clients])
    order = [4, 0, 9, 2, 7, 1, 3, 8, 6, 5]
    server, agg = _round(clients, order, aggregation_rule="mean_around_median", byzantine=2)
    assert server.round == 1
    assert all(torch.isfinite(v).all() for v in agg.values())
    assert np.array_equal(_flat_bits(lay, agg), M.mean_around_median_bits(X, 8))
    # the default rule: the same bits with and without its name
    _, a1 = _round(clients, order)
    _, a2 = _round(clients, order, aggregation_rule="mean")
    assert np.array_equal(_flat_bits(lay, a1), _flat_bits(lay, a2))


def test_get_subset_model_applies_the_rules():
    from distributed_learning_simulator_amd.layout import ParameterLayout
    from distributed_learning_simulator_amd.servers.fed_server import FedServer
    clients = _clients(10, (3, 7))
    lay = ParameterLayout.from_dict(clients[0])
    X = np.stack([lay.flatten(c).numpy() for c in clients])
    server = FedServer(tester=None, worker_number=10, synchronous=True, device=DEV,
                       aggregation_rule="mean_around_median", byzantine=2)
    for w in (5, 3, 0, 7, 9, 1):
        server.parameters[w] = (50 + w, clients[w])
    subset = (9, 3, 0, 7, 5)  # both bad clients among five: keep = 3
    model = server.get_subset_model(subset)
    assert np.array_equal(_flat_bits(lay, model), M.mean_around_median_bits(X[list(subset)], 3))
    assert all(torch.isfinite(v).all() for v in model.values())
    with pytest.raises(ValueError, match="2\\*byzantine < len\\(subset\\)"):
        server.get_subset_model((0, 1, 5, 9))
    server.stop()
    server = FedServer(tester=None, worker_number=10, synchronous=True, device=DEV,
                       aggregation_rule="bulyan", byzantine=1)
    for w in range(8):
        server.parameters[w] = (50 + w, clients[w])
    model = server.get_subset_model((6, 3, 0, 1, 2, 5, 4))  # K = 7: theta = 5, keep = 3
    sel = server.last_selection
    assert len(sel) == 5 and 3 not in sel
    assert np.array_equal(_flat_bits(lay, model), M.mean_around_median_bits(X[sorted(sel)], 3))
    with pytest.raises(ValueError, match="4\\*byzantine \\+ 3 <= len\\(subset\\)"):
        server.get_subset_model((0, 1, 2, 4, 5, 6))
    server.stop()


def test_simulator_bulyan_round(tmp_path):
    from distributed_learning_simulator_amd import simulator
    cfg = simulator.get_config(["--distributed_algorithm", "fed", "--aggregation_rule", "bulyan",
                                "--byzantine", "1", "--worker_number", "7", "--round", "1",
                                "--model_name", "LeNet5", "--train_size", "96", "--test_size", "32",
                                "--batch_size", "32", "--log_dir", str(tmp_path / "log")])
    server = simulator.run(cfg)
    assert server.round == 1 and server.aggregation_rule == "bulyan"
    assert len(server.last_selection) == 5
    assert server.prev_model and all(torch.isfinite(v).all() for v in server.prev_model.values())
