"""GPU tests of dls_weiszfeld_step_f32 / dls_rows_sqdist_to_f32 and of the
geometric-median layers above them.  The iterate z is compared bit for bit with the
numpy reference tests/geomedian_ref.py, the distances at the contract's relative
tolerance 2^-17, and the exact properties (zero distance, equal rows, repeatability,
layout and arrival-order independence) as bits."""
import functools

import numpy as np
import pytest
import torch

from tests import geomedian_ref as GR
from tests import pairdist_ref as PR
from tests import robust_ref

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
TOL = PR.TOL
assert TOL == GR.TOL == 2.0 ** -17
SENTINEL = 0x7FC0BEEF

# The dispatcher's instantiations: KP = 4, 8, 16, 32 wires with four coordinates per
# lane (tiles of 256 coordinates), KP = 64 with two (tiles of 128).  The smallest, a
# middle and the largest K of each: both sides of every boundary.
KS = [1, 2, 3, 4, 5, 6, 8, 9, 12, 16, 17, 24, 32, 33, 48, 64]
# A flush period is 4 tiles: 1024 (K <= 32) or 512 (K > 32) coordinates.  1060 ends 36
# coordinates into the tile after one period's worth.
PS = [4, 64, 1060, 1088, 70004]
# The plan (csrc/weiszfeld.hip, make_plan): tiles = ceil(P / tile), tiles per wave
# tpw = ceil(tiles / 2048), nW = ceil(tiles / tpw), tile n is visit n / nW of wave
# n % nW, and a wave flushes after every 4th visit.  A wave takes more than one
# flush period when tpw > 4, i.e. tiles > 8192: P > 8192 * 128 = 1,048,576 for K > 32
# and P > 8192 * 256 = 2,097,152 for K <= 32.  1,048,980 gives 8196 tiles of 128 (the
# last one 20 coordinates long), tpw = 5, nW = 1640: waves 0..1635 make a fifth visit.
# 2,097,700 gives 8195 tiles of 256 (the last one 36 long), tpw = 5, nW = 1639.
MULTI_PERIOD = [(33, 1048980), (3, 2097700)]


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def honest_rows(K, P, scale, seed):
    """base + noise (1 % of the scale): rows that differ in the 3rd or 4th digit; a few
    coordinates exactly equal between rows."""
    rng = np.random.default_rng(seed)
    base = (scale * rng.standard_normal(P, dtype=np.float32)).astype(np.float32)
    X = base[None, :] + np.float32(0.01 * scale) * rng.standard_normal((K, P), dtype=np.float32)
    X = X.astype(np.float32)
    X[:, ::7] = X[0, ::7]  # equal in every row
    if K > 2:
        X[1, 1::5] = X[2, 1::5]  # equal in one pair only
    return X


def random_weights(K, seed):
    """Random positive weights normalised in fp32."""
    rng = np.random.default_rng(seed)
    w = (rng.random(K) + 0.05).astype(np.float32)
    return (w / w.sum(dtype=np.float32)).astype(np.float32)


def place(X, rows=None, ld=None, store_rows=None):
    """fp32 [K, P] -> (device store [n, ld] viewed to P columns, device rows).  rows:
    where client k lies in a store of store_rows rows at pitch ld (default: dense, in
    order); every other row and the pad columns are NaN."""
    X = np.ascontiguousarray(X, dtype=np.float32)
    K, P = X.shape
    ld = P if ld is None else ld
    rows = list(range(K)) if rows is None else [int(r) for r in rows]
    n = max(rows) + 1 if store_rows is None else store_rows
    U = np.full((n, ld), SENTINEL, np.uint32)
    U[rows, :P] = X.view(np.uint32)
    Ud = torch.from_numpy(U.view(np.float32)).to(DEV)
    Uv = Ud[:, :P] if ld != P else Ud
    return Uv, torch.tensor(rows, dtype=torch.int32, device=DEV)


def _on(stream, fn):
    if stream is None:
        return fn(None)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):
        out = fn(stream)
    stream.synchronize()
    return out


def gpu_step(X, w, stream=None, **where):
    """(z bits uint32 [P], dist2 fp64 [K]) of one step; z is written into a longer
    buffer whose tail must stay untouched."""
    from distributed_learning_simulator_amd import _native
    K, P = np.asarray(X).shape
    Uv, r = place(X, **where)
    wd = torch.from_numpy(np.asarray(w, dtype=np.float32)).to(DEV)
    zbuf = torch.from_numpy(np.full(P + 8, SENTINEL, np.uint32).view(np.float32)).to(DEV)
    _, d2 = _on(stream, lambda s: _native.weiszfeld_step(Uv, r, wd, P, zbuf, stream=s))
    zb = zbuf.cpu().numpy().view(np.uint32)
    assert (zb[P:] == SENTINEL).all(), "nothing is written past P"
    assert d2.dtype == torch.float64 and tuple(d2.shape) == (K,)
    return zb[:P].copy(), d2.cpu().numpy()


def gpu_dist(X, z, stream=None, **where):
    from distributed_learning_simulator_amd import _native
    K, P = np.asarray(X).shape
    Uv, r = place(X, **where)
    zd = torch.from_numpy(np.ascontiguousarray(z, dtype=np.float32)).to(DEV)
    d2 = _on(stream, lambda s: _native.rows_sqdist_to(Uv, r, P, zd, stream=s))
    assert d2.dtype == torch.float64 and tuple(d2.shape) == (K,)
    return d2.cpu().numpy()


def check_close(d2, want, what=""):
    """|d2 - want| <= 2^-17 * want entrywise, the largest figure printed first."""
    with np.errstate(all="ignore"):
        rel = np.where(want > 0, np.abs(d2 - want) / want, np.abs(d2))
    print(f"{what}: max relative error {rel.max():.3e} (bound {TOL:.3e})")
    assert np.isfinite(d2).all() and (d2 >= 0).all() and not np.signbit(d2).any()
    assert rel.max() <= TOL, (what, float(rel.max()))


# ------------------------------------------------------------ the step's iterate
@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("K", KS)
def test_step_iterate_bits_and_distances(K, P):
    X = honest_rows(K, P, 1.0, seed=1000 * K + P % 997)
    w = random_weights(K, seed=K)
    z, d2 = gpu_step(X, w)
    assert np.array_equal(z, GR.step_bits(X, w))
    check_close(d2, GR.sqdist_to(X, z.view(np.float32)), f"step K={K} P={P}")


@pytest.mark.parametrize("K, P", MULTI_PERIOD)
def test_more_than_one_flush_period_per_wave(K, P):
    """See MULTI_PERIOD: rows long enough that waves flush twice, ending mid-tile."""
    X = honest_rows(K, P, 1.0, seed=K)
    w = random_weights(K, seed=K + 1)
    z, d2 = gpu_step(X, w)
    assert np.array_equal(z, GR.step_bits(X, w))
    zf = z.view(np.float32)
    want = GR.sqdist_to(X, zf)
    check_close(d2, want, f"step K={K} P={P}")
    d2r = gpu_dist(X, zf)
    check_close(d2r, want, f"distances K={K} P={P}")
    assert np.array_equal(bits64(d2r), bits64(d2))  # one kernel: z read or z computed


def test_step_edge_values():
    """-0.0, denormals and denormal products; w = [1.0] returns the row's own bits."""
    P = 64
    row = np.zeros(P, np.float32)
    row[0:8] = [-0.0, 0.0, 1e-45, -1e-45, 1e-38, -3e-39, 1.17549435e-38, -1.0]
    row[8:16] = [3.4e38, -3.4e38, 1.0, 2.0 ** -126, 2.0 ** -149, 5e-324, 123.456, -0.0]
    z, d2 = gpu_step(row[None, :], [1.0])
    assert np.array_equal(z, row.view(np.uint32)) and z[0] == 0x80000000
    assert bits64(d2)[0] == 0  # the row is its own aggregate: +0.0
    # products that fall into the denormal range and sums of denormals
    X = np.stack([row, row[::-1].copy(), np.full(P, 1e-38, np.float32)])
    for w in ([0.5, 0.25, 0.25], [1e-3, 1e-7, 0.999], [2.0 ** -20, 2.0 ** -23, 1.0]):
        w = np.array(w, np.float32)
        z, _ = gpu_step(X, w)
        assert np.array_equal(z, GR.step_bits(X, w)), w
    # -0.0 survives every wire past K: K = 2 rows of -0.0 on the 4-wire kernel
    Z = np.full((2, P), -0.0, np.float32)
    z, d2 = gpu_step(Z, [0.5, 0.5])
    assert (z == 0x80000000).all() and (bits64(d2) == 0).all()


# ------------------------------------------------------------------- distances
@pytest.mark.parametrize("P", [4, 1060, 70004])
@pytest.mark.parametrize("K", [1, 3, 8, 17, 33, 64])
def test_distance_accuracy_both_entry_points(K, P):
    for scale in (1e-3, 1.0, 1e3):
        XX = honest_rows(K + 1, P, scale, seed=77 * K + P % 991)
        X, z = XX[:K], XX[K]  # a point as near as the rows are to each other
        check_close(gpu_dist(X, z), GR.sqdist_to(X, z), f"distances K={K} P={P} scale={scale}")
        w = random_weights(K, seed=K + 2)
        zs, d2 = gpu_step(X, w)
        assert np.array_equal(zs, GR.step_bits(X, w))
        check_close(d2, GR.sqdist_to(X, zs.view(np.float32)), f"step K={K} P={P} scale={scale}")


@pytest.mark.parametrize("K, P", [(5, 1088), (40, 2052)])
def test_zero_distance_and_equal_rows(K, P):
    X = honest_rows(K, P, 1.0, seed=K + 3)
    a, b = 1, K - 2
    X[b] = X[a]
    z = X[0].copy()
    d2 = gpu_dist(X, z)
    assert bits64(d2)[0] == 0, "a row equal to z gives +0.0"
    assert bits64(d2)[a] == bits64(d2)[b] and d2[a] > 0
    check_close(d2, GR.sqdist_to(X, z), f"K={K} P={P}")
    _, d2s = gpu_step(X, random_weights(K, seed=K))
    assert bits64(d2s)[a] == bits64(d2s)[b]


@pytest.mark.parametrize("K", [7, 64])
def test_non_finite_rows_do_not_touch_the_others(K):
    P = 1088
    X = honest_rows(K, P, 1.0, seed=K + 4)
    z = X.astype(np.float64).mean(axis=0).astype(np.float32)
    clean = gpu_dist(X, z)
    check_close(clean, GR.sqdist_to(X, z), f"K={K} clean")
    bad = (2, K - 3)
    Y = X.copy()
    Y[bad[0], [3, 100, 700]] = [np.inf, -np.inf, np.inf]
    Y[bad[1], [10, 1087]] = [np.nan, 1.0]
    d2 = gpu_dist(Y, z)
    assert not np.isfinite(d2[list(bad)]).any()
    others = [k for k in range(K) if k not in bad]
    assert np.array_equal(bits64(d2[others]), bits64(clean[others]))


# ---------------------------------------------------- layout and repeatability
@pytest.mark.parametrize("K, P", [(7, 1088), (20, 70004), (64, 4)])
def test_layout_does_not_matter(K, P):
    rng = np.random.default_rng(K)
    X = honest_rows(K, P, 1.0, seed=K + 1)
    w = random_weights(K, seed=K)
    z, d2 = gpu_step(X, w)
    assert np.array_equal(z, GR.step_bits(X, w))
    dz = gpu_dist(X, z.view(np.float32))
    assert np.array_equal(bits64(dz), bits64(d2))
    for extra, pad in ((9, 12), (11, 4)):
        rows = rng.permutation(K + extra)[:K]
        where = dict(rows=rows, ld=P + pad, store_rows=K + extra)
        z2, d22 = gpu_step(X, w, **where)
        assert np.array_equal(z2, z) and np.array_equal(bits64(d22), bits64(d2))
        assert np.array_equal(bits64(gpu_dist(X, z.view(np.float32), **where)), bits64(dz))


def test_repeatable_on_any_stream():
    X = honest_rows(33, 70004, 1.0, seed=3)
    w = random_weights(33, seed=4)
    z, d2 = gpu_step(X, w)
    for stream in (None, torch.cuda.Stream(DEV)):
        z2, d22 = gpu_step(X, w, stream=stream)
        assert np.array_equal(z2, z) and np.array_equal(bits64(d22), bits64(d2))
        dz = gpu_dist(X, z.view(np.float32), stream=stream)
        assert np.array_equal(bits64(dz), bits64(d2))


def test_zero_length_rows():
    from distributed_learning_simulator_amd import _native
    U = torch.randn(5, 64, device=DEV)
    r = torch.tensor([4, 0, 2], dtype=torch.int32, device=DEV)
    z = torch.full((64,), 7.0, device=DEV)
    out = torch.full((3,), -1.0, dtype=torch.float64, device=DEV)
    assert _native.rows_sqdist_to(U, r, 0, z, out=out) is out
    assert (bits64(out.cpu().numpy()) == 0).all()
    out.fill_(-1.0)
    w = torch.full((3,), 1.0 / 3.0, device=DEV)
    z2, d2 = _native.weiszfeld_step(U, r, w, 0, z, dist2=out)
    assert z2 is z and d2 is out and (bits64(out.cpu().numpy()) == 0).all()
    assert (z.cpu().numpy() == 7.0).all(), "P == 0 writes nothing to z"


# --------------------------------------------------------------- the whole rule
def make_store(X, rows=None, capacity=None):
    """A ClientUpdateStore whose layout is one tensor of X.shape[1] elements (the row is
    padded with zeros to a multiple of 64); client k in row rows[k]."""
    from distributed_learning_simulator_amd.aggregation import ClientUpdateStore
    from distributed_learning_simulator_amd.layout import ParameterLayout
    K, P = X.shape
    rows = list(range(K)) if rows is None else [int(r) for r in rows]
    lay = ParameterLayout([("a", (P,))])
    store = ClientUpdateStore(lay, DEV, capacity=max(rows) + 1 if capacity is None else capacity)
    store.U.fill_(float("nan"))
    full = np.zeros((K, lay.P), np.float32)
    full[:, :P] = X
    store.U[torch.tensor(rows, device=DEV)] = torch.from_numpy(full).to(DEV)
    return store, rows, full


@pytest.mark.parametrize("K, P", [(5, 1088), (17, 70004), (64, 2052)])
def test_replay_of_the_whole_rule(K, P):
    """Every pass of store.geometric_median against the reference, given the previous
    pass's GPU distances: no tolerance on the iterated result."""
    from distributed_learning_simulator_amd import _native
    iters, nu = 3, 1e-6
    rng = np.random.default_rng(K)
    X = honest_rows(K, P, 1.0, seed=K + 5)
    X[K // 2] += np.float32(0.3)  # one client off by 30 sigma
    store, rows, full = make_store(X, rows=rng.permutation(K + 3)[:K])
    ids = [int(i) for i in rng.permutation(1000)[:K]]
    flat, info = store.geometric_median(rows, ids, iters, nu, trace=True)
    trace = info["trace"]
    assert len(trace) == iters + 1 and len(info["objective"]) == iters + 1
    order = sorted(range(K), key=lambda k: ids[k])
    S = full[order]  # the clients in id order
    sid = [ids[k] for k in order]
    # the start: the coordinate-wise median and the distances to it
    t_ids, t_w, t_d2 = trace[0]
    assert t_ids == sid and t_w is None
    z0 = robust_ref.median_bits(S).view(np.float32)
    check_close(np.array(t_d2), GR.sqdist_to(S, z0), f"K={K} P={P} start")
    prev = t_d2
    for p in range(1, iters + 1):
        t_ids, t_w, t_d2 = trace[p]
        kept, want_w = GR.weights(prev, nu)
        assert kept == list(range(K)) and t_ids == sid
        assert np.array_equal(bits32(t_w), want_w.view(np.uint32)), f"weights of pass {p}"
        want_z = GR.step_bits(S, want_w)
        zbuf = torch.empty(store.layout.P, device=DEV)
        r = torch.tensor([rows[k] for k in order], dtype=torch.int32, device=DEV)
        _, d2 = _native.weiszfeld_step(store.U, r, torch.from_numpy(want_w).to(DEV),
                                       store.layout.P, zbuf)
        assert np.array_equal(zbuf.cpu().numpy().view(np.uint32), want_z), f"z of pass {p}"
        assert np.array_equal(bits64(d2.cpu().numpy()), bits64(t_d2)), f"dist2 of pass {p}"
        check_close(np.array(t_d2), GR.sqdist_to(S, want_z.view(np.float32)),
                    f"K={K} P={P} pass {p}")
        want_obj = 0.0
        for v in t_d2:
            want_obj += float(np.sqrt(v))
        assert info["objective"][p] == want_obj
        prev = t_d2
    assert np.array_equal(flat.cpu().numpy().view(np.uint32), want_z)
    assert info["rejected"] == []
    assert info["distances"] == {i: float(np.sqrt(v)) for i, v in zip(sid, prev)}


def test_arrival_order_does_not_matter():
    K, P = 9, 2052
    X = honest_rows(K, P, 1.0, seed=21)
    X[4] *= np.float32(3.0)
    ids = [40, 7, 19, 3, 88, 21, 5, 64, 12]
    rng = np.random.default_rng(2)
    first = None
    for _ in range(5):
        perm = rng.permutation(K)  # client perm[j] arrives j-th and takes row j
        store, rows, _ = make_store(X[perm])
        flat, info = store.geometric_median(rows, [ids[k] for k in perm], 3, 1e-6)
        got = (flat.cpu().numpy().view(np.uint32), info)
        if first is None:
            first = got
            assert sorted(info["distances"]) == sorted(ids) and info["rejected"] == []
        assert np.array_equal(got[0], first[0])
        assert got[1] == first[1]


# The fp64 reference alone (tests/geomedian_ref.weiszfeld64, seeds 11 / 12 / 13, run on
# the CPU): the aggregate lies 0.569 / 0.569 / 0.571 of the largest honest pairwise
# distance from the honest mean (the bound is 1; the colluders' pull of about
# 4 * (1 / 3.3e5) / (6 / 0.33) * 1e4 per coordinate is what uses the room), the
# objective falls from 1319395.21 by 0.17 (the four colluders, 3.3e5 away each, are
# nearly all of it, so a distance error at the 2^-17 bound could reach 10: this
# condition has room only because the kernel's chains are 8 terms long and its
# errors stay near 5e-9 relative, 0.007 here), and the plain mean lies 2.9e5 of that
# distance away.
@pytest.mark.parametrize("seed", [11, 12, 13])
def test_colluding_minority_moves_the_mean_not_the_geometric_median(seed):
    P, H, B = 1088, 6, 4
    honest = honest_rows(H, P, 1.0, seed=seed)
    hmean = honest.astype(np.float64).mean(axis=0)
    bad = np.tile((hmean + 1e4).astype(np.float32), (B, 1))
    X = np.concatenate([honest, bad])[[6, 0, 1, 7, 2, 3, 8, 4, 9, 5]]
    spread = np.sqrt(PR.sqdist(honest).max())
    zr, objr = GR.weiszfeld64(X, 3, 1e-6)
    # the precondition: the reference itself meets both conditions with room
    assert np.linalg.norm(zr - hmean) <= 0.6 * spread and objr[0] - objr[-1] >= 0.15
    store, rows, full = make_store(X)
    flat, info = store.geometric_median(rows, list(range(H + B)), 3, 1e-6)
    z = flat.cpu().numpy().astype(np.float64)[:P]
    off = np.linalg.norm(z - hmean)
    print(f"seed {seed}: |z - honest mean| = {off:.4f}, largest honest pairwise distance "
          f"{spread:.4f}, objective {info['objective'][0]:.6f} -> {info['objective'][-1]:.6f}")
    assert off <= spread
    assert info["objective"][-1] <= info["objective"][0]
    assert info["rejected"] == [] and len(info["distances"]) == H + B
    mean = store.fedavg(rows, [1] * (H + B)).cpu().numpy().astype(np.float64)[:P]
    assert np.linalg.norm(mean - hmean) > spread


def _fed(n, **kw):
    from distributed_learning_simulator_amd.servers.fed_server import FedServer
    return FedServer(tester=None, worker_number=n, synchronous=True, device=DEV, **kw)


def test_non_finite_clients_are_rejected():
    """A NaN client and a -inf client sit at opposite ends of every sorted column, so
    the median start of the 7 is the median of the other 5, and so is all that follows."""
    P = 1088
    X = honest_rows(7, P, 1.0, seed=31)
    X[2] = np.nan
    X[5] = -np.inf
    ids = [13, 4, 9, 21, 2, 7, 30]
    store, rows, _ = make_store(X)
    flat, info = store.geometric_median(rows, ids, 3, 1e-6)
    assert info["rejected"] == [7, 9] and sorted(info["distances"]) == [2, 4, 13, 21, 30]
    assert torch.isfinite(flat).all()
    keep = [0, 1, 3, 4, 6]
    store5, rows5, _ = make_store(X[keep])
    flat5, info5 = store5.geometric_median(rows5, [ids[k] for k in keep], 3, 1e-6)
    assert np.array_equal(flat.cpu().numpy().view(np.uint32), flat5.cpu().numpy().view(np.uint32))
    assert info5["rejected"] == [] and info5["distances"] == info["distances"]
    assert info5["objective"] == info["objective"]
    # an inf and a NaN client at the same end of the columns: rejected as well
    X[5] = np.inf
    store, rows, _ = make_store(X)
    flat, info = store.geometric_median(rows, ids, 3, 1e-6)
    assert info["rejected"] == [7, 9] and torch.isfinite(flat).all()
    # through the server
    server = _fed(7, aggregation_rule="geometric_median")
    for k in (3, 0, 6, 2, 5, 1, 4):
        server.parameters[ids[k]] = (10 + k, {"a": torch.from_numpy(X[k])})
    model = server.get_subset_model(tuple(ids))
    assert server.last_rejected == (7, 9) and sorted(server.last_distances) == [2, 4, 13, 21, 30]
    assert np.array_equal(model["a"].cpu().numpy().view(np.uint32),
                          flat.cpu().numpy().view(np.uint32)[:P])
    server.stop()
    # a NaN majority leaves no finite start
    X = honest_rows(7, P, 1.0, seed=32)
    X[[0, 2, 3, 6]] = np.nan
    store, rows, _ = make_store(X)
    with pytest.raises(ValueError, match="0 of 7 finite"):
        store.geometric_median(rows, ids, 3, 1e-6)


# ------------------------------------------------------------ server, end to end
@functools.lru_cache(maxsize=None)
def _clients(n=5):
    g = torch.Generator().manual_seed(5)
    base = {"w": torch.randn(30, 37, generator=g), "b": torch.randn(37, generator=g)}
    out = []
    for i in range(n):
        d = {k: v + 0.01 * torch.randn(v.shape, generator=g) for k, v in base.items()}
        if i == 3:
            d = {k: v + 2.0 for k, v in d.items()}
        out.append(d)
    return tuple(out)


def _round(clients, order, **kw):
    server = _fed(len(clients), **kw)
    for w in order:
        server._process_worker_data((w, 100 + 7 * w, clients[w]), None)
    return server


def test_fed_server_round():
    from distributed_learning_simulator_amd.aggregation import ClientUpdateStore
    from distributed_learning_simulator_amd.layout import ParameterLayout
    clients = _clients()
    lay = ParameterLayout.from_dict(clients[0])
    store = ClientUpdateStore(lay, DEV, capacity=5)
    for w in range(5):
        store.write(w, clients[w])
    want, info = store.geometric_median([0, 1, 2, 3, 4], [0, 1, 2, 3, 4], 3, 1e-6)
    want_views = lay.views(want)
    for order in ([4, 0, 2, 1, 3], [3, 1, 0, 2, 4]):
        server = _round(clients, order, aggregation_rule="geometric_median")
        assert server.round == 1 and set(server.prev_model) == {"w", "b"}
        for k, v in server.prev_model.items():
            assert v.shape == clients[0][k].shape
            assert np.array_equal(v.cpu().numpy().view(np.uint32),
                                  want_views[k].cpu().numpy().view(np.uint32))
        assert server.last_distances == info["distances"] and len(server.last_distances) == 5
        assert server.last_rejected == ()
        # the outlier is the farthest client
        assert max(server.last_distances, key=server.last_distances.get) == 3
        server.stop()
    # other budgets reach the store
    server = _round(clients, [0, 1, 2, 3, 4], aggregation_rule="geometric_median", gm_iters=1,
                    gm_nu=0.5)
    want1, _ = store.geometric_median([0, 1, 2, 3, 4], [0, 1, 2, 3, 4], 1, 0.5)
    got = lay.flatten(server.prev_model, device=DEV)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), want1.cpu().numpy().view(np.uint32))
    assert not np.array_equal(want1.cpu().numpy().view(np.uint32),
                              want.cpu().numpy().view(np.uint32))
    server.stop()


@pytest.mark.parametrize("rule, kw", [("mean", {}), ("median", {}), ("trimmed_mean", {"trim": 1}),
                                      ("multi_krum", {"byzantine": 1})])
def test_defaults_leave_the_other_rules_unchanged(rule, kw):
    clients = _clients()
    a = _round(clients, [4, 0, 2, 1, 3], aggregation_rule=rule, **kw)
    b = _round(clients, [4, 0, 2, 1, 3], aggregation_rule=rule, gm_iters=3, gm_nu=1e-6, **kw)
    for k in a.prev_model:
        assert np.array_equal(a.prev_model[k].cpu().numpy().view(np.uint32),
                              b.prev_model[k].cpu().numpy().view(np.uint32))
    a.stop()
    b.stop()
