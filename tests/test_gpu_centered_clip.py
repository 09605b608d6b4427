"""GPU tests of dls_centered_clip_step_f32 and of the centered-clipping layers above it.
The iterate z' is compared bit for bit with the numpy reference
tests/centered_clip_ref.py, the distances at the contract's relative tolerance 2^-17,
and the exact properties (zero distance, equal rows, repeatability, layout and
arrival-order independence) as bits.  The shapes, the store helpers and the honest
rows are those of tests/test_gpu_geomedian.py: one kernel template, one plan."""
import functools

import numpy as np
import pytest
import torch

import tests.test_gpu_geomedian as G
from tests import centered_clip_ref as CR
from tests import geomedian_ref as GR

pytestmark = pytest.mark.gpu

DEV = G.DEV
SENTINEL = G.SENTINEL
bits32, bits64, check_close, honest_rows = G.bits32, G.bits64, G.check_close, G.honest_rows
assert CR.TOL == G.TOL == 2.0 ** -17

# Both sides of every boundary of the dispatcher (KP = 4, 8, 16, 32 wires with four
# coordinates per lane, KP = 64 with two) and of the VW switch at K = 32 / 33.
KS = [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64]
# A partial tile, less than a tile, 36 coordinates into the tile after one flush
# period's worth (1024 for K <= 32), an exact number of 64-element groups, many waves.
PS = [4, 64, 1060, 1088, 70004]


def coefficients(K, seed):
    """Random positive fp32 coefficients that add up to about one, one of them an exact
    1 / K (a client inside the radius)."""
    rng = np.random.default_rng(seed)
    c = ((rng.random(K) + 0.05) * (2.0 / (1.1 * K))).astype(np.float32)
    c[K // 2] = np.float32(1.0 / K)
    return c


def old_point(X, seed):
    """A perturbed row: as near the rows as they are to each other."""
    rng = np.random.default_rng(seed)
    z = X[X.shape[0] // 3] + np.float32(0.003) * rng.standard_normal(X.shape[1], dtype=np.float32)
    return z.astype(np.float32)


def gpu_clip(X, c, z, stream=None, steps=1, **where):
    """(z' bits uint32 [P], dist2 fp64 [K]) after ``steps`` steps in place from z; z lies
    in a longer buffer whose tail must stay untouched."""
    from distributed_learning_simulator_amd import _native
    K, P = np.asarray(X).shape
    Uv, r = G.place(X, **where)
    cd = torch.from_numpy(np.asarray(c, dtype=np.float32)).to(DEV)
    buf = np.full(P + 8, SENTINEL, np.uint32)
    buf[:P] = bits32(z)
    zbuf = torch.from_numpy(buf.view(np.float32)).to(DEV)

    def run(s):
        for _ in range(steps):
            got, d2 = _native.centered_clip_step(Uv, r, cd, P, zbuf, stream=s)
            assert got is zbuf
        return d2

    d2 = G._on(stream, run)
    zb = zbuf.cpu().numpy().view(np.uint32)
    assert (zb[P:] == SENTINEL).all(), "nothing is written past P"
    assert d2.dtype == torch.float64 and tuple(d2.shape) == (K,)
    return zb[:P].copy(), d2.cpu().numpy()


# ------------------------------------------------------------ the step's iterate
@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("K", KS)
def test_step_iterate_bits_and_distances(K, P):
    X = honest_rows(K, P, 1.0, seed=1000 * K + P % 997)
    c, z = coefficients(K, seed=K), old_point(X, seed=P)
    z1, d2 = gpu_clip(X, c, z)
    assert np.array_equal(z1, CR.step_bits(X, c, z))
    check_close(d2, CR.sqdist_to(X, z1.view(np.float32)), f"clip step K={K} P={P}")


@pytest.mark.parametrize("K, P", G.MULTI_PERIOD)
def test_more_than_one_flush_period_per_wave(K, P):
    """tests/test_gpu_geomedian.py, MULTI_PERIOD: the same plan, so the same rows are
    long enough that waves flush twice and end mid-tile."""
    X = honest_rows(K, P, 1.0, seed=K)
    c, z = coefficients(K, seed=K + 1), old_point(X, seed=K + 2)
    z1, d2 = gpu_clip(X, c, z)
    assert np.array_equal(z1, CR.step_bits(X, c, z))
    z1f = z1.view(np.float32)
    check_close(d2, CR.sqdist_to(X, z1f), f"clip step K={K} P={P}")
    assert np.array_equal(bits64(G.gpu_dist(X, z1f)), bits64(d2))  # one kernel, one order


# ------------------------------------------------------ in place and repeatable
def test_in_place_and_repeatable_on_any_stream():
    K, P = 33, 70004
    X = honest_rows(K, P, 1.0, seed=3)
    c, z = coefficients(K, seed=4), old_point(X, seed=5)
    z1, d2 = gpu_clip(X, c, z)
    want1 = CR.step_bits(X, c, z)
    assert np.array_equal(z1, want1)
    for stream in (None, torch.cuda.Stream(DEV)):
        z1s, d2s = gpu_clip(X, c, z, stream=stream)
        assert np.array_equal(z1s, z1) and np.array_equal(bits64(d2s), bits64(d2))
    # a second step starts from what the first one wrote
    want2 = CR.step_bits(X, c, want1.view(np.float32))
    assert not np.array_equal(want2, want1)
    for stream in (None, torch.cuda.Stream(DEV)):
        z2, d22 = gpu_clip(X, c, z, stream=stream, steps=2)
        assert np.array_equal(z2, want2)
        check_close(d22, CR.sqdist_to(X, z2.view(np.float32)), "second step")


@pytest.mark.parametrize("K, P", [(3, 1060), (40, 2052)])
def test_zero_coefficients_leave_z(K, P):
    X = honest_rows(K, P, 1.0, seed=K + 6)
    z = old_point(X, seed=K)
    z1, d2 = gpu_clip(X, np.zeros(K, np.float32), z)
    assert np.array_equal(z1.view(np.float32), z)  # the value: 0 * d is a zero of either sign
    check_close(d2, CR.sqdist_to(X, z), f"c = 0, K={K} P={P}")
    assert np.array_equal(bits64(d2), bits64(G.gpu_dist(X, z)))


# ---------------------------------------------------------- layout independence
@pytest.mark.parametrize("K, P", [(7, 1088), (20, 70004), (64, 4)])
def test_layout_does_not_matter(K, P):
    rng = np.random.default_rng(K)
    X = honest_rows(K, P, 1.0, seed=K + 1)
    c, z = coefficients(K, seed=K), old_point(X, seed=K + 2)
    z1, d2 = gpu_clip(X, c, z)
    assert np.array_equal(z1, CR.step_bits(X, c, z))
    # permuted positions in a larger store whose other rows and pad columns are NaN
    for extra, pad in ((9, 12), (11, 4)):
        rows = rng.permutation(K + extra)[:K]
        z2, d22 = gpu_clip(X, c, z, rows=rows, ld=P + pad, store_rows=K + extra)
        assert np.array_equal(z2, z1) and np.array_equal(bits64(d22), bits64(d2))


# -------------------------------------------------------------- exact properties
def test_zero_distance_and_equal_rows():
    # K = 1, c = 1, from the origin: z' = 0 + 1 * (x - 0) is the row itself
    P = 1088
    X = honest_rows(1, P, 1.0, seed=8)
    z1, d2 = gpu_clip(X, [1.0], np.zeros(P, np.float32))
    assert np.array_equal(z1, bits32(X[0])) and bits64(d2)[0] == 0, "a row equal to z' gives +0.0"
    # one row at z, two mirrored about it with equal coefficients, all on a 2^-10 grid:
    # every operation is exact, the step is zero and z' = z = row 0
    rng = np.random.default_rng(9)
    z = (rng.integers(-1024, 1025, P) / 1024.0).astype(np.float32)
    e = (rng.integers(-64, 65, P) / 1024.0).astype(np.float32)
    Y = np.stack([z, z + e, z - e]).astype(np.float32)
    z1, d2 = gpu_clip(Y, [0.25, 0.375, 0.375], z)
    assert np.array_equal(z1.view(np.float32), z)
    assert bits64(d2)[0] == 0 and bits64(d2)[1] == bits64(d2)[2] and d2[1] > 0
    # rows of equal contents get equal bits
    for K, P in ((5, 1088), (40, 2052)):
        X = honest_rows(K, P, 1.0, seed=K + 3)
        a, b = 1, K - 2
        X[b] = X[a]
        c, z = coefficients(K, seed=K), old_point(X, seed=K + 1)
        z1, d2 = gpu_clip(X, c, z)
        assert np.array_equal(z1, CR.step_bits(X, c, z))
        assert bits64(d2)[a] == bits64(d2)[b] and d2[a] > 0


def test_zero_length_rows():
    from distributed_learning_simulator_amd import _native
    U = torch.randn(5, 64, device=DEV)
    r = torch.tensor([4, 0, 2], dtype=torch.int32, device=DEV)
    z = torch.full((64,), 7.0, device=DEV)
    out = torch.full((3,), -1.0, dtype=torch.float64, device=DEV)
    c = torch.full((3,), 1.0 / 3.0, device=DEV)
    z2, d2 = _native.centered_clip_step(U, r, c, 0, z, dist2=out)
    assert z2 is z and d2 is out and (bits64(out.cpu().numpy()) == 0).all()
    assert (z.cpu().numpy() == 7.0).all(), "P == 0 touches nothing of z"


# --------------------------------------------------------------- the whole rule
def dev32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def flat_bits(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("K, P", [(5, 1088), (17, 70004), (64, 2052)])
def test_replay_of_the_whole_rule(K, P):
    """Every pass of store.centered_clip against the reference, given the previous
    pass's GPU distances: no tolerance on the iterated result.  The start lies about
    0.013 sqrt(P) from most honest clients and tau is 0.012 sqrt(P): clients that are
    clipped at first stop being clipped as the iterate reaches them; the outlier,
    0.3 sqrt(P) away, is clipped throughout."""
    from distributed_learning_simulator_amd import _native
    iters, tau = 3, 0.012 * float(np.sqrt(P))
    rng = np.random.default_rng(K)
    X = honest_rows(K, P, 1.0, seed=K + 5)
    X[K // 2] += np.float32(0.3)  # one client off by 30 sigma
    store, rows, full = G.make_store(X, rows=rng.permutation(K + 3)[:K])
    LP = store.layout.P
    ids = [int(i) for i in rng.permutation(1000)[:K]]
    start_np = np.zeros(LP, np.float32)
    start_np[:P] = old_point(X, seed=K + 7)
    start = dev32(start_np)
    flat, info = store.centered_clip(rows, ids, start, tau, iters, trace=True)
    assert np.array_equal(flat_bits(start), bits32(start_np)), "the start is never modified"
    trace = info["trace"]
    assert len(trace) == iters + 1 and len(info["moved"]) == iters
    order = sorted(range(K), key=lambda k: ids[k])
    S = full[order]  # the clients in id order
    sid = [ids[k] for k in order]
    t_ids, t_c, t_d2 = trace[0]
    assert t_ids == sid and t_c is None
    check_close(np.array(t_d2), CR.sqdist_to(S, start_np), f"K={K} P={P} start")
    prev, zprev = t_d2, start_np
    r = torch.tensor([rows[k] for k in order], dtype=torch.int32, device=DEV)
    for p in range(1, iters + 1):
        t_ids, t_c, t_d2 = trace[p]
        kept, want_s, want_c = CR.scales(prev, tau)
        assert kept == list(range(K)) and t_ids == sid
        assert np.array_equal(bits32(t_c), want_c.view(np.uint32)), f"coefficients of pass {p}"
        want_z = CR.step_bits(S, want_c, zprev)
        zbuf = dev32(zprev)
        _, d2 = _native.centered_clip_step(store.U, r, torch.from_numpy(want_c).to(DEV), LP, zbuf)
        assert np.array_equal(flat_bits(zbuf), want_z), f"z of pass {p}"
        assert np.array_equal(bits64(d2.cpu().numpy()), bits64(t_d2)), f"dist2 of pass {p}"
        check_close(np.array(t_d2), CR.sqdist_to(S, want_z.view(np.float32)),
                    f"K={K} P={P} pass {p}")
        step = want_z.view(np.float32).astype(np.float64) - zprev.astype(np.float64)
        assert abs(info["moved"][p - 1] - np.linalg.norm(step)) <= 1e-6 * np.linalg.norm(step)
        assert want_s[order.index(K // 2)] < 0.2  # the outlier
        prev, zprev = t_d2, want_z.view(np.float32)
    assert np.array_equal(flat_bits(flat), want_z)
    assert info["rejected"] == []
    assert info["distances"] == {i: float(np.sqrt(v)) for i, v in zip(sid, prev)}
    assert info["scales"] == dict(zip(sid, want_s.tolist()))
    # out= receives the iterate
    out = torch.empty(LP, device=DEV)
    flat2, _ = store.centered_clip(rows, ids, start, tau, iters, out=out)
    assert flat2 is out and np.array_equal(flat_bits(out), want_z)


def test_arrival_order_does_not_matter():
    K, P = 9, 2052
    X = honest_rows(K, P, 1.0, seed=21)
    X[4] *= np.float32(3.0)
    ids = [40, 7, 19, 3, 88, 21, 5, 64, 12]
    rng = np.random.default_rng(2)
    first = None
    for _ in range(5):
        perm = rng.permutation(K)  # client perm[j] arrives j-th and takes row j
        store, rows, full = G.make_store(X[perm])
        start = dev32(np.zeros(store.layout.P, np.float32))
        flat, info = store.centered_clip(rows, [ids[k] for k in perm], start, 30.0, 3)
        got = (flat_bits(flat), info)
        if first is None:
            first = got
            assert sorted(info["distances"]) == sorted(ids) and info["rejected"] == []
            assert sorted(info["scales"]) == sorted(ids)
            assert min(info["scales"].values()) < 1.0 == max(info["scales"].values())
        assert np.array_equal(got[0], first[0])
        assert got[1] == first[1]


# ------------------------------------------------------------ the step is bounded
def test_every_step_is_at_most_tau_long():
    """The step is the mean of K vectors no longer than tau, so it is no longer than
    tau; 1e-5 covers the fp32 rounding of a P = 1088 vector of magnitude ~1."""
    P, K, tau = 1088, 10, 0.2
    X = honest_rows(K, P, 1.0, seed=41)
    X[7:] += np.float32(50.0)  # three clients far away on one side
    store, rows, full = G.make_store(X)
    start = dev32(full[0] - np.float32(1.0))  # farther than tau from everyone, on one side
    flat, info = store.centered_clip(rows, list(range(K)), start, tau, 4)
    print("steps of length", info["moved"], "tau", tau)
    assert len(info["moved"]) == 4 and all(0.0 < m <= tau * (1 + 1e-5) for m in info["moved"])
    assert info["moved"][0] >= 0.5 * tau  # everyone pulls the same way at first
    total = np.linalg.norm(flat.cpu().numpy().astype(np.float64)
                           - (full[0] - np.float32(1.0)).astype(np.float64))
    assert total <= 4 * tau * (1 + 1e-5)


def test_inside_the_radius_one_step_is_the_mean():
    P, K = 1088, 10
    X = honest_rows(K, P, 1.0, seed=42)
    store, rows, full = G.make_store(X)
    start = dev32(full[3])
    flat, info = store.centered_clip(rows, list(range(K)), start, 100.0, 1)
    assert set(info["scales"].values()) == {1.0}
    mean = full.astype(np.float64).mean(axis=0)
    err = np.linalg.norm(flat.cpu().numpy().astype(np.float64) - mean) / np.linalg.norm(mean)
    print(f"one unclipped step against the fp64 mean: normwise {err:.3e} (bound 1e-5)")
    assert err <= 1e-5


# The fp64 reference alone (tests/centered_clip_ref.centered_clip64 from the fp64
# coordinate-wise median, seeds 11 / 12 / 13, run on the CPU): the start lies 0.306 to
# 0.308 from the honest mean, the aggregate after 3 steps 0.6411 to 0.6413, the
# farthest honest client is 0.676 from the iterate in the last step (inside tau = 1)
# and the plain mean lies 1.32e5 away.  While the honest clients stay inside the radius
# the offset obeys off' <= (1 - H/K) off + tau B/K, so it stays below tau B/H = 0.6667.
@pytest.mark.parametrize("seed", [11, 12, 13])
def test_colluding_minority_moves_the_mean_not_the_clipped_aggregate(seed):
    P, H, B, tau, iters = 1088, 6, 4, 1.0, 3
    honest = honest_rows(H, P, 1.0, seed=seed)
    hmean = honest.astype(np.float64).mean(axis=0)
    bad = np.tile((hmean + 1e4).astype(np.float32), (B, 1))
    perm = [6, 0, 1, 7, 2, 3, 8, 4, 9, 5]
    X = np.concatenate([honest, bad])[perm]
    honest_ids = [k for k, src in enumerate(perm) if src < H]
    bad_ids = [k for k, src in enumerate(perm) if src >= H]
    bound = tau * B / H
    # the precondition: the reference itself meets the conditions with room
    vr, sr, _ = CR.centered_clip64(X, GR.median0(X), tau, iters)
    assert np.linalg.norm(vr - hmean) <= 0.65
    assert (sr[-1][honest_ids] == 1.0).all() and (sr[-1][bad_ids] < 1e-4).all()
    store, rows, full = G.make_store(X)
    ids = list(range(H + B))
    flat, info = store.centered_clip(rows, ids, store.median(rows), tau, iters)
    off = np.linalg.norm(flat.cpu().numpy().astype(np.float64)[:P] - hmean)
    mean = store.fedavg(rows, [1] * (H + B)).cpu().numpy().astype(np.float64)[:P]
    print(f"seed {seed}: |aggregate - honest mean| = {off:.4f} (reference "
          f"{np.linalg.norm(vr - hmean):.4f}, bound {bound:.4f}), plain mean "
          f"{np.linalg.norm(mean - hmean):.4e}, scales {info['scales']}")
    assert off <= bound
    assert np.linalg.norm(mean - hmean) > bound
    assert all(info["scales"][i] < 1e-4 for i in bad_ids)
    assert all(info["scales"][i] == 1.0 for i in honest_ids)
    assert info["rejected"] == [] and len(info["distances"]) == H + B


# ---------------------------------------------------------- non-finite clients
def _fed(n, **kw):
    from distributed_learning_simulator_amd.servers.fed_server import FedServer
    return FedServer(tester=None, worker_number=n, synchronous=True, device=DEV, **kw)


def test_non_finite_clients_are_rejected():
    P, tau = 1088, 0.4
    X = honest_rows(7, P, 1.0, seed=31)
    X[2] = np.nan
    X[5] = -np.inf
    ids = [13, 4, 9, 21, 2, 7, 30]
    keep = [0, 1, 3, 4, 6]
    store, rows, full = G.make_store(X)
    start = dev32(full[0] + np.float32(0.01))
    flat, info = store.centered_clip(rows, ids, start, tau, 3)
    assert info["rejected"] == [7, 9] and sorted(info["distances"]) == [2, 4, 13, 21, 30]
    assert sorted(info["scales"]) == [2, 4, 13, 21, 30]
    assert torch.isfinite(flat).all()
    store5, rows5, _ = G.make_store(X[keep])
    flat5, info5 = store5.centered_clip(rows5, [ids[k] for k in keep], start, tau, 3)
    assert np.array_equal(flat_bits(flat), flat_bits(flat5))
    assert info5["rejected"] == [] and info5["distances"] == info["distances"]
    assert info5["scales"] == info["scales"] and info5["moved"] == info["moved"]
    # a start that is not finite is at no finite distance from anyone
    for bad in (np.nan, np.inf):
        s = start.clone()
        s[17] = bad
        with pytest.raises(ValueError, match="0 of 7 finite"):
            store.centered_clip(rows, ids, s, tau, 3)
    # through the server: round 1 of a server without a tester starts from the
    # coordinate-wise median, where the NaN and the -inf client sit at opposite ends of
    # every sorted column
    want, winfo = store.centered_clip(rows, ids, store.median(rows), tau, 3)
    assert winfo["rejected"] == [7, 9] and torch.isfinite(want).all()
    server = _fed(7, aggregation_rule="centered_clip", cc_tau=tau)
    for k in (3, 0, 6, 2, 5, 1, 4):
        server.parameters[ids[k]] = (10 + k, {"a": torch.from_numpy(X[k])})
    model = server.get_subset_model(tuple(ids))
    assert server.last_rejected == (7, 9) and sorted(server.last_distances) == [2, 4, 13, 21, 30]
    assert server.last_distances == winfo["distances"]
    assert server.last_clip_scales == winfo["scales"]
    assert np.array_equal(model["a"].cpu().numpy().view(np.uint32), flat_bits(want)[:P])
    server.stop()


# ------------------------------------------------------------ server, end to end
@functools.lru_cache(maxsize=None)
def _clients(shift=0.0, n=5):
    g = torch.Generator().manual_seed(5)
    base = {"w": torch.randn(30, 37, generator=g), "b": torch.randn(37, generator=g)}
    g = torch.Generator().manual_seed(6 + int(100 * shift))  # the round's own noise
    out = []
    for i in range(n):
        d = {k: v + shift + 0.01 * torch.randn(v.shape, generator=g) for k, v in base.items()}
        if i == 3:
            d = {k: v + 2.0 for k, v in d.items()}
        out.append(d)
    return tuple(out)


def _feed(server, clients, order):
    for w in order:
        server._process_worker_data((w, 100 + 7 * w, clients[w]), None)
    return server


def _same_bits(model, views):
    assert set(model) == set(views)
    for k, v in model.items():
        assert v.shape == views[k].shape
        assert np.array_equal(v.cpu().numpy().view(np.uint32),
                              views[k].cpu().numpy().view(np.uint32)), k


def test_fed_server_rounds():
    from distributed_learning_simulator_amd.aggregation import ClientUpdateStore
    from distributed_learning_simulator_amd.layout import ParameterLayout
    clients, later = _clients(), _clients(shift=0.25)
    lay = ParameterLayout.from_dict(clients[0])
    all5 = [0, 1, 2, 3, 4]

    def stored(cl):
        store = ClientUpdateStore(lay, DEV, capacity=5)
        for w in all5:
            store.write(w, cl[w])
        return store

    store, store2 = stored(clients), stored(later)
    # round 1 of a server without a tester: from the coordinate-wise median
    want, info = store.centered_clip(all5, all5, store.median(all5), 10.0, 3)
    # round 2: from round 1's aggregate
    want2, info2 = store2.centered_clip(all5, all5, want, 10.0, 3)
    for order in ([4, 0, 2, 1, 3], [3, 1, 0, 2, 4]):
        server = _feed(_fed(5, aggregation_rule="centered_clip"), clients, order)
        assert server.round == 1
        _same_bits(server.prev_model, lay.views(want))
        assert server.last_distances == info["distances"] and len(server.last_distances) == 5
        assert server.last_rejected == () and server.last_clip_scales == info["scales"]
        # the outlier is the farthest client and the one that is clipped
        assert max(server.last_distances, key=server.last_distances.get) == 3
        assert [i for i, s in server.last_clip_scales.items() if s < 1.0] == [3]
        _feed(server, later, order[::-1])
        assert server.round == 2
        _same_bits(server.prev_model, lay.views(want2))
        assert server.last_distances == info2["distances"]
        assert server.last_clip_scales == info2["scales"]
        server.stop()
    assert not np.array_equal(flat_bits(want2), flat_bits(want))
    # another radius and budget reach the store
    server = _feed(_fed(5, aggregation_rule="centered_clip", cc_iters=1, cc_tau=0.5), clients,
                   all5)
    want1, _ = store.centered_clip(all5, all5, store.median(all5), 0.5, 1)
    _same_bits(server.prev_model, lay.views(want1))
    assert not np.array_equal(flat_bits(want1), flat_bits(want))
    server.stop()


@pytest.mark.parametrize("rule, kw", [("mean", {}), ("median", {}), ("trimmed_mean", {"trim": 1}),
                                      ("multi_krum", {"byzantine": 1})])
def test_defaults_leave_the_other_rules_unchanged(rule, kw):
    clients = _clients()
    a = _feed(_fed(5, aggregation_rule=rule, **kw), clients, [4, 0, 2, 1, 3])
    b = _feed(_fed(5, aggregation_rule=rule, cc_tau=10.0, cc_iters=3, **kw), clients,
              [4, 0, 2, 1, 3])
    _same_bits(a.prev_model, b.prev_model)
    a.stop()
    b.stop()
