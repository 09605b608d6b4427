"""GPU: every fp32 mantissa, every binade and the guard edges through the exact
division kernels (dls_fedavg_f32, dls_subset_fedavg_f32, dls_subset_fedavg_union_f32,
dequant-FedAvg), bit for bit against the plain numpy reference of
tests/division_ref.py.  tests/test_division_host.py proves the division
ALGORITHMS for the same divisor table on the CPU, so a mismatch here is device
code: a guard, a packed constant, a denormal mode, a slow-path branch.

Sizes: the mantissa sweep is 2^23 elements because that is every fp32 mantissa;
the binade sweep (stride 4096: 2049 mantissas x 255 binades x 2 signs + the guard
neighbours, ~1.05 M elements) is the smallest that still has every binade's
first and last mantissa and takes the narrow per-wave forms."""
import functools

import numpy as np
import pytest
import torch

from oracle import quant as oquant
from tests import division_ref as R

pytestmark = pytest.mark.gpu

dev = torch.device("cuda")
DIVISORS = R.DIVISORS
QUANT_TOTALS = (11735695, 55123, 2147483648, 2147483904)


same_bits = R.same_bits  # the GPU tests' helper: NaN positions, then every bit pattern


def check(got, ref, x=None, tag=None):
    assert same_bits(got, ref), (tag, R.first_mismatch(got, ref, x))


@pytest.fixture(scope="module")
def mant():
    return R.mantissa_sweep()


@pytest.fixture(scope="module")
def mant_d(mant):
    return torch.from_numpy(mant).to(dev)


@pytest.fixture(scope="module")
def sweep():
    return R.device_sweep(4096)


@pytest.fixture(scope="module")
def sweep_d(sweep):
    return torch.from_numpy(sweep).to(dev)


@pytest.fixture(scope="module")
def sweep3(sweep):
    """Three client rows of the binade sweep whose in-order sum meets -0 + +0,
    denormal partial sums and inf - inf: the sweep, its negation rolled by one
    binade's worth, and the sweep reversed."""
    U = np.stack([sweep, np.roll(-sweep, 2049), sweep[::-1]])
    return U, torch.from_numpy(U).to(dev)


# ------------------------------------------------------------ (a) dls_fedavg_f32
def run_fedavg(Ud, weights, total):
    from distributed_learning_simulator_amd import _native
    K, P = Ud.shape
    out = torch.empty(P, dtype=torch.float32, device=dev)
    _native.fedavg(Ud, torch.arange(K, dtype=torch.int32, device=dev),
                   torch.tensor(weights, dtype=torch.float32, device=dev), float(total), P, out)
    return out.cpu().numpy()


@pytest.mark.parametrize("N", DIVISORS, ids=R.div_id)
def test_fedavg_mantissa_sweep(mant, mant_d, N):
    """k_fedavg_exact_pipe, widest form (22 KB of a row per wave: P = 2^23 gives
    1490 such waves), K = 1, weight 1: every fp32 mantissa of the dividend over
    one divisor per case.  2^23 elements because that is the whole mantissa space."""
    check(run_fedavg(mant_d[None], [1.0], N), R.weighted_terms(mant, 1.0, N), mant)


@pytest.mark.parametrize("scale,N", [(2.0 ** -60, 2147483648.0), (2.0 ** -60, 11735695.0),
                                     (2.0 ** -60, 7.0), (2.0 ** 60, 1.0), (2.0 ** 60, 11735695.0),
                                     (2.0 ** 60, 7.0)])
def test_fedavg_edge_binades_full_mantissa(mant, scale, N):
    """The widest k_fedavg_exact_pipe form on every mantissa of the lowest
    ([2^-60, 2^-59)) and the highest full ([2^60, 2^61)) binade the guard admits to
    Markstein's quotient, where its intermediates are closest to leaving the normal
    range (largest divisor below, smallest above)."""
    x = mant * np.float32(scale)  # exact: a power of two
    got = run_fedavg(torch.from_numpy(x).to(dev)[None], [1.0], N)
    check(got, R.weighted_terms(x, 1.0, N), x)


@pytest.mark.parametrize("w", [1.0, 3.0, 1000.0, 16777216.0, 0.5])
@pytest.mark.parametrize("N", DIVISORS, ids=R.div_id)
def test_fedavg_binade_sweep_one_client(sweep, sweep_d, N, w):
    """k_fedavg_exact_pipe, 1 KB-per-wave form (~1.05 M elements are too few waves
    for the wide forms): every binade, denormals, zeros, inf, nan and the values
    one ulp either side of 2^-60 and 2^61, times a weight that moves the product
    across the guard, through the guarded term4 (fast path and per-element IEEE
    fix-up in one f32x4)."""
    check(run_fedavg(sweep_d[None], [w], N), R.weighted_terms(sweep, w, N), sweep, w)


@pytest.mark.parametrize("N", DIVISORS, ids=R.div_id)
def test_fedavg_binade_sweep_three_clients(sweep3, N):
    """The same 1 KB form, K = 3 with weights 3, 0.5 and 1000: the running sum
    (started at -0) sees -0 + +0, denormal partial sums and inf - inf in the
    reference's order."""
    U, Ud = sweep3
    w = [3.0, 0.5, 1000.0]
    ref = R.fold([R.weighted_terms(U[i], w[i], N) for i in range(3)])
    check(run_fedavg(Ud, w, N), ref)


# ----------------------------------------------------- (b) dls_subset_fedavg_f32
def run_subsets_of_row0(Ud, weights, totals):
    """S single-member subsets {row 0} with their own weight and divisor."""
    from distributed_learning_simulator_amd import _native
    S, P = len(totals), Ud.shape[1]
    out = torch.full((S, P), float("nan"), device=dev)
    _native.subset_fedavg(Ud, torch.arange(S + 1, dtype=torch.int32, device=dev),
                          torch.zeros(S, dtype=torch.int32, device=dev),
                          torch.tensor(weights, dtype=torch.float32, device=dev),
                          torch.tensor(totals, dtype=torch.float32, device=dev), P, out)
    return out


@pytest.mark.parametrize("w", [1.0, 3.0, 0.5])
def test_subset_binade_sweep_all_divisors(sweep, sweep_d, w):
    """k_subset_exact: the binade sweep divided by every table divisor as 18
    single-member subsets of one launch; the divisor and RN(1/N) are derived on the
    device here (the in-kernel `b <= 2^31` test sees 2147483648 and 2147483904)."""
    got = run_subsets_of_row0(sweep_d[None], [w] * len(DIVISORS), DIVISORS).cpu().numpy()
    for s, N in enumerate(DIVISORS):
        check(got[s], R.weighted_terms(sweep, w, N), sweep, N)


@pytest.mark.parametrize("lo", [0, 8, 16])
def test_subset_mantissa_sweep(mant, mant_d, lo):
    """k_subset_exact on every mantissa, 8 divisors per launch (a 256 MB output,
    the largest single allocation; 2^23 elements because that is the mantissa
    space).  Slices [0:8], [8:16], [16:18] of the table: both sides of 2^31 in the
    second."""
    divs = DIVISORS[lo:lo + 8]
    out = run_subsets_of_row0(mant_d[None], [1.0] * len(divs), divs)
    for s, N in enumerate(divs):
        check(out[s].cpu().numpy(), R.weighted_terms(mant, 1.0, N), mant, N)


# ----------------------------------------------- (c) dls_subset_fedavg_union_f32
def run_union(Ud, uweights, members, totals, P=None):
    """members[j]: the coalitions (indices into totals) client j belongs to."""
    from distributed_learning_simulator_amd import _native
    P = P or Ud.shape[1]
    Ku, S = len(uweights), len(totals)
    masks = [sum(1 << c for c in m) for m in members]
    masks = [m - (1 << 64) if m >= 1 << 63 else m for m in masks]
    out = torch.full((S, P), float("nan"), device=dev)
    _native.subset_fedavg_union(Ud, torch.arange(Ku, dtype=torch.int32, device=dev),
                                torch.tensor(uweights, dtype=torch.float32, device=dev),
                                torch.tensor(masks, dtype=torch.int64, device=dev),
                                [float(t) for t in totals], P, out)
    return out


UNION_SLICE = 1 << 21
UNION_WAVES = 8  # k_subset_union's waves per block


def union_launch(slow, fast):
    """16 divisors ordered for k_subset_union's plan.  Its waves take the fast walk
    only if EVERY coalition dealt to them has a divisor in [1, 2^31], and the plan
    (longest first to the least loaded wave, ties to the lower index) deals 16
    equally long coalitions c and c + 8 to wave c % 8.  So the out-of-range
    divisors are paired at positions (w, w + 8) of the same waves, and every
    in-range divisor shares its wave with another in-range one."""
    assert len(slow) % 2 == 0 and len(slow) + len(fast) == 2 * UNION_WAVES
    pairs = list(slow) + list(fast)
    order = [None] * (2 * UNION_WAVES)
    for i, b in enumerate(pairs):
        order[i // 2 + UNION_WAVES * (i % 2)] = b
    for w in range(UNION_WAVES):
        assert R.in_fast_divisor_range(order[w]) == R.in_fast_divisor_range(order[w + UNION_WAVES])
    return tuple(order)


_FAST = [b for b in DIVISORS if R.in_fast_divisor_range(b)]
_SLOW = [b for b in DIVISORS if not R.in_fast_divisor_range(b)]
assert len(_FAST) == 13 and len(_SLOW) == 5
# two launches of 16 cover the table: 4 out-of-range + the first 12 in-range, then
# the fifth out-of-range (twice, one wave) + all 13 in-range and 11735695 again
UNION_DIVS = (union_launch(_SLOW[:4], _FAST[:12]),
              union_launch([_SLOW[4], _SLOW[0]], _FAST + [11735695.0]))
assert set(UNION_DIVS[0]) | set(UNION_DIVS[1]) == set(DIVISORS)


@pytest.mark.parametrize("sl", range(4))
def test_union_mantissa_sweep(mant, mant_d, sl):
    """k_subset_union: one client row (weight 1) and 16 coalitions {client 0} per
    launch, so one launch divides the same row by 16 divisors; slices of 2^21
    mantissas, two launches per slice covering the whole table, ordered by
    union_launch so that every in-range divisor is on a wave that takes the packed
    fast walk: the packed two-constant quotient (the accepted divisors), the
    packed Markstein quotient (11735695, 16777218, 8388607, in both launches), and
    the scalar slow walk on the waves that hold the out-of-range divisors."""
    x = mant[sl * UNION_SLICE:(sl + 1) * UNION_SLICE]
    xd = mant_d[sl * UNION_SLICE:(sl + 1) * UNION_SLICE][None]
    for divs in UNION_DIVS:
        got = run_union(xd, [1.0], [list(range(len(divs)))], divs).cpu().numpy()
        for s, N in enumerate(divs):
            check(got[s], R.weighted_terms(x, 1.0, N), x, N)


POISON = np.array([0x00000000, 0x80000000, 0x000116C2, 0x5E000000, 0x7F800000, 0x7FC00000],
                  np.uint32).view(np.float32)  # 0, -0, 1e-40, 2^61, inf, nan


def poisoned(x, every=2):
    """x with one out-of-range element planted in every `every`-th 256-element
    tile, cycling through POISON; returns (copy, mask of planted positions)."""
    y = x.copy()
    tiles = np.arange(0, len(x) // 256, every)
    idx = tiles * 256 + (tiles * 37) % 256
    y[idx] = POISON[np.arange(len(idx)) % len(POISON)]
    mask = np.zeros(len(x), bool)
    mask[idx] = True
    return y, mask


def test_union_poisoned_tiles(mant):
    """k_subset_union's wave-uniform switch: a 256-parameter tile with ONE
    out-of-range element (0, -0, 1e-40, 2^61, inf, nan in turn) takes the scalar
    slow walk for all its elements, its neighbours the packed fast walk.  Every
    in-range element of a poisoned tile keeps the bits of the un-poisoned run, and
    everything equals the reference.  2^21 mantissas (one launch slice); the
    second union_launch order: one wave holds the out-of-range divisor (slow walk
    in both runs), the other seven hold all 13 in-range divisors, so the switch
    between the packed and the slow walk is compared for the two-constant AND the
    packed Markstein quotient (11735695 on two waves, 16777218, 8388607)."""
    assert float(POISON[2]) == float(np.float32(1e-40)) and float(POISON[3]) == 2.0 ** 61
    x = mant[:UNION_SLICE]
    y, mask = poisoned(x)
    divs = UNION_DIVS[1]
    members = [list(range(len(divs)))]
    clean = run_union(torch.from_numpy(x).to(dev)[None], [1.0], members, divs).cpu().numpy()
    got = run_union(torch.from_numpy(y).to(dev)[None], [1.0], members, divs).cpu().numpy()
    for s, N in enumerate(divs):
        check(got[s], R.weighted_terms(y, 1.0, N), y, N)
        assert np.array_equal(got[s].view(np.uint32)[~mask], clean[s].view(np.uint32)[~mask]), N


@pytest.mark.parametrize("w1", [16777216.0, 16777218.0, 0.5])
def test_union_weights_at_the_fast_bound(mant, w1):
    """k_subset_union's launch-wide weight test (1 <= n_j <= 2^24): a second client
    with weight 2^24 keeps the packed fast walk, 2^24 + 2 or 0.5 sends every tile
    of the launch down the slow walk.  Coalitions {0}, {0, 1}, {1} for four fast
    divisors; all equal the reference, and the fast client's own coalitions {0}
    have the bits of a launch whose second weight is 3.  2^20 strided mantissas:
    enough tiles for every block of the persistent grid."""
    x0 = mant[::8].copy()
    x1 = np.roll(-x0, 4099) * np.float32(2.0 ** -20)
    U = np.stack([x0, x1])
    Ud = torch.from_numpy(U).to(dev)
    divs = [7.0, 55123.0, 11735695.0, 2147483648.0]
    totals = [N for N in divs for _ in range(3)]  # coalition 3i: {0}, 3i+1: {0,1}, 3i+2: {1}
    members = [[3 * i for i in range(4)] + [3 * i + 1 for i in range(4)],
               [3 * i + 1 for i in range(4)] + [3 * i + 2 for i in range(4)]]
    base = run_union(Ud, [1.0, 3.0], members, totals).cpu().numpy()
    got = run_union(Ud, [1.0, w1], members, totals).cpu().numpy()
    for i, N in enumerate(divs):
        t0, t1 = R.weighted_terms(x0, 1.0, N), R.weighted_terms(x1, w1, N)
        check(got[3 * i], t0, x0, N)
        check(got[3 * i + 1], R.fold([t0, t1]), None, N)
        check(got[3 * i + 2], t1, x1, N)
        check(base[3 * i], t0, x0, N)
        assert np.array_equal(got[3 * i].view(np.uint32), base[3 * i].view(np.uint32)), N


def test_union_two_chained_launches(sweep):
    """Ku = 65: dls_subset_fedavg_union_f32 chains a second launch (k_subset_union
    <ACC>) that continues the running sums in `out`.  Every client row is a
    rolled / negated binade sweep, so the clients on both sides of the chunk seam
    (63 | 64) carry every binade, zeros, denormals, inf and nan; coalitions that
    sit in the first launch, in the second, and across the seam, with divisors of
    both two-constant classes, 2^31 and the first slow divisor."""
    Ku, P = 65, len(sweep)
    U = np.stack([np.roll(sweep if j % 2 == 0 else -sweep, 2049 * 3 * j + j) for j in range(Ku)])
    w = [float(1 + (37 * j) % 1000) for j in range(Ku)]
    w[64] = 3.0
    coalitions = [list(range(Ku)), [63, 64], [64], [0, 64], [60, 61, 62, 63, 64], [0], [63]]
    totals = [55123.0, 11735695.0, 7.0, 2147483648.0, 2147483904.0, 3.0, 16777218.0]
    members = [[c for c, co in enumerate(coalitions) if j in co] for j in range(Ku)]
    got = run_union(torch.from_numpy(U).to(dev), w, members, totals).cpu().numpy()
    for c, co in enumerate(coalitions):
        ref = R.fold([R.weighted_terms(U[j], w[j], totals[c]) for j in co])
        check(got[c], ref, None, (c, totals[c]))


# ------------------------------------------------------------ (d) dequant-FedAvg
def store_of(payloads):
    from distributed_learning_simulator_amd.quant_store import QuantizedClientStore
    store = QuantizedClientStore(payloads[0], dev, capacity=len(payloads))
    rows = []
    for p in payloads:
        r = store.acquire()
        store.write(r, p)
        rows.append(r)
    return store, rows


def store_fedavg(store, rows, weights, total, mode=0):
    out = torch.full((store.layout.P,), float("nan"), device=dev)
    store.fedavg(rows, torch.tensor(weights, dtype=torch.float32, device=dev), out=out,
                 total=float(total), mode=mode)
    return out.cpu().numpy()


def only_groups(store, mode, groups):
    """The tile table of `mode` has tiles in exactly these groups and no general tile."""
    _, ntiles, nfast = store.table(mode)
    assert [g for g in range(len(nfast)) if nfast[g]] == sorted(groups), nfast
    assert ntiles == sum(nfast), (ntiles, nfast)


@functools.lru_cache(maxsize=None)
def f32_sweep_store():
    x = R.device_sweep(4096)
    U = np.stack([x, np.roll(-x, 2049), x[::-1]])
    store, rows = store_of([{"f": torch.from_numpy(u.copy())} for u in U])
    return U, store, rows


@pytest.mark.parametrize("mode", [0, 1], ids=["exact", "fma"])
@pytest.mark.parametrize("N", QUANT_TOTALS)
def test_dequant_f32_tensor_binade_sweep(N, mode):
    """f32_side_tile (tile group 8; in FMA mode the same exact walk inside
    quant_fma.hip's kernel): an fp32 tensor holding the binade sweep, K = 1 with
    weight 1 and K = 3 with weights 3, 0.5, 1000 (-0 + +0, denormal sums,
    inf - inf).  The wave-uniform `__ballot(!ok)` switch sees all-fast, all-slow
    and mixed waves.  ~1.05 M elements: every binade's first and last mantissa."""
    U, store, rows = f32_sweep_store()
    only_groups(store, mode, [8])
    n = U.shape[1]
    got = store_fedavg(store, rows[:1], [1.0], N, mode)
    check(got[:n], R.weighted_terms(U[0], 1.0, N), U[0], "K=1")
    assert not got[n:].any()  # the row padding stays zero
    w = [3.0, 0.5, 1000.0]
    got = store_fedavg(store, rows, w, N, mode)
    check(got[:n], R.fold([R.weighted_terms(U[i], w[i], N) for i in range(3)]), None, "K=3")


@pytest.mark.parametrize("mode", [0, 1], ids=["exact", "fma"])
@pytest.mark.parametrize("N", QUANT_TOTALS)
def test_dequant_f32_tensor_poisoned_tiles(mant, N, mode):
    """f32_side_tile's wave-uniform switch: 2^16 strided mantissas (256 tiles of
    256) with one out-of-range value in every third tile only, so a wave's 64
    lanes are all fast (common branch) or one lane is not (div_exact branch for
    all).  In-range neighbours keep the bits of the clean run; K = 2 so the
    switch is taken per client."""
    x = mant[::128].copy()
    y, mask = poisoned(x, every=3)
    z = np.roll(x, 77)
    store, rows = store_of([{"f": torch.from_numpy(a.copy())} for a in (x, y, z)])
    only_groups(store, mode, [8])
    w = [3.0, 1.0]
    clean = store_fedavg(store, [rows[0], rows[2]], w, N, mode)
    got = store_fedavg(store, [rows[1], rows[2]], w, N, mode)
    tz = R.weighted_terms(z, 1.0, N)
    check(clean, R.fold([R.weighted_terms(x, 3.0, N), tz]), x)
    check(got, R.fold([R.weighted_terms(y, 3.0, N), tz]), y)
    assert np.array_equal(got.view(np.uint32)[~mask], clean.view(np.uint32)[~mask])


QUANT_C = 4096


def quant_weights(N):
    """Sample counts [n_0, n_1] with n_0 + n_1 = N, both positive, n_0 a power of two
    (so scale * n_0 is exact and the edge scales sit exactly on scale_fast's
    bounds): 2^15 for 55123, 2^20 for the larger totals."""
    w0 = 1 << 15 if N < 1 << 21 else 1 << 20
    assert 0 < w0 < N
    return [w0, N - w0]


def _scales(w0):
    """Client 0's per-channel scales: 4096 strided mantissas of [1, 2) times 2^-10,
    then six channels whose scale * w0 sits one ulp below / at / one ulp above
    scale_fast's bounds 2^-59 and 2^50."""
    # stride 2048 with a per-channel offset: bare multiples of 2048 have 11 zero low
    # bits, and then fl(zp * s) would be exact for every 8-bit zero point
    c = np.arange(QUANT_C)
    s = (R.mantissa_sweep()[c * 2048 + (c * 977) % 2048] * np.float32(2.0 ** -10)).astype(np.float32)
    assert len(s) == QUANT_C
    edge = []
    for v in (2.0 ** -59 / w0, 2.0 ** 50 / w0):
        b = int(np.float32(v).view(np.uint32))
        edge += [b - 1, b, b + 1]
    return np.concatenate([s, np.array(edge, np.uint32).view(np.float32)])


@functools.lru_cache(maxsize=None)
def int_clients(rl, w0):
    """Two clients x (int8 tensor "a", zero point 0; uint8 tensor "b", zero points
    128 / c % 256) of C = 4102 channels with rows of rl elements holding every
    byte value in turn (so q == zero_point occurs)."""
    s0 = _scales(w0)
    C = len(s0)
    s1 = np.concatenate([s0[:QUANT_C][::-1], s0[:C - QUANT_C]]).astype(np.float32)
    c = np.arange(C)[:, None]
    e = np.arange(rl)[None, :]
    zb = np.where(np.arange(C) % 2 == 0, 128, np.arange(C) % 256).astype(np.int64)
    clients = []
    for k, s in enumerate((s0, s1)):
        q = ((c * (7 - 2 * k) + e * (1 + 2 * k) + k) % 256).astype(np.uint8)
        clients.append({"a": (q.view(np.int8).copy(), s.astype(np.float64), np.zeros(C, np.int64)),
                        "b": (q[::-1].copy(), s.astype(np.float64), zb)})
    assert all((cl["b"][0] == zb[:, None]).any() and (cl["a"][0] == 0).any() for cl in clients)
    return clients, [("a", (C, rl)), ("b", (C, rl))]


@functools.lru_cache(maxsize=None)
def int_store(rl, w0):
    clients, layout = int_clients(rl, w0)
    payloads = [{k: tuple(torch.from_numpy(t) for t in v) for k, v in cl.items()} for cl in clients]
    store, rows = store_of(payloads)
    return clients, store, rows, layout


def _int_reference(clients, layout, n, N):
    ref = oquant.dequant_fedavg(clients, n, [0, 1], layout)
    # the same, written out: fl(fl(fl(fl(q - zp) * s) * n) / N), summed in order
    parts = []
    for name, _ in layout:
        terms = [R.dequant_terms(cl[name][0].astype(np.int64), cl[name][2][:, None],
                                 cl[name][1].astype(np.float32)[:, None], n[k], N).reshape(-1)
                 for k, cl in enumerate(clients)]
        parts.append(R.fold(terms))
    assert same_bits(np.concatenate(parts), ref)
    return ref


def common_channels(clients, name, n, N):
    """Per channel: does EVERY client meet the kernels' common-path conditions
    (restated: N in [1, 2^31], fl(zp * s) exact, 2^-59 <= fl(s * n_i) <= 2^50)?
    The one-channel walk decides per (channel, 64-client chunk), the staged lane
    walk per (tile of <= 4 channels, chunk); K = 2 is one chunk."""
    ok = np.full(len(clients[0][name][1]), R.in_fast_divisor_range(N))
    for cl, w in zip(clients, n):
        s = cl[name][1].astype(np.float32)
        z = cl[name][2].astype(np.float32)
        sw = s * np.float32(w)
        ok &= (z.astype(np.float64) * s.astype(np.float64) == (z * s).astype(np.float64))
        ok &= (sw >= np.float32(2.0 ** -59)) & (sw <= np.float32(2.0 ** 50))
    return ok


def assert_branch_coverage(clients, n, N):
    """Which branches the case reaches, from the inputs: for a total inside
    [1, 2^31] tensor "a" (zero point 0) is on the common path in every channel but
    the two edge channels one ulp outside scale_fast's bounds, tensor "b" in its
    even channels (zero point 128) and off it in most odd ones (inexact fl(zp * s));
    for 2147483904 nothing is."""
    a, b = common_channels(clients, "a", n, N), common_channels(clients, "b", n, N)
    if not R.in_fast_divisor_range(N):
        assert not a.any() and not b.any()
        return
    assert np.array_equal(np.flatnonzero(~a), [QUANT_C, QUANT_C + 5]), np.flatnonzero(~a)
    assert b[0:QUANT_C:2].all() and (~b[1:QUANT_C:2]).sum() > QUANT_C // 4
    # four consecutive channels of "a" on the common path: staged lane tiles run accum16_pk
    assert a[:QUANT_C].all()


# row length -> the tile group its tensors land in (exact-mode table)
INT_WALKS = {1024: 3, 400: 7, 16: 7, 27: 9}


@pytest.mark.parametrize("N", QUANT_TOTALS)
@pytest.mark.parametrize("rl", sorted(INT_WALKS))
def test_dequant_int_tensors_scale_sweep(rl, N):
    """Exact dequant-FedAvg of int8 / uint8 tensors whose 4096 per-channel scales
    sweep strided mantissas, plus channels with scale * weight one ulp either side
    of scale_fast's 2^-59 and 2^50.  Both sample counts are positive
    (quant_weights), so the chunk-wide common paths run; assert_branch_coverage
    derives from the inputs which channels take them.  Row lengths pick the walk:
      1024: the one-channel walk (group 3; k_dequant_fast<1>): the common chunk
            loop for "a" and the even channels of "b", the per-client ZFMA /
            non-ZFMA / IEEE paths for the odd channels of "b" and the two
            out-of-range edge channels;
      400:  lane tiles of <= 4 channels (group 7; lane_tile's staged LDS table and
            accum16_pk for "a", the per-client path for "b", whose every tile
            holds an odd channel);
      16:   lane tiles spanning 64 channels (group 7; lane_tile's per-client path);
      27:   the short-row walk (group 9; small_side_tile).
    Totals pick the quotient on those common paths:
      55123:      two-constant with yl != 0 (accum16_one<TWO>; accum16_pk's
                  inline-asm two-constant quotient);
      2147483648: two-constant with yl == 0 (the quotient is fma(t, yh, 0));
      11735695:   rejected by the two-constant proof: packed Markstein;
      2147483904: outside [1, 2^31]: IEEE division everywhere, no common path.
    Reference: oracle.quant.dequant_fedavg (all totals are integers), cross-checked
    against the formula written out in numpy fp32.
    Not reached by these shapes: one-channel tiles of 2-4 KiB (groups 0-2), lane
    tiles wider than 1 KiB (groups 4-6: the exact table always cuts 1 KiB lane
    tiles), and the general tiles of rows shorter than 4 elements
    (k_dequant_general: int_lane_channels, int_tiny_rows)."""
    n = quant_weights(N)
    clients, store, rows, layout = int_store(rl, n[0])
    only_groups(store, 0, [INT_WALKS[rl]])
    assert_branch_coverage(clients, n, N)
    got = store_fedavg(store, rows, [float(np.float32(x)) for x in n], N)
    views = store.layout.views(torch.from_numpy(got))
    flat = np.concatenate([views[name].reshape(-1).numpy() for name, _ in layout])
    check(flat, _int_reference(clients, layout, n, N), None, (rl, N))


@pytest.mark.parametrize("N", QUANT_TOTALS)
def test_dequant_short_rows_exact_in_fma_mode(N):
    """quant_fma.hip's group 9 (the short-row walk small_side_tile inside the FMA
    mode's kernel) is exact arithmetic too: rows of 27 elements, the same scale
    sweep, bit for bit."""
    n = quant_weights(N)
    clients, store, rows, layout = int_store(27, n[0])
    only_groups(store, 1, [9])
    got = store_fedavg(store, rows, [float(np.float32(x)) for x in n], N, mode=1)
    views = store.layout.views(torch.from_numpy(got))
    flat = np.concatenate([views[name].reshape(-1).numpy() for name, _ in layout])
    check(flat, _int_reference(clients, layout, n, N), None, N)
