"""GPU: the MFMA subset contraction (dls_subset_gemm_f32) element by element, at every
edge of its dispatch (csrc/shapley.hip; the plan is restated in
tests/subset_gemm_ref.py), against the fp64 product: bit for bit on exact cases, within
the derived elementwise bound on real weights.

Every direct call goes through ``launch``: ``out`` is [S + 2, ldo > P] prefilled with
a NaN payload pattern, ``U`` is [K + 3, ldu > P] with NaN in U[:, P:] and in the rows
that ``rows`` does not name; out[:, P:], out[S:] and all of U must come back with the
same bits, and an element of out[:S, :P] the kernel did not write still holds its NaN."""
import numpy as np
import pytest
import torch

from tests import subset_gemm_ref as R

pytestmark = pytest.mark.gpu

dev = torch.device("cuda")
NAN = float("nan")
SMALL_P = (4, 124, 128, 132, 388)  # one lane; ragged / exact / just past one tile; 3 tiles + 4


def ibits(t):
    return t.view(torch.int32)


def payload(nrows, ld):
    """int32 [nrows, ld]: a different quiet-NaN payload in every element."""
    idx = torch.arange(nrows * ld, dtype=torch.int64, device=dev)
    return (0x7FC00000 | ((idx * 2654435761 + 12345) % 0x3FFFFF + 1)).to(torch.int32).reshape(nrows, ld)


def store(Uc, rows, ldu):
    """fp32 [K + 3, ldu] device tensor: NaN everywhere but U[rows[k], :P] = Uc[k]
    (rows listed twice must hold equal contents)."""
    K, P = Uc.shape
    assert ldu > P and ldu % 4 == 0
    U = torch.full((K + 3, ldu), NAN, dtype=torch.float32, device=dev)
    U[torch.as_tensor(np.asarray(rows), device=dev).long(), :P] = torch.as_tensor(Uc, device=dev)
    return U


def launch(C, U, rows, P, ldo=None):
    """One call on sentinel-guarded buffers; returns out[:S, :P] (device)."""
    from distributed_learning_simulator_amd import _native
    C = torch.as_tensor(np.ascontiguousarray(C, dtype=np.float32)).to(dev) \
        if not torch.is_tensor(C) else C
    rows = torch.as_tensor(np.asarray(rows).astype(np.int32)).to(dev) \
        if not torch.is_tensor(rows) else rows
    S = C.shape[0]
    ldo = P + 12 if ldo is None else ldo
    assert ldo > P and ldo % 4 == 0 and U.stride(0) > P and U.stride(0) % 4 == 0
    want = payload(S + 2, ldo)
    out = want.clone().view(torch.float32)
    assert U.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    U0 = U.clone()
    _native.subset_gemm(C, U, rows, P, out)
    torch.cuda.synchronize()
    assert torch.equal(ibits(U), ibits(U0)), "U was written"
    assert torch.equal(ibits(out)[:, P:], want[:, P:]), "out[:, P:ldo] was written"
    assert torch.equal(ibits(out)[S:], want[S:]), "rows of out past S were written"
    return out[:S, :P]


def same_bits(got, ref):
    """got: device fp32; ref: numpy or device fp32.  Every element, bit for bit."""
    ref = torch.as_tensor(np.ascontiguousarray(ref, dtype=np.float32)).to(dev) \
        if not torch.is_tensor(ref) else ref
    return got.shape == ref.shape and torch.equal(ibits(got.contiguous()), ibits(ref.contiguous()))


def first_diff(got, ref):
    g, r = got.cpu().numpy(), np.asarray(ref, np.float32)
    bad = np.argwhere(g.view(np.uint32) != r.view(np.uint32))
    s, p = bad[0]
    return f"{len(bad)} of {g.size} elements differ, first at [{s}, {p}]: {g[s, p]!r} != {r[s, p]!r}"


def rows_of(kind, K, rng):
    """(rows, duplicate pairs): a random permutation prefix of the K + 3 store rows,
    the reversed range, or a permutation prefix with client rows listed twice."""
    if kind == "permuted":
        return rng.permutation(K + 3)[:K], []
    if kind == "reversed":
        return np.arange(K)[::-1].copy(), []
    r = rng.permutation(K + 3)[:K]
    pairs = [(K - 1, 0)] if K < 8 else [(K - 1, 0), (K // 2, K // 2 - 1), (min(K - 2, 256), 1)]
    for a, b in pairs:
        r[a] = r[b]
    return r, pairs


def run_exact(S, K, P, kind, seed):
    rng = np.random.default_rng([S, K, P, seed])
    C, Uc, ref, unit = R.exact_case(S, K, P, seed)
    rows, pairs = rows_of(kind, K, rng)
    if pairs:
        for a, b in pairs:
            Uc[a] = Uc[b]  # one store row, two coefficients
        ref = R.exact_result(C, Uc, unit)
    got = launch(C, store(Uc, rows, P + 4 * (1 + seed % 3)), rows, P, ldo=P + 4 * (1 + (seed + 1) % 3))
    assert same_bits(got, ref), (S, K, P, kind, first_diff(got, ref))


# ---------------------------------------------------------------- a. exact sweep
KS = [1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 13, 15, 16, 17, 18, 25, 26, 49, 50, 255, 256, 257, 258, 511,
      512, 513]
SS = [1, 31, 32, 33, 63, 64, 65, 96, 97, 128, 129]
# one K per (depth, padding) class of the rule, and one with a BETA chunk
CLASS_K = {(4, 0): 8, (4, 1): 5, (4, 3): 1, (5, 0): 10, (5, 1): 17, (5, 2): 25, "beta": 257}


def test_sweep_covers_the_dispatch():
    """The sets above against the rule in csrc/shapley.hip (restated in
    subset_gemm_ref.depth_of and tied to the source text by the host tests): both
    depths with no, one and the most padded k-steps, odd and even chunks in both,
    BETA with Kc in {1, 2, 255, 256}, a third chunk; a full S chunk followed by an
    MT = 1 and by an MT = 2 chunk.  Needs no device, but belongs to the sweep."""
    chunks = [(d["Kc"], d["beta"], d["depth"], d["padded"]) for K in KS for d in R.dispatch(1, K)]
    for depth in (4, 5):
        top = R.max_padding(depth)
        assert top >= 2
        for padded in (0, 1, top):
            hit = {Kc % 2 for Kc, _, d, p in chunks if (d, p) == (depth, padded)}
            assert hit, (depth, padded)
            assert CLASS_K[(depth, padded)] in KS
            assert R.depth_of(CLASS_K[(depth, padded)]) == (depth, padded)
        assert {Kc % 2 for Kc, _, d, _ in chunks if d == depth} == {0, 1}
        # the half-used k-step of an odd chunk next to padded steps, and alone
        assert any(Kc % 2 and p for Kc, _, d, p in chunks if d == depth)
        assert any(Kc % 2 and not p for Kc, _, d, p in chunks if d == depth)
    assert {Kc for Kc, beta, _, _ in chunks if beta} >= {1, 2, 255, 256}
    assert max(len(R.dispatch(1, K)) for K in KS) == 3
    assert len(R.dispatch(1, CLASS_K["beta"])) == 2
    tails = {(len(pl), pl[-1]["Sc"], pl[-1]["MT"]) for pl in (R.dispatch(S, 1) for S in SS)}
    assert {(1, 1, 1), (1, 32, 1), (1, 33, 2), (1, 64, 2), (2, 1, 1), (2, 32, 1), (2, 33, 2),
            (2, 64, 2), (3, 1, 1)} <= tails


@pytest.mark.parametrize("K", KS)
def test_exact_every_k(K):
    """Every K of the sweep, with one and with two M tiles, under each kind of
    ``rows``; P walks the small set."""
    i = KS.index(K)
    for j, kind in enumerate(("permuted", "reversed", "duplicated")):
        if kind == "duplicated" and K < 3:
            continue
        for m, S in enumerate((5, 40)):
            run_exact(S, K, SMALL_P[(i + j + 2 * m) % len(SMALL_P)], kind, seed=i + j)


@pytest.mark.parametrize("S", SS)
def test_exact_every_s(S):
    """Every S of the sweep against one K of each (depth, padding) class and one
    with a BETA chunk."""
    i = SS.index(S)
    for j, K in enumerate(CLASS_K.values()):
        kind = ("permuted", "reversed", "duplicated")[(i + j) % 3]
        run_exact(S, K, SMALL_P[(i + j) % len(SMALL_P)], kind if K >= 3 else "permuted", seed=i + j)


def test_exact_both_chunkings_at_once():
    """S and K chunked together: the C and out offsets of a second S chunk under a
    BETA launch, pitched."""
    for S, K, P in ((65, 257, 132), (97, 513, 124), (129, 258, 388), (70, 300, 128)):
        run_exact(S, K, P, "duplicated", seed=S)


# ------------------------------------------------ b. identity and one-hot layout
def grid_rows(K, P):
    """U[k][p] = 1 + k * P + p: a distinct integer for every (k, p), exact in fp32."""
    assert K * P + 1 < 2 ** 24
    return (1 + np.arange(K * P, dtype=np.int64).reshape(K, P)).astype(np.float32)


@pytest.mark.parametrize("S,K,P", [(70, 40, 388), (33, 40, 132), (129, 50, 128), (5, 300, 124)])
def test_identity_rows(S, K, P):
    """C rows of the identity (S > K wraps around): out[s] is one client row, bit for
    bit, which a swapped row, column, N tile or M tile anywhere in the 4-way
    interleave breaks."""
    rng = np.random.default_rng([S, K, P])
    pick = (7 * np.arange(S) + 3) % K
    C = np.zeros((S, K), np.float32)
    C[np.arange(S), pick] = 1.0
    Uc = grid_rows(K, P)
    rows = rng.permutation(K + 3)[:K]
    got = launch(C, store(Uc, rows, P + 8), rows, P)
    assert same_bits(got, Uc[pick]), first_diff(got, Uc[pick])


@pytest.mark.parametrize("K,hot", [(257, 256), (513, 511), (513, 512), (258, 257)])
def test_one_hot_in_a_later_chunk(K, hot):
    """All weight on one client of the second or third K chunk: the chunk offsets of
    ``rows`` and of C, and the BETA hand-over of exact zeros."""
    S, P = 65, 388
    rng = np.random.default_rng([K, hot])
    C = np.zeros((S, K), np.float32)
    C[:, hot] = 1.0
    C[1::2, hot] = 0.5
    C[2, hot], C[2, 3] = 0.0, 1.0  # one coalition that looks at the first chunk
    Uc = grid_rows(K, P)
    rows = rng.permutation(K + 3)[:K]
    ref = np.where(C[:, hot, None] > 0, C[:, hot, None] * Uc[hot][None, :], Uc[3][None, :])
    got = launch(C, store(Uc, rows, P + 4), rows, P)
    assert same_bits(got, ref.astype(np.float32)), first_diff(got, ref.astype(np.float32))


# ------------------------------------------------------------------ c. tile seam
# 256 CUs x at most 8 blocks of 256 threads x 4 waves = 8192 waves at the very most, so
# with more than 2 * 8192 tiles every wave of every launch walks at least two tiles
# (the flattened stream's seam and its prefetch of the next tile), and the + 388 ends
# the walk on three more tiles, the last one ragged (one lane wide).
SEAM_P = R.TILE_P * 8192 * 2 + R.TILE_P * 3 + 4


@pytest.mark.parametrize("S,K", [(1, 2), (33, 10), (5, 257)])
def test_tile_seam(S, K):
    """(1, 2): MT = 1, depth 4, three padded steps; (33, 10): MT = 2, depth 5; (5, 257):
    BETA, whose U [260, P + 4] is 2.18 GB of fp32 (it is generated, contracted in fp64
    and compared on the device).  U comes from integer randint on the device; the
    reference of the two small shapes is the host's fp64 product."""
    P = SEAM_P
    assert (P + R.TILE_P - 1) // R.TILE_P > 2 * 8192 and P % R.TILE_P == 4
    C, _, _, unit = R.exact_case(S, K, 4, seed=K, scale_exp=0)
    g = torch.Generator(device=dev).manual_seed(S * 1000 + K)
    rows = np.random.default_rng([S, K]).permutation(K + 3)[:K]
    rows_t = torch.as_tensor(rows, device=dev)
    U = torch.full((K + 3, P + 4), NAN, dtype=torch.float32, device=dev)
    for r in rows.tolist():  # row by row: no second copy of the 2 GB
        U[r, :P] = torch.randint(-64, 65, (P,), generator=g, device=dev).float()
    if K <= 16:
        Uh = U[rows_t, :P].cpu().numpy()
        ref = torch.from_numpy(R.exact_result(C, Uh, unit)).to(dev)
    else:
        # |C| . |U| <= K * 64 in units of 1/16: far below 2^24, every order is exact
        R.check_exact(C, np.full((K, 1), 64.0, np.float32), unit)
        assert float(U[rows_t, :P].abs().max()) <= 64
        ref64 = torch.matmul(torch.from_numpy(C).double().to(dev), U[rows_t, :P].double())
        ref = (ref64 + 0.0).float()
        assert torch.equal(ref.double(), ref64)
        del ref64
    got = launch(C, U, rows, P, ldo=P + 4)
    assert same_bits(got, ref), first_diff(got, ref.cpu().numpy())


# ------------------------------------------ d. elementwise bound on real weights
@pytest.mark.parametrize("S,K,P", [(50, 50, 4096 + 4), (70, 300, 2048 + 64), (129, 513, 388),
                                   (1, 1, 4)])
def test_elementwise_bound_real_weights(S, K, P):
    """Coefficients n_i / N_S of random coalitions as the servers build them, U ~
    0.05 N(0, 1): |got - C.U| <= g (|C| . |U|) in EVERY element, g = (K+1)u / (1 -
    (K+1)u) (subset_gemm_ref.abs_bound: derived, nothing added).  K = 1 is one
    rounded product: fl32(c u) bit for bit."""
    rng = np.random.default_rng([S, K, P])
    subsets, n = R.random_coalitions(S, K, rng)
    subsets[-1] = list(range(K))
    C, union = R.server_coefficients(subsets, n)
    assert union == list(range(K))
    Uc = (0.05 * rng.standard_normal((K, P))).astype(np.float32)
    # the bound's derivation assumes the normal range: no product of a non-zero
    # coefficient is below 2^-100 (a zero coefficient's products are exact zeros)
    assert np.abs(C[C != 0]).min() * np.abs(Uc).min() >= 2.0 ** -100
    rows = rng.permutation(K + 3)[:K]
    U = store(Uc, rows, P + 4)
    got = launch(C, U, rows, P).cpu().numpy()
    Un = U.cpu().numpy()
    ref, bound = R.contract(C, Un, rows, P), R.abs_bound(C, Un, rows, P)
    err = np.abs(got.astype(np.float64) - ref)
    worst = float((err / bound).max())
    print(f"S={S} K={K} P={P}: worst |err| / bound = {worst:.3f}, "
          f"worst |err| / (|C|.|U|) = {float((err * R.gamma(K) / bound).max()):.3e}")
    assert (err <= bound).all(), worst
    if K == 1:
        want = (C.astype(np.float32) * Uc.astype(np.float32)).astype(np.float32)
        assert same_bits(torch.from_numpy(got).to(dev), want)


# -------------------------------------------------------- e. non-finite rows
def test_non_finite_row_poisons_its_column_in_every_coalition():
    """The contract of include/dls_hip.h: the contraction multiplies every selected
    row by its coefficient, so a non-finite element of client i's row makes that
    column non-finite in EVERY coalition of the batch: NaN where the row holds NaN
    and wherever c_si = 0 (0 * inf), +inf where c_si > 0 meets +inf (IEEE 754, and
    what the fp64 product gives).  No other element changes by a bit, and a NaN in a
    row that ``rows`` does not name changes nothing."""
    S, K, P = 4, 6, 132
    C, Uc, _, unit = R.exact_case(S, K, P, seed=2)
    C[:, 2] = [0.5, 0.0, 0.25, 0.0]  # client 2 is a member of coalitions 0 and 2 only
    C[:, 0] = [0.0, 1.0, 0.0, 0.5]
    ref = R.exact_result(C, Uc, unit)
    rows = np.array([4, 0, 7, 2, 8, 5])  # store rows 1, 3, 6 hold NaN and are not named
    clean = launch(C, store(Uc, rows, P + 4), rows, P)
    assert same_bits(clean, ref), first_diff(clean, ref)
    bad = Uc.copy()
    bad[2, 5], bad[2, 77] = np.inf, np.nan
    got = launch(C, store(bad, rows, P + 4), rows, P).cpu().numpy()
    assert np.isnan(got[:, 77]).all()
    assert np.isnan(got[[1, 3], 5]).all()  # c = 0: 0 * inf
    assert np.isposinf(got[[0, 2], 5]).all()  # c > 0: the fp64 product says +inf too
    with np.errstate(all="ignore"):
        r64 = R.contract(C, bad, np.arange(K), P)
    assert np.array_equal(np.isnan(got), np.isnan(r64)) and np.array_equal(np.isinf(got), np.isinf(r64))
    keep = np.ones(P, bool)
    keep[[5, 77]] = False
    assert np.array_equal(got[:, keep].view(np.uint32), ref[:, keep].view(np.uint32))


# ------------------------------------------------------------ f. argument checks
def test_argument_checks_raise_and_write_nothing():
    from distributed_learning_simulator_amd import _native
    S, K, P = 3, 5, 8
    C = torch.full((S, K), 0.25, device=dev)
    rows = torch.arange(K, dtype=torch.int32, device=dev)
    wide = torch.ones((K, 16), device=dev)
    odd = torch.ones((K, 14), device=dev)  # a pitch that is no multiple of 4
    want = payload(S, 16)
    out = want.clone().view(torch.float32)
    want_odd = payload(S, 14)
    out_odd = want_odd.clone().view(torch.float32)
    bad = [("P % 4", C, wide, rows, 6, out),
           ("ldu % 4", C, odd, rows, P, out),
           ("ldo % 4", C, wide, rows, P, out_odd),
           ("U 4 bytes off", C, wide[:, 1:], rows, P, out),
           ("out 4 bytes off", C, wide, rows, P, out[:, 1:]),
           ("U 8 bytes off", C, wide[:, 2:], rows, P, out),
           ("S = 0", C[:0], wide, rows, P, out),
           ("K = 0", torch.empty((S, 0), device=dev), wide, rows[:0], P, out),
           ("P = 0", C, wide, rows, 0, out)]
    for name, c, u, r, p, o in bad:
        with pytest.raises(RuntimeError):
            _native.subset_gemm(c, u, r, p, o)
            pytest.fail(f"{name}: accepted")
        torch.cuda.synchronize()
        assert torch.equal(ibits(out), want) and torch.equal(ibits(out_odd), want_odd), name
    _native.subset_gemm(C, wide, rows, P, out)  # the same operands, well formed
    torch.cuda.synchronize()
    assert torch.equal(out[:, :P], torch.full((S, P), 1.25, device=dev))
    assert torch.equal(ibits(out)[:, P:], want[:, P:])


# ------------------------------------------------------------ g. through the store
def _filled_store(integer):
    from distributed_learning_simulator_amd.aggregation import ClientUpdateStore
    from distributed_learning_simulator_amd.layout import ParameterLayout
    lay = ParameterLayout([("w", (33, 31)), ("b", (5,))])
    st = ClientUpdateStore(lay, dev, capacity=14)
    g = torch.Generator().manual_seed(7)
    rows = [st.acquire() for _ in range(14)]
    for r in rows:
        if integer:
            d = {"w": torch.randint(-64, 65, (33, 31), generator=g).float(),
                 "b": torch.randint(-64, 65, (5,), generator=g).float()}
        else:
            d = {"w": torch.randn(33, 31, generator=g) * 0.05, "b": torch.randn(5, generator=g) * 0.05}
        st.write(r, d)
    spare = [rows[3], rows[13]]  # members of no coalition: never read
    st.U[spare[0]] = NAN
    st.U[spare[1]] = float("inf")
    return st, [r for r in rows if r not in spare]


def test_store_gemm_elementwise():
    """ClientUpdateStore.subset_models(method="gemm"): 70 coalitions (two S chunks)
    over 12 of the store's 14 rows, against the fp64 product of the coefficients it
    must build, within the elementwise bound; the two other rows hold NaN and inf."""
    st, rows = _filled_store(integer=False)
    rng = np.random.default_rng(3)
    n = {r: 50 + 13 * r for r in rows}
    subs = [sorted(rng.permutation(rows)[: 1 + s % 12].tolist()) for s in range(70)]
    U0 = st.U.clone()
    got = st.subset_models(subs, n, method="gemm").cpu().numpy()
    assert torch.equal(ibits(st.U), ibits(U0))
    C, union = R.server_coefficients(subs, n)
    assert union == sorted(rows)
    U, P = U0.cpu().numpy(), st.layout.P
    assert got.shape == (70, P)
    err = np.abs(got.astype(np.float64) - R.contract(C, U, union, P))
    assert (err <= R.abs_bound(C, U, union, P)).all()


def test_store_gemm_equals_exact_on_dyadic_coalitions():
    """Integer-valued rows, equal n, coalitions of 1, 2, 4 and 8 clients: c = 1/|S| is a
    power of two, every product and sum is exact on both paths, so method="gemm" and
    method="exact" give the same bits."""
    st, rows = _filled_store(integer=True)
    rng = np.random.default_rng(4)
    n = {r: 100 for r in rows}
    subs = [sorted(rng.permutation(rows)[: 1 << (s % 4)].tolist()) for s in range(70)]
    a = st.subset_models(subs, n, method="gemm")
    b = st.subset_models(subs, n, method="exact")
    assert same_bits(a, b), first_diff(a, b.cpu().numpy())
    C, union = R.server_coefficients(subs, n)
    ref = R.contract(C, st.U.cpu().numpy(), union, st.layout.P)
    assert np.array_equal(a.cpu().numpy().astype(np.float64), ref)
