"""GPU tests of dls_rows_gram_f32 / dls_history_gram_f32 (Gram matrix of client rows,
read-only and fused with the in-place history fold).  The folded history is compared
bit for bit with the numpy float32 reference tests/foolsgold_ref.py, G entrywise with
the exact Gram matrix at the contract's bound (120 + 8) * 2^-24 * sum_p |h_a h_b|, and
the exact properties (symmetry, permutation, equal rows, repeats, streams, layout) as
bits."""
import ctypes

import numpy as np
import pytest
import torch

from tests import foolsgold_ref as FR

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SENTINEL = 0x7FC0BEEF  # a NaN: pad columns, unlisted rows

KS = [1, 2, 7, 8, 9, 16, 17, 33, 64]
MAX_WAVES = 1024  # the kernel's kMaxWaves


def period(K):
    """Coordinates per flush period of the kernel's work split for K rows (GramCfg)."""
    g = 1 if K <= 8 else 2 if K <= 16 else 4 if K <= 32 else 8
    sl, tw = 64 // (g * g), 256 // g
    return (120 // (tw // sl)) * tw


def sizes(K):
    """P = 4; below every tile; a period plus 36 (ends in a partial quad group); an exact
    period; the smallest P at which a wave takes more than one period; many waves."""
    return [4, 28, period(K) + 36, period(K), MAX_WAVES * period(K) + 4, 70004]


def bits64(G):
    return np.ascontiguousarray(G, dtype=np.float64).view(np.uint64)


def dev_rows(rows):
    return torch.tensor([int(r) for r in rows], dtype=torch.int32, device=DEV)


def store(X, rows, n, ld):
    """A [n, ld] uint32 store holding fp32 row X[k] at rows[k], SENTINEL elsewhere."""
    K, P = X.shape
    U = np.full((n, ld), SENTINEL, np.uint32)
    U[list(rows), :P] = np.ascontiguousarray(X, np.float32).view(np.uint32)
    return U


def to_dev(U32, P):
    t = torch.from_numpy(U32.view(np.float32)).to(DEV)
    return t, (t[:, :P] if t.shape[1] != P else t)


def gram(X, rows=None, ld=None, n=None, base=None, stream=None):
    """dls_rows_gram_f32 on fp32 [K, P] rows placed in a store: fp64 [K, K] (numpy)."""
    from distributed_learning_simulator_amd import _native
    X = np.ascontiguousarray(X, np.float32)
    K, P = X.shape
    rows = list(range(K)) if rows is None else [int(r) for r in rows]
    _, Uv = to_dev(store(X, rows, max(rows) + 1 if n is None else n, P if ld is None else ld), P)
    b = None if base is None else torch.from_numpy(np.ascontiguousarray(base, np.float32)).to(DEV)
    if stream is None:
        return _native.rows_gram(Uv, dev_rows(rows), P, base=b).cpu().numpy()
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):
        G = _native.rows_gram(Uv, dev_rows(rows), P, base=b, stream=stream)
    stream.synchronize()
    return G.cpu().numpy()


def check_bound(G, Hh, what):
    """|G - exact| <= TOL * sum |h_a h_b| entrywise, the worst ratio printed first."""
    want, scale = FR.gram_and_abs(Hh)
    err = np.abs(G - want)
    with np.errstate(all="ignore"):
        worst = np.where(scale > 0, err / scale, err).max()
    print(f"{what}: max |G - exact| / sum|h_a h_b| = {worst:.3e} (bound {FR.TOL:.3e})")
    assert np.isfinite(G).all()
    assert (err <= FR.TOL * scale).all(), (what, float(worst))
    assert np.array_equal(bits64(G), bits64(G).T), "G[a][b] has the bits of G[b][a]"


def rows_for(K, P, seed, corr=0.3, like=None):
    """fp32 [K, P] rows.  Short ones: Gaussian values of mixed scale (the exact sums go
    through Sum2); long ones: grid values, whose exact sums are a matrix product.  ``like``:
    the row count that decides which (a base follows the rows it is subtracted from)."""
    like = K if like is None else like
    if like * like * P <= 4_000_000:
        rng = np.random.default_rng(seed)
        X = corr * rng.standard_normal(P)[None, :] + rng.standard_normal((K, P))
        return (X * 10.0 ** rng.integers(-2, 3, (1, P))).astype(np.float32)
    return FR.grid_rows(K, P, seed, corr=corr)


# ------------------------------------------------------ the fold and its Gram matrix
@pytest.mark.parametrize("with_base", [False, True])
@pytest.mark.parametrize("size", range(6))
@pytest.mark.parametrize("K", KS)
def test_fold_and_gram(K, size, with_base):
    from distributed_learning_simulator_amd import _native
    P = sizes(K)[size]
    seed = 1000 * K + P % 997 + with_base
    rng = np.random.default_rng(seed)
    X, H0 = rows_for(K, P, seed), rows_for(K, P, seed + 1, corr=0.0)
    base = rows_for(1, P, seed + 2, like=K)[0] if with_base else None
    extra = 5 if K * P < 4_000_000 else 1
    rows, hrows = rng.permutation(K + extra)[:K], rng.permutation(K + extra + 2)[:K]
    ldu, ldh = P + 8, P + 4  # ldu != ldh, both with pad columns
    Ufull, Uv = to_dev(store(X, rows, K + extra, ldu), P)
    Hfull, Hv = to_dev(store(H0, hrows, K + extra + 2, ldh), P)
    b = None if base is None else torch.from_numpy(base).to(DEV)
    r, hr = dev_rows(rows), dev_rows(hrows)
    want = H0
    for fold in (1, 2, 3):
        Hret, G = _native.history_gram(Uv, r, Hv, hr, P, base=b)
        assert Hret is Hv
        want = FR.fold_bits(want, X, base).view(np.float32)
        if fold == 2:
            continue
        got = Hfull.cpu().numpy().view(np.uint32)
        what = f"K={K} P={P} base={with_base} fold {fold}"
        assert np.array_equal(got[hrows, :P], want.view(np.uint32)), what
        rest = np.ones(got.shape, bool)
        rest[hrows, :P] = False
        assert (got[rest] == SENTINEL).all(), "pad columns and unlisted rows keep the sentinel"
        # the bits of the read-only call on the folded history, no base
        G, again = G.cpu().numpy(), _native.rows_gram(Hv, hr, P).cpu().numpy()
        assert np.array_equal(bits64(again), bits64(G)), what
        if fold == 3:
            check_bound(G, want, what)
    # U is only read
    assert np.array_equal(Ufull.cpu().numpy().view(np.uint32), store(X, rows, K + extra, ldu))
    # the read-only call on the updates
    Gu = _native.rows_gram(Uv, r, P, base=b).cpu().numpy()
    check_bound(Gu, FR.updates(X, base), f"K={K} P={P} base={with_base} rows_gram")


# ----------------------------------------------------------- exact properties
@pytest.mark.parametrize("K, P", [(7, 1088), (10, 2052), (33, 484), (64, 70004)])
def test_permutation_layout_repeat_and_stream(K, P):
    rng = np.random.default_rng(K)
    X = rows_for(K, P, K + 2)
    base = rows_for(1, P, K + 3, like=K)[0]
    first = bits64(gram(X, base=base))
    assert np.array_equal(bits64(gram(X, base=base)), first)
    assert np.array_equal(bits64(gram(X, base=base, stream=torch.cuda.Stream(DEV))), first)
    for _ in range(3):
        perm = rng.permutation(K)
        assert np.array_equal(bits64(gram(X[perm], base=base)), first[np.ix_(perm, perm)])
    rows = rng.permutation(K + 9)[:K]  # scattered rows at another pitch: the same bits
    assert np.array_equal(bits64(gram(X, rows=rows, ld=P + 12, n=K + 9, base=base)), first)


def test_permuting_rows_and_hrows_permutes_the_fold():
    from distributed_learning_simulator_amd import _native
    K, P = 17, 1000
    rng = np.random.default_rng(5)
    X, H0 = rows_for(K, P, 1), rows_for(K, P, 2)
    out = []
    for perm in (np.arange(K), rng.permutation(K)):
        _, Uv = to_dev(store(X, range(K), K, P), P)
        Hfull, Hv = to_dev(store(H0, range(K), K, P), P)
        _, G = _native.history_gram(Uv, dev_rows(perm), Hv, dev_rows(perm), P)
        out.append((perm, bits64(G.cpu().numpy()), Hfull.cpu().numpy().view(np.uint32)))
    (_, G0, Ha), (perm, G1, Hb) = out
    assert np.array_equal(G1, G0[np.ix_(perm, perm)]) and np.array_equal(Ha, Hb)


def test_history_gram_on_a_side_stream_gives_the_current_stream_bits():
    from distributed_learning_simulator_amd import _native
    K, P = 3, 8
    g = torch.Generator().manual_seed(11)
    U, H0 = torch.randn(8, 16, generator=g).to(DEV), torch.randn(8, 16, generator=g).to(DEV)
    base = torch.randn(16, generator=g).to(DEV)
    r, hr = dev_rows([5, 0, 2]), dev_rows([1, 7, 4])
    Ha, Ga = _native.history_gram(U, r, H0.clone(), hr, P, base=base)
    side, Hb = torch.cuda.Stream(DEV), H0.clone()
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        _, Gb = _native.history_gram(U, r, Hb, hr, P, base=base, stream=side)
    side.synchronize()
    assert torch.equal(Ha.view(torch.int32), Hb.view(torch.int32))
    assert torch.equal(Ga.view(torch.int64), Gb.view(torch.int64))
    assert not torch.equal(Ha, H0)  # the fold happened


@pytest.mark.parametrize("K, P", [(5, 1088), (9, 484), (40, 2052)])
def test_equal_rows_give_equal_diagonal_and_off_diagonal_bits(K, P):
    X = rows_for(K, P, K + 3)
    a, b = 1, K - 1  # the last row: next to the padding
    X[b] = X[a]
    G = bits64(gram(X))
    assert G[a, b] == G[a, a] == G[b, b] == G[b, a]
    assert np.array_equal(G[a], G[b])
    # ... and for histories that became equal by the fold
    from distributed_learning_simulator_amd import _native
    _, Uv = to_dev(store(X, range(K), K, P), P)
    _, Hv = to_dev(np.zeros((K, P), np.uint32), P)
    _, Gh = _native.history_gram(Uv, dev_rows(range(K)), Hv, dev_rows(range(K)), P)
    assert np.array_equal(bits64(Gh.cpu().numpy()), G)  # 0 + x == x: the rows' own Gram


@pytest.mark.parametrize("K", [9, 64])
def test_non_finite_row_poisons_its_own_row_and_column_only(K):
    P = 1088
    X = rows_for(K, P, K + 4)
    bad = (2, K - 1)
    X[bad[0], [3, 100, 700]] = [np.inf, -np.inf, np.nan]
    X[bad[1], 1087] = np.nan
    G = gram(X)
    involved = np.zeros((K, K), bool)
    involved[list(bad), :] = involved[:, list(bad)] = True
    assert (~np.isfinite(G[involved])).all() and np.isfinite(G[~involved]).all()
    clean = [k for k in range(K) if k not in bad]
    check_bound(G[np.ix_(clean, clean)], X[clean], f"K={K} clean rows")


# ------------------------------------------------------- P == 0 and the error codes
def test_zero_length_rows_write_zeros_and_touch_nothing_else():
    from distributed_learning_simulator_amd import _native
    U = torch.randn(5, 64, device=DEV)
    H = torch.randn(6, 64, device=DEV)
    H0 = H.clone()
    r = dev_rows([4, 0, 2])
    out = torch.full((3, 3), -1.0, dtype=torch.float64, device=DEV)
    assert _native.rows_gram(U, r, 0, out=out) is out and (bits64(out.cpu().numpy()) == 0).all()
    out.fill_(-1.0)
    _, G = _native.history_gram(U, r, H, dev_rows([5, 1, 3]), 0, out=out)
    assert G is out and (bits64(out.cpu().numpy()) == 0).all() and torch.equal(H, H0)


def test_argument_errors_return_their_codes_without_a_launch():
    from distributed_learning_simulator_amd import _native
    L = _native.lib()
    U = torch.zeros(4, 64, device=DEV)
    H = torch.ones(4, 64, device=DEV)
    r = dev_rows([0, 1, 2])
    G = torch.full((3, 3), -1.0, dtype=torch.float64, device=DEV)
    W = torch.zeros(int(L.dls_rows_gram_workspace(3, 64)), dtype=torch.uint8, device=DEV)
    p = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)  # noqa: E731

    def fold(U_=p(U), ldu=64, rows=p(r), H_=p(H), ldh=64, hrows=p(r), K=3, P=64, base=None,
             G_=p(G), W_=p(W)):
        return L.dls_history_gram_f32(U_, ldu, rows, H_, ldh, hrows, K, P, base, G_, W_, None)

    def read(U_=p(U), ldu=64, rows=p(r), K=3, P=64, base=None, G_=p(G), W_=p(W)):
        return L.dls_rows_gram_f32(U_, ldu, rows, K, P, base, G_, W_, None)

    for arg in ("U_", "rows", "H_", "hrows", "G_", "W_"):
        assert fold(**{arg: None}) == -1 and b"null pointer" in L.dls_last_error()
    for arg in ("U_", "rows", "G_", "W_"):
        assert read(**{arg: None}) == -1 and b"null pointer" in L.dls_last_error()
    for f in (fold, read):
        assert f(K=0) == -1 and f(K=65) == -1 and b"DLS_ROBUST_MAX_K=64" in L.dls_last_error()
        assert f(P=-4) == -1
        assert f(P=62) == -2 and f(ldu=60) == -2 and f(ldu=66) == -2
        assert f(U_=p(U, 4)) == -2 and f(base=p(U, 8)) == -2 and f(W_=p(W, 8)) == -2
        assert f(G_=p(G, 4)) == -2 and b"alignment" in L.dls_last_error()
    assert fold(ldh=60) == -2 and fold(ldh=66) == -2 and fold(H_=p(H, 4)) == -2
    assert L.dls_rows_gram_workspace(0, 64) == -1 and L.dls_rows_gram_workspace(3, -4) == -1
    torch.cuda.synchronize(DEV)
    assert (G == -1.0).all() and (H == 1.0).all()  # nothing ran
    # the wrapper refuses a repeated history row before the call
    with pytest.raises(RuntimeError, match="hrows must be distinct"):
        _native.history_gram(U, r, H, dev_rows([1, 2, 1]), 64)
    with pytest.raises(RuntimeError, match="outside the matrix"):
        _native.history_gram(U, r, H, dev_rows([1, 2, 4]), 64)
    with pytest.raises(RuntimeError, match="must not overlap"):
        _native.history_gram(U, r, U, r, 64)
    assert (H == 1.0).all()


# ----------------------------------------------------------------------- store
def test_store_gram_and_fold_history():
    from distributed_learning_simulator_amd.aggregation import ClientUpdateStore
    from distributed_learning_simulator_amd.layout import ParameterLayout
    lay = ParameterLayout([("a", (1000,)), ("b", (37,)), ("c", (3, 50))])
    st = ClientUpdateStore(lay, DEV, capacity=12)
    rng = np.random.default_rng(3)
    U = rng.standard_normal((12, lay.P)).astype(np.float32)
    st.U.copy_(torch.from_numpy(U))
    base = rng.standard_normal(lay.P).astype(np.float32)
    b = torch.from_numpy(base).to(DEV)
    rows, ids = [7, 1, 10, 4], [3, 20, 0, 5]
    G = st.gram(rows, base=b)
    assert G.dtype == torch.float64 and tuple(G.shape) == (4, 4)
    check_bound(G.cpu().numpy(), FR.updates(U[rows], base), "store.gram")
    assert st.history is None
    G1 = st.fold_history(rows, ids, b).cpu().numpy()
    assert st.history.shape[0] >= 21 and st.history.shape[1] == lay.P
    H1 = FR.fold_bits(np.zeros((4, lay.P), np.float32), U[rows], base)
    got = st.history.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[ids], H1)
    assert (np.delete(got, ids, axis=0) == 0).all()
    check_bound(G1, H1.view(np.float32), "store.fold_history")
    st.fold_history(rows[:2], [40, 3], b)  # grows, contents kept
    got = st.history.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[[20, 0, 5]], H1[1:])
    assert np.array_equal(got[3], FR.fold_bits(H1[:1].view(np.float32), U[[1]], base)[0])
    st.reset_history(20)
    assert (st.history[20] == 0).all() and (st.history[5] != 0).any()
    st.reset_history()
    assert (st.history == 0).all()
    for bad in ([3, 3, 0, 5], [3, -1, 0, 5]):
        with pytest.raises(ValueError, match="distinct non-negative"):
            st.fold_history(rows, bad, b)
