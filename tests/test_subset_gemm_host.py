"""CPU checks of the subset-contraction reference (tests/subset_gemm_ref.py), of the
numpy double that stands in for the kernel in the host tests, and of the host path
``ClientUpdateStore.subset_models(method="gemm")``."""
import os

import numpy as np
import pytest
import torch

from tests import cpu_doubles
from tests import subset_gemm_ref as R

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture
def doubles(monkeypatch):
    cpu_doubles.install(monkeypatch)


# ------------------------------------------------------------- fp32 evaluations
def _terms(C, U, fused):
    """[K, S, P] terms; unfused: fl32(c * u); fused: the exact products in fp64 (a
    fused multiply-add rounds only the sum)."""
    t = C.T.astype(np.float64)[:, :, None] * U.astype(np.float64)[:, None, :]
    return t if fused else t.astype(np.float32)


def _add(acc, t):
    """fl32(acc + t): acc fp32; t fp32, or the exact fp64 product of a fused step (the
    fp64 sum of an fp32 value and a 48-bit product can round twice, which no case
    here is sensitive to: the exact cases never round, and the bound allows it)."""
    return (acc.astype(np.float64) + t.astype(np.float64)).astype(np.float32)


def forwards(C, U, fused=False, skip=None, twice=None):
    t = _terms(C, U, fused)
    acc = np.zeros(t.shape[1:], np.float32)
    for k in range(t.shape[0]):
        if k == skip:
            continue
        acc = _add(acc, t[k])
        if k == twice:
            acc = _add(acc, t[k])
    return acc


def backwards(C, U):
    return forwards(C[:, ::-1], U[::-1])


def pairwise(C, U):
    t = list(_terms(C, U, False))
    while len(t) > 1:
        t = [_add(t[i], t[i + 1]) if i + 1 < len(t) else t[i] for i in range(0, len(t), 2)]
    return t[0]


def chunked(C, U, chunk=R.K_CHUNK):
    """Chunks of 256 clients, each a fused chain that starts from the carried fp32
    partial of the chunks before it: the kernel's own order."""
    t = _terms(C, U, True)
    acc = np.zeros(t.shape[1:], np.float32)
    for k0 in range(0, t.shape[0], chunk):
        carried = acc.copy()  # stored as fp32, re-read by the next launch
        for k in range(k0, min(k0 + chunk, t.shape[0])):
            carried = _add(carried, t[k])
        acc = carried
    return acc


@pytest.mark.parametrize("S,K,P,seed", [(1, 1, 4, 0), (5, 7, 12, 1), (3, 50, 8, 2), (4, 257, 8, 3),
                                        (2, 513, 4, 4), (33, 10, 4, 5), (6, 300, 8, 6)])
def test_exact_case_is_order_independent(S, K, P, seed):
    C, U, ref, unit = R.exact_case(S, K, P, seed)
    assert ref.dtype == np.float32 and ref.shape == (S, P)
    assert (C == 0).any() or K == 1
    assert (C != 0).any(axis=1).all()
    want = bits(R.contract(C, U, np.arange(K), P).astype(np.float32))
    assert np.array_equal(bits(ref), want)
    for f in (forwards, backwards, pairwise, chunked, lambda c, u: forwards(c, u, fused=True)):
        assert np.array_equal(bits(f(C, U)), want), f


def test_exact_case_zero_fraction_and_scales():
    C, U, _, _ = R.exact_case(64, 200, 4, 9)
    assert 0.3 < float((C == 0).mean()) < 0.5
    assert np.array_equal(C * 16, np.rint(C * 16)) and C.min() >= 0 and C.max() <= 1
    units = {R.exact_case(2, 3, 4, s)[3] for s in range(40)}
    assert len(units) > 1  # more than one binade is exercised
    with pytest.raises(AssertionError):  # the precondition is asserted, not assumed
        R.check_exact(np.full((1, 3), 0.3, np.float32), U[:3], 1.0 / 16)
    with pytest.raises(AssertionError):
        R.check_exact(C[:, :3], U[:3] * 1.5, 1.0 / 16)
    big = np.full((1, 1 << 15), 1.0, np.float32)
    with pytest.raises(AssertionError):  # 2^15 * 64 * 16 = 2^25 units
        R.check_exact(big, np.full((1 << 15, 1), 64.0, np.float32), 1.0 / 16)


def _real_case(S, K, P, seed):
    rng = np.random.default_rng([S, K, P, seed])
    subsets, n = R.random_coalitions(S, K, rng)
    subsets[-1] = list(range(K))  # the union is every client: C has K columns
    C, rows = R.server_coefficients(subsets, n)
    assert rows == list(range(K))
    return C, (0.05 * rng.standard_normal((K, P))).astype(np.float32)


@pytest.mark.parametrize("K", [1, 50, 257, 513])
def test_abs_bound_holds_and_is_not_vacuous(K):
    S, P = 6, 64
    C, U = _real_case(S, K, P, 11)
    ref = R.contract(C, U, np.arange(K), P)
    bound = R.abs_bound(C, U, np.arange(K), P)
    assert bound.shape == (S, P) and (bound > 0).all()
    for got in (forwards(C, U), forwards(C, U, fused=True), backwards(C, U), chunked(C, U)):
        assert (np.abs(got.astype(np.float64) - ref) <= bound).all()
    # one term dropped, one term taken twice: each leaves the bound somewhere
    k = int(np.argmax((C != 0).sum(axis=0)))
    assert (C[:, k] != 0).any()
    for wrong in (forwards(C, U, skip=k), forwards(C, U, twice=k)):
        assert (np.abs(wrong.astype(np.float64) - ref) > bound).any()


def test_gamma_is_the_stated_formula():
    for K in (1, 50, 513):
        assert R.gamma(K) == (K + 1) * 2.0 ** -24 / (1 - (K + 1) * 2.0 ** -24)
    C, U, _, _ = R.exact_case(2, 3, 4, 0)
    want = R.gamma(3) * (np.abs(C.astype(np.float64)) @ np.abs(U.astype(np.float64)))
    assert np.array_equal(R.abs_bound(C, U, np.arange(3), 4), want)


# --------------------------------------------------------------- the launch plan
def test_dispatch_restates_the_kernel_source():
    """The plan in subset_gemm_ref is a restatement; tie it to the text of
    csrc/shapley.hip, so a change of the rule there fails here and the GPU sweep's
    coverage is looked at again."""
    with open(os.path.join(ROOT, "distributed_learning_simulator_amd", "csrc", "shapley.hip")) as f:
        src = f.read()
    for text in ("constexpr int kMaxK = 256;",
                 "for (int s0 = 0; s0 < S; s0 += 64)",
                 "const int steps = (Kc + 1) / 2;",
                 "((steps + 4) / 5 * 5 - steps) < ((steps + 3) / 4 * 4 - steps) ? 5 : 4;",
                 "const int MT = Sc > 32 ? 2 : 1;",
                 "#define DLS_GEMM_NT 4"):
        assert text in src, text
    assert (R.K_CHUNK, R.S_CHUNK, R.TILE_P) == (256, 64, 128)
    for Kc in range(1, 257):
        steps = (Kc + 1) // 2
        depth = 5 if ((steps + 4) // 5 * 5 - steps) < ((steps + 3) // 4 * 4 - steps) else 4
        assert R.depth_of(Kc) == (depth, (steps + depth - 1) // depth * depth - steps)
    assert R.depth_of(50) == (5, 0) and R.depth_of(1) == (4, 3) and R.depth_of(25) == (5, 2)
    assert (R.max_padding(4), R.max_padding(5)) == (3, 2)
    plan = R.dispatch(129, 513)
    assert [(d["s0"], d["Sc"], d["MT"]) for d in plan[::3]] == [(0, 64, 2), (64, 64, 2), (128, 1, 1)]
    assert [(d["k0"], d["Kc"], d["beta"]) for d in plan[:3]] == \
        [(0, 256, False), (256, 256, True), (512, 1, True)]


def test_gpu_sweep_covers_the_dispatch():
    """The coverage assertion of the GPU sweep's S and K sets needs no device: run it
    wherever the suite runs."""
    from tests import test_gpu_subset_gemm as G
    G.test_sweep_covers_the_dispatch()


# ---------------------------------------------------------- the numpy double
def _pitched(Uc, rows, ldu, spare=3):
    K, P = Uc.shape
    U = np.full((K + spare, ldu), np.nan, np.float32)
    U[np.asarray(rows), :P] = Uc
    return U


def _rows_kinds(K, rng):
    yield "permuted", rng.permutation(K + 3)[:K]
    yield "reversed", np.arange(K)[::-1].copy()
    if K >= 3:
        r = rng.permutation(K + 3)[:K]
        r[K - 1] = r[0]  # the same client row listed twice, with two coefficients
        yield "duplicated", r


@pytest.mark.parametrize("S,K,P", [(5, 7, 12), (3, 300, 8), (70, 50, 20)])
def test_double_matches_contract(S, K, P):
    rng = np.random.default_rng([S, K, P])
    ldu, ldo = P + 4, P + 12
    for exact in (True, False):
        for kind, rows in _rows_kinds(K, rng):
            if exact:
                C, Uc, _, unit = R.exact_case(S, K, P, 3)
            else:
                C, Uc = _real_case(S, K, P, 4)
            if kind == "duplicated":
                Uc[K - 1] = Uc[0]
            U = _pitched(Uc, rows, ldu)
            out = torch.full((S + 2, ldo), 7.25)
            U0 = U.copy()
            cpu_doubles.subset_gemm(torch.from_numpy(C), torch.from_numpy(U),
                                    torch.from_numpy(rows.astype(np.int32)), P, out)
            got = out.numpy()
            assert (got[:, P:] == 7.25).all() and (got[S:] == 7.25).all(), kind
            assert np.array_equal(bits(U), bits(U0))
            ref = R.contract(C, U, rows, P)
            if exact:
                assert np.array_equal(bits(got[:S, :P]), bits(R.exact_result(C, Uc, unit))), kind
                assert np.array_equal(got[:S, :P].astype(np.float64), ref), kind
            else:
                assert (np.abs(got[:S, :P].astype(np.float64) - ref)
                        <= R.abs_bound(C, U, rows, P)).all(), kind


def test_double_non_finite_rows_as_ieee():
    """What the kernel's header states and tests/test_gpu_subset_gemm.py pins on the
    device: a non-finite element of a selected row makes that column non-finite in
    every coalition, the zero-coefficient ones included."""
    C, Uc, ref, _ = R.exact_case(4, 6, 8, 1)
    C[:, 2] = [0.5, 0.0, 0.25, 0.0]
    Uc[2, 1], Uc[2, 5] = np.inf, np.nan
    out = torch.zeros((4, 8))
    cpu_doubles.subset_gemm(torch.from_numpy(C), torch.from_numpy(Uc),
                            torch.arange(6, dtype=torch.int32), 8, out)
    got = out.numpy()
    assert np.isnan(got[:, 5]).all()
    assert np.isposinf(got[[0, 2], 1]).all() and np.isnan(got[[1, 3], 1]).all()
    assert np.isfinite(np.delete(got, [1, 5], axis=1)).all()


# ------------------------------------------------------------------ host path
def _store(n_rows, seed):
    from distributed_learning_simulator_amd.aggregation import ClientUpdateStore
    from distributed_learning_simulator_amd.layout import ParameterLayout
    lay = ParameterLayout([("w", (3, 5)), ("b", (5,))])
    st = ClientUpdateStore(lay, CPU, capacity=n_rows)
    g = torch.Generator().manual_seed(seed)
    rows = [st.acquire() for _ in range(n_rows)]
    for r in rows:
        w, b = torch.randn(3, 5, generator=g) * 0.05, torch.randn(5, generator=g) * 0.05
        st.write(r, {"w": w, "b": b})
    return st, rows


def _spy(monkeypatch):
    from distributed_learning_simulator_amd import _native
    calls = []
    inner = _native.subset_gemm

    def spy(C, U, rows, P, out, stream=None):
        calls.append((C.clone(), rows.clone(), P))
        return inner(C, U, rows, P, out, stream)

    monkeypatch.setattr(_native, "subset_gemm", spy)
    return calls


def test_store_gemm_coefficients_and_rows(doubles, monkeypatch):
    st, rows = _store(14, 3)
    calls = _spy(monkeypatch)
    n = {r: 50 + 13 * r for r in rows}
    rng = np.random.default_rng(5)
    members = [r for r in rows if r not in (rows[4], rows[13])]  # two rows in no coalition
    st.U[rows[4]] = float("nan")
    st.U[rows[13]] = float("inf")
    subs = [sorted(rng.permutation(members)[: 1 + s % 12].tolist()) for s in range(20)]
    out = st.subset_models(subs, n, method="gemm")
    assert len(calls) == 1
    C, r, P = calls[0]
    union = sorted({x for s in subs for x in s})
    assert r.dtype == torch.int32 and r.tolist() == union
    assert rows[4] not in r.tolist() and rows[13] not in r.tolist()
    assert C.dtype == torch.float32 and tuple(C.shape) == (20, len(union)) and P == st.layout.P
    want = np.zeros((20, len(union)), np.float32)
    for s, sub in enumerate(subs):
        tot = sum(n[x] for x in sub)
        for x in sub:
            want[s, union.index(x)] = np.float32(n[x] / tot)  # fp64 quotient, rounded once
    assert np.array_equal(bits(C.numpy()), bits(want))
    Cr, rr = R.server_coefficients(subs, n)
    assert rr == union and np.array_equal(bits(Cr), bits(want))
    got = out.numpy()
    assert np.isfinite(got).all()  # the NaN and inf rows were never read
    U = st.U.numpy()
    ref = R.contract(want, U, union, P)
    assert (np.abs(got.astype(np.float64) - ref) <= R.abs_bound(want, U, union, P)).all()
    # unsorted coalitions: the same C, the same models
    shuffled = [rng.permutation(s).tolist() for s in subs]
    assert any(a != b for a, b in zip(shuffled, subs))
    out2 = st.subset_models(shuffled, n, method="gemm")
    assert len(calls) == 2
    assert np.array_equal(bits(calls[1][0].numpy()), bits(want)) and calls[1][1].tolist() == union
    assert np.array_equal(bits(out2.numpy()), bits(got))


def test_store_gemm_is_one_call_past_both_chunk_sizes(doubles, monkeypatch):
    """More than 64 coalitions over more than 256 rows: one call (the kernel wrapper
    chunks, not the store), into the caller's ``out``."""
    K, S = 260, 70
    st, rows = _store(K + 2, 8)
    calls = _spy(monkeypatch)
    n = {r: 100 + (7 * r) % 901 for r in rows}
    rng = np.random.default_rng(6)
    subs = [sorted(rng.permutation(K)[: 1 + (37 * s) % K].tolist()) for s in range(S - 1)]
    subs.append(list(range(K)))  # the union is rows 0..K-1
    out = torch.full((S, st.layout.P), float("nan"))
    res = st.subset_models(subs, n, method="gemm", out=out)
    assert res is out and len(calls) == 1
    C, r, P = calls[0]
    assert tuple(C.shape) == (S, K) and r.tolist() == list(range(K))
    Cr, rr = R.server_coefficients(subs, n)
    assert np.array_equal(bits(C.numpy()), bits(Cr))
    U = st.U.numpy()
    err = np.abs(out.numpy().astype(np.float64) - R.contract(Cr, U, rr, P))
    assert (err <= R.abs_bound(Cr, U, rr, P)).all()
    with pytest.raises(ValueError):
        st.subset_models(subs, n, method="mfma")
