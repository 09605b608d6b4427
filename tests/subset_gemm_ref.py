"""numpy reference of the MFMA subset contraction (dls_subset_gemm_f32), tests only.

``contract`` is the plain fp64 product, ``abs_bound`` the derived elementwise bound a
correct fp32 evaluation stays within, ``exact_case`` inputs on which every correct
fp32 evaluation gives the same bits, ``dispatch`` the launch plan of
``csrc/shapley.hip`` restated (tests/test_subset_gemm_host.py ties it to the source
text), ``server_coefficients`` the C matrix as ``ClientUpdateStore.subset_models``
builds it.  No torch, no GPU."""
import numpy as np

U_ROUND = 2.0 ** -24  # unit roundoff of fp32, round to nearest

# csrc/shapley.hip: S in chunks of 64 coalitions (two 32-row MFMA tiles), K in chunks
# of 256 clients, one wave per 128-parameter column tile
S_CHUNK, K_CHUNK, TILE_P = 64, 256, 128


def contract(C, U, rows, P):
    """C . U[rows, :P] in fp64 (a product of two fp32 values is exact in fp64)."""
    rows = np.asarray(rows, dtype=np.int64)
    return np.asarray(C).astype(np.float64) @ np.asarray(U)[rows, :P].astype(np.float64)


def gamma(K):
    """g = (K+1)u / (1 - (K+1)u), u = 2^-24."""
    n = (K + 1) * U_ROUND
    return n / (1.0 - n)


def abs_bound(C, U, rows, P):
    """The elementwise bound g * (|C| @ |U[rows, :P]|), in fp64, on |fp32 result -
    exact result| for any correct fp32 evaluation of the contraction.

    Derivation (nothing is measured and nothing is added on top): write the computed
    element as a sum over the K terms c_k u_k, each multiplied by its own factor
    prod (1 + d_i), |d_i| <= u.  A term's product is rounded at most once (once when
    the multiplication and the addition are separate operations, not at all under a
    fused multiply-add), and the term then passes through at most K fp32 additions:
    the additions of the chain it enters and of every later term, whatever the order
    or the tree.  That covers the MFMA chain and the hand-over between the launches
    of two client chunks, where the running sum is stored and re-read as fp32
    without another rounding.  So each factor has at most K + 1 roundings and
    |prod (1 + d_i) - 1| <= g  (Higham, Accuracy and Stability of Numerical
    Algorithms, lemma 3.1), hence |computed - exact| <= g * sum_k |c_k| |u_k|.  It
    assumes no product or partial sum leaves the normal range."""
    rows = np.asarray(rows, dtype=np.int64)
    K = np.asarray(C).shape[1]
    mag = np.abs(np.asarray(C).astype(np.float64)) @ np.abs(np.asarray(U)[rows, :P].astype(np.float64))
    return gamma(K) * mag


def check_exact(C, U, unit):
    """The precondition of an exact case, asserted in fp64: every entry of C
    is a multiple of 1/16 in [0, 1], every entry of U an integer multiple of 16 *
    ``unit`` of magnitude at most 64 * 16 * unit, and max_sp (|C| @ |U|) / unit <
    2^24.  Every product is then an integer multiple of ``unit``, and so is every
    partial sum in any order, none larger than 2^24 units: fp32 holds them all
    exactly, whatever the order, fused or not."""
    C = np.asarray(C, dtype=np.float64)
    U = np.asarray(U, dtype=np.float64)
    c16 = C * 16.0
    assert np.array_equal(c16, np.rint(c16)) and C.min() >= 0.0 and C.max() <= 1.0
    ui = U / (16.0 * unit)
    assert np.array_equal(ui, np.rint(ui)) and np.abs(ui).max() <= 64
    top = (c16 @ np.abs(ui)).max()  # integers far below 2^53: the fp64 product is exact
    assert top < 2 ** 24, top
    return int(top)


def exact_coefficients(S, K, rng):
    """fp32 [S, K]: multiples of 1/16 in [0, 1], about 40 % zero, no zero row."""
    C = rng.integers(1, 17, size=(S, K)).astype(np.float64) / 16.0
    C *= rng.random((S, K)) < 0.6
    for s in np.flatnonzero(~C.any(axis=1)):
        C[s, (3 * s + 1) % K] = rng.integers(1, 17) / 16.0
    return C.astype(np.float32)


def exact_case(S, K, P, seed, scale_exp=None):
    """Inputs on which EVERY correct fp32 evaluation of C . U gives the same bits:
    (C fp32 [S, K], U fp32 [K, P], ref fp32 [S, P], unit).  U holds integers of
    magnitude <= 64 times 2^scale_exp (drawn from the seed when None), C as
    ``exact_coefficients``; ``check_exact`` asserts the precondition (with K <= 513
    the largest magnitude sum is at most 513 * 64 * 16 < 2^20 units).  ``ref`` is the
    exact result; a zero result is +0.0, as a chain that starts from +0.0 gives."""
    rng = np.random.default_rng([S, K, P, seed])
    if scale_exp is None:
        scale_exp = int(rng.choice([-20, -3, 0, 0, 6]))
    C = exact_coefficients(S, K, rng)
    U = (rng.integers(-64, 65, size=(K, P)).astype(np.float64) * 2.0 ** scale_exp).astype(np.float32)
    unit = 2.0 ** scale_exp / 16.0
    return C, U, exact_result(C, U, unit), unit


def exact_result(C, U, unit):
    """The exact product of checked exact operands, as fp32 (U: the K selected rows)."""
    check_exact(C, U, unit)
    ref64 = contract(C, U, np.arange(U.shape[0]), U.shape[1]) + 0.0  # -0.0 -> +0.0
    ref = ref64.astype(np.float32)
    assert np.array_equal(ref.astype(np.float64), ref64)  # nothing was rounded
    return ref


def server_coefficients(subsets, n_of_row):
    """(C fp32 [S, K], rows): c_sr = fl32(n_r / N_s) (the fp64 quotient rounded to
    fp32) in the column of client row r in the sorted union ``rows`` of the subsets,
    0 elsewhere: what ClientUpdateStore.subset_models(method="gemm") hands the kernel,
    restated independently."""
    rows = sorted(set().union(*[set(s) for s in subsets]))
    C = np.zeros((len(subsets), len(rows)), np.float32)
    for s, sub in enumerate(subsets):
        tot = sum(int(n_of_row[r]) for r in sub)
        for r in sub:
            C[s, rows.index(r)] = np.float32(np.float64(int(n_of_row[r])) / np.float64(tot))
    return C, rows


def random_coalitions(S, K, rng):
    """S non-empty sorted coalitions of the clients 0..K-1 (sizes spread over 1..K)
    and the clients' sample counts n (100..1000)."""
    n = [int(x) for x in rng.integers(100, 1001, size=K)]
    subsets = [sorted(rng.permutation(K)[: 1 + (7 * s + int(rng.integers(0, K))) % K].tolist())
               for s in range(S)]
    return subsets, n


# ------------------------------------------------------------------ launch plan
def depth_of(Kc):
    """(pipeline depth, zero-padded k-steps) of one client chunk, csrc/shapley.hip:
    a k-step is two clients (the half-used last one of an odd chunk included); the
    depth, 4 or 5, is whichever pads the chunk's k-steps to a whole number of rounds
    with fewer padded steps (4 on a tie)."""
    steps = (Kc + 1) // 2
    pad5, pad4 = -steps % 5, -steps % 4
    return (5, pad5) if pad5 < pad4 else (4, pad4)


def dispatch(S, K):
    """The launches of dls_subset_gemm_f32(S, K), in order: dicts of s0, Sc, MT, k0,
    Kc, beta, depth, padded."""
    plan = []
    for s0 in range(0, S, S_CHUNK):
        Sc = min(S - s0, S_CHUNK)
        for k0 in range(0, K, K_CHUNK):
            Kc = min(K - k0, K_CHUNK)
            depth, padded = depth_of(Kc)
            plan.append(dict(s0=s0, Sc=Sc, MT=2 if Sc > 32 else 1, k0=k0, Kc=Kc, beta=k0 > 0,
                             depth=depth, padded=padded))
    return plan


def max_padding(depth):
    """The most padded k-steps the rule ever gives a chunk of this depth."""
    return max(p for d, p in map(depth_of, range(1, K_CHUNK + 1)) if d == depth)
