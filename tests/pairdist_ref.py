"""CPU reference of the pairwise squared distances (include/dls_hip.h,
dls_pairwise_sqdist_f32) and of multi-Krum on them - TEST INFRASTRUCTURE ONLY (the
package has no CPU path).  Written independently of
``aggregation.multi_krum_select``; the final mean is
``robust_ref.trimmed_mean_bits(X[selected], 0)``.
"""
import numpy as np

from tests import robust_ref

TOL = 2.0 ** -17  # the contract's bound: (120 + 8) * 2^-24 relative


def sqdist(X):
    """fp64 [K, K] squared distances of the fp32 rows of X, every term from the
    difference of the two values; a row with inf / NaN gives inf / NaN entries."""
    X = np.asarray(X, dtype=np.float32).astype(np.float64)
    K = X.shape[0]
    D = np.zeros((K, K), np.float64)
    with np.errstate(all="ignore"):
        for a in range(K):
            d = X[a][None, :] - X
            D[a] = np.einsum("kp,kp->k", d, d) if np.isfinite(d).all() else (d * d).sum(axis=1)
    D[np.arange(K), np.arange(K)] = 0.0
    return D


def krum_scores(D, f):
    """score[i] = the sum of the K - f - 2 smallest distances from i to the others;
    non-finite distances count as +inf."""
    D = np.array(D, dtype=np.float64)
    K = D.shape[0]
    D[~np.isfinite(D)] = np.inf
    out = np.empty(K, np.float64)
    for i in range(K):
        others = np.sort(np.delete(D[i], i))
        out[i] = np.cumsum(others[:K - f - 2])[-1] if K - f - 2 > 0 else 0.0
    return out


def multi_krum_ref(X, ids, f, m):
    """(selected ids in (score, id) order, {id: score}, uint32 bits of the ascending
    unweighted mean of the selected rows)."""
    X = np.asarray(X, dtype=np.float32)
    ids = list(ids)
    assert X.shape[0] == len(ids) >= 2 * f + 3 and 1 <= m <= len(ids) - f
    sc = krum_scores(sqdist(X), f)
    ranked = sorted(zip(sc.tolist(), ids, range(len(ids))))
    chosen = ranked[:m]
    assert np.isfinite(chosen[-1][0])
    rows = [k for _, _, k in chosen]
    return [i for _, i, _ in chosen], dict(zip(ids, sc.tolist())), \
        robust_ref.trimmed_mean_bits(X[rows], 0)


def score_gap(X, f, m):
    """Relative gap between the m-th and the (m+1)-th best score (inf when the next
    one is not finite or there is none)."""
    sc = np.sort(krum_scores(sqdist(X), f))
    if m >= len(sc) or not np.isfinite(sc[m]):
        return np.inf
    return (sc[m] - sc[m - 1]) / sc[m]
