"""numpy reference of FetchSGD's Count Sketch (include/dls_hip.h: dls_sketch_f32,
dls_unsketch_f32) and of FedSketchServer's round - TEST INFRASTRUCTURE ONLY.  Every fp32 step
is a numpy float32 operation (one rounding each).  The Philox words are tests/dp_ref.py's,
which the Random123 known answers pin."""
import numpy as np

from tests import topk_ref
from tests.dp_ref import words
from tests.drive_ref import flip
from tests.topk_ref import bits  # noqa: F401

F32 = np.float32
QSEG = 32


def hashes(P, R, C, seed, stream_id):
    """(m int64 [NQ, R], neg bool [R, NQ * C]): the masks m_r(q) and where s_r(j) = -1 (never
    past P)."""
    NQ = -(-P // C)
    m = (words(8 * NQ, seed, stream_id).reshape(NQ, 8)[:, :R] & np.uint32(C - 1)).astype(np.int64)
    neg = np.zeros((R, NQ * C), bool)
    for r in range(R):
        w = words(-(-P // 32), seed, stream_id, first=2 ** 32 + r * 2 ** 26)
        neg[r, :P] = ((w[:, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)).reshape(-1)[:P]
    return m, neg


def sketch(w, base, P, R, C, seed, stream_id):
    """(table fp32 [R, C], nonfinite)."""
    m, neg = hashes(P, R, C, seed, stream_id)
    NQ, b = m.shape[0], np.arange(C)
    with np.errstate(all="ignore"):
        u = np.asarray(w[:P], F32) if base is None else (w[:P] - base[:P]).astype(F32)
        x = np.concatenate([u, np.zeros(NQ * C - P, F32)])
        T = np.empty((R, C), F32)
        for r in range(R):
            g = flip(x, neg[r]).reshape(NQ, C)
            tot = None
            for q0 in range(0, NQ, QSEG):
                part = None
                for q in range(q0, min(q0 + QSEG, NQ)):
                    term = g[q, b ^ m[q, r]]
                    part = term if part is None else (part + term).astype(F32)
                tot = part if tot is None else (tot + part).astype(F32)
            T[r] = tot
    return T, int((~np.isfinite(u)).sum())


def key(x):
    b = np.ascontiguousarray(x).view(np.int32)
    return np.where(b >= 0, b, b ^ np.int32(0x7FFFFFFF))


def unsketch(T, P, R, C, seed, stream_id):
    """est fp32 [P]: the element of middle rank of the R signed buckets under key()."""
    m, neg = hashes(P, R, C, seed, stream_id)
    j = np.arange(P)
    e = np.stack([flip(np.asarray(T, F32)[r, (j % C) ^ m[j // C, r]], neg[r, :P]) for r in range(R)])
    return key(np.sort(key(e), axis=0)[R // 2]).view(F32)


def server_round(u, v, tables, ns, prev, P, R, C, k, rho, seed, stream_id):
    """One round of FedSketchServer on the flat row: (u, v, model), all new."""
    N = F32(sum(int(n) for n in ns))
    with np.errstate(all="ignore"):
        S = None
        for T, n in zip(tables, ns):
            term = ((np.asarray(T, F32) * F32(int(n))).astype(F32) / N).astype(F32)
            S = term if S is None else (S + term).astype(F32)
        u = ((F32(rho) * u).astype(F32) + S).astype(F32)
        v = (v + u).astype(F32)
        est = unsketch(v, P, R, C, seed, stream_id)
        zero = np.zeros(P, F32)
        idx, val, _, _ = topk_ref.compress(est, zero, zero, k)
        model = topk_ref.sparse_fedavg(prev[:P], [(idx, val)], [1])
        D, _ = sketch(model, prev, P, R, C, seed, stream_id)
        v = (v - D).astype(F32)
        u = np.where(D != 0, F32(0.0), u)
    return u, v, model
