"""numpy reference of the top-k sparsifier and the sparse FedAvg (include/dls_hip.h:
dls_topk_compress_f32, dls_sparse_fedavg_f32), and CPU doubles of their wrappers - TEST
INFRASTRUCTURE ONLY.  Every operation is a numpy float32 operation (one rounding each), so
the kernels' outputs are compared bit for bit."""
import numpy as np
import torch

from distributed_learning_simulator_amd import _native

F32 = np.float32
ABS = np.uint32(0x7FFFFFFF)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def update(w, base, e):
    """u = fl(fl(w - base) + e)."""
    w, base, e = (np.asarray(a, dtype=F32) for a in (w, base, e))
    with np.errstate(all="ignore"):
        return ((w - base).astype(F32) + e).astype(F32)


def keys(u):
    return bits(u) & ABS


def compress(w, base, e, k):
    """(idx int32 [k] ascending, val fp32 [k], e_new fp32 [P], nonfinite): the k largest
    keys by a stable sort on (-key, index), so equal keys go to the lowest indices."""
    u = update(w, base, e)
    k = int(k)
    assert 1 <= k <= u.size
    order = np.argsort(-keys(u).astype(np.int64), kind="stable")
    sel = np.sort(order[:k])
    e_new = u.copy()
    e_new[sel] = F32(0.0)
    return sel.astype(np.int32), u[sel].copy(), e_new, int((~np.isfinite(u)).sum())


def sparse_fedavg(base, payloads, ns):
    """out = base, and where a client sent the coordinate fl(base + acc): acc the chain of
    fl(fl(v * n_i) / N) over the coordinate's senders in the order of ``payloads`` (a list
    of (idx, val)), the first assigning and the later ones adding."""
    base = np.asarray(base, dtype=F32)
    N = F32(sum(int(n) for n in ns))
    acc = np.zeros(base.size, F32)
    has = np.zeros(base.size, bool)
    with np.errstate(all="ignore"):
        for (idx, val), n in zip(payloads, ns):
            idx = np.asarray(idx).astype(np.int64)
            term = ((np.asarray(val, dtype=F32) * F32(int(n))).astype(F32) / N).astype(F32)
            first = ~has[idx]
            acc[idx[first]] = term[first]
            later = idx[~first]
            acc[later] = (acc[later] + term[~first]).astype(F32)
            has[idx] = True
        out = base.copy()
        out[has] = (base[has] + acc[has]).astype(F32)
    return out


# ------------------------------------------------------------------ the launch plan
# A model of csrc/topk.hip's work split, from the DLS_TOPK_* constants alone
# (tests/test_topk_host.py holds it against dls_topk_workspace).
WS_HEAD_WORDS = 3 * 2048 + 16  # the three digit histograms (2048 words each) and the state


def nchunks(P):
    return -(-int(P) // _native.TOPK_CHUNK)


def hist_trips(P):
    """Chunks the busiest block of the histogram passes (form, refine) walks."""
    return -(-nchunks(P) // _native.TOPK_HIST_BLOCKS)


def scan_per(P):
    """Consecutive chunks per thread of the scan block."""
    return -(-nchunks(P) // _native.TOPK_SCAN_BLOCK)


def workspace_bytes(P):
    """Histograms and state, then two count arrays of nchunks + 1 words."""
    return 4 * (WS_HEAD_WORDS + 2 * (nchunks(P) + 1))


# The smallest rows that reach each path past a launch cap, and the workload's own size
# (ResNet-18 after padding); tests/test_gpu_topk_scale.py runs them.
P_SCAN2 = (_native.TOPK_SCAN_BLOCK + 1) * _native.TOPK_CHUNK + 4    # two chunks per scan thread
P_STRIDE = (_native.TOPK_HIST_BLOCKS + 1) * _native.TOPK_CHUNK + 68  # a second histogram trip
P_RESNET = 11_173_964


# ------------------------------------------------------------------ CPU doubles
def _np(t):
    return t.detach().cpu().numpy()


def _topk_workspace(P, device):
    return torch.empty(16, dtype=torch.uint8, device=device)


def _topk_compress(w, base, e, k, P, idx, val, stats, workspace, stream=None):
    i, v, e_new, bad = compress(_np(w)[:P], _np(base)[:P], _np(e)[:P], k)
    idx[:k].copy_(torch.from_numpy(i))
    val[:k].copy_(torch.from_numpy(v))
    e[:P].copy_(torch.from_numpy(e_new))
    stats[0], stats[1] = k, bad
    return idx, val


def _sparse_fedavg(base, idx, val, off, weight, total, P, out, stream=None):
    o = _np(off)
    ns = [int(x) for x in _np(weight)]
    assert float(np.float32(sum(ns))) == float(np.float32(total))
    pay = [(_np(idx)[o[i]:o[i + 1]], _np(val)[o[i]:o[i + 1]]) for i in range(len(ns))]
    out[:P].copy_(torch.from_numpy(sparse_fedavg(_np(base)[:P], pay, ns)))
    return out


def install(monkeypatch):
    """cpu_doubles.install plus doubles for the three top-k wrappers, built on the
    reference, so FedTopKWorker / FedTopKServer run without a GPU."""
    from tests import cpu_doubles
    cpu_doubles.install(monkeypatch)
    monkeypatch.setattr(_native, "topk_workspace", _topk_workspace)
    monkeypatch.setattr(_native, "topk_compress", _topk_compress)
    monkeypatch.setattr(_native, "sparse_fedavg", _sparse_fedavg)
