"""Loaders for the golden fixtures written by make_golden.py (data only)."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


PART_BYTES = 900 * 1024  # raw array bytes per part file (every committed file stays under 1 MiB)


class Fixture(dict):
    """The arrays of one fixture by name, with NpzFile's ``files``."""

    @property
    def files(self):
        return list(self)


def save(name, arrays):
    """Write a fixture.  One compressed ``name`` where its arrays fit PART_BYTES,
    else ``<stem>.partNN.npz`` files: each holds whole arrays, and blocks of rows
    ``<key>@rows<i>`` of an array that is too large for one part."""
    stem = os.path.join(HERE, name[:-len(".npz")])
    arrays = {k: np.asarray(v) for k, v in arrays.items()}
    if sum(a.nbytes for a in arrays.values()) <= PART_BYTES:
        np.savez_compressed(stem + ".npz", **arrays)
        return
    pieces = []
    for k, a in arrays.items():
        if a.nbytes <= PART_BYTES:
            pieces.append((k, a))
            continue
        rows = max(1, PART_BYTES // (a.nbytes // a.shape[0]))
        pieces += [(f"{k}@rows{i:04d}", a[r:r + rows])
                   for i, r in enumerate(range(0, a.shape[0], rows))]
    parts, size = [{}], 0
    for k, a in pieces:
        if parts[-1] and size + a.nbytes > PART_BYTES:
            parts.append({})
            size = 0
        parts[-1][k] = a
        size += a.nbytes
    for i, p in enumerate(parts):
        np.savez_compressed(f"{stem}.part{i:02d}.npz", **p)


def load(name):
    """A fixture written by save(): the npz file, or its parts put together again."""
    path = os.path.join(HERE, name)
    if os.path.exists(path):
        return np.load(path, allow_pickle=False)
    stem = name[:-len(".npz")]
    names = sorted(f for f in os.listdir(HERE)
                   if f.startswith(stem + ".part") and f.endswith(".npz"))
    if not names:
        raise FileNotFoundError(path)
    out, blocks = Fixture(), {}
    for f in names:
        with np.load(os.path.join(HERE, f), allow_pickle=False) as z:
            for k in z.files:
                if "@rows" in k:
                    blocks.setdefault(k.split("@rows")[0], []).append((k, z[k]))
                else:
                    out[k] = z[k]
    for k, bl in blocks.items():
        out[k] = np.concatenate([a for _, a in sorted(bl, key=lambda t: t[0])])
    return out


def meta(npz):
    return json.loads(str(npz["meta"]))


def shapley_cases():
    with open(os.path.join(HERE, "shapley.json")) as f:
        return json.load(f)


def layout_size(layout):
    return sum(int(np.prod(s)) for _, s in layout)


def split(flat, layout):
    out, off = {}, 0
    for name, shape in layout:
        m = int(np.prod(shape))
        out[name] = np.asarray(flat[off:off + m]).reshape(shape)
        off += m
    return out


def shapley_large_cases():
    """GTG N=50 / multiround N=12 (shapley_large.npz) in the shapley_cases() form;
    'evaluated' as sorted tuples decoded from the stored bit masks."""
    z = load("shapley_large.npz")
    cases = []
    for m in meta(z):
        t = m["tag"]
        K = m["K"]
        case = dict(m)
        case.update(U=z[f"{t}_U"], n=[int(x) for x in z[f"{t}_n"]], prev=z[f"{t}_prev"],
                    target=z[f"{t}_target"],
                    sv={str(i): float(v) for i, v in enumerate(z[f"{t}_sv"])},
                    evaluated=[tuple(i for i in range(K) if (int(b) >> i) & 1)
                               for b in z[f"{t}_evaluated"]],
                    metric_pickle=(z[f"{t}_metric_pickle"].tobytes()
                                   if f"{t}_metric_pickle" in z.files else None))
        cases.append(case)
    return cases
