"""Characterization of the robust-aggregation host path, CPU only: what every rejected
call raises (type and message, byte for byte) and what the accepted ones return, in
the order the checks fire, recorded in ``tests/golden/robust_messages.json``.

The inputs are enumerated in a fixed order, section by section, and each outcome,
``"ok"``, a repr of what came back or ``"<ExceptionType>: <message>"``, is compared
with the recorded string (the fixture lists each distinct string once and, per input,
its index).  A recorded string never changes: a difference is a change of behaviour.  ``python -m tests.test_robust_messages_host`` rewrites the fixture (to add
inputs); to see that a change of the package kept every message, run this file against
the fixture with the package directory of the parent commit in place of the new one.

Servers are constructed on the CPU doubles (``cpu_doubles.install``); ``_native.lib`` is
a stub, so no case needs the library: a well-formed wrapper call ends in "not on the
GPU" before anything reaches it.
"""
import hashlib
import itertools
import json
import os
import textwrap

import pytest
import torch

from tests import cpu_doubles

CPU = torch.device("cpu")
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                       "robust_messages.json")
NAN, INF = float("nan"), float("inf")

RULES = ("mean", "median", "trimmed_mean", "multi_krum", "geometric_median", "centered_clip",
         "mean_around_median", "bulyan", "foolsgold")
ATTACKS = ("alie", "ipm", "sign_flip")
WORKER_NUMBERS = (None, 2, 3, 7, 10, 64, 65)
MODES = ("exact", "fma")
ONE_SET = (("trim", 1), ("byzantine", 1), ("byzantine", 2), ("krum_select", 1), ("gm_iters", 2),
           ("gm_nu", 1e-3), ("cc_tau", 1.0), ("cc_iters", 2), ("fg_kappa", 2.0))
OWNERS = {"trim": ("trimmed_mean",), "byzantine": ("multi_krum", "bulyan", "mean_around_median"),
          "krum_select": ("multi_krum",), "gm_iters": ("geometric_median",),
          "gm_nu": ("geometric_median",), "cc_tau": ("centered_clip",),
          "cc_iters": ("centered_clip",), "fg_kappa": ("foolsgold",),
          "attack_z": ("alie",), "attack_eps": ("ipm",), "attack_scale": ("sign_flip",)}
BAD_VALUES = (True, -1, 0, 1.5, "1", NAN, INF)
LAST = ("last_selection", "last_scores", "last_distances", "last_rejected", "last_clip_scales",
        "last_weights", "last_similarity")


TOPK_BYTES = 32  # what the stub's dls_topk_workspace asks for, for every P


class _StubLibrary:
    """Stands in for the loaded library: nothing recorded here reaches an entry point
    (but for the host-only size query of the top-k workspace, answered with TOPK_BYTES)."""

    def dls_topk_workspace(self, P):
        return TOPK_BYTES

    def __getattr__(self, name):
        def entry(*args):
            raise AssertionError(f"{name} reached the library stub")
        return entry


def _outcome(call):
    try:
        result = call()
    except Exception as e:  # the type and the text are what is recorded
        return f"{type(e).__name__}: {e}"
    return "ok" if result is None else result


def _kw(kw):
    return ",".join(f"{k}={v!r}" for k, v in kw.items())


def _construct(make, **kw):
    def call():
        make(**kw).stop()
    return _outcome(call)


def _fed(**kw):
    from distributed_learning_simulator_amd.servers.fed_server import FedServer
    return FedServer(tester=None, device=CPU, synchronous=True, **kw)


# ---------------------------------------------------------------- the constructor
def constructor_grid():
    for rule, wn, mode in itertools.product(RULES, WORKER_NUMBERS, MODES):
        for extra in ((),) + tuple((p,) for p in ONE_SET):
            kw = dict(aggregation_rule=rule, worker_number=wn, aggregation_mode=mode, **dict(extra))
            yield _kw(kw), _construct(_fed, **kw)


def constructor_values():
    for name, owners in OWNERS.items():
        for owner, value in itertools.product(owners, BAD_VALUES):
            if name.startswith("attack"):
                kw = dict(worker_number=10, attack=owner, attackers=(1,), **{name: value})
            else:
                kw = dict(worker_number=10, aggregation_rule=owner, **{name: value})
            yield _kw(kw), _construct(_fed, **kw)


def constructor_pairs():
    for wn, select in itertools.product((10, None), (0, 1, 8, 9)):
        kw = dict(aggregation_rule="multi_krum", byzantine=2, krum_select=select, worker_number=wn)
        yield _kw(kw), _construct(_fed, **kw)
    for wn in (6, 7):
        kw = dict(aggregation_rule="bulyan", byzantine=1, worker_number=wn)
        yield _kw(kw), _construct(_fed, **kw)
    kw = dict(aggregation_rule="mean_around_median", byzantine=5, worker_number=10)
    yield _kw(kw), _construct(_fed, **kw)
    for rule, wn in itertools.product(RULES, (0, -1)):  # no client at all
        kw = dict(aggregation_rule=rule, worker_number=wn)
        yield _kw(kw), _construct(_fed, **kw)


def constructor_attacks():
    foreign = ((), ("attack_z", 1.0), ("attack_eps", 0.2), ("attack_scale", 2.0))
    attackers = ((), (1,), (1, 1), (9,), (10,), (-1,), (True,), 5)
    for attack, ids, extra, wn in itertools.product((None,) + ATTACKS, attackers, foreign,
                                                    (10, None)):
        kw = dict(attack=attack, attackers=ids, worker_number=wn, **dict((extra,) if extra else ()))
        yield _kw(kw), _construct(_fed, **kw)


def subclasses():
    from distributed_learning_simulator_amd import factory
    combos = [(a, False) for a in ("fed_quant", "GTG_shapley_value", "multiround_shapley_value")]
    combos += [(a, True) for a in ("fed", "fed_quant", "GTG_shapley_value",
                                   "multiround_shapley_value")]
    for (algo, sharded), kw in itertools.product(combos, (
            dict(aggregation_rule="median"), dict(byzantine=1),
            dict(attack="alie", attackers=(1,)))):
        def make(**kw):
            return factory.get_server(algo, sharded=sharded, tester=None, worker_number=5,
                                      synchronous=True, device=CPU, **kw)
        yield f"{algo},sharded={sharded},{_kw(kw)}", _construct(make, **kw)


# ---------------------------------------------------------------- get_subset_model
def subset_models():
    configs = [dict(aggregation_rule=r) for r in RULES]
    for kw in configs:
        kw.update({"trimmed_mean": dict(trim=2), "multi_krum": dict(byzantine=2),
                   "bulyan": dict(byzantine=1),
                   "mean_around_median": dict(byzantine=2)}.get(kw["aggregation_rule"], {}))
    configs.append(dict(aggregation_rule="multi_krum", byzantine=1, krum_select=9))
    for kw in configs:
        s = _fed(worker_number=10, **kw)
        for w in range(10):
            s.parameters[w] = (w + 1, {"w": torch.arange(16.0).reshape(4, 4) * (w - 4.5)})
        for subset in ([0], [0, 1], list(range(6)), list(range(10))):
            def call():
                model = s.get_subset_model(subset)
                return repr(({k: v.tolist() for k, v in model.items()},
                             {a: getattr(s, a) for a in LAST}))
            yield f"{_kw(kw)},subset={subset}", _outcome(call)
        s.stop()


# ---------------------------------------------------------------- the _native wrappers
K0 = 3  # clients of a well-formed call; matrices are [8, 16], P = 8


def _strided(flat, defects):
    """``flat`` (a new 1-D tensor of twice the length + 1) cut to what the defects ask."""
    off = 1 if "misaligned" in defects else 0
    n = (flat.numel() - 1) // 2
    return flat[off:off + 2 * n:2] if "stride" in defects else flat[off:off + n]


def _matrix(defects):
    width = 32 if "stride" in defects else 16
    pitch = width + (2 if "pitch" in defects else 0)
    off = 1 if "misaligned" in defects else 0
    buf = torch.zeros(8 * pitch + off,
                      dtype=torch.float64 if "dtype" in defects else torch.float32)
    t = buf[off:].view(8, pitch)[:, :width]
    t = t[:, ::2] if "stride" in defects else t
    return t[None] if "rank" in defects else t


def _table(defects):
    K = 0 if "K0" in defects else 65 if "K65" in defects else K0
    values = [k % 8 for k in range(K)]
    if "range" in defects:
        values[-1] = 99
    if "dup" in defects:
        values[0] = values[1]
    t = torch.zeros(2 * K + 1, dtype=torch.int64 if "dtype" in defects else torch.int32)
    t = _strided(t, defects)
    t.copy_(torch.tensor(values, dtype=t.dtype))
    return t[None] if "rank" in defects else t


def _vector(n, dtype, wrong, short=4):
    def make(defects):
        m = (short if "short" in defects else n + 1 if "shape" in defects
             else 0 if "empty" in defects else n)
        t = _strided(torch.zeros(2 * m + 1, dtype=wrong if "dtype" in defects else dtype,
                                 device="meta" if "device" in defects else None), defects)
        return t[None] if "rank" in defects else t
    return make


def _square(defects):
    cols = K0 + 1 if "shape" in defects else K0
    t = _strided(torch.zeros(2 * K0 * cols + 1,
                             dtype=torch.float32 if "dtype" in defects else torch.float64), defects)
    t = t.view(K0, cols) if t.is_contiguous() else t.unflatten(0, (K0, cols))
    return t[None] if "rank" in defects else t


MATRIX = (_matrix, ("dtype", "rank", "stride", "pitch", "misaligned"))
TABLE = (_table, ("dtype", "rank", "stride", "misaligned", "K0", "K65", "range", "dup"))
F32VEC = (_vector(16, torch.float32, torch.float64),
          ("dtype", "rank", "stride", "misaligned", "short"))
KVEC32 = (_vector(K0, torch.float32, torch.float64),
          ("dtype", "rank", "stride", "misaligned", "shape"))
KVEC64 = (_vector(K0, torch.float64, torch.float32),
          ("dtype", "rank", "stride", "misaligned", "shape"))
SQUARE = (_square, ("dtype", "rank", "stride", "misaligned", "shape"))
EXCLUSIVE = ({"K0", "K65"}, {"K0", "range"}, {"K0", "dup"}, {"range", "dup"}, {"short", "shape"})

# the scalar arguments: (the well-formed value, the values no call accepts)
SCALARS = {"trim": (1, (-1, 2)), "keep": (2, (0, 4)), "a": (1.0, (NAN,))}

# wrapper -> (its tensor operands in call order, the call on the built operands o and P)
WRAPPERS = {
    "trimmed_mean": ({"U": MATRIX, "rows": TABLE, "out": F32VEC},
                     lambda n, o, P: n.trimmed_mean(o["U"], o["rows"], o["trim"], P, o["out"])),
    "mean_around_median": ({"U": MATRIX, "rows": TABLE, "out": F32VEC},
                           lambda n, o, P: n.mean_around_median(o["U"], o["rows"], o["keep"], P,
                                                                o["out"])),
    "pairwise_sqdist": ({"U": MATRIX, "rows": TABLE, "out": SQUARE},
                        lambda n, o, P: n.pairwise_sqdist(o["U"], o["rows"], P, out=o["out"])),
    "rows_gram": ({"U": MATRIX, "rows": TABLE, "base": F32VEC, "out": SQUARE},
                  lambda n, o, P: n.rows_gram(o["U"], o["rows"], P, base=o["base"], out=o["out"])),
    "history_gram": ({"U": MATRIX, "rows": TABLE, "H": MATRIX, "hrows": TABLE, "base": F32VEC,
                      "out": SQUARE},
                     lambda n, o, P: n.history_gram(o["U"], o["rows"], o["H"], o["hrows"], P,
                                                    base=o["base"], out=o["out"])),
    "craft_rows": ({"U": MATRIX, "hrows": TABLE, "arows": TABLE, "base": F32VEC},
                   lambda n, o, P: n.craft_rows(o["U"], o["hrows"], o["arows"], o["a"], -0.5, P,
                                                base=o["base"])),
    "rows_sqdist_to": ({"U": MATRIX, "rows": TABLE, "z": F32VEC, "out": KVEC64},
                       lambda n, o, P: n.rows_sqdist_to(o["U"], o["rows"], P, o["z"], out=o["out"])),
    "weiszfeld_step": ({"U": MATRIX, "rows": TABLE, "w": KVEC32, "z": F32VEC, "dist2": KVEC64},
                       lambda n, o, P: n.weiszfeld_step(o["U"], o["rows"], o["w"], P, o["z"],
                                                        dist2=o["dist2"])),
    "centered_clip_step": ({"U": MATRIX, "rows": TABLE, "c": KVEC32, "z": F32VEC, "dist2": KVEC64},
                           lambda n, o, P: n.centered_clip_step(o["U"], o["rows"], o["c"], P,
                                                                o["z"], dist2=o["dist2"])),
}
OPTIONAL = ("base", "out", "dist2")  # the defaults (None) are a base case of their own


def _wrapper_cases(name):
    from distributed_learning_simulator_amd import _native
    operands, call = WRAPPERS[name]
    defects = [(op, kind) for op, (_, kinds) in operands.items() for kind in kinds]
    defects += [("P", p) for p in (-4, 0, 2, 20)]
    if "H" in operands:
        defects.append(("H", "overlap"))
    scalar = {"trimmed_mean": "trim", "mean_around_median": "keep", "craft_rows": "a"}.get(name)
    if scalar:
        defects += [(scalar, v) for v in SCALARS[scalar][1]]
    singles = [()] + [(d,) for d in defects]
    pairs = [(a, b) for a, b in itertools.combinations(defects, 2)
             if not (a[0] == b[0] and (a[0] in ("P", scalar) or {a[1], b[1]} in EXCLUSIVE
                                       or "overlap" in (a[1], b[1])))]

    def run(case, omit=()):
        P = 8
        asked = {op: set() for op in operands}
        o = {scalar: SCALARS[scalar][0]} if scalar else {}
        for op, kind in case:
            if op == "P":
                P = kind
            elif op == scalar:
                o[op] = kind
            else:
                asked[op].add(kind)
        o.update({op: make(asked[op]) for op, (make, _) in operands.items()})
        if "overlap" in asked.get("H", ()):
            o["H"] = o["U"]
        if name in ("trimmed_mean", "mean_around_median"):
            omit = ()  # out is not optional there
        for op in omit:
            if op in o:
                o[op] = None

        def invoke():
            result = call(_native, o, P)
            return "ok" if torch.is_tensor(result) or isinstance(result, tuple) else result
        return _outcome(invoke)

    yield "defaults", run((), omit=OPTIONAL)
    for case in singles + pairs:
        yield "+".join(f"{op}:{kind}" for op, kind in case) or "well-formed", run(case)


# ------------------------------------- the vector wrappers: server optimizer and top-k
VEC_KINDS = ("dtype", "rank", "stride", "misaligned", "short", "device")
EXACT_KINDS = ("dtype", "rank", "stride", "misaligned", "shape", "device")
TK = 6  # k of a well-formed topk_compress call (P = 8)
NNZ = 16  # pairs of a well-formed sparse_fedavg call


def _vec(n, dtype, wrong, kinds=VEC_KINDS, short=4):
    return _vector(n, dtype, wrong, short), kinds


P_VEC = _vec(16, torch.float32, torch.float64)  # an fp32 vector of at least P = 8 elements

# wrapper -> (tensor operands in call order, scalars {name: (good, bad values)}, the
# overlaps it names as (a, b, how), the call on the built operands o and P)
VECTOR_WRAPPERS = {
    "server_opt_step": (
        {name: P_VEC for name in ("agg", "x", "m", "v", "out")},
        {"kind": (2, (True, -1, 4, 1.5, "adam", 0, 1)), "lr": (0.5, (NAN, INF, 1e39)),
         "beta1": (0.9, (NAN, -INF, 0.0)), "beta2": (0.99, (NAN, 1e39)), "tau": (1e-3, (NAN, INF))},
        [(a, b, "alias") for a, b in itertools.combinations(("agg", "x", "m", "v", "out"), 2)]
        + [("x", "out", "shifted")],
        lambda n, o, P: n.server_opt_step(o["kind"], o["agg"], o["x"], o["m"], o["v"], o["out"], P,
                                          o["lr"], o["beta1"], o["beta2"], o["tau"])),
    "topk_compress": (
        {"w": P_VEC, "base": P_VEC, "e": P_VEC, "idx": _vec(8, torch.int32, torch.int64),
         "val": _vec(8, torch.float32, torch.float64),
         "stats": _vec(2, torch.int32, torch.int64, short=1),
         "workspace": _vec(TOPK_BYTES, torch.uint8, torch.int8)},
        {"k": (TK, (True, 0, 9, 1.5, "2"))},
        [("e", "w", "alias"), ("e", "base", "alias")]
        + [(a, b, "alias") for a, b in
           itertools.combinations(("e", "idx", "val", "stats", "workspace"), 2)],
        lambda n, o, P: n.topk_compress(o["w"], o["base"], o["e"], o["k"], P, o["idx"], o["val"],
                                        o["stats"], o["workspace"])),
    "sparse_fedavg": (
        {"base": P_VEC, "idx": _vec(NNZ, torch.int32, torch.int64, EXACT_KINDS + ("empty", "list")),
         "val": _vec(NNZ, torch.float32, torch.float64, EXACT_KINDS + ("empty", "list")),
         "off": _vec(K0 + 1, torch.int64, torch.int32, EXACT_KINDS),
         "weight": _vec(K0, torch.float32, torch.float64, EXACT_KINDS + ("empty",)),
         "out": P_VEC},
        {"total": (6.0, (0.0, -1.0, NAN, INF, 1e39))},
        [("out", b, "alias") for b in ("base", "idx", "val", "off", "weight")],
        lambda n, o, P: n.sparse_fedavg(o["base"], o["idx"], o["val"], o["off"], o["weight"],
                                        o["total"], P, o["out"])),
}
OPTIONAL_VEC = {"server_opt_step": ("m", "v")}  # operands that may be None


def _alias(o, a, b, how):
    """Make o[a] and o[b] share storage: the smaller becomes a view of the larger's first
    bytes with its own dtype and length (``shifted``: b starts 16 bytes into a's buffer)."""
    if how == "shifted":
        buf = torch.zeros(o[a].numel() + 4, dtype=o[a].dtype)
        o[a], o[b] = buf[:-4], buf[4:]
        return
    if o[a].numel() * o[a].element_size() < o[b].numel() * o[b].element_size():
        a, b = b, a
    nbytes = o[b].numel() * o[b].element_size()
    o[b] = o[a].view(torch.uint8)[:nbytes].view(o[b].dtype)


def _vector_wrapper_cases(name):
    from distributed_learning_simulator_amd import _native
    operands, scalars, overlaps, call = VECTOR_WRAPPERS[name]
    defects = [(op, kind) for op, (_, kinds) in operands.items() for kind in kinds]
    defects += [(op, "none") for op in OPTIONAL_VEC.get(name, ())]
    defects += [("P", p) for p in (-4, 0, 2, 20, 1 << 31)]
    defects += [(s, v) for s, (_, bad) in scalars.items() for v in bad]
    defects += [(a, f"{how}:{b}") for a, b, how in overlaps]

    def touched(d):  # the operands a defect rebuilds
        return {d[0], d[1].split(":")[1]} if isinstance(d[1], str) and ":" in d[1] else {d[0]}

    def compatible(a, b):
        if a[0] == b[0] and (a[0] == "P" or a[0] in scalars or {a[1], b[1]} in EXCLUSIVE
                             or "none" in (a[1], b[1]) or "list" in (a[1], b[1])
                             or "empty" in (a[1], b[1])):
            return False
        aliasing = [d for d in (a, b) if len(touched(d)) == 2]
        return not (aliasing and touched(a) & touched(b))

    pairs = [(a, b) for a, b in itertools.combinations(defects, 2) if compatible(a, b)]

    def run(case):
        P = 8
        asked = {op: set() for op in operands}
        o = {s: good for s, (good, _) in scalars.items()}
        for op, kind in case:
            if op == "P":
                P = kind
            elif op in scalars:
                o[op] = kind
            else:
                asked[op].add(kind)
        for op, (make, _) in operands.items():
            kinds = asked[op]
            plain = {k for k in kinds if ":" not in k and k not in ("none", "list")}
            o[op] = None if "none" in kinds else [0] * NNZ if "list" in kinds else make(plain)
        for op, kinds in asked.items():
            for k in kinds:
                if ":" in k:
                    _alias(o, op, k.split(":")[1], k.split(":")[0])

        def invoke():
            result = call(_native, o, P)
            return "ok" if torch.is_tensor(result) or isinstance(result, tuple) else result
        return _outcome(invoke)

    for case in [()] + [(d,) for d in defects] + pairs:
        yield "+".join(f"{op}:{kind}" for op, kind in case) or "well-formed", run(case)


def topk_workspace_cases():
    from distributed_learning_simulator_amd import _native
    for P in (-4, 0, 2, 3, 4, 8, 10, (1 << 31) - 4, (1 << 31) - 1, 1 << 31, 8.0, "8", None):
        def call():
            t = _native.topk_workspace(P, CPU)
            return repr((t.dtype, tuple(t.shape), str(t.device)))
        yield f"P={P!r}", _outcome(call)


def required_none_cases():
    """Every wrapper with each of its tensor operands None in turn, the others well formed
    (the optional ones, where None is the default, included: they end in "not on the GPU")."""
    from distributed_learning_simulator_amd import _native
    for name, (operands, call) in WRAPPERS.items():
        scalar = {"trimmed_mean": "trim", "mean_around_median": "keep", "craft_rows": "a"}.get(name)
        for missing in operands:
            o = {scalar: SCALARS[scalar][0]} if scalar else {}
            o.update({op: make(set()) for op, (make, _) in operands.items()})
            o[missing] = None
            yield f"{name}:{missing}", _outcome(lambda: call(_native, o, 8) and "ok")
    for name, (operands, scalars, _, call) in VECTOR_WRAPPERS.items():
        for missing in operands:
            o = {s: good for s, (good, _) in scalars.items()}
            o.update({op: make(set()) for op, (make, _) in operands.items()})
            o[missing] = None
            yield f"{name}:{missing}", _outcome(lambda: call(_native, o, 8) and "ok")


# ------------------------------------- every option, every feature, every server class
SERVER_OPTIMIZERS = ("sgd", "adagrad", "adam", "yogi")
OPT_OWNERS = {"server_lr": SERVER_OPTIMIZERS, "server_momentum": SERVER_OPTIMIZERS,
              "server_beta2": ("adam", "yogi"), "server_tau": ("adagrad", "adam", "yogi")}
KIND_VALUES = BAD_VALUES + (None, 1, 2, -0.5, 0.5, 1.0, 1e-3, -INF)
# what switches an option's feature on with a value that owns the option
ATTACKED = dict(attackers=(1,))


def _owned(name, owner):
    """The keywords under which ``owner`` (a rule, an attack or an optimizer) is on."""
    if name in OPT_OWNERS:
        return dict(server_optimizer=owner)
    if name.startswith("attack"):
        return dict(attack=owner, **ATTACKED)
    return dict(aggregation_rule=owner)


def constructor_kinds():
    """Every option at every kind of value, under its first owner and with its feature
    off (a wrong kind is told before a wrong place), and the selectors' own values."""
    for name, owners in {**OWNERS, **OPT_OWNERS}.items():
        for value, on in itertools.product(KIND_VALUES, (True, False)):
            kw = dict(worker_number=10, **(_owned(name, owners[0]) if on else {}), **{name: value})
            yield _kw(kw), _construct(_fed, **kw)
    selectors = {"aggregation_mode": (None, "EXACT", 1, ""), "aggregation_rule": (None, "krum", 1),
                 "attack": ("ALIE", 1, ""), "server_optimizer": ("SGD", 1, "", "adamw"),
                 "attackers": (None, "12", [1.5], ((1,),), [1, True], range(3), range(10))}
    for name, values in selectors.items():
        for value in values:
            kw = dict(worker_number=10, **{name: value})
            yield _kw(kw), _construct(_fed, **kw)
            kw = dict(worker_number=10, aggregation_rule="median", attack="ipm", attackers=(1,),
                      server_optimizer="adam")
            kw[name] = value
            yield _kw(kw), _construct(_fed, **kw)


def constructor_owners():
    """Every option at a value of its own under every rule, attack and optimizer, the
    feature off included."""
    values = dict(ONE_SET, attack_z=1.0, attack_eps=0.2, attack_scale=2.0, server_lr=0.5,
                  server_momentum=0.5, server_beta2=0.9, server_tau=0.01)
    for name, value in values.items():
        feature = (SERVER_OPTIMIZERS if name in OPT_OWNERS else ATTACKS
                   if name.startswith("attack") else RULES)
        for chosen in (None,) + feature:
            kw = dict(worker_number=10, **({} if chosen is None else _owned(name, chosen)),
                      **{name: value})
            yield _kw(kw), _construct(_fed, **kw)


def constructor_attributes():
    """What an accepted construction holds of every option: value and type."""
    names = tuple(OWNERS) + tuple(OPT_OWNERS)
    for kw in (dict(), dict(aggregation_rule="trimmed_mean", trim=2),
               dict(aggregation_rule="multi_krum", byzantine=2, krum_select=3),
               dict(aggregation_rule="geometric_median", gm_iters=5, gm_nu=1),
               dict(aggregation_rule="centered_clip", cc_tau=2, cc_iters=4),
               dict(aggregation_rule="foolsgold", fg_kappa=3),
               dict(attack="alie", attackers=(2, 1), attack_z=1),
               dict(attack="ipm", attackers=(1,), attack_eps=1),
               dict(attack="sign_flip", attackers=(1,), attack_scale=3),
               dict(server_optimizer="sgd"), dict(server_optimizer="sgd", server_lr=1),
               dict(server_optimizer="adam", server_momentum=0, server_beta2=0, server_tau=1)):
        def call():
            s = _fed(worker_number=10, **kw)
            s.stop()
            return repr({n: getattr(s, n) for n in names + ("attackers",)})
        yield _kw(kw), _outcome(call)


def checker_misuse():
    """The three checkers called with arguments their signatures do not take."""
    from distributed_learning_simulator_amd.servers.fed_server import FedServer as F
    calls = {
        "_check_server_opt('sgd',0.5,server_lr=0.7)":
            lambda: F._check_server_opt("sgd", 0.5, server_lr=0.7),
        "_check_server_opt('sgd',0.5,0.5,0.9,0.01,1)":
            lambda: F._check_server_opt("sgd", 0.5, 0.5, 0.9, 0.01, 1),
        "_check_server_opt('sgd',bogus=1)": lambda: F._check_server_opt("sgd", bogus=1),
        "_check_server_opt()": lambda: F._check_server_opt(),
        "_check_attack('alie',(1,),bogus=1)": lambda: F._check_attack("alie", (1,), bogus=1),
        "_check_attack('alie')": lambda: F._check_attack("alie"),
        "_check_attack('alie',(1,),1.0,attack_z=2.0)":
            lambda: F._check_attack("alie", (1,), 1.0, attack_z=2.0),
        "_check_attack('alie',(1,),1.0,0.1,1.0,8,9)":
            lambda: F._check_attack("alie", (1,), 1.0, 0.1, 1.0, 8, 9),
        "_check_rule('median')": lambda: F._check_rule("median"),
        "_check_rule('median','exact',5,bogus=1)":
            lambda: F._check_rule("median", "exact", 5, bogus=1),
        "_check_rule('median','exact',5,6)": lambda: F._check_rule("median", "exact", 5, 6),
    }
    for key, call in calls.items():
        yield key, _outcome(lambda: repr(call()))


# one fault each: (what is wrong, the keywords that make it so on any of BASES)
FAULTS = (
    [("mode", dict(aggregation_mode="fast")), ("rule", dict(aggregation_rule="krum")),
     ("attack", dict(attack="ALIE")), ("attackers", dict(attackers=5)),
     ("attackers twice", dict(attackers=(1, 1))), ("optimizer", dict(server_optimizer="SGD")),
     ("no attack", dict(attack=None, attackers=(1,))),
     ("no attackers", dict(attack="sign_flip", attackers=())),
     ("fma", dict(aggregation_mode="fma", aggregation_rule="median")),
     ("count", dict(aggregation_rule="bulyan", byzantine=2)),
     ("select", dict(aggregation_rule="multi_krum", byzantine=1, krum_select=10)),
     ("beyond", dict(attack="ipm", attackers=(10,))),
     ("fp32", dict(server_optimizer="adam", server_lr=1e-46))]
    + [(f"kind {n}", {n: v}) for n, v in dict(
        trim=-1, byzantine=True, krum_select=1.5, gm_iters=0, gm_nu=0.0, cc_tau=NAN, cc_iters=1.5,
        fg_kappa=-1.0, attack_z="1", attack_eps=INF, attack_scale=NAN, server_lr=0.0,
        server_momentum=1.0, server_beta2=-0.1, server_tau=INF).items()]
    + [(f"place {n}", {n: v}) for n, v in dict(
        trim=1, byzantine=1, krum_select=2, gm_iters=2, gm_nu=1e-3, cc_tau=1.0, cc_iters=2,
        fg_kappa=2.0, attack_z=1.0, attack_eps=0.2, attack_scale=2.0, server_lr=0.5,
        server_momentum=0.5, server_beta2=0.9, server_tau=0.01).items()])
BASES = (dict(worker_number=10),
         dict(worker_number=10, aggregation_rule="median", attack="ipm", attackers=(1,),
              server_optimizer="sgd"))


def constructor_precedence():
    """Two faults at once, every pair that can be set together: which one is told."""
    for base, ((a, fa), (b, fb)) in itertools.product(BASES, itertools.combinations(FAULTS, 2)):
        if set(fa) & set(fb):
            continue
        kw = {**base, **fa, **fb}
        yield f"{a}+{b}:{_kw(kw)}", _construct(_fed, **kw)


def _server_classes():
    from distributed_learning_simulator_amd import distributed as d
    from distributed_learning_simulator_amd.servers.fed_quant_server import FedQuantServer
    from distributed_learning_simulator_amd.servers.fed_server import FedServer
    from distributed_learning_simulator_amd.servers.fed_topk_server import FedTopKServer
    from distributed_learning_simulator_amd.servers.GTG_shapley_value_server import \
        GTGShapleyValueServer
    from distributed_learning_simulator_amd.servers.multiround_shapley_value_server import \
        MultiRoundShapleyValueServer
    return (FedServer, FedQuantServer, FedTopKServer, GTGShapleyValueServer,
            MultiRoundShapleyValueServer, d.ShardedFedServer, d.ShardedFedQuantServer,
            d.ShardedGTGShapleyValueServer, d.ShardedMultiRoundShapleyValueServer)


FEATURES_ON = (
    dict(aggregation_rule="median"), dict(aggregation_rule="trimmed_mean", trim=1),
    dict(aggregation_rule="median", aggregation_mode="fma"), dict(trim=1), dict(fg_kappa=0.0),
    dict(attack="alie", attackers=(1,)), dict(attack="sign_flip", attackers=()),
    dict(attack_eps=0.5), dict(attack="ipm", attackers=(1,), attack_eps=NAN),
    dict(server_optimizer="sgd"), dict(server_optimizer="adam", server_beta2=0.9),
    dict(server_optimizer="adam", server_lr=1e-46), dict(server_lr=0.5),
    dict(server_optimizer="yogi", server_tau=0.0),
    dict(aggregation_rule="median", attack="alie", attackers=(1,), server_optimizer="sgd"),
    dict(attack="alie", attackers=(1,), server_optimizer="sgd"))


def subclass_features():
    """Every feature on every server class: through the constructor, and through the
    three checkers as the callers outside the class call them."""
    for cls in _server_classes():
        extra = dict(initial_model={"w": torch.zeros(4)}) if cls.__name__ == "FedTopKServer" else {}
        for kw in FEATURES_ON:
            def make(**kw):
                return cls(tester=None, worker_number=5, synchronous=True, device=CPU, **extra,
                           **kw)
            yield f"{cls.__name__}({_kw(kw)})", _construct(make, **kw)
        calls = {
            "_check_rule('median','exact',5)": lambda: cls._check_rule("median", "exact", 5),
            "_check_rule('mean','fma',None,trim=0)":
                lambda: cls._check_rule("mean", "fma", None, trim=0),
            "_check_rule('bulyan','exact',6,byzantine=1)":
                lambda: cls._check_rule("bulyan", "exact", 6, byzantine=1),
            "_check_attack(None,())": lambda: cls._check_attack(None, ()),
            "_check_attack('ipm',(1,),worker_number=8)":
                lambda: cls._check_attack("ipm", (1,), worker_number=8),
            "_check_attack('alie',[7,3],1.0,0.1,1.0,11)":
                lambda: cls._check_attack("alie", [7, 3], 1.0, 0.1, 1.0, 11),
            "_check_attack('alie',[7,3],None,0.1,2.0,11)":
                lambda: cls._check_attack("alie", [7, 3], None, 0.1, 2.0, 11),
            "_check_server_opt(None)": lambda: cls._check_server_opt(None),
            "_check_server_opt('adam')": lambda: cls._check_server_opt("adam"),
            "_check_server_opt('sgd',0.5,0.5)": lambda: cls._check_server_opt("sgd", 0.5, 0.5),
            "_check_server_opt('sgd',server_tau=0.01)":
                lambda: cls._check_server_opt("sgd", server_tau=0.01),
        }
        for key, call in calls.items():
            yield f"{cls.__name__}.{key}", _outcome(lambda: repr(call()))


# ---------------------------------------------------------------- ClientUpdateStore
def store_calls():
    """What ``ClientUpdateStore`` refuses before a launch, on a store of 4 CPU rows (a
    well-formed call ends in the wrapper's "not on the GPU")."""
    from distributed_learning_simulator_amd.aggregation import ClientUpdateStore
    from distributed_learning_simulator_amd.layout import ParameterLayout
    st = ClientUpdateStore(ParameterLayout.from_dict({"w": torch.zeros(2, 4)}), CPU, capacity=4)
    P = st.layout.P
    vectors = {"good": torch.zeros(P), "None": None, "list": [0.0] * P,
               "fp64": torch.zeros(P, dtype=torch.float64), "2-D": torch.zeros(1, P),
               "short": torch.zeros(P - 1), "long": torch.zeros(P + 1),
               "meta": torch.zeros(P, device="meta")}
    many = list(range(65))
    G2 = [[1.0, 0.0], [0.0, 1.0]]
    row_lists = {"[]": [], "[0,0]": [0, 0], "[-1]": [-1], "[4]": [4], "65": many, "[0,1]": [0, 1],
                 "[1,2]": [1, 2]}
    cases = {}
    for (h, honest), (a, bad) in itertools.product(row_lists.items(), repeat=2):
        cases[f"craft({h},{a})"] = lambda honest=honest, bad=bad: st.craft(honest, bad, 1.0, 0.0)
    pairs = {"[0,1]": [0, 1], "[0]": [0], "[]": [], "[0,0]": [0, 0], "[-1,0]": [-1, 0],
             "[3,4]": [3, 4], "65": many}
    for (r, rows), (h, hrows) in itertools.product(pairs.items(), repeat=2):
        cases[f"fold_history({r},{h})"] = lambda rows=rows, hrows=hrows: st.fold_history(rows, hrows)
    id_lists = {"[5,3]": [5, 3], "[5,5]": [5, 5], "[5]": [5], "[5,'a']": [5, "a"]}
    for (i, ids), (v, vec) in itertools.product(id_lists.items(), vectors.items()):
        cases[f"foolsgold([0,1],{i},G,{v})"] = lambda ids=ids, vec=vec: st.foolsgold(
            [0, 1], ids, G2, vec)
        cases[f"centered_clip([0,1],{i},{v},1.0,2)"] = lambda ids=ids, vec=vec: st.centered_clip(
            [0, 1], ids, vec, 1.0, 2)
        cases[f"centered_clip([0,1],{i},{v},1.0,0)"] = lambda ids=ids, vec=vec: st.centered_clip(
            [0, 1], ids, vec, 1.0, 0)
    for kappa in (0.0, NAN, "1"):
        cases[f"foolsgold(kappa={kappa!r})"] = lambda kappa=kappa: st.foolsgold(
            [0, 1], [5, 3], G2, vectors["good"], kappa)
    cases["foolsgold(G 1x1)"] = lambda: st.foolsgold([0, 1], [5, 3], [[1.0]], vectors["good"])
    for (i, ids), f in itertools.product({**id_lists, "[1,2,3]": [1, 2, 3]}.items(), (-1, 0, 1)):
        cases[f"bulyan([0,1,2],{i},{f})"] = lambda ids=ids, f=f: st.bulyan([0, 1, 2], ids, f)
    for (i, ids), iters in itertools.product(id_lists.items(), (0, -1, 1, 1.5, "x")):
        cases[f"geometric_median([0,1],{i},{iters!r})"] = lambda ids=ids, iters=iters: \
            st.geometric_median([0, 1], ids, iters, 1e-6)
    for v, vec in vectors.items():
        cases[f"set_model({v})"] = lambda vec=vec: st.set_model(vec)
    cases["server_opt_step without a model"] = lambda: (
        setattr(st, "model", None), st.server_opt_step(vectors["good"], 0, (1.0,) * 6))[1]
    for key, call in cases.items():
        yield key, _outcome(lambda: (call(), "ok")[1])


SECTIONS = {"constructor_grid": constructor_grid, "constructor_values": constructor_values,
            "constructor_pairs": constructor_pairs, "constructor_attacks": constructor_attacks,
            "subclasses": subclasses, "subset_models": subset_models}
SECTIONS.update({f"native_{name}": (lambda name=name: _wrapper_cases(name)) for name in WRAPPERS})
SECTIONS.update({f"native_{name}": (lambda name=name: _vector_wrapper_cases(name))
                 for name in VECTOR_WRAPPERS})
SECTIONS["native_topk_workspace"] = topk_workspace_cases
SECTIONS["native_required_none"] = required_none_cases
SECTIONS.update({"constructor_kinds": constructor_kinds, "constructor_owners": constructor_owners,
                 "constructor_precedence": constructor_precedence,
                 "subclass_features": subclass_features, "store_calls": store_calls})
SECTIONS["constructor_attributes"] = constructor_attributes
SECTIONS["checker_misuse"] = checker_misuse


def enumerate_section(section):
    """[(key, outcome)] of one section, on the CPU doubles and the library stub."""
    from distributed_learning_simulator_amd import _native
    with pytest.MonkeyPatch.context() as mp:
        cpu_doubles.install(mp)
        mp.setattr(_native, "lib", _StubLibrary)
        return list(SECTIONS[section]())


# The fixture holds every distinct outcome once ("messages") and per section the digest
# of its inputs' keys in order and, input by input, the index of the recorded outcome.
def _digest(cases):
    return hashlib.sha256("\n".join(k for k, _ in cases).encode()).hexdigest()[:16]


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as fh:
        return json.load(fh)


@pytest.mark.parametrize("section", list(SECTIONS))
def test_outcomes_are_the_recorded_ones(section, recorded):
    got = enumerate_section(section)
    want = [recorded["messages"][i] for i in recorded["sections"][section]["outcomes"]]
    assert (len(got), _digest(got)) == (len(want), recorded["sections"][section]["inputs"]), \
        "the enumeration and the fixture list other inputs"
    differ = [(k, v, w) for (k, v), w in zip(got, want) if v != w]
    assert not differ, f"{len(differ)} of {len(got)} outcomes changed; the first: {differ[0]}"


def test_the_fixture_holds_every_section(recorded):
    assert list(recorded["sections"]) == list(SECTIONS)
    assert len(set(recorded["messages"])) == len(recorded["messages"])


if __name__ == "__main__":
    messages, sections = {}, {}
    for section_name in SECTIONS:
        cases = enumerate_section(section_name)
        assert len({k for k, _ in cases}) == len(cases), f"{section_name}: a key repeats"
        sections[section_name] = {
            "inputs": _digest(cases),
            "outcomes": [messages.setdefault(v, len(messages)) for _, v in cases]}
    with open(FIXTURE, "w") as fh:  # one message per line, the indices in lines of 100 columns
        fh.write('{"messages": [\n' + ",\n".join(json.dumps(m) for m in messages) + '],\n')
        fh.write('"sections": {\n' + ",\n".join(
            f'{json.dumps(name)}: {{"inputs": {json.dumps(sec["inputs"])}, "outcomes": [\n'
            + "\n".join(textwrap.wrap(", ".join(map(str, sec["outcomes"])), 100)) + "]}"
            for name, sec in sections.items()) + "}}\n")
    print({k: len(v["outcomes"]) for k, v in sections.items()}, len(messages), "messages",
          os.path.getsize(FIXTURE), "bytes")
