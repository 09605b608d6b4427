"""Characterization of the operand checks of the rows-family entry points, CPU only: the
status and ``dls_last_error()`` text of every rejected call, byte for byte and in the
order the checks fire, recorded in ``tests/golden/rows_entry_messages.json``.

The library is called directly with dummy pointers that are never dereferenced (as in
``tests/test_native_abi.py``): every check runs before any device call, and no case is
well formed, so none reaches a launch.  Per entry point one defect per argument in
turn, and every pair of defects on two different arguments (which of the two is
reported pins the order of the checks).  ``python -m tests.test_rows_entry_messages_host``
rewrites the fixture (to add inputs); a recorded outcome never changes.
"""
import ctypes
import itertools
import json
import os

import pytest

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                       "rows_entry_messages.json")
NAN, INF = float("nan"), float("inf")
K0, P0, LD0 = 3, 8, 16  # a well-formed call: 3 rows of 8 elements at a pitch of 16

# argument kinds: "ptr" a required pointer, "a16" / "a8" / "a2" a required pointer that
# must also be 16- / 8- / 4-byte aligned (the defect: offset 4, 4 and 2), "opt16" an
# optional 16-byte aligned one (null is well formed), "K", "ld", "P", "stream", or a
# (good value, bad values) pair for the rule's scalar
ENTRIES = {
    "dls_trimmed_mean_f32": [("U", "a16"), ("ldu", "ld"), ("rows", "ptr"), ("K", "K"),
                             ("trim", (1, (-1, 2))), ("P", "P"), ("out", "a16"), ("s", "stream")],
    "dls_mean_around_median_f32": [("U", "a16"), ("ldu", "ld"), ("rows", "ptr"), ("K", "K"),
                                   ("keep", (2, (0, 4))), ("P", "P"), ("out", "a16"),
                                   ("s", "stream")],
    "dls_craft_rows_f32": [("U", "a16"), ("ldu", "ld"), ("hrows", "ptr"), ("Kh", "K"),
                           ("arows", "ptr"), ("Ka", "K"), ("a", (1.0, (NAN, INF))),
                           ("b", (-0.5, (NAN, -INF))), ("base", "opt16"), ("P", "P"),
                           ("s", "stream")],
    "dls_pairwise_sqdist_f32": [("U", "a16"), ("ldu", "ld"), ("rows", "ptr"), ("K", "K"),
                                ("P", "P"), ("D", "a8"), ("workspace", "a16"), ("s", "stream")],
    "dls_rows_gram_f32": [("U", "a16"), ("ldu", "ld"), ("rows", "ptr"), ("K", "K"), ("P", "P"),
                          ("base", "opt16"), ("G", "a8"), ("workspace", "a16"), ("s", "stream")],
    "dls_history_gram_f32": [("U", "a16"), ("ldu", "ld"), ("rows", "ptr"), ("H", "a16"),
                             ("ldh", "ld"), ("hrows", "ptr"), ("K", "K"), ("P", "P"),
                             ("base", "opt16"), ("G", "a8"), ("workspace", "a16"),
                             ("s", "stream")],
    "dls_rows_sqdist_to_f32": [("U", "a16"), ("ldu", "ld"), ("rows", "ptr"), ("K", "K"),
                               ("P", "P"), ("z", "a16"), ("dist2", "a8"), ("workspace", "a16"),
                               ("s", "stream")],
    "dls_weiszfeld_step_f32": [("U", "a16"), ("ldu", "ld"), ("rows", "ptr"), ("K", "K"),
                               ("w", "a2"), ("P", "P"), ("z", "a16"), ("dist2", "a8"),
                               ("workspace", "a16"), ("s", "stream")],
    "dls_centered_clip_step_f32": [("U", "a16"), ("ldu", "ld"), ("rows", "ptr"), ("K", "K"),
                                   ("c", "a2"), ("P", "P"), ("z", "a16"), ("dist2", "a8"),
                                   ("workspace", "a16"), ("s", "stream")],
    # the queries: a P that is no multiple of 4 is well formed there, so it is left out
    "dls_pairwise_sqdist_workspace": [("K", "K"), ("P", "Pq")],
    "dls_rows_gram_workspace": [("K", "K"), ("P", "Pq")],
    "dls_weiszfeld_workspace": [("K", "K"), ("P", "Pq")],
}
OFFSET = {"a16": 4, "a8": 4, "a2": 2}


def _defects(kind):
    if isinstance(kind, tuple):
        return list(kind[1])
    return {"ptr": ["null"], "a16": ["null", "misaligned"], "a8": ["null", "misaligned"],
            "a2": ["null", "misaligned"], "opt16": ["misaligned"], "K": [0, 65], "ld": [P0 - 4, P0 + 2],
            "P": [-4, 2], "Pq": [-4], "stream": []}[kind]


def _value(i, kind, defect):
    """The value of argument number i: its defect, else the well-formed one."""
    if isinstance(kind, tuple):
        return kind[0] if defect is None else defect
    if kind in ("ptr", "a16", "a8", "a2", "opt16"):
        if defect == "null":
            return None
        base = 0x1000 * (i + 1)  # never dereferenced: validation comes first
        return ctypes.c_void_p(base + (OFFSET.get(kind, 4) if defect == "misaligned" else 0))
    if kind == "stream":
        return None
    return {"K": K0, "ld": LD0, "P": P0, "Pq": P0}[kind] if defect is None else defect


def enumerate_entry(L, name):
    """[(key, [status, message])] of one entry point's rejected calls, in a fixed order."""
    args = ENTRIES[name]
    defects = [(arg, d) for arg, kind in args for d in _defects(kind)]
    cases = [(d,) for d in defects]
    cases += [(a, b) for a, b in itertools.combinations(defects, 2) if a[0] != b[0]]
    out = []
    for case in cases:
        asked = dict(case)
        status = getattr(L, name)(*[_value(i, kind, asked.get(arg))
                                    for i, (arg, kind) in enumerate(args)])
        out.append(("+".join(f"{arg}:{d}" for arg, d in case),
                    [int(status), L.dls_last_error().decode()]))
    return out


@pytest.fixture(scope="module")
def recorded():
    with open(FIXTURE) as fh:
        return json.load(fh)


@pytest.mark.parametrize("name", list(ENTRIES))
def test_rejections_are_the_recorded_ones(name, recorded):
    from distributed_learning_simulator_amd import _native
    got = enumerate_entry(_native.lib(), name)
    want = recorded["entries"][name]
    assert [k for k, _ in got] == list(want), "the enumeration and the fixture list other inputs"
    assert all(status != 0 for _, (status, _) in got), "a well-formed call slipped in"
    differ = [(k, v, recorded["messages"][want[k]]) for k, v in got
              if v != recorded["messages"][want[k]]]
    assert not differ, f"{len(differ)} of {len(got)} outcomes changed; the first: {differ[0]}"


def test_the_fixture_holds_every_entry(recorded):
    assert list(recorded["entries"]) == list(ENTRIES)


if __name__ == "__main__":
    from distributed_learning_simulator_amd import _native
    messages, entries = [], {}
    for entry_name in ENTRIES:
        entries[entry_name] = {}
        for key, outcome in enumerate_entry(_native.lib(), entry_name):
            assert outcome[0] != 0 and key not in entries[entry_name], (entry_name, key)
            if outcome not in messages:
                messages.append(outcome)
            entries[entry_name][key] = messages.index(outcome)
    with open(FIXTURE, "w") as fh:  # one message, and one entry point, per line
        fh.write('{"messages": [\n' + ",\n".join(json.dumps(m) for m in messages) + '],\n')
        fh.write('"entries": {\n' + ",\n".join(f"{json.dumps(n)}: {json.dumps(e)}"
                                               for n, e in entries.items()) + "}}\n")
    print({n: len(e) for n, e in entries.items()}, len(messages), "messages",
          os.path.getsize(FIXTURE), "bytes")
