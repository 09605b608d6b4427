"""Host tests of the sign vote's launch geometry (csrc/sign_geometry.h through
dls_sign_vote_geometry / dls_sign_vote_wave_ranges), without a GPU: how
dls_sign_vote and dls_sign_vote_count split a model over waves.  The launch, the
kernel and the two queries call the same two functions, so what is pinned here is
what k_sign_vote runs.

The cover property: wave w of nwaves owns the vote groups [wlo, whi) (64 parameters
a group) and its 64 lanes own G groups each, so a range longer than 64 G groups
leaves its tail without counts, signs or packed vote.

The formula this replaces sized the ranges as follows (``parent_geometry`` below,
evaluated for P = 33,030,400 on 256 CUs, a narrow counter class):

    vote_groups = 516,100             waves = 4 * 256 = 1,024
    r = ceil(516100 / 1024) + 7 = 512  > 256, so waves *= ceil(512 / 256) = 2
    r = ceil(516100 / 2048) + 7 = 260  G = ceil(260 / 64) = 5

There is no 5-groups-per-lane kernel: the launch ran G = 4.  The last wave owns
[floor(2047 * 516100 / 2048) & ~7, 516100) = [515840, 516100), 260 groups, of which
its lanes cover 256: groups 516,096..516,099 (256 parameters) were never written.
``test_cover_property`` fails on that formula at this size (G = 5 and a range of
260 > 256 groups); ``test_parent_formula_dropped_groups_at_33m_parameters`` keeps the
arithmetic above executable.

A library built with other compile-time knobs is checked by path, for instance the
fixed-range variant (one wave per block, G = 4 from 130,820 groups):
``python tools/build_variants.py wpc0:-DDLS_VOTE_WPC=0``, then
``DLS_HIP_LIB=tools/_variants/libdls_wpc0.so pytest tests/test_sign_geometry_host.py -k test_cover_property``
(test_cover_property holds for any build; the other tests pin the default build's
values and are left out by that selector)."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

from distributed_learning_simulator_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = (1, 8, 64, 104, 128, 256, 304)
K_NARROW, K_WIDE = 24, 40_000  # counter classes CB <= 12 and CB = 16
MAX_GROUPS = 800_000           # P up to 51.2M: two of the old formula's bands at 256 CUs
DENSE = 4                      # sizes whose ranges are checked either side of a change of (nwaves, G)
STRIDE = 97                    # ... and every STRIDE-th size elsewhere (the scalar query runs at every size)


def groups_of(P):
    return _native.sign_words(P) // 2


def parent_geometry(vote_groups, cus, wide=False, wpc=4, wpb=4, max_g=4):
    """(nwaves, G, waves per block) as launch_vote computed them before the geometry
    had a function of its own."""
    nwaves, G, w = (vote_groups + 63) // 64, 1, 1
    if not wide:
        if wpc > 0:
            waves = wpc * cus
            r = (vote_groups + waves - 1) // waves + 7
            if r > 64 * max_g:
                waves *= (r + 64 * max_g - 1) // (64 * max_g)
                r = (vote_groups + waves - 1) // waves + 7
            if r > 64:
                nwaves, G, w = waves, (r + 63) // 64, wpb
        elif (vote_groups + 64 * max_g - 1) // (64 * max_g) >= 512:
            nwaves, G = (vote_groups + 64 * max_g - 1) // (64 * max_g), max_g
    return nwaves, G, w


def rule_range(wave, vote_groups, nwaves, G):
    """vote_wave_range restated (used only where the old formula's nwaves are wanted)."""
    lo, hi = wave * vote_groups // nwaves, (wave + 1) * vote_groups // nwaves
    if G > 1:
        lo, hi = lo & ~7, (vote_groups if wave + 1 == nwaves else hi & ~7)
    return lo, hi


@functools.lru_cache(maxsize=None)
def geometry_table(K, cus):
    """(tiles, nwaves, G, waves per block): the geometry of every model of 1, 2, ...,
    MAX_GROUPS / 4 tiles of 256 parameters, one query each.  Shared by the tests,
    read only."""
    f = _native.lib().dls_sign_vote_geometry
    n = MAX_GROUPS // 4
    nw, g, wpb = np.full(n, -1, np.int64), np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    a, b, c = nw.ctypes.data, g.ctypes.data, wpb.ctypes.data  # the query writes element i in place
    rcs = 0
    for P, pn, pg, pw in zip(range(256, 256 * n + 1, 256), range(a, a + 8 * n, 8), range(b, b + 4 * n, 4),
                             range(c, c + 4 * n, 4)):
        rcs |= f(P, K, cus, pn, pg, pw)
    assert rcs == 0
    out = (np.arange(1, n + 1, dtype=np.int64), nw, g.astype(np.int64), wpb.astype(np.int64))
    for a in out:
        a.flags.writeable = False
    return out


def check_ranges(P, K, cus, nwaves, G):
    """The cover property of one model, on the ranges the kernel's own function gives."""
    vg = groups_of(P)
    wlo, whi = _native.sign_vote_wave_ranges(P, K, cus)
    where = (P, K, cus, nwaves, G)
    assert wlo.size == nwaves, where
    assert wlo[0] == 0 and whi[-1] == vg, where
    assert np.array_equal(wlo[1:], whi[:-1]), where       # contiguous: a partition
    assert np.all(whi >= wlo), where
    assert int((whi - wlo).max()) <= 64 * G, (where, int((whi - wlo).max()))
    if G > 1:
        assert not np.any(wlo & 7), where                 # 128-byte aligned starts


def tiles_to_check(tiles, nwaves, G, dense=DENSE, stride=STRIDE):
    """Every size within ``dense`` tiles of a change of (nwaves, G), every ``stride``-th
    other size, the smallest and the largest: indices into the table."""
    n = tiles.size
    change = np.flatnonzero((nwaves[1:] != nwaves[:-1]) | (G[1:] != G[:-1])) + 1  # differs from the one before
    pick = np.zeros(n, bool)
    for d in range(-dense, dense):
        pick[np.clip(change + d, 0, n - 1)] = True
    pick[::stride] = True
    pick[[0, n - 1]] = True
    return np.flatnonzero(pick)


@pytest.mark.parametrize("cus", CUS)
def test_cover_property(cus):
    """Models of 4, 8, ..., 800,000 vote groups, both counter classes.  On every one
    of those sizes: 1 <= G <= 4, 1 to 4 waves per block (1 at G = 1) and the
    arithmetic bound ceil(vote_groups / nwaves) + 7 <= 64 G (no 7 at G = 1) that the
    range rule needs.  On the ranges the kernel's own function returns, either side
    of every change of (nwaves, G) and on a stride elsewhere: contiguous, a partition
    of [0, vote_groups), 8-aligned starts for G > 1, no range longer than 64 G.
    Holds for any build of the library (DLS_HIP_LIB, the module docstring)."""
    for K in (K_NARROW, K_WIDE):
        tiles, nwaves, G, wpb = geometry_table(K, cus)
        assert wpb.min() >= 1 and wpb.max() <= 4 and np.all(wpb[G == 1] == 1), (K, cus)
        assert G.min() >= 1 and G.max() <= 4, (K, cus, int(G.max()), int(256 * tiles[G.argmax()]))
        longest = -(-4 * tiles // nwaves) + np.where(G > 1, 7, 0)
        bad = np.flatnonzero(longest > 64 * G)
        assert bad.size == 0, (K, cus, int(256 * tiles[bad[0]]))
        if K == K_WIDE:
            # wide counters: one group per lane, 64-group ranges, no CU term; nwaves steps
            # every 16 tiles, so the ranges are checked either side of every step up to
            # 2^16 groups and of every 23rd step from there
            assert G.max() == 1 and np.array_equal(nwaves, (4 * tiles + 63) // 64)
            idx = tiles_to_check(tiles, nwaves, G, dense=1, stride=10 ** 9)
            idx = np.concatenate([idx[tiles[idx] <= 1 << 14], idx[tiles[idx] > 1 << 14][::23], [tiles.size - 1]])
        else:
            idx = tiles_to_check(tiles, nwaves, G)
        for i in idx.tolist():
            check_ranges(256 * int(tiles[i]), K, cus, int(nwaves[i]), int(G[i]))


def test_parent_formula_dropped_groups_at_33m_parameters():
    """The case of the module docstring, and what the library gives there now."""
    P, cus = 33_030_400, 256
    vg = groups_of(P)
    assert vg == 516_100
    nw, G, _ = parent_geometry(vg, cus)
    assert (nw, G) == (2048, 5)
    lo, hi = rule_range(nw - 1, vg, nw, G)
    assert (lo, hi) == (515_840, 516_100) and hi - lo == 260 > 64 * 4
    assert _native.sign_vote_geometry(P, K_NARROW, cus) == (3072, 3, 4)
    check_ranges(P, K_NARROW, cus, 3072, 3)
    # the whole first band of the old formula at 256 CUs, every tile
    first, last = 32_637_184, 33_095_680
    assert parent_geometry(groups_of(first - 256), cus)[1] == 4 and parent_geometry(groups_of(first), cus)[1] == 5
    assert parent_geometry(groups_of(last), cus)[1] == 5 and parent_geometry(groups_of(last + 256), cus)[1] == 3
    for P in range(first, last + 1, 256):
        nw, G, wpb = _native.sign_vote_geometry(P, K_NARROW, cus)
        assert (nw, G, wpb) == (3072, 3, 4), P
    for P in (first, first + 256 * 7, last - 256, last):
        check_ranges(P, K_NARROW, cus, 3072, 3)


# (P, nwaves, G) at 256 CUs in the narrow counter class, from the formula before the
# fix: the sizes the GPU tests and the benchmark launch, and both sides of every
# transition below the first band (G 1 -> 2, 2 -> 3, 3 -> 4, the multiplier's first step)
PINS_256 = [
    (4_000_000, 1024, 2), (5_000_004, 1024, 2), (9_000_004, 1024, 3), (11_173_964, 1024, 3),
    (14_000_000, 1024, 4), (70_000_000, 5120, 4),
    (3_735_808 - 256, 912, 1), (3_735_808, 1024, 2),
    (7_930_112 - 256, 1024, 2), (7_930_112, 1024, 3),
    (12_124_416 - 256, 1024, 3), (12_124_416, 1024, 4),
    (16_318_720 - 256, 1024, 4), (16_318_720, 2048, 3),
]


@pytest.mark.parametrize("P,nwaves,G", PINS_256)
def test_geometry_pins(P, nwaves, G):
    for K in (1, 13, K_NARROW, 1000, 32_760):  # every narrow width class
        assert _native.sign_vote_geometry(P, K, 256) == (nwaves, G, 4 if G > 1 else 1), K
    assert parent_geometry(groups_of(P), 256)[:2] == (nwaves, G)
    check_ranges(P, K_NARROW, 256, nwaves, G)
    # wide counters (CB = 16 from K = 32,761): one group per lane, 64-group ranges
    assert _native.sign_vote_geometry(P, 32_761, 256) == ((groups_of(P) + 63) // 64, 1, 1)


@pytest.mark.parametrize("cus", CUS)
def test_geometry_is_the_parents_outside_its_bands(cus):
    """Where the old formula gave G <= 4 the geometry is unchanged (so every such
    shape runs the instantiation it ran); where it gave 5, the multiplier grew."""
    tiles, nwaves, G, _ = geometry_table(K_NARROW, cus)
    changed = 0
    for t, nw, g in zip(tiles.tolist(), nwaves.tolist(), G.tolist()):
        pn, pg, _ = parent_geometry(4 * t, cus)
        if pg <= 4:
            assert (nw, g) == (pn, pg), (cus, t)
        else:
            changed += 1
            assert pg == 5 and nw > pn and nw % (4 * cus) == 0 and 3 <= g <= 4, (cus, t)
    assert changed  # every CU count of the sweep has such a band below 800,000 groups
    wpb = geometry_table(K_NARROW, cus)[3]
    assert np.array_equal(wpb, np.where(G > 1, 4, 1))  # the default build: blocks of 4 waves


def test_query_arguments():
    L = _native.lib()
    nw = ctypes.c_int64()
    assert L.dls_sign_vote_geometry(0, 4, 256, ctypes.byref(nw), None, None) == -1
    assert b"P=0" in L.dls_last_error()
    assert L.dls_sign_vote_geometry(1024, 0, 256, ctypes.byref(nw), None, None) == -1
    assert L.dls_sign_vote_geometry(1024, 1 << 20, 256, ctypes.byref(nw), None, None) == -1
    assert b"2^20-1" in L.dls_last_error()
    assert L.dls_sign_vote_geometry(1024, 4, 256, ctypes.byref(nw), None, None) == 0 and nw.value == 1
    with pytest.raises(RuntimeError, match="waves"):
        _native.sign_vote_wave_ranges(4_000_000, 13, 256, first_wave=1000, count=25)
    with pytest.raises(RuntimeError, match="waves"):
        _native.sign_vote_wave_ranges(4_000_000, 13, 256, first_wave=-1, count=1)
    assert L.dls_sign_vote_wave_ranges(4_000_000, 13, 256, 0, 1, None, None) == -1
    lo, hi = _native.sign_vote_wave_ranges(4_000_000, 13, 256, first_wave=1023, count=1)
    assert hi[0] == groups_of(4_000_000) and lo[0] % 8 == 0 and 0 < hi[0] - lo[0] <= 128
    # P that is no whole tile: the vote walks whole tiles
    assert _native.sign_vote_geometry(3_735_808 - 252, 13, 256) == (1024, 2, 4)


def test_header_declares_and_binding_exposes_the_queries():
    text = open(os.path.join(ROOT, "include", "dls_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("dls_sign_vote_geometry", "dls_sign_vote_wave_ranges"):
        assert re.search(r"\bint " + name + r"\s*\(", text), name
        assert name in _native.SIGNATURES and hasattr(_native.lib(), name)
    assert "int64_t *nwaves, int32_t *G,\n                           int32_t *waves_per_block);" in text
    assert "sign_geometry.h" in _native.CSRC_HASHED
    with open(os.path.join(ROOT, "distributed_learning_simulator_amd", "csrc", "Makefile")) as fh:
        assert "sign_geometry.h" in next(line for line in fh if line.startswith("HASHED :="))
    assert callable(_native.sign_vote_geometry) and callable(_native.sign_vote_wave_ranges)


def test_unknown_groups_per_lane_has_no_default_kernel():
    """The launch's switch over G has no arm that stands for "4 or anything else"."""
    src = open(os.path.join(ROOT, "distributed_learning_simulator_amd", "csrc", "sign.hip")).read()
    assert "default: DLS_VOTE_LAUNCH" not in src
