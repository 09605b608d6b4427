"""Host tests of the convolution dispatch (csrc/conv.hip conv_choose through
dls_conv_kernel_choice / dls_conv_stem_kernel_choice): which kernel a shape runs
on, without a GPU.  The launch and the query share the decision code, so what is
pinned here is what dls_conv_bn_act_split launches."""
import os
import subprocess
import sys

import pytest

from distributed_learning_simulator_amd import _native

GENERIC64, GENERIC128, PIPE64_H10, PIPE64_H12, PIPE128_W4, PIPE128_W8_H5, PIPE128_W8_H6 = range(1, 8)
HALO128, HALO128_SKEW, HALO64, HALO64_SKEW, PHASE = range(8, 13)

# what the sweep below returns, written out; the 64-channel halo forms
# (k_conv3x3_halo<1,4,11,*>) are compiled but no shape of the sweep reaches them:
# every 64-channel shape their halo tile fits is taken by the pipeline first
REACHABLE = {GENERIC64, GENERIC128, PIPE64_H10, PIPE64_H12, PIPE128_W4, PIPE128_W8_H5, PIPE128_W8_H6,
             HALO128, HALO128_SKEW, PHASE}
UNREACHABLE = {HALO64, HALO64_SKEW}


def choice(B, H, W, C, Cout, k=3, s=1, p=1):
    return _native.conv_kernel_choice(B, H, W, C, Cout, (k, k), s, p)


@pytest.fixture(scope="module")
def sweep():
    """id -> first shape, for H, W in 1..128, Cout in {64, 128}, B in {1, 3}, C = 32,
    3x3 pad 1 at stride 1 and 2."""
    f = _native.lib().dls_conv_kernel_choice
    found = {}
    for s in (1, 2):
        for H in range(1, 129):
            for W in range(1, 129):
                for co in (64, 128):
                    for B in (1, 3):
                        found.setdefault(f(B, H, W, 32, co, 3, 3, s, 1), (B, H, W, co, s))
    return found


def test_header_ids_match_binding():
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "dls_hip.h")).read()
    conv = {int(v) for v in re.findall(r"#define DLS_CONV_KERNEL_\w+ (\d+)", text)}
    stem = {int(v) for v in re.findall(r"#define DLS_STEM_KERNEL_\w+ (\d+)", text)}
    assert conv == set(_native.CONV_KERNELS) == REACHABLE | UNREACHABLE | {0}
    assert stem == set(_native.STEM_KERNELS) == {0, 1, 2, 3}


def test_reachability_sweep(sweep):
    assert set(sweep) == REACHABLE, {k: v for k, v in sweep.items() if k not in REACHABLE}
    assert not set(sweep) & UNREACHABLE


def test_whole_dispatch_table_is_pinned():
    """Every id of the sweep, in the sweep's order, one byte each: the table a
    refactor of conv_choose / fit_* must reproduce (131,072 shapes; the digest is
    of the table the library gave before the probe knobs were folded in)."""
    import hashlib
    f = _native.lib().dls_conv_kernel_choice
    table = bytes(f(B, H, W, 32, co, 3, 3, s, 1) for s in (1, 2) for H in range(1, 129)
                  for W in range(1, 129) for co in (64, 128) for B in (1, 3))
    assert len(table) == 131072
    counts = {i: table.count(i) for i in set(table)}
    assert counts == {1: 65448, 2: 65188, 3: 104, 4: 4, 5: 14, 6: 68, 7: 8, 8: 160, 9: 16, 12: 62}
    assert hashlib.sha256(table).hexdigest() == \
        "78db64fde289234d8d1c1dd7e7fa8518bcf2c31f72f6ff24cf947c24a93031fa"


def test_halo_forms_are_reached_where_the_fit_rules_say():
    assert choice(1, 64, 64, 32, 128) == HALO128        # 32 % 64: no pipeline
    assert choice(2, 12, 32, 32, 128) == HALO128        # the pipelines refuse H % TR or the halo's size
    assert choice(1, 2, 16, 32, 128) == HALO128_SKEW    # a 32-pixel image: no pipeline tile
    assert choice(1, 4, 8, 64, 128) == HALO128_SKEW
    assert choice(1, 2, 16, 32, 64) == GENERIC64        # 8 images' halo exceeds the 64-channel form
    assert choice(1, 64, 64, 32, 64) == GENERIC64
    assert choice(2, 28, 28, 64, 64) == GENERIC64       # 28 divides neither 128 nor 256
    assert choice(1, 12, 32, 32, 64) == GENERIC64


def test_choice_does_not_depend_on_history_or_environment():
    shapes = [(3, 32, 32, 64, 64, 3, 1, 1), (2, 16, 16, 128, 128, 3, 1, 1), (1, 64, 64, 32, 128, 3, 1, 1),
              (5, 8, 8, 32, 128, 3, 2, 1), (2, 7, 7, 128, 128, 3, 1, 1), (2, 8, 8, 64, 64, 1, 2, 0)]
    first = [choice(*t) for t in shapes]
    assert [choice(*t) for t in reversed(shapes)] == first[::-1]
    assert [choice(*t) for t in shapes for _ in range(2)] == [i for i in first for _ in range(2)]
    # a fresh process with another environment (the library reads none; the
    # variables carry the names of compile-time knobs the dispatch once had)
    code = ("from distributed_learning_simulator_amd import _native as n;"
            f"print([n.conv_kernel_choice(t[0],t[1],t[2],t[3],t[4],(t[5],t[5]),t[6],t[7]) for t in {shapes!r}])")
    env = dict(os.environ, DLS_CONV_GENERIC_ONLY="1", DLS_CONV_PIPE="0", DLS_PIPE_NARROW="7", HIP_VISIBLE_DEVICES="")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.check_output([sys.executable, "-c", code], env=env, cwd=root, text=True)
    assert out.strip() == repr(first)


def test_resnet18_layers_run_on_the_kernels_design_names():
    """at 32x32 every 3x3 stride-1 layer runs on the LDS-DMA pipeline,
    the stride-2 ones on the phase pipeline, the 1x1 shortcuts on the generic
    kernel; at 28x28 (14, 7, 4 after the strides) nothing fits a row tiling but
    the 4x4 layer."""
    B = 500
    at32 = {(64, 64, 3, 1, 32): PIPE64_H10, (64, 128, 3, 2, 32): PHASE, (64, 128, 1, 2, 32): GENERIC128,
            (128, 128, 3, 1, 16): PIPE64_H10, (128, 256, 3, 2, 16): PHASE, (128, 256, 1, 2, 16): GENERIC128,
            (256, 256, 3, 1, 8): PIPE128_W8_H5, (256, 512, 3, 2, 8): PHASE, (256, 512, 1, 2, 8): GENERIC128,
            (512, 512, 3, 1, 4): PIPE128_W8_H6, (32, 64, 1, 1, 32): GENERIC64}
    for (cin, cout, k, s, hw), want in at32.items():
        assert choice(B, hw, hw, cin, cout, k, s, k // 2) == want, (cin, cout, k, s, hw)
    at28 = {(64, 64, 3, 1, 28): GENERIC64, (64, 128, 3, 2, 28): GENERIC128, (128, 128, 3, 1, 14): GENERIC128,
            (128, 256, 3, 2, 14): GENERIC128, (256, 256, 3, 1, 7): GENERIC128, (256, 512, 3, 2, 7): GENERIC128,
            (512, 512, 3, 1, 4): PIPE128_W8_H6}
    for (cin, cout, k, s, hw), want in at28.items():
        assert choice(B, hw, hw, cin, cout, k, s, k // 2) == want, (cin, cout, k, s, hw)
    stem = _native.conv_stem_kernel_choice
    assert stem(B, 3, 32, 32, 64, (3, 3), 1, 1) == 1 and stem(B, 3, 28, 28, 64, (3, 3), 1, 1) == 2
    assert stem(B, 1, 28, 28, 64, (5, 5), 1, 2) == 3 and stem(0, 3, 32, 32, 64, (3, 3), 1, 1) == 0


def test_query_returns_the_launch_status_for_rejected_shapes():
    L = _native.lib()
    assert choice(0, 8, 8, 32, 64) == 0  # an empty batch launches nothing
    assert choice(2, 8, 8, 48, 64) == -1 and b"multiple of 32" in L.dls_last_error()
    assert choice(2, 8, 8, 64, 96) == -1 and b"Cout" in L.dls_last_error()
    assert choice(2, 1, 8, 32, 64, 3, 1, 0) == -1  # the kernel does not fit the image
    assert choice(1 << 26, 8, 8, 32, 64) == -1 and b"output pixels" in L.dls_last_error()
    assert _native.conv_stem_kernel_choice(2, 4, 8, 8, 64, (3, 3), 1, 1) == -1
    assert b"KH*KW*C" in L.dls_last_error()


def test_exact_gpu_cases_cover_every_reachable_kernel(sweep):
    """The coverage tie: the case table of tests/test_gpu_conv_exact.py reaches
    every kernel id the sweep proves reachable, and every stem form."""
    from tests.test_gpu_conv_exact import CASES, STEM_CASES
    ids = {_native.conv_kernel_choice(B, H, W, cin, cout, (kh, kw), s, p)
           for cin, cout, kh, kw, s, p, H, W, B in CASES}
    assert ids == set(sweep) == REACHABLE
    stems = {_native.conv_stem_kernel_choice(B, c, H, W, cout, (kh, kw), s, p)
             for c, cout, kh, kw, s, p, H, W, B in STEM_CASES}
    assert stems == {1, 2, 3}
    assert all(B * H * W * max(cin, cout) <= 2 ** 21 for cin, cout, _, _, _, _, H, W, B in CASES)
