"""CPU checks of dls_lenet5_eval_f32: every argument is validated before any
device call (the device pointers below are never dereferenced; offsets is the
entry point's one host array)."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "distributed_learning_simulator_amd", "libdls_hip.so")

EINVAL, ELAYOUT = -1, -2
# ParameterLayout.offsets of a 10-output LeNet-5 (tensors start at multiples of 64)
OFFSETS = [0, 192, 256, 2688, 2752, 50752, 50880, 60992, 61120, 62016]
LDM = 62080


@pytest.fixture(scope="module")
def call():
    if not os.path.exists(LIB):
        pytest.fail("libdls_hip.so is not built (run __graft_entry__.build())")
    L = ctypes.CDLL(LIB)
    L.dls_last_error.restype = ctypes.c_char_p
    f = L.dls_lenet5_eval_f32
    f.restype = ctypes.c_int
    i64, i32, p = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p
    f.argtypes = [p, i64, i32, p, p, i64, p, i32, p, p, p]
    d = 4096  # 16-byte aligned, never dereferenced

    def run(**kw):
        a = dict(models=d, ldm=LDM, S=2, offsets=OFFSETS, x=d, B=5, labels=d, O=10, logits=d,
                 correct=d)
        a.update(kw)
        off = None if a["offsets"] is None else (ctypes.c_int64 * 10)(*a["offsets"])
        rc = f(a["models"], a["ldm"], a["S"], off, a["x"], a["B"], a["labels"], a["O"],
               a["logits"], a["correct"], None)
        return rc, L.dls_last_error()

    return run


def test_layout_offsets_are_the_flat_layouts():
    """The offsets the cases below use are ParameterLayout's for models.LeNet5."""
    from distributed_learning_simulator_amd.models import LeNet5
    lay = LeNet5().split_layout()
    assert lay.offsets == OFFSETS and lay.P == LDM


@pytest.mark.parametrize("kw, what", [
    (dict(models=None), b"models"),
    (dict(offsets=None), b"offsets"),
    (dict(x=None), b"x"),
    (dict(logits=None, correct=None), b"both null"),
    (dict(labels=None), b"labels"),
    (dict(S=0), b"S=0"),
    (dict(S=-3), b"S=-3"),
    (dict(B=-1), b"B=-1"),
    (dict(O=0), b"O=0"),
    (dict(O=33), b"O=33"),
])
def test_rejects_bad_arguments(call, kw, what):
    rc, msg = call(**kw)
    assert rc == EINVAL and what in msg, (rc, msg)


@pytest.mark.parametrize("kw, what", [
    (dict(models=4096 + 8), b"models"),
    (dict(x=4096 + 4), b"x"),
    (dict(logits=4096 + 8), b"logits"),
    (dict(labels=4096 + 4), b"labels"),
    (dict(correct=4096 + 4), b"correct"),
    (dict(ldm=LDM + 2), b"ldm"),
    (dict(offsets=OFFSETS[:4] + [2754] + OFFSETS[5:]), b"fc1.weight"),
    (dict(offsets=OFFSETS[:9] + [62014]), b"fc3.bias"),
])
def test_rejects_bad_layout(call, kw, what):
    rc, msg = call(**kw)
    assert rc == ELAYOUT and what in msg, (rc, msg)


def test_rejects_a_tensor_past_the_row(call):
    """An offset that would read past ldm is refused (no out-of-bounds read)."""
    rc, msg = call(offsets=OFFSETS[:9] + [LDM - 8])  # fc3.bias: 10 elements from ldm - 8
    assert rc == EINVAL and b"fc3.bias" in msg and b"ldm" in msg
    rc, msg = call(ldm=60000)
    assert rc == EINVAL and b"ldm" in msg


def test_labels_may_be_null_without_correct_and_empty_batch_is_ok(call):
    """B == 0 returns 0 without a launch (no device is touched: this runs without a
    GPU), also with labels null when no count is asked for."""
    assert call(B=0)[0] == 0
    assert call(B=0, labels=None, correct=None)[0] == 0
    assert call(B=0, logits=None)[0] == 0
