"""CPU checks of the loss utilities: dls_softmax_ce_f32, dls_lenet5_eval_loss_f32 and
dls_sum_rows_f64 validate every argument before any device call (the device
pointers below are never dereferenced), the Shapley servers reject an unknown
utility metric, and the simulator carries --utility_metric to them alone."""
import ctypes
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "distributed_learning_simulator_amd", "libdls_hip.so")

EINVAL, ELAYOUT = -1, -2
# ParameterLayout.offsets of a 10-output LeNet-5 (tests/test_lenet_host.py)
OFFSETS = [0, 192, 256, 2688, 2752, 50752, 50880, 60992, 61120, 62016]
LDM = 62080
D = 4096  # 16-byte aligned, never dereferenced
i64, i32, p = ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(LIB):
        pytest.fail("libdls_hip.so is not built (run __graft_entry__.build())")
    lib = ctypes.CDLL(LIB)
    lib.dls_last_error.restype = ctypes.c_char_p
    lib.dls_softmax_ce_f32.restype = ctypes.c_int
    lib.dls_softmax_ce_f32.argtypes = [p, i32, i64, i32, p, p, i64, p]
    lib.dls_sum_rows_f64.restype = ctypes.c_int
    lib.dls_sum_rows_f64.argtypes = [p, i64, i32, i64, p, p]
    lib.dls_lenet5_eval_loss_f32.restype = ctypes.c_int
    lib.dls_lenet5_eval_loss_f32.argtypes = [p, i64, i32, p, p, i64, p, i32, p, p, p, i64, p]
    return lib


def _ce(L, **kw):
    a = dict(logits=D, S=2, B=5, O=10, labels=D, loss=D, ldn=8)
    a.update(kw)
    rc = L.dls_softmax_ce_f32(a["logits"], a["S"], a["B"], a["O"], a["labels"], a["loss"],
                              a["ldn"], None)
    return rc, L.dls_last_error()


def _sum(L, **kw):
    a = dict(v=D, ldn=8, S=2, n=5, out=D)
    a.update(kw)
    rc = L.dls_sum_rows_f64(a["v"], a["ldn"], a["S"], a["n"], a["out"], None)
    return rc, L.dls_last_error()


def _lenet(L, **kw):
    a = dict(models=D, ldm=LDM, S=2, offsets=OFFSETS, x=D, B=5, labels=D, O=10, logits=D,
             correct=D, loss=D, ldn=8)
    a.update(kw)
    off = None if a["offsets"] is None else (ctypes.c_int64 * 10)(*a["offsets"])
    rc = L.dls_lenet5_eval_loss_f32(a["models"], a["ldm"], a["S"], off, a["x"], a["B"],
                                    a["labels"], a["O"], a["logits"], a["correct"], a["loss"],
                                    a["ldn"], None)
    return rc, L.dls_last_error()


@pytest.mark.parametrize("kw, rc, what", [
    (dict(logits=None), EINVAL, b"logits"),
    (dict(labels=None), EINVAL, b"labels"),
    (dict(loss=None), EINVAL, b"loss"),
    (dict(S=0), EINVAL, b"S=0"),
    (dict(S=-2), EINVAL, b"S=-2"),
    (dict(B=-1), EINVAL, b"B=-1"),
    (dict(O=0), EINVAL, b"O=0"),
    (dict(ldn=4), EINVAL, b"ldn=4"),
    (dict(S=2 ** 31 - 1, B=2 ** 40, ldn=2 ** 40), EINVAL, b"grid"),
    (dict(logits=D + 8), ELAYOUT, b"logits"),
    (dict(labels=D + 4), ELAYOUT, b"labels"),
    (dict(loss=D + 2), ELAYOUT, b"loss"),
])
def test_softmax_ce_rejects_bad_arguments(L, kw, rc, what):
    got, msg = _ce(L, **kw)
    assert got == rc and what in msg and b"dls_softmax_ce_f32" in msg, (got, msg)


def test_softmax_ce_takes_wide_rows_and_an_empty_batch(L):
    """O has no upper bound of 32 (the check passes validation only with B == 0
    here: nothing may be launched without a GPU), and B == 0 is a no-op."""
    assert _ce(L, B=0, O=1000, ldn=0)[0] == 0
    assert _ce(L, B=0, O=1)[0] == 0


@pytest.mark.parametrize("kw, rc, what", [
    (dict(v=None), EINVAL, b"v"),
    (dict(out=None), EINVAL, b"out"),
    (dict(S=0), EINVAL, b"S=0"),
    (dict(n=-1), EINVAL, b"n=-1"),
    (dict(ldn=4), EINVAL, b"ldn=4"),
    (dict(v=D + 2), ELAYOUT, b"v:"),
    (dict(out=D + 4), ELAYOUT, b"out"),
])
def test_sum_rows_rejects_bad_arguments(L, kw, rc, what):
    got, msg = _sum(L, **kw)
    assert got == rc and what in msg and b"dls_sum_rows_f64" in msg, (got, msg)


@pytest.mark.parametrize("kw, rc, what", [
    (dict(models=None), EINVAL, b"models"),
    (dict(offsets=None), EINVAL, b"offsets"),
    (dict(x=None), EINVAL, b"x"),
    (dict(logits=None, correct=None, loss=None), EINVAL, b"all null"),
    (dict(labels=None), EINVAL, b"labels"),
    (dict(labels=None, correct=None), EINVAL, b"labels"),  # loss alone needs labels
    (dict(labels=None, loss=None), EINVAL, b"labels"),  # correct alone too
    (dict(S=0), EINVAL, b"S=0"),
    (dict(B=-1), EINVAL, b"B=-1"),
    (dict(O=0), EINVAL, b"O=0"),
    (dict(O=33), EINVAL, b"O=33"),
    (dict(ldn=4), EINVAL, b"ldn=4"),
    (dict(S=2 ** 20, B=2 ** 20, ldn=2 ** 20), EINVAL, b"grid"),
    (dict(ldm=60000), EINVAL, b"ldm"),
    (dict(models=D + 8), ELAYOUT, b"models"),
    (dict(x=D + 4), ELAYOUT, b"x"),
    (dict(logits=D + 8), ELAYOUT, b"logits"),
    (dict(labels=D + 4), ELAYOUT, b"labels"),
    (dict(correct=D + 4), ELAYOUT, b"correct"),
    (dict(loss=D + 2), ELAYOUT, b"loss"),
    (dict(ldm=LDM + 2), ELAYOUT, b"ldm"),
    (dict(offsets=OFFSETS[:9] + [62014]), ELAYOUT, b"fc3.bias"),
])
def test_lenet5_eval_loss_rejects_bad_arguments(L, kw, rc, what):
    got, msg = _lenet(L, **kw)
    assert got == rc and what in msg and b"dls_lenet5_eval_loss_f32" in msg, (got, msg)


def test_lenet5_eval_loss_outputs_are_each_optional(L):
    """Any one output alone passes validation (B == 0: no launch, no device), labels
    may be null with logits alone, and ldn is not looked at without loss."""
    assert _lenet(L, B=0)[0] == 0
    assert _lenet(L, B=0, logits=None, correct=None)[0] == 0
    assert _lenet(L, B=0, logits=None, loss=None)[0] == 0
    assert _lenet(L, B=0, correct=None, loss=None, labels=None)[0] == 0
    assert _lenet(L, B=0, loss=None, ldn=-5)[0] == 0


def test_python_wrappers_validate_before_the_library():
    """softmax_ce / sum_rows_f64 / lenet5_eval(loss=) reject operands the kernels
    would read or write out of bounds (CPU tensors: the checks come first)."""
    import torch
    from distributed_learning_simulator_amd import _native
    lg = torch.zeros(2, 5, 10)
    y = torch.zeros(5, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="logits"):
        _native.softmax_ce(lg.double(), y)
    with pytest.raises(RuntimeError, match="logits"):
        _native.softmax_ce(torch.zeros(2, 5, 20)[:, :, ::2], y)
    with pytest.raises(RuntimeError, match="labels"):
        _native.softmax_ce(lg, y.int())
    with pytest.raises(RuntimeError, match="labels"):
        _native.softmax_ce(lg, torch.zeros(4, dtype=torch.int64))
    for bad in (torch.zeros(2, 4), torch.zeros(2, 5, dtype=torch.float64),
                torch.zeros(2, 10)[:, ::2], torch.zeros(5, 2).t()):
        with pytest.raises(RuntimeError, match="loss"):
            _native.softmax_ce(lg, y, loss=bad)
    with pytest.raises(RuntimeError, match="v must be"):
        _native.sum_rows_f64(torch.zeros(2, 5, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="v must be"):
        _native.sum_rows_f64(torch.zeros(5))
    with pytest.raises(RuntimeError, match="v must be"):
        _native.sum_rows_f64(torch.zeros(5, 2).t())
    with pytest.raises(RuntimeError, match="out must be"):
        _native.sum_rows_f64(torch.zeros(2, 5), out=torch.zeros(2))
    models, x = torch.zeros(2, LDM), torch.zeros(5, 1, 32, 32)
    with pytest.raises(RuntimeError, match="loss needs labels"):
        _native.lenet5_eval(models, OFFSETS, x, loss=torch.zeros(2, 5), num_out=10)
    with pytest.raises(RuntimeError, match="loss must be"):
        _native.lenet5_eval(models, OFFSETS, x, labels=y, loss=torch.zeros(2, 6), num_out=10)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # valid operands reach _ptr
        _native.lenet5_eval(models, OFFSETS, x, labels=y, loss=torch.zeros(2, 8)[:, 1:6],
                            num_out=10)


def test_shapley_servers_reject_an_unknown_utility_metric():
    """The keyword is checked before anything else is built (no GPU needed)."""
    from distributed_learning_simulator_amd.distributed import get_sharded_server  # noqa: F401
    from distributed_learning_simulator_amd.servers.GTG_shapley_value_server import \
        GTGShapleyValueServer
    from distributed_learning_simulator_amd.servers.multiround_shapley_value_server import \
        MultiRoundShapleyValueServer
    from distributed_learning_simulator_amd.servers.shapley_value_server import ShapleyValueServer
    for cls in (ShapleyValueServer, GTGShapleyValueServer, MultiRoundShapleyValueServer):
        with pytest.raises(ValueError, match="utility_metric"):
            cls(utility_metric="x", tester=None, worker_number=2)


def test_simulator_carries_the_flag_to_the_shapley_servers_only():
    from distributed_learning_simulator_amd.simulator import get_config, server_kwargs
    base = ["--worker_number", "2", "--round", "1", "--distributed_algorithm"]
    for algo in ("GTG_shapley_value", "multiround_shapley_value"):
        assert get_config(base + [algo]).utility_metric == "acc"
        assert server_kwargs(get_config(base + [algo]))["utility_metric"] == "acc"
        cfg = get_config(base + [algo, "--utility_metric", "loss"])
        assert server_kwargs(cfg) == {"aggregation_mode": "exact", "utility_metric": "loss"}
    for algo in ("fed", "fed_quant", "sign_SGD"):
        cfg = get_config(base + [algo, "--utility_metric", "loss"])
        assert "utility_metric" not in server_kwargs(cfg)
    with pytest.raises(SystemExit):
        get_config(base + ["fed", "--utility_metric", "f1"])
