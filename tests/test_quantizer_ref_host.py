"""tests/quantizer_ref.py against torch on the CPU (never against the code under
test) and the committed quantize.npz vectors: finite, in-range inputs, where
torch's behaviour is defined.  Scales and dequantized values bit for bit,
integers exactly.  Runs on any machine."""
import numpy as np
import pytest
import torch
from torch.ao.quantization.observer import MinMaxObserver, PerChannelMinMaxObserver

from tests import golden as G
from tests import quantizer_ref as R

DTYPE_RANGE = {torch.quint8: (0, 255), torch.qint8: (-128, 127)}
# (dtype, custom quant_min / quant_max or None)
OBSERVER_CASES = [(torch.quint8, None), (torch.qint8, None), (torch.quint8, (0, 15)),
                  (torch.quint8, (0, 127)), (torch.qint8, (0, 15)), (torch.qint8, (0, 127))]
IDS = ["quint8", "qint8", "quint8-0..15", "quint8-0..127", "qint8-0..15", "qint8-0..127"]


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def tensors():
    """Inputs whose (min, max) cover both signs, one side only, zero, and a tiny range."""
    g = torch.Generator().manual_seed(5)
    r = torch.randn(257, generator=g)
    return [r, r.abs() + 0.25, -r.abs() - 0.25, r * 1e-3 + 7.0, r * 1e4, torch.zeros(9),
            torch.tensor([0.0, 1e-9]), torch.tensor([-3.0, 0.5]), torch.tensor([-0.5, 3.0]),
            torch.tensor([-1.0, 254.0]), torch.tensor([-127.5, 127.5]), torch.tensor([-2.5, 252.5])]


def qrange(dtype, custom):
    return custom if custom is not None else DTYPE_RANGE[dtype]


def observer_kwargs(dtype, custom):
    kw = dict(dtype=dtype)
    if custom is not None:
        kw.update(quant_min=custom[0], quant_max=custom[1])
    return kw


@pytest.mark.parametrize("dtype,custom", OBSERVER_CASES, ids=IDS)
def test_affine_qparams_vs_minmax_observer(dtype, custom):
    qmin, qmax = qrange(dtype, custom)
    for x in tensors():
        obs = MinMaxObserver(qscheme=torch.per_tensor_affine, **observer_kwargs(dtype, custom))
        obs(x)
        sc_t, zp_t = obs.calculate_qparams()
        lo, hi = R.segment_minmax(x.numpy(), [0, x.numel()])
        assert float(lo[0]) == float(x.min()) and float(hi[0]) == float(x.max())
        sc, zp = R.qparams(lo, hi, qmin, qmax)
        assert np.array_equal(bits(sc), bits(sc_t.float().numpy().reshape(1))), (x.min(), x.max())
        assert int(zp[0]) == int(zp_t), (x.min(), x.max())


@pytest.mark.parametrize("dtype,custom", OBSERVER_CASES, ids=IDS)
def test_symmetric_qparams_vs_per_channel_observer(dtype, custom):
    """Scales bit for bit in every case.  Zero points where torch's rule and the
    header's coincide: the dtypes' own ranges (0 for qint8, 128 for quint8).  With a
    custom range torch chooses by dtype (qint8: 0) and down-rounds the midpoint
    (quint8: (qmin + qmax) // 2, which would make [0, 255] 127, not 128); the header
    chooses by the sign of qmin and up-rounds, so there the header's value is pinned."""
    qmin, qmax = qrange(dtype, custom)
    x = torch.stack([t[:2] for t in tensors()] + [torch.tensor([-0.0, -7.0])])  # [C, 2]
    x = torch.cat([x, x.flip(1) * 0.37], 1)
    obs = PerChannelMinMaxObserver(ch_axis=0, qscheme=torch.per_channel_symmetric,
                                   **observer_kwargs(dtype, custom))
    obs(x)
    sc_t, zp_t = obs.calculate_qparams()
    C, row = x.shape
    lo, hi = R.segment_minmax(x.numpy(), np.arange(C + 1) * row)
    assert np.array_equal(lo, x.min(1).values.numpy()) and np.array_equal(hi, x.max(1).values.numpy())
    sc, zp = R.qparams(lo, hi, qmin, qmax, symmetric=True)
    assert np.array_equal(bits(sc), bits(sc_t.float().numpy()))
    if custom is None:
        assert np.array_equal(zp, zp_t.numpy().astype(np.int32))
    else:
        assert np.array_equal(zp, np.full(C, (qmin + qmax + 1) // 2, np.int32))
        torch_rule = 0 if dtype == torch.qint8 else (qmin + qmax) // 2
        assert np.array_equal(zp_t.numpy(), np.full(C, torch_rule))  # the divergence, as stated


def quantize_inputs(scale, zp, qmin, qmax):
    """Values around every tie and both clamps of the range, and random ones."""
    g = torch.Generator().manual_seed(9)
    k = torch.arange(qmin - zp - 3, qmax - zp + 4, dtype=torch.float32)
    ties = torch.cat([k, k + 0.5, k + 0.25, k - 0.25]) * scale
    rnd = (torch.rand(2048, generator=g) * (qmax - qmin + 6) + (qmin - zp - 3)) * scale
    return torch.cat([ties, rnd, torch.tensor([0.0, -0.0])])


@pytest.mark.parametrize("dtype,scale,zp", [
    (torch.quint8, 0.0625, 10), (torch.quint8, 0.1, 0), (torch.quint8, 3.0, 255),
    (torch.quint8, 0.0123, 128), (torch.qint8, 0.0625, 0), (torch.qint8, 0.1, 5),
    (torch.qint8, 3.0, -128), (torch.qint8, 0.0123, 127)])
def test_quantize_vs_torch_quantize_per_tensor(dtype, scale, zp):
    qmin, qmax = DTYPE_RANGE[dtype]
    x = quantize_inputs(scale, zp, qmin, qmax)
    qt = torch.quantize_per_tensor(x, scale, zp, dtype)
    q, deq = R.quantize(x.numpy(), [0, x.numel()], [scale], [zp], qmin, qmax)
    assert np.array_equal(q, qt.int_repr().numpy().astype(np.int32))
    assert np.array_equal(R.as_bytes(q, qmin), qt.int_repr().numpy())
    assert np.array_equal(bits(deq), bits(qt.dequantize().numpy()))


@pytest.mark.parametrize("qmin,qmax,scale,zp", [(0, 15, 0.25, 3), (0, 127, 0.1, 64), (0, 1, 3.0, 1),
                                                (-128, 127, 3.0, 5)])
def test_quantize_custom_range_vs_torch_fake_quantize(qmin, qmax, scale, zp):
    x = quantize_inputs(scale, zp, qmin, qmax)
    fq = torch.fake_quantize_per_tensor_affine(x, scale, zp, qmin, qmax)
    _, deq = R.quantize(x.numpy(), [0, x.numel()], [scale], [zp], qmin, qmax)
    assert np.array_equal(bits(deq), bits(fq.numpy()))


@pytest.mark.parametrize("dtype", [torch.quint8, torch.qint8], ids=["quint8", "qint8"])
def test_quantize_vs_torch_quantize_per_channel(dtype):
    qmin, qmax = DTYPE_RANGE[dtype]
    g = torch.Generator().manual_seed(13)
    C, row = 7, 45
    scales = torch.tensor([0.0625, 0.1, 3.0, 0.0123, 1e-3, 0.5, 2.0 ** -23], dtype=torch.float32)
    zps = torch.tensor([0, 5, qmin, qmax, (qmin + qmax + 1) // 2, 1, 0])
    x = (torch.rand(C, row, generator=g) * (qmax - qmin + 6) + (qmin - 3)
         - zps[:, None].float()) * scales[:, None]
    x[:, 0] = (torch.tensor([0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 3.5])) * scales  # ties
    qt = torch.quantize_per_channel(x, scales.double(), zps, 0, dtype)
    q, deq = R.quantize(x.numpy(), np.arange(C + 1) * row, scales.numpy(), zps.numpy(), qmin, qmax)
    assert np.array_equal(q.reshape(C, row), qt.int_repr().numpy().astype(np.int32))
    assert np.array_equal(bits(deq).reshape(C, row), bits(qt.dequantize().numpy()))


def test_golden_quantize_vectors():
    z = G.load("quantize.npz")
    x = z["pt_x"]
    q, deq = R.quantize(x, [0, x.size], [np.float32(z["pt_scale"])], [int(z["pt_zp"])], 0, 255)
    assert np.array_equal(R.as_bytes(q, 0), z["pt_q"])
    assert np.array_equal(bits(deq), bits(z["pt_deq"]))
    xt = z["tie_x"]
    qt, _ = R.quantize(xt, [0, xt.size], [0.0625], [10], 0, 255)
    assert np.array_equal(R.as_bytes(qt, 0), z["tie_q"])
    w = z["pc_x"]
    C, row = w.shape[0], w[0].size
    qc, dc = R.quantize(w, np.arange(C + 1) * row, z["pc_scale"].astype(np.float32),
                        np.zeros(C, np.int32), -128, 127)
    assert np.array_equal(R.as_bytes(qc, -128).reshape(w.shape), z["pc_q"])
    want = z["pc_q"].astype(np.float32) * z["pc_scale"].astype(np.float32)[:, None, None]
    assert np.array_equal(bits(dc).reshape(w.shape), bits(want))


def test_special_values_are_defined():
    """What the header states for the values torch leaves open."""
    nan, inf = np.float32("nan"), np.float32("inf")
    lo, hi = R.segment_minmax([nan, nan, 1.0, nan, -0.0], [0, 0, 2, 2, 4, 5, 5])
    assert lo.tolist() == [inf, inf, inf, 1.0, 0.0, inf]
    assert hi.tolist() == [-inf, -inf, -inf, 1.0, 0.0, -inf]
    sc, zp = R.qparams(lo, hi, -128, 127)
    assert sc[0] == R.EPS and zp[0] == -128  # the identities: the range [0, 0]
    sc, zp = R.qparams([-inf, -1.0, -inf], [1.0, inf, inf], 0, 255)
    assert np.all(np.isposinf(sc)) and zp.tolist() == [0, 0, 0]
    x = np.array([nan, inf, -inf, 3.4028235e38, -3.4028235e38, -0.0], np.float32)
    q, deq = R.quantize(x, [0, 6], [0.5], [5], -128, 127)
    assert q.tolist() == [-128, 127, -128, 127, -128, 5]
    assert np.array_equal(bits(deq), bits(np.array([-66.5, 61.0, -66.5, 61.0, -66.5, 0.0])))
    a, b = R.stochastic_bracket(np.array([0.6, -0.6, nan, inf, 63.9], np.float32), [0, 5], [0.5], [5],
                                -128, 127)
    assert a.tolist() == [6, 3, -128, 127, 127] and b.tolist() == [7, 4, -128, 127, 127]
