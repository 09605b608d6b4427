"""The pack kernels of the deterministic convolutions against a CPU emulation of
the documented split format (include/dls_hip.h: hi = rne_bf16(x), lo =
rne_bf16(x - hi), lo = 0 under a non-finite hi, zeros in channel / K padding),
bit for bit, and the pooled linear layer (dls_pool_linear_split) against fp64."""
import pytest
import torch
import torch.nn.functional as F

from tests.test_gpu_conv_exact import _i16, bits_to_f32, split2_ref

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)

FLT_MAX = 3.4028234663852886e38


def _bits(v):
    return torch.tensor([x - (1 << 32) if x >= (1 << 31) else x for x in v], dtype=torch.int32).view(torch.float32)


# +-0, fp32 denormals, bf16 rounding ties (to even down and up, and just off the
# tie), +-inf, NaN, FLT_MAX and the smallest fp32 that rounds to bf16 infinity
SPECIALS = _bits([0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00400000,
                  0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0xBF808000, 0xBF818000,
                  0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001,
                  0x7F7FFFFF, 0xFF7FFFFF, 0x7F7F8000, 0xFF7F8000, 0x7F7F7FFF, 0x7F7F0000])


def _values(shape, seed):
    """Random fp32 over many binades with the special values scattered in."""
    g = torch.Generator().manual_seed(seed)
    n = 1
    for s in shape:
        n *= s
    x = torch.randn(n, generator=g) * torch.exp2(torch.randint(-20, 21, (n,), generator=g).float())
    idx = torch.randperm(n, generator=g)[:2 * SPECIALS.numel()]
    x[idx] = SPECIALS.repeat(2)[:idx.numel()]
    return x.view(shape)


def _assert_split_equal(got, want_hi, want_lo):
    """got: int16 [..., 2K] (K hi then K lo); NaN positions compared as NaN-ness."""
    k = got.shape[-1] // 2
    g = got.cpu().to(torch.int64) & 0xFFFF
    gh, gl = g[..., :k], g[..., k:]
    nan = (want_hi & 0x7FFF) > 0x7F80
    assert torch.equal((gh & 0x7FFF) > 0x7F80, nan)
    assert torch.equal(gh[~nan], want_hi[~nan])
    assert torch.equal(gl, want_lo)  # a NaN's lo is 0 too


def _pad_last(t, n):
    out = torch.zeros(*t.shape[:-1], n, dtype=t.dtype)
    out[..., :t.shape[-1]] = t
    return out


def test_split_of_special_values():
    """The rule at the edges: hi + lo is x to 16 bits, never inf - inf."""
    from distributed_learning_simulator_amd import _native
    x = SPECIALS.view(1, -1, 1, 1).contiguous()
    ys = _native.conv_pack_input(x.to(dev))
    hi, lo = split2_ref(SPECIALS)
    cp = ys.shape[-1] // 2
    _assert_split_equal(ys.view(1, 2 * cp), _pad_last(hi.view(1, -1), cp), _pad_last(lo.view(1, -1), cp))
    back = _native.split_to_f32(ys).cpu().view(-1)[:SPECIALS.numel()]
    big = SPECIALS.abs() >= _bits([0x7F7F8000])[0]  # rounds to bf16 infinity
    fin = torch.isfinite(SPECIALS)
    assert torch.equal(back[big & fin], torch.sign(SPECIALS[big & fin]) * float("inf"))  # as bf16 rounds it
    assert torch.equal(torch.isnan(back), torch.isnan(SPECIALS))
    assert float(back[SPECIALS == FLT_MAX][0]) == float("inf")


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (1, 40, 9, 3), (3, 64, 4, 4)], ids=str)
def test_pack_input_matches_format(shape):
    from distributed_learning_simulator_amd import _native
    x = _values(shape, 1)
    ys = _native.conv_pack_input(x.to(dev))
    cp = _native.split_channels(shape[1])
    assert ys.shape == (shape[0], shape[2], shape[3], 2 * cp)
    hi, lo = (_pad_last(b.permute(0, 2, 3, 1), cp) for b in split2_ref(x))
    _assert_split_equal(ys, hi, lo)
    # hi + lo reproduces x to 2^-16 |x| below the overflow boundary (0 for bf16-denormal lo halves aside)
    back = _native.split_to_f32(ys).cpu()[:, :shape[1]]
    ok = torch.isfinite(x) & (x.abs() < 3.3895e38) & (x.abs() > 2.0 ** -100)
    assert ((back - x).abs()[ok] <= x.abs()[ok] * 2.0 ** -16).all()


@pytest.mark.parametrize("shape", [(64, 40, 3, 5), (70, 3, 3, 3), (64, 64, 1, 1), (5, 40, 5, 1)], ids=str)
def test_pack_weights_matches_format(shape):
    from distributed_learning_simulator_amd import _native
    co, ci, kh, kw = shape
    w = _values(shape, 2)
    ws = _native.conv_pack_weights(w.to(dev))
    cp = _native.split_channels(ci)
    assert ws.shape == (co, 2 * kh * kw * cp)
    hi, lo = (_pad_last(b.permute(0, 2, 3, 1), cp).reshape(co, -1) for b in split2_ref(w))
    _assert_split_equal(ws, hi, lo)


@pytest.mark.parametrize("shape", [(64, 3, 3, 3), (5, 1, 5, 5), (64, 3, 1, 3), (70, 2, 3, 5)], ids=str)
def test_pack_weights_im2col_matches_format(shape):
    from distributed_learning_simulator_amd import _native
    co, ci, kh, kw = shape
    w = _values(shape, 3)
    ws = _native.conv_pack_weights_im2col(w.to(dev))
    kp = _native.split_channels(ci * kh * kw)
    assert ws.shape == (co, 2 * kp) and kp > ci * kh * kw
    hi, lo = (_pad_last(b.permute(0, 2, 3, 1).reshape(co, -1), kp) for b in split2_ref(w))
    _assert_split_equal(ws, hi, lo)


@pytest.mark.parametrize("geom", [(3, 3, 3, 1, 1, 9, 7), (3, 3, 3, 2, 1, 9, 7), (1, 5, 5, 1, 2, 7, 9),
                                  (3, 3, 3, 1, 0, 6, 5), (2, 3, 5, 2, 2, 8, 11), (40, 1, 1, 1, 0, 3, 5)], ids=str)
def test_pack_im2col_matches_format(geom):
    from distributed_learning_simulator_amd import _native
    c, kh, kw, s, p, H, W = geom
    x = _values((2, c, H, W), 4)
    x[0, 0, 0, 0] = FLT_MAX
    ys = _native.conv_pack_im2col(x.to(dev), (kh, kw), s, p)
    kp = _native.split_channels(c * kh * kw)
    ho, wo = (H + 2 * p - kh) // s + 1, (W + 2 * p - kw) // s + 1
    assert ys.shape == (2, ho, wo, 2 * kp)
    # the gather on the bits (F.unfold would turn 0 * NaN paddings into NaN): k = (ky*KW + kx)*C + ci
    hi, lo = split2_ref(x)
    cols = []
    for b in (hi, lo):
        bp = F.pad(b, (p, p, p, p))  # the split of the zero padding is (0, 0)
        taps = [bp[:, :, ky:ky + s * (ho - 1) + 1:s, kx:kx + s * (wo - 1) + 1:s]
                for ky in range(kh) for kx in range(kw)]
        cols.append(_pad_last(torch.stack(taps, 1).permute(0, 3, 4, 1, 2).reshape(2, ho, wo, -1), kp))
    _assert_split_equal(ys, cols[0], cols[1])


# ------------------------------------------------------------------ pool_linear
# (B, HW, C, O): every HW in {1, 16, 49}, C in {32, 96, 512, 2048}, O in {1, 10, 1000}, B in {1, 5}
POOL_SHAPES = [(5, 1, 32, 10), (5, 16, 512, 10), (1, 49, 96, 1000), (5, 1, 2048, 1), (1, 16, 2048, 1000),
               (5, 49, 32, 1), (1, 49, 512, 10), (5, 16, 96, 1000)]


def _pool_operands(B, HW, C, O, seed=5):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, HW, 1, generator=g)
    wt = torch.randn(O, C, generator=g) / C ** 0.5
    bias = torch.randn(O, generator=g)
    return x, wt, bias


@pytest.mark.parametrize("shape", POOL_SHAPES, ids=lambda t: "b{}_hw{}_c{}_o{}".format(*t))
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "nobias"])
def test_pool_linear_within_8x_torch_fp32_error_of_fp64(shape, with_bias):
    """The forward-error convention of tests/test_gpu_loss.py: max |kernel - fp64|
    <= 8 * max |torch CPU fp32 mean + linear - fp64| on the same (16-bit split)
    activation, both normalised by the magnitude sum."""
    from distributed_learning_simulator_amd import _native
    B, HW, C, O = shape
    x, wt, bias = _pool_operands(B, HW, C, O)
    xs = _native.conv_pack_input(x.to(dev))
    xv = _native.split_to_f32(xs).cpu()  # the activation the kernel reads: hi + lo, exact in fp32
    b = bias if with_bias else None
    got = _native.pool_linear(xs, wt.to(dev), None if b is None else b.to(dev)).cpu()
    again = _native.pool_linear(xs.clone(), wt.to(dev), None if b is None else b.to(dev)).cpu()
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))
    feat64 = xv.double().mean(dim=(2, 3))
    ref = F.linear(feat64, wt.double(), None if b is None else b.double())
    den = F.linear(xv.double().abs().mean(dim=(2, 3)), wt.double().abs()) + (0 if b is None else b.double().abs())
    t32 = F.linear(xv.mean(dim=(2, 3)), wt, b)
    err = ((got.double() - ref).abs() / den).max().item()
    err_t = ((t32.double() - ref).abs() / den).max().item()
    print(f"pool_linear B={B} HW={HW} C={C} O={O} bias={with_bias}: kernel err {err:.3e}, "
          f"torch fp32 err {err_t:.3e}, ratio {err / err_t:.2f}")
    assert err <= 8 * err_t, (shape, err, err_t)


def test_pool_linear_does_not_depend_on_the_batch_position():
    from distributed_learning_simulator_amd import _native
    x, wt, bias = _pool_operands(5, 16, 512, 10, seed=6)
    xs = _native.conv_pack_input(x.to(dev))
    whole = _native.pool_linear(xs, wt.to(dev), bias.to(dev))
    moved = _native.pool_linear(xs[[3, 0, 4]].contiguous(), wt.to(dev), bias.to(dev))
    assert torch.equal(whole[[3, 0, 4]].view(torch.int32), moved.view(torch.int32))


@pytest.mark.parametrize("HW,C,O", [(16, 512, 10), (1, 96, 1000), (4, 2048, 3)])
def test_pool_linear_exact_on_integers(HW, C, O):
    """Integer activations and weights with a power-of-two HW: every pooled
    feature is a multiple of 1 / HW and every partial sum exact, so the logits
    are the integers (or multiples of 1 / HW) of the fp64 evaluation, bit for bit."""
    from distributed_learning_simulator_amd import _native
    g = torch.Generator().manual_seed(7)
    x = torch.randint(-300, 301, (3, C, HW, 1), generator=g).float()  # non-zero lo halves
    x = x - x.sum(dim=2, keepdim=True) % HW * (torch.arange(HW).view(1, 1, HW, 1) == 0)  # pixel sums % HW == 0
    wt = torch.randint(-3, 4, (O, C), generator=g).float()
    bias = torch.randint(-9, 10, (O,), generator=g).float()
    xs = _native.conv_pack_input(x.to(dev))
    assert torch.equal(_native.split_to_f32(xs).cpu(), x)
    ref = F.linear(x.double().mean(dim=(2, 3)), wt.double(), bias.double())
    assert torch.equal(ref, ref.round()) and ref.abs().max() < 2 ** 24
    got = _native.pool_linear(xs, wt.to(dev), bias.to(dev)).cpu()
    assert torch.equal(got.double(), ref)
