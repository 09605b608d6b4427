"""Exact-value tests of every convolution kernel the dispatcher can pick
(csrc/conv.hip; the ids of _native.conv_kernel_choice).

Operands are chosen so that the required output is one set of bits: every
partial sum of the bf16x3 products is an integer below 2^24 in magnitude (fp32
accumulation is exact in any order) and every result an integer below 2^16 (it
survives the output's 16-bit hi + lo split).  The reference is computed on the
CPU in fp64 from a CPU emulation of the split (hi = rne_bf16(x), lo =
rne_bf16(x - hi)): conv(xh, wh) + conv(xh, wl) + conv(xl, wh) — no lo * lo term,
as bf16x3 has none — then the epilogue, then the emulated split, and compared
with torch.equal on the 16-bit images.  Both magnitude preconditions are
asserted on the reference itself.

CASES is importable without a GPU: tests/test_conv_dispatch_host.py asserts that
it reaches every kernel id the dispatcher can return.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
dev = torch.device("cuda", 0)


# ------------------------------------------------------- CPU emulation of split2
def bf16_rne_bits(x):
    """fp32 tensor -> the bf16 bits (int64 in 0..0xffff) of round-to-nearest-even;
    a NaN stays a quiet NaN (csrc/conv.hip bf16_rne)."""
    u = x.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return torch.where(nan, (u >> 16) | 0x40, r)


def bits_to_f32(b):
    return (b.to(torch.int32) << 16).view(torch.float32)


def split2_ref(x):
    """(hi bits, lo bits) of the documented split: hi = rne_bf16(x), lo =
    rne_bf16(x - hi), lo = 0 whenever hi is not finite (include/dls_hip.h)."""
    x = x.float()
    hi = bf16_rne_bits(x)
    lo = bf16_rne_bits(x - bits_to_f32(hi))
    lo = torch.where((hi & 0x7F80) == 0x7F80, torch.zeros_like(lo), lo)
    return hi, lo


def _i16(b):
    return ((b + 0x8000) % 0x10000 - 0x8000).to(torch.int16)


def split_nhwc_ref(x):
    """fp32 NCHW -> the split NHWC int16 image [B, H, W, 2C] (no channel padding)."""
    hi, lo = split2_ref(x)
    return _i16(torch.cat([hi.permute(0, 2, 3, 1), lo.permute(0, 2, 3, 1)], dim=3)).contiguous()


def split_weights_ref(w, cp=None):
    """fp32 [Cout, Cin, KH, KW] -> split weights [Cout, 2K], k = (ky*KW + kx)*Cp + ci."""
    co, ci, kh, kw = w.shape
    cp = cp or ci
    wp = torch.zeros(co, kh, kw, cp)
    wp[..., :ci] = w.permute(0, 2, 3, 1)
    hi, lo = split2_ref(wp.reshape(co, -1))
    return _i16(torch.cat([hi, lo], dim=1)).contiguous()


def nan_mask_of_split(ys):
    """NaN-ness of a split NHWC image's hi halves."""
    c = ys.shape[-1] // 2
    hi = ys[..., :c].to(torch.int64) & 0xFFFF
    return (hi & 0x7FFF) > 0x7F80


# -------------------------------------------------------------------- the cases
# (cin, cout, kh, kw, stride, pad, H, W, B); the kernel each runs on is what
# _native.conv_kernel_choice returns (tests/test_conv_dispatch_host.py pins the
# union).  The smallest shapes that exercise each form.
CASES = [
    # LDS-DMA pipeline, 64-channel blocks: 4 whole 8x8 images per tile with B = 3
    # (M = 192 < 256), a 32x32 image (4 row tiles), Cout = 192 with M % 256 != 0
    (32, 64, 3, 3, 1, 1, 8, 8, 3), (32, 64, 3, 3, 1, 1, 32, 32, 1), (64, 192, 3, 3, 1, 1, 8, 8, 5),
    # 16-wide 128-multiples in 64-channel blocks: whole 16x16 images, and the
    # 12-DMA form (4x16: 4 images per tile, B = 3)
    (64, 128, 3, 3, 1, 1, 16, 16, 2), (32, 128, 3, 3, 1, 1, 4, 16, 3),
    # 128-channel 4-wave blocks (24x16, 3 row tiles per image, an odd chunk count)
    (96, 128, 3, 3, 1, 1, 24, 16, 1),
    # 128-channel 8-wave blocks: 8x8 (TI = 4, B = 3) and 4x4 (TI = 16: M = 80 and M = 48 < 64)
    (32, 128, 3, 3, 1, 1, 8, 8, 3), (64, 128, 3, 3, 1, 1, 4, 4, 5), (32, 256, 3, 3, 1, 1, 4, 4, 3),
    # register-staged halo kernel: 64x64 (row tiles), 12x32 (the pipelines refuse
    # H % TR), 2x32 (TI = 2, B = 3); skewed rows: 2x16 (TI = 4, B = 5), 4x8
    (32, 128, 3, 3, 1, 1, 64, 64, 1), (32, 128, 3, 3, 1, 1, 12, 32, 2), (64, 128, 3, 3, 1, 1, 2, 32, 3),
    (32, 128, 3, 3, 1, 1, 2, 16, 5), (96, 128, 3, 3, 1, 1, 4, 8, 3),
    # stride-2 phase pipeline (whole images, B not a multiple of TI; row tiles) and
    # its refusals: a 6-wide output, odd H and W (7x7, 15x9), Cout = 64
    (32, 128, 3, 3, 2, 1, 8, 8, 5), (64, 128, 3, 3, 2, 1, 16, 32, 3), (32, 128, 3, 3, 2, 1, 12, 12, 2),
    (32, 128, 3, 3, 2, 1, 7, 7, 3), (32, 64, 3, 3, 2, 1, 15, 9, 2), (32, 64, 3, 3, 2, 1, 8, 8, 2),
    # generic kernel off the ResNet path: 3x3 pad 0, 1x1 pad 1, 5x5 pad 2, 7x7
    # stride 2 pad 3 (where (H + 2 pad - K) % stride != 0), 1x3 and 3x1, stride 3,
    # 12x32 with 64 channels, Cout = 192, 1x1 stride 2
    (32, 64, 3, 3, 1, 0, 9, 9, 2), (32, 64, 1, 1, 1, 1, 6, 6, 2), (32, 64, 5, 5, 1, 2, 10, 10, 2),
    (32, 128, 7, 7, 2, 3, 10, 12, 2), (64, 64, 1, 3, 1, 1, 5, 8, 2), (32, 128, 3, 1, 1, 0, 8, 5, 2),
    (32, 64, 3, 3, 3, 1, 10, 11, 2), (32, 64, 3, 3, 1, 1, 12, 32, 1), (32, 192, 1, 1, 1, 0, 8, 8, 3),
    (96, 128, 1, 1, 2, 0, 8, 8, 3),
]

# (C, Cout, kh, kw, stride, pad, H, W, B) of the few-channel first layer: the
# window form with an odd pixel-tile count (B = 3, 8x32: 3 tiles of 256) and one
# partial tile; 12x32 (H % 8 != 0: the non-window 3x3 form); 1-channel 5x5;
# stride 2; Cout = 192
STEM_CASES = [
    (3, 64, 3, 3, 1, 1, 8, 32, 3), (3, 64, 3, 3, 1, 1, 8, 32, 1), (3, 64, 3, 3, 1, 1, 12, 32, 2),
    (1, 64, 5, 5, 1, 2, 12, 12, 2), (3, 128, 3, 3, 2, 1, 16, 16, 2), (3, 192, 3, 3, 1, 1, 8, 32, 2),
]

EPILOGUES = [(bn, res, relu) for bn in (0, 1) for res in (0, 1) for relu in (0, 1)]


def case_id(t):
    return "c{}-{}k{}x{}s{}p{}_{}x{}_b{}".format(*t)


def _out_hw(case):
    _, _, kh, kw, s, p, H, W, _ = case
    return (H + 2 * p - kh) // s + 1, (W + 2 * p - kw) // s + 1


def _gen(case, salt):
    return torch.Generator().manual_seed(1000 * salt + sum((i + 1) * v for i, v in enumerate(case)) % 997)


# --------------------------------------------------------------- the reference
def conv_ref(x, w, case):
    """The bf16x3 convolution of fp32 NCHW x and OIHW w in fp64 from the emulated
    split operands, with the exact-accumulation precondition asserted."""
    _, _, _, _, s, p, _, _, _ = case
    xh, xl = (bits_to_f32(b).double() for b in split2_ref(x))
    wh, wl = (bits_to_f32(b).double() for b in split2_ref(w))
    ref = F.conv2d(xh, wh + wl, stride=s, padding=p) + F.conv2d(xl, wh, stride=s, padding=p)
    mag = (F.conv2d(xh.abs(), wh.abs() + wl.abs(), stride=s, padding=p)
           + F.conv2d(xl.abs(), wh.abs(), stride=s, padding=p))
    assert torch.equal(ref, ref.round()) and mag.max() < 2 ** 24, "partial sums must be integers < 2^24"
    return ref


def epilogue_ref(v, consts, res, relu):
    """fma(w, (v - mean) * iv, b) + residual, ReLU on integers (each step exact)."""
    if consts is not None:
        c = consts.double().view(4, 1, -1, 1, 1)
        v = c[2] * ((v - c[0]) * c[1]) + c[3]
    if res is not None:
        v = v + res.double()
    if relu:
        v = v.clamp_min(0)
    return v


def expect_split(v):
    """The unique output bits of an integer result below 2^16."""
    assert torch.equal(v, v.round()) and v.abs().max() < 2 ** 16, "results must be integers < 2^16"
    return split_nhwc_ref((v + 0.0).float())  # a zero result is +0, as the fp32 sum of its terms is


def int_consts(cout, g):
    """Eval batch-norm constants [mean | iv | w | b] with integer mean, w, b and
    iv in {1, 2}: exact arithmetic, a different value per channel."""
    mean = torch.randint(-4, 5, (cout,), generator=g)
    iv = torch.randint(1, 3, (cout,), generator=g)
    w = torch.randint(-2, 3, (cout,), generator=g)
    w[w == 0] = 1
    b = torch.randint(-9, 10, (cout,), generator=g)
    return torch.cat([mean, iv, w, b]).float()


def launch(case, x, w, consts=None, res=None, relu=False):
    """conv_bn_act on CPU-built split operands (independent of the pack kernels)."""
    from distributed_learning_simulator_amd import _native
    _, _, kh, kw, s, p, _, _, _ = case
    ys = _native.conv_bn_act(split_nhwc_ref(x).to(dev), split_weights_ref(w).to(dev), (kh, kw), s, p,
                             None if consts is None else consts.to(dev),
                             None if res is None else split_nhwc_ref(res).to(dev), relu=relu)
    return ys.cpu()


# ------------------------------------------------------------- operand classes
def dense_operands(case, nonzero_w=False):
    cin, cout, kh, kw, _, _, H, W, B = case
    g = _gen(case, 1)
    x = torch.randint(-3, 4, (B, cin, H, W), generator=g).float()
    w = torch.randint(-2, 3, (cout, cin, kh, kw), generator=g).float()
    if nonzero_w:
        w[w == 0] = 1.0
    return x, w, g


def select_weights(cout, cin, kh, kw):
    """One or two entries of +-1 per output channel at (tap, ci) positions that walk
    every tap, both 16-channel k-steps of a chunk and every chunk."""
    taps = kh * kw
    w = torch.zeros(cout, cin, taps)
    seen = set()
    for co in range(cout):
        picks = [(co % taps, (13 * co + 7 * (co // taps)) % cin)]
        if co % 2:
            second = ((3 * co + 1) % taps, (11 * co + 16) % cin)
            if second != picks[0]:
                picks.append(second)
        for n, (tap, ci) in enumerate(picks):
            w[co, ci, tap] = -1.0 if (co + n) % 3 == 0 else 1.0
            seen.add((tap, (ci % 32) // 16, ci // 32))
    return w.view(cout, cin, kh, kw), seen


def impulse_positions(n, k, b, B):
    """Coordinates at least k + 1 apart along a side of length n: from 0 with the far
    edge forced in on the first and last image, shifted by the image index on the
    others (so every row / column phase of a pixel tile is hit on some image)."""
    step = k + 1
    if 0 < b < B - 1:
        return list(range(b % step, n, step))
    pos = list(range(0, n, step))
    if pos[-1] != n - 1:
        if n - 1 - pos[-1] < k and len(pos) > 1:
            pos.pop()
        if n - 1 - pos[-1] >= k:
            pos.append(n - 1)
        elif b == B - 1 and B > 1:  # a side shorter than the kernel: the far edge on the last image
            pos = [n - 1]
    return pos


def impulse_input(case, g):
    cin, _, kh, kw, _, _, H, W, B = case
    x = torch.zeros(B, cin, H, W)
    for b in range(B):
        for iy in impulse_positions(H, kh, b, B):
            for ix in impulse_positions(W, kw, b, B):
                ci = int(torch.randint(0, cin, (1,), generator=g))
                x[b, ci, iy, ix] = 1.0 if (iy + ix + b) % 2 else -1.0
    return x


# ------------------------------------------------------------------- the tests
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_dense_integers_every_epilogue(case):
    """Class 1 (hi * hi; every tap, channel and pixel index): dense small integers
    through all eight (batch norm, residual, ReLU) epilogues."""
    cin, cout, *_ = case
    x, w, g = dense_operands(case)
    ho, wo = _out_hw(case)
    consts = int_consts(cout, g)
    res = torch.randint(-300, 301, (x.shape[0], cout, ho, wo), generator=g).float()  # non-zero lo halves
    v = conv_ref(x, w, case)
    for bn, rs, relu in EPILOGUES:
        c, r = (consts if bn else None), (res if rs else None)
        want = expect_split(epilogue_ref(v, c, r, relu))
        got = launch(case, x, w, c, r, relu)
        assert torch.equal(got, want), (bn, rs, relu, int((got != want).sum()))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_activation_lo_selection(case):
    """Class 2 (hi_w * lo_x): x = 1024 a + b carries a non-zero lo half; each output
    channel selects one or two of them with +-1 weights."""
    cin, cout, kh, kw, _, _, H, W, B = case
    g = _gen(case, 2)
    a = torch.randint(0, 2, (B, cin, H, W), generator=g) * 2 - 1
    b = torch.randint(-3, 4, (B, cin, H, W), generator=g)
    x = (1024 * a + b).float()
    _, lo = split2_ref(x)
    assert ((lo != 0) == (b != 0)).all() and (lo != 0).any()
    w, seen = select_weights(cout, cin, kh, kw)
    assert {t for t, _, _ in seen} == set(range(kh * kw))
    assert {s for _, s, _ in seen} == {0, 1} and {c for _, _, c in seen} == set(range(cin // 32))
    want = expect_split(conv_ref(x, w, case))
    got = launch(case, x, w)
    assert torch.equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_impulse_response(case):
    """Class 3 (lo_w * hi_x and the zero padding): isolated +-1 impulses on the
    corners and edges of the first and last image return +-w at the shifted
    positions and exact +0 everywhere else."""
    cin, cout, kh, kw, s, p, H, W, B = case
    g = _gen(case, 3)
    a = torch.randint(0, 2, (cout, cin, kh, kw), generator=g) * 2 - 1
    b = torch.randint(-3, 4, (cout, cin, kh, kw), generator=g)
    w = (1024 * a + b).float()
    assert (split2_ref(w)[1] != 0).any()
    x = impulse_input(case, g)
    assert x[0, :, 0, 0].abs().sum() == 1 and x[B - 1].abs().sum() > 0
    seen = F.conv2d(x.abs().sum(1, keepdim=True), torch.ones(1, 1, kh, kw), stride=s, padding=p)
    assert seen.max() == 1, "no output may see two impulses"
    ref = conv_ref(x, w, case)
    want = expect_split(ref)
    got = launch(case, x, w)
    assert torch.equal(got, want), int((got != want).sum())
    if (seen == 0).any():
        zero = (seen == 0).permute(0, 2, 3, 1).expand(-1, -1, -1, 2 * cout)
        assert (got[zero] == 0).all()  # +0: hi and lo bits all clear


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_nan_containment(case):
    """Class 4: one NaN in x makes NaN exactly the outputs whose receptive field
    holds it; every other output keeps the bits of the NaN-free run."""
    cin, cout, kh, kw, s, p, H, W, B = case
    x, w, g = dense_operands(case, nonzero_w=True)
    clean = launch(case, x, w)
    assert torch.equal(clean, expect_split(conv_ref(x, w, case)))
    bi, ci = B - 1, int(torch.randint(0, cin, (1,), generator=g))
    for iy, ix in ((H // 2, W - 1), (H // 2, W - 2), (0, 0)):  # the first an output reads (strides skip some)
        hit = torch.zeros(B, 1, H, W)
        hit[bi, 0, iy, ix] = 1.0
        hit = F.conv2d(hit, torch.ones(1, 1, kh, kw), stride=s, padding=p) > 0
        if hit.any():
            break
    assert hit.any() and not hit.all()
    xn = x.clone()
    xn[bi, ci, iy, ix] = float("nan")
    got = launch(case, xn, w)
    nan = nan_mask_of_split(got)
    assert torch.equal(nan, hit.permute(0, 2, 3, 1).expand(-1, -1, -1, cout))
    keep = ~torch.cat([nan, nan], dim=3)
    assert torch.equal(got[keep], clean[keep])
    assert (got[..., cout:][nan] == 0).all()  # a NaN's lo half is 0


def test_empty_batch_launches_nothing():
    """B = 0 is DLS_OK with no launch: the output (a canary here) is not touched.
    (An empty torch tensor has a null data pointer, which the library refuses, so
    the call goes to the C entry points with a live buffer and B = 0.)"""
    from distributed_learning_simulator_amd import _native
    L = _native.lib()
    assert _native.conv_kernel_choice(0, 8, 8, 32, 64, (3, 3), 1, 1) == 0
    x = torch.zeros(1, 8, 8, 64, dtype=torch.int16, device=dev)
    w = split_weights_ref(torch.ones(64, 32, 3, 3)).to(dev)
    y = torch.full((1, 8, 8, 128), 0x5A5A, dtype=torch.int16, device=dev)
    st = _native._stream(None, x)
    assert L.dls_conv_bn_act_split(_native._ptr(x), 0, 8, 8, 32, _native._ptr(w), 64, 3, 3, 1, 1, None, None, 1,
                                   _native._ptr(y), st) == 0
    xs = torch.zeros(1, 3, 8, 32, device=dev)
    ws = _native.conv_pack_weights_im2col(torch.ones(64, 3, 3, 3, device=dev))
    assert _native.conv_stem_kernel_choice(0, 3, 8, 32, 64, (3, 3), 1, 1) == 0
    assert L.dls_conv_stem_bn_act_f32(_native._ptr(xs), 0, 3, 8, 32, _native._ptr(ws), 64, 3, 3, 1, 1, None, 1,
                                      _native._ptr(y), st) == 0
    torch.cuda.synchronize()
    assert (y == 0x5A5A).all()


# -------------------------------------------------------------------- the stem
def _stem_both(case, x, w, consts, relu):
    """The im2col + 1x1 convolution and the fused stem kernel on the same operands."""
    from distributed_learning_simulator_amd import _native
    _, _, kh, kw, s, p, _, _, _ = case
    xd, wd = x.to(dev), w.to(dev)
    c = None if consts is None else consts.to(dev)
    ws = _native.conv_pack_weights_im2col(wd)
    a = _native.conv_bn_act(_native.conv_pack_im2col(xd, (kh, kw), s, p), ws, (1, 1), 1, 0, c, None, relu=relu)
    b = _native.conv_stem_bn_act(xd, ws, (kh, kw), s, p, c, relu=relu)
    return a.cpu(), b.cpu()


@functools.lru_cache(maxsize=None)
def _stem_operands(case, cls):
    cin, cout, kh, kw, s, p, H, W, B = case
    g = _gen(case, 10 + cls)
    if cls == 1:
        x = torch.randint(-3, 4, (B, cin, H, W), generator=g).float()
        w = torch.randint(-2, 3, (cout, cin, kh, kw), generator=g).float()
    elif cls == 2:
        x = (1024 * (torch.randint(0, 2, (B, cin, H, W), generator=g) * 2 - 1)
             + torch.randint(-3, 4, (B, cin, H, W), generator=g)).float()
        w = torch.zeros(cout, cin * kh * kw)
        for co in range(cout):
            w[co, co % (cin * kh * kw)] = -1.0 if co % 3 == 0 else 1.0
        assert (w != 0).any(0).all()  # every (channel, tap) selected
        w = w.view(cout, cin, kh, kw)
    else:
        w = (1024 * (torch.randint(0, 2, (cout, cin, kh, kw), generator=g) * 2 - 1)
             + torch.randint(-3, 4, (cout, cin, kh, kw), generator=g)).float()
        x = impulse_input(case, g)
    return x, w, conv_ref(x, w, case)


@pytest.mark.parametrize("cls", [1, 2, 3], ids=["dense", "lo_x", "impulse"])
@pytest.mark.parametrize("case", STEM_CASES, ids=case_id)
def test_stem_exact(case, cls):
    """The few-channel first layer, as im2col + 1x1 convolution and as the fused
    stem kernel: both exact, hence equal; with and without batch norm and ReLU."""
    cout = case[1]
    x, w, v = _stem_operands(case, cls)
    consts = int_consts(cout, _gen(case, 20))
    for c, relu in ((None, False), (consts, True), (consts, False), (None, True)) if cls == 1 else ((None, False),):
        want = expect_split(epilogue_ref(v, c, None, relu))
        a, b = _stem_both(case, x, w, c, relu)
        assert torch.equal(a, want), ("im2col", relu, int((a != want).sum()))
        assert torch.equal(b, want), ("stem", relu, int((b != want).sum()))


@pytest.mark.parametrize("case", STEM_CASES, ids=case_id)
def test_stem_nan_containment(case):
    cin, cout, kh, kw, s, p, H, W, B = case
    x, w, _ = _stem_operands(case, 1)
    w = torch.where(w == 0, torch.ones_like(w), w)
    clean_a, clean_b = _stem_both(case, x, w, None, False)
    assert torch.equal(clean_a, clean_b)
    xn = x.clone()
    xn[B - 1, cin - 1, H // 2, W - 1] = float("nan")
    hit = torch.zeros(B, 1, H, W)
    hit[B - 1, 0, H // 2, W - 1] = 1.0
    hit = (F.conv2d(hit, torch.ones(1, 1, kh, kw), stride=s, padding=p) > 0).permute(0, 2, 3, 1)
    for got, clean in zip(_stem_both(case, xn, w, None, False), (clean_a, clean_b)):
        nan = nan_mask_of_split(got)
        assert torch.equal(nan, hit.expand(-1, -1, -1, cout))
        keep = ~torch.cat([nan, nan], dim=3)
        assert torch.equal(got[keep], clean[keep])
