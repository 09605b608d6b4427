"""numpy reference of the batched LeNet-5 evaluation (dls_lenet5_eval_f32 and
dls_lenet5_eval_loss_f32, csrc/lenet.hip), tests only.

``forward`` is the plain fp64 network with IEEE special values, ``bound`` the
derived per-logit bound a correct fp32 evaluation stays within, ``certificate``
the per-layer magnitude sums that make an integer model exact in fp32 whatever
the summation order, ``argmax_torch`` the count's argmax.  The rest builds the
models and images both test files use: ``cases()`` is every launch of
tests/test_gpu_lenet_exact.py, and tests/test_lenet_ref_host.py asserts on the
CPU what each of them claims about its inputs.  No torch, no GPU."""
import functools

import numpy as np

U_ROUND = 2.0 ** -24  # unit roundoff of fp32, round to nearest

NAMES = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "fc1.weight",
         "fc1.bias", "fc2.weight", "fc2.bias", "fc3.weight", "fc3.bias")
LAYERS = ("conv1", "conv2", "fc1", "fc2", "fc3")
K_OF = (25, 150, 400, 120, 84)  # reduction length of each layer


def shapes(O):
    return ((6, 1, 5, 5), (6,), (16, 6, 5, 5), (16,), (120, 400), (120,), (84, 120), (84,),
            (O, 84), (O,))


# ------------------------------------------------------------------ flat rows
def layout(O, order=range(10), gap=0):
    """(offsets in NAMES order, P): the ten tensors placed in ``order``, each start
    a multiple of 4 with ``gap`` unused elements in front of it."""
    offsets, at = [0] * 10, 0
    for i in order:
        at = (at + gap + 3) // 4 * 4
        offsets[i] = at
        at += int(np.prod(shapes(O)[i]))
    return offsets, (at + gap + 3) // 4 * 4


def pack(params, offsets, P, fill=0.0):
    """The fp32 row of ten tensors; elements no tensor owns hold ``fill``."""
    row = np.full(P, fill, np.float32)
    for p, o in zip(params, offsets):
        row[o:o + p.size] = np.asarray(p, np.float32).reshape(-1)
    return row


def unpack(row, offsets, O):
    """The ten tensors of a flat fp32 row, as fp64 (exact)."""
    row = np.asarray(row)
    return [row[o:o + int(np.prod(s))].astype(np.float64).reshape(s)
            for o, s in zip(offsets, shapes(O))]


# ------------------------------------------------------------------ the network
def _windows(h):  # [B, C, H, W] -> [B, C, H-4, W-4, 5, 5]
    return np.lib.stride_tricks.sliding_window_view(h, (5, 5), axis=(2, 3))


def _lin(h, w):
    """sum_k w[j, k] h[.., k] of a conv (5x5 valid) or fc layer, no bias.  einsum's
    own loops: every product is formed and added, so 0 * inf = NaN as IEEE has it."""
    with np.errstate(all="ignore"):
        if w.ndim == 4:
            return np.einsum("bcyxij,ocij->boyx", _windows(h), w)
        return np.einsum("bk,jk->bj", h, w)


def _bias(b, z):
    return b[None, :, None, None] if z.ndim == 4 else b[None, :]


def relu(z):
    """max(z, 0) that keeps NaN, as torch.relu: -inf and -0 give +0."""
    with np.errstate(invalid="ignore"):
        return np.where(z > 0, z, np.where(np.isnan(z), z, 0.0))


def _members(a):  # the four members of every 2x2 window, [4, B, C, H/2, W/2]
    return np.stack([a[:, :, dy::2, dx::2] for dy in (0, 1) for dx in (0, 1)])


def pool(a):
    """2x2 max-pool that keeps NaN, as torch.max_pool2d: a window with a NaN is NaN."""
    with np.errstate(invalid="ignore"):
        return np.maximum.reduce(_members(a))  # np.maximum propagates NaN


def _forward(params, x):
    h = np.asarray(x).astype(np.float64)
    pre, acts = [], []
    for l in range(5):
        w, b = params[2 * l], params[2 * l + 1]
        if l == 2:
            h = h.reshape(h.shape[0], -1)  # co * 25 + py * 5 + px
        acts.append(h)
        with np.errstate(all="ignore"):
            z = _lin(h, w)
            z = z + _bias(b, z)
        pre.append(z)
        if l < 4:
            h = relu(z)
            if l < 2:
                h = pool(h)
    return pre, acts


def forward(row, offsets, x, O):
    """(fp64 logits [B, O], the five layers' fp64 pre-activations) of a flat fp32
    model row on x [B, 1, 32, 32]."""
    pre, _ = _forward(unpack(row, offsets, O), x)
    return pre[4], pre


def forward_params(params, x):
    """``forward`` of ten tensors given directly."""
    pre, _ = _forward([np.asarray(p, np.float32).astype(np.float64) for p in params], x)
    return pre[4], pre


def gamma(n):
    """g(n) = n u / (1 - n u), u = 2^-24."""
    return n * U_ROUND / (1.0 - n * U_ROUND)


def bound(row, offsets, x, O):
    """The per-logit bound [B, O] on |fp32 logit - fp64 logit| for any correct fp32
    evaluation, carried through the layers.

    Derivation (nothing is measured): in a layer of reduction length K every term
    w_k h_k goes through at most one product rounding (none when fused), at most
    K - 1 additions of its chain whatever the order or the tree, the merge of two
    accumulators and the bias addition: at most K + 2 roundings, so the layer's own
    rounding error is at most g(K + 2) (sum |w| |h'| + |b|) over the inputs h' it
    actually sees (Higham, Accuracy and Stability of Numerical Algorithms, lemma
    3.1), and |h'| <= |h| + e_in with h the fp64 activation and e_in the bound on
    the input error.  The input error itself arrives as sum |w| e_in.  ReLU and max
    are 1-Lipschitz: e passes through ReLU, and a pooling window takes the largest
    e of its members.  e = 0 at the pixels.  No underflow is assumed: every
    non-zero |w h| is asserted to lie above 2^-100."""
    params = unpack(row, offsets, O)
    pre, acts = _forward(params, x)
    e = np.zeros_like(acts[0])
    for l in range(5):
        aw, ab = np.abs(params[2 * l]), np.abs(params[2 * l + 1])
        h = np.abs(acts[l])
        assert np.isfinite(h).all() and np.isfinite(aw).all() and np.isfinite(ab).all()
        if l == 2:
            e = e.reshape(e.shape[0], -1)
        if aw.any() and h.any():
            assert aw[aw > 0].min() * h[h > 0].min() > 2.0 ** -100, LAYERS[l]
        mag = _lin(h + e, aw)
        e = _lin(e, aw) + gamma(K_OF[l] + 2) * (mag + _bias(ab, mag))
        if l < 2:
            e = _members(e).max(0)
    return e


def certificate(row, offsets, x, O):
    """Per layer, max over neurons and images of sum |w| |h| + |b| (h the fp64
    input activations).  With integer weights, biases and pixels and every entry
    below 2^24, each partial sum of each neuron, in any order, fused or not, is an
    integer of magnitude below 2^24: fp32 holds them all, and the fp32 logits have
    the bits of the fp64 ones whatever an MFMA does inside."""
    return certificate_params(unpack(row, offsets, O), x)


def certificate_params(params, x):
    """``certificate`` of ten tensors.  Non-finite weights, biases and activations
    count as zero: a partial sum that is finite holds finite terms only, so the
    certificate still covers every finite intermediate of a special-value case."""
    params = [np.asarray(p, np.float32).astype(np.float64) for p in params]
    _, acts = _forward(params, x)
    fin = lambda a: np.where(np.isfinite(a), np.abs(a), 0.0)
    out = []
    for l in range(5):
        mag = _lin(fin(acts[l]), fin(params[2 * l]))
        out.append(float((mag + _bias(fin(params[2 * l + 1]), mag)).max()))
    return out


def is_integer_model(params, x):
    return all(np.array_equal(np.asarray(a, np.float64), np.rint(np.asarray(a, np.float64)))
               for a in list(params) + [x])


def argmax_torch(logits):
    """torch.argmax over the last axis: the lowest index among equal maxima, and a
    NaN counts as a maximum (the first NaN wins, also over +inf)."""
    z = np.asarray(logits)
    nan = np.isnan(z)
    finite_best = np.argmax(np.where(nan, -np.inf, z), axis=-1)  # first of equal maxima
    return np.where(nan.any(-1), np.argmax(nan, axis=-1), finite_best)


# ------------------------------------------------------------------ generators
DENSITY = (1.0, 0.5, 0.15, 0.3, 0.5)  # share of non-zero weights per layer
BIAS_MAX = (8, 64, 256, 256, 256)


def int_params(O, seed):
    """Ten integer tensors: conv1 dense in {-3..3}; the other layers non-zero with
    DENSITY, magnitudes 1, 2, 3 with probability 0.5, 0.3, 0.2 and a fair sign (so a
    swap of two weights is rarely a swap of equals); integer biases up to BIAS_MAX."""
    rng = np.random.default_rng([1005, O, seed])
    out = []
    for l in range(5):
        ws, bs = shapes(O)[2 * l], shapes(O)[2 * l + 1]
        if l == 0:
            w = rng.integers(-3, 4, size=ws)
        else:
            w = rng.choice([1, 2, 3], p=[0.5, 0.3, 0.2], size=ws) * rng.choice([-1, 1], size=ws)
            w = w * (rng.random(ws) < DENSITY[l])
        out += [w.astype(np.float32),
                rng.integers(-BIAS_MAX[l], BIAS_MAX[l] + 1, size=bs).astype(np.float32)]
    return out


def int_images(B, seed, low=0):
    """fp32 [B, 1, 32, 32] with pixels in {low..3}."""
    rng = np.random.default_rng([2005, seed])
    return rng.integers(low, 4, size=(B, 1, 32, 32)).astype(np.float32)


def labels_for(ref, seed):
    """int64 [B]: about half the images carry the first model's prediction, the
    rest a random class, so that every count is neither 0 nor B by construction."""
    rng = np.random.default_rng([3005, seed])
    B, O = ref.shape[1:]
    y = rng.integers(0, O, size=B)
    keep = rng.random(B) < 0.5
    return np.where(keep, argmax_torch(ref[0]), y).astype(np.int64)


def _copy(params):
    return [np.array(p, np.float32) for p in params]


def _with(params, i, fn):
    out = _copy(params)
    fn(out[i])
    return out


# ---- localising models: a general integer model with one layer reduced to the
# ---- part under test, so that what reaches the logits went through that part
def conv2_tap_model(k, O=32, seed=11):
    """The only non-zero conv2 weights are tap k = (ci, ky, kx), with weight co + 1
    in output channel co: another tap, or another channel, gives other logits."""
    p = _copy(int_params(O, seed))
    w = np.zeros((16, 150), np.float32)
    w[:, k] = np.arange(1, 17)
    p[2] = w.reshape(16, 6, 5, 5)
    return p


def conv1_tap_model(t, O=32, seed=12):
    """The only non-zero conv1 weights are tap t = (ky, kx), weight co + 1 in
    channel co, no conv1 bias."""
    p = _copy(int_params(O, seed))
    w = np.zeros((6, 25), np.float32)
    w[:, t] = np.arange(1, 7)
    p[0] = w.reshape(6, 1, 5, 5)
    p[1] = np.zeros(6, np.float32)
    return p


def fc_step_model(which, O=32, seed=13):
    """Dense non-zero fc weights in {-3..3} \\ {0} restricted to some k steps (a k
    step is four consecutive inputs): "tail" keeps only fc3's k = 80..83, "even" /
    "odd" the even / odd k steps of all three fc layers (the two accumulators)."""
    rng = np.random.default_rng([4005, seed])
    p = _copy(int_params(O, seed))
    for l in (2, 3, 4):
        ws = shapes(O)[2 * l]
        w = rng.choice([1, 2, 3], size=ws) * rng.choice([-1, 1], size=ws)
        step = np.arange(ws[1]) // 4
        if which == "tail":
            keep = step == 20 if l == 4 else rng.random(ws[1]) < DENSITY[l]
        else:
            keep = step % 2 == (0 if which == "even" else 1)
        p[2 * l] = (w * keep[None, :]).astype(np.float32)
    if which == "tail":  # the four inputs of the tail step are active on every image
        p[7][80:84] = 1 << 19
    return p


def inf_channel_model(O, seed=14):
    """conv1 channel 0 is +inf everywhere (its bias), every conv2 weight of ci = 0
    and every fc1 / fc2 weight strictly positive, every fc3 row of one sign: the
    logits are +-inf and nothing is NaN unless a product with a zero is formed."""
    p = _copy(int_params(O, seed))
    p[1][0] = np.inf
    p[2][:, 0] = np.abs(p[2][:, 0]) + 1
    for i in (4, 6, 8):
        p[i] = np.abs(p[i]) + 1
    p[8] *= np.where(np.arange(O) % 2 == 0, 1, -1)[:, None].astype(np.float32)
    return p


def inf_fc2_model(O, seed=15):
    """fc2 neuron 83 is +inf (its bias) and fc3's column 83 has no zero: logit o is
    sign(w[o, 83]) inf."""
    p = _copy(int_params(O, seed))
    p[7][83] = np.inf
    p[8][:, 83] = np.where(np.arange(O) % 3 == 0, -2, 3)
    return p


def neg_inf_model(O, seed=16):
    """-inf pre-activations in every hidden layer (a bias each): ReLU gives +0, the
    logits stay finite integers."""
    p = _copy(int_params(O, seed))
    for i, j in ((1, 1), (3, 3), (5, 7), (7, 9)):
        p[i][j] = -np.inf
    return p


def corner_nan_images(seed=17):
    """Four integer images with a NaN in one corner pixel each: (0, 0) reaches only
    conv1 output (0, 0), member (0, 0) of its pooling window, and through it only
    conv2 output (0, 0), member (0, 0) again; (0, 31), (31, 0), (31, 31) likewise
    reach members (0, 1), (1, 0), (1, 1) of both pools.  Image 4 is clean."""
    x = int_images(5, seed)
    for b, (r, c) in enumerate(((0, 0), (0, 31), (31, 0), (31, 31))):
        x[b, 0, r, c] = np.nan
    return x


def subnormal_models(O=4):
    """Pixels of 2^-130 (``subnormal_images``) through unit weights, no bias:
    "sub": one unit tap per neuron everywhere, so every activation and the logits
           are the subnormal 2^-130;
    "sum": as "sub" with all 150 conv2 taps 1: subnormal inputs, normal sums;
    "fc":  conv1 tap 16 (activations 2^-126, normal) and fc1 weights 2^-4: the
           first subnormal is fc1's output, fc2 and fc3 read it;
    "ctl": conv1 tap 16 and unit taps: normal throughout."""
    def unit(conv1, conv2_all, fc1):
        p = [np.zeros(s, np.float32) for s in shapes(O)]
        p[0][:, 0, 2, 2] = conv1
        if conv2_all:
            p[2][:] = 1
        else:
            p[2][:, 0, 2, 2] = 1
        for i, v in ((4, fc1), (6, 1), (8, 1)):
            p[i][np.arange(p[i].shape[0]), np.arange(p[i].shape[0]) % 16] = v
        return p
    return {"sub": unit(1, False, 1), "sum": unit(1, True, 1), "fc": unit(16, False, 2.0 ** -4),
            "ctl": unit(16, False, 1)}


def subnormal_images(B=3):
    return np.full((B, 1, 32, 32), 2.0 ** -130, np.float32)


ARGMAX_ROWS = {  # fc3 biases of models whose fc3 weights are zero: the logits themselves
    "tie": [1, 5, 2, 5, 0, 5, -3, 4],
    "zeros": [-1, -0.0, 0.0, -0.0, 0.0, -2, -0.0, -5],
    "neg_inf": [-np.inf] * 8,
    "nan_first": [np.nan, 7, 1, 2, 9, 0, 3, 4],
    "nan_later": [1, 7, np.nan, 2, 9, 0, 3, 4],
    "two_nans": [1, 2, np.nan, 3, np.nan, 99, np.inf, 0],
    "inf_then_nan": [np.inf, 2, 1, np.nan, 0, 0, 0, 0],
}


# class i is asked for by i + 1 of the 36 images, so the count names the index the
# kernel picked: no two picks count the same
ARGMAX_LABELS = np.repeat(np.arange(8), np.arange(1, 9)).astype(np.int64)


def argmax_model(name, seed=18):
    p = _copy(int_params(8, seed))
    p[8][:] = 0
    p[9] = np.array(ARGMAX_ROWS[name], np.float32)
    return p


# ------------------------------------------------------------------ the launches
GENERAL = ([(2, B, 32) for B in (1, 15, 16, 17, 33, 48)]            # every batch edge
           + [(S, 33, 10) for S in (1, 2, 5)]                        # rows at ldm > P
           # every fc3 tile edge; five models where one or two logits per image would
           # leave the share of positive logits to two coin tosses
           + [(5 if O <= 2 else 2, 33, O) for O in (1, 2, 10, 15, 16, 17, 31, 32)]
           + [(2, 17, 10), (2, 17, 7)])                              # layout, sentinels


def general_case(S, B, O):
    seed = 100 * S + O
    return [int_params(O, seed + s) for s in range(S)], int_images(48, O)[:B]


SPECIAL_NAMES = tuple(
    [f"pixel-{t}-B{B}" for t in ("nan",) for B in (32, 21)] + ["weight-nan"]
    + [f"pixel-{t}-B{B}" for t in ("inf",) for B in (32, 21)] + ["weight-inf"]
    + [f"inf-weight-ragged-{t}" for t in ("conv1", "fc1", "fc3")]
    + [f"inf-conv1-channel-O{O}" for O in (10, 32)] + [f"inf-fc2-O{O}" for O in (7, 17)]
    + ["neg-inf-preactivations", "nan-corners", "argmax-a", "argmax-b"])
# every case by name, without building a model (the test files parametrise over it)
CASE_NAMES = tuple(
    list(dict.fromkeys(f"general-S{S}-B{B}-O{O}" for S, B, O in GENERAL))
    + [f"conv2-taps-{5 * g}" for g in range(30)] + [f"conv1-taps-{5 * g}" for g in range(5)]
    + [f"fc-steps-O{O}" for O in (32, 17)]
    + ["pixel-clean-B32", "pixel-clean-B21", "weight-clean"] + list(SPECIAL_NAMES))


@functools.lru_cache(maxsize=None)
def cases():
    """{name: (kind, [ten tensors per model], x, O)} of every launch of
    tests/test_gpu_lenet_exact.py.  kind "general": random integer models under
    all four conditions of the host file; "local" / "special": built for one
    purpose, exact (certificate) wherever finite."""
    out = {}
    for S, B, O in GENERAL:
        out[f"general-S{S}-B{B}-O{O}"] = ("general",) + tuple(general_case(S, B, O)) + (O,)
    x = int_images(3, 21)
    for g in range(30):
        out[f"conv2-taps-{5 * g}"] = ("local", [conv2_tap_model(k) for k in range(5 * g, 5 * g + 5)],
                                      x, 32)
    for g in range(5):
        out[f"conv1-taps-{5 * g}"] = ("local", [conv1_tap_model(t) for t in range(5 * g, 5 * g + 5)],
                                      x, 32)
    for O in (32, 17):
        out[f"fc-steps-O{O}"] = ("local", [fc_step_model(w, O) for w in ("tail", "even", "odd")],
                                 int_images(17, 22), O)
    # ---- special values
    base = [int_params(10, 31 + s) for s in range(3)]
    for B in (32, 21):  # the launches the poisoned ones are compared with
        out[f"pixel-clean-B{B}"] = ("local", base[:2], int_images(B, 23), 10)
    out["weight-clean"] = ("local", base, int_images(33, 24), 10)
    for tag, v in (("nan", np.nan), ("inf", np.inf)):
        for B, b in ((32, 5), (21, 18)):  # a full tile; the ragged last tile
            xs = int_images(B, 23)
            xs[b, 0, 9, 13] = v
            out[f"pixel-{tag}-B{B}"] = ("special", base[:2], xs, 10)
        out[f"weight-{tag}"] = ("special", [base[0], _with(base[1], 4, lambda w: w.__setitem__((5, 7), v)),
                                            base[2]], int_images(33, 24), 10)
    for tag, i, at in (("conv1", 0, (2, 0, 1, 3)), ("fc1", 4, (3, 4)), ("fc3", 8, (3, 5))):
        out[f"inf-weight-ragged-{tag}"] = (
            "special", [_with(base[0], i, lambda w: w.__setitem__(at, np.inf)), base[1]],
            int_images(17, 25, low=1), 10)
    for O in (10, 32):
        out[f"inf-conv1-channel-O{O}"] = ("special", [inf_channel_model(O)], int_images(17, 26), O)
    for O in (7, 17):
        out[f"inf-fc2-O{O}"] = ("special", [inf_fc2_model(O), int_params(O, 41)], int_images(17, 27), O)
    out["neg-inf-preactivations"] = ("special", [neg_inf_model(10), base[0]], int_images(17, 28), 10)
    out["nan-corners"] = ("special", base[:2], corner_nan_images(), 10)
    names = list(ARGMAX_ROWS)
    xa = int_images(len(ARGMAX_LABELS), 29)
    out["argmax-a"] = ("special", [argmax_model(n) for n in names[:4]], xa, 8)
    out["argmax-b"] = ("special", [argmax_model(n) for n in names[4:]], xa, 8)
    assert tuple(out) == CASE_NAMES
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """(ref fp64 [S, B, O], pre-activations per model, labels int64 [B]) of a case."""
    _, models, x, O = cases()[name]
    res = [forward_params(p, x) for p in models]
    ref = np.stack([r[0] for r in res])
    if name.startswith("argmax"):
        labels = ARGMAX_LABELS
    elif name in ("weight-nan", "weight-inf"):
        labels = reference("weight-clean")[2]  # the other models' counts are compared
    else:
        labels = labels_for(ref, len(name))
    return ref, [r[1] for r in res], labels
