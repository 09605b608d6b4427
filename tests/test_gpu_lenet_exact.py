"""dls_lenet5_eval_f32 / dls_lenet5_eval_loss_f32 (csrc/lenet.hip) against the fp64
reference of tests/lenet_ref.py, every logit of every launch compared.

Integer models whose certificate (tests/test_lenet_ref_host.py) makes every fp32
partial sum exact in any order are compared bit for bit, special values by NaN
mask and bits, real weights against the derived per-logit bound; the correct
count is the reference's argmax count.  Each launch is at most 5 models x 48
images (64 for the real weights)."""
import numpy as np
import pytest
import torch

from tests import lenet_ref as R

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)
NAN = float("nan")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _launch(rows, offsets, x, O, labels, how="plain", loss=False):
    """(logits fp32 [S, B, O], correct int64 [S]) as numpy.  how: "plain" contiguous
    rows; "pitch" rows at ldm > P with NaN in the padding and a NaN row between
    any two models; "sentinel" logits inside a larger buffer that must stay as it
    was around [S, B, O]."""
    from distributed_learning_simulator_amd import _native
    S, P = rows.shape
    B = x.shape[0]
    if how == "pitch":
        M = torch.full((2 * S, P + 68), NAN, device=dev)
        M[::2, :P] = torch.from_numpy(rows).to(dev)
        models = M[::2]
        assert S == 1 or models.stride(0) == 2 * (P + 68)
    else:
        models = torch.from_numpy(rows).to(dev)
    n = S * B * O
    buf = torch.full((64 + n + 64,), 123.0, device=dev)
    logits = buf[64:64 + n].view(S, B, O)
    correct = torch.zeros(S, dtype=torch.int64, device=dev)
    lossbuf = torch.empty((S, B), device=dev) if loss else None
    _native.lenet5_eval(models, offsets, torch.from_numpy(x).to(dev),
                        labels=torch.from_numpy(labels).to(dev), logits=logits, correct=correct,
                        loss=lossbuf)
    torch.cuda.synchronize()
    assert bool((buf[:64] == 123.0).all()) and bool((buf[64 + n:] == 123.0).all()), how
    return logits.cpu().numpy(), correct.cpu().numpy()


def _explain(pre, b, bad_o, O):
    """A hint at the layer behind a difference on image b, from the reference alone
    (the kernel's own intermediates never leave the chip): the first layer whose
    fp64 pre-activations are non-finite on that image, else fc3 when only some of
    the image's logits differ, else "fc2 or earlier".  The localising cases (one
    tap, one k step) narrow a finite difference further by which of them fail."""
    for l in range(5):
        if not np.isfinite(pre[l][b]).all():
            return f"{R.LAYERS[l]} is the first layer with a non-finite fp64 pre-activation on this image"
    if len(bad_o) < O:
        return f"fc3: only logits {bad_o} of the image differ, and every earlier value feeds all {O}"
    near = [R.LAYERS[l] for l in range(4) if (pre[l][b] == 0).any()]
    return f"all {O} logits of the image differ: fc2 or earlier (layers with a zero pre-activation: {near})"


def _assert_same(got, ref, pres, what):
    """NaN masks equal, every other logit the reference's bits; on failure the first
    differing (model, image, logit) and _explain's hint at the layer."""
    want = ref.astype(np.float32)
    bad = (np.isnan(got) != np.isnan(want)) | (~np.isnan(want) & (_bits(got) != _bits(want)))
    if bad.any():
        s, b, o = (int(i) for i in np.argwhere(bad)[0])
        bad_o = np.flatnonzero(bad[s, b]).tolist()
        pytest.fail(f"{what}: {int(bad.sum())} of {bad.size} logits differ; first at (model {s}, image "
                    f"{b}, logit {o}): kernel {got[s, b, o]!r}, reference {want[s, b, o]!r}; "
                    f"{_explain(pres[s], b, bad_o, ref.shape[2])}")


def _run(name, how="plain", entries=(False, True), offsets=None, P=None, fill=0.0):
    """Launch a case of lenet_ref.cases() through both entry points and compare all
    S * B * O logits and the S counts with the reference."""
    _, models, x, O = R.cases()[name]
    ref, pres, labels = R.reference(name)
    if offsets is None:
        offsets, P = R.layout(O)
    rows = np.stack([R.pack(p, offsets, P, fill) for p in models])
    want_correct = (R.argmax_torch(ref) == labels).sum(-1)
    out = None
    for loss in entries:
        got, correct = _launch(rows, offsets, x, O, labels, how, loss)
        what = f"{name} ({how}, {'loss' if loss else 'plain'} entry)"
        _assert_same(got, ref, pres, what)
        assert np.array_equal(correct, want_correct), (what, correct, want_correct)
        out = (got, correct)
    return out


def _general(S, B, O):
    return f"general-S{S}-B{B}-O{O}"


@pytest.mark.parametrize("B", [1, 15, 16, 17, 33, 48])
def test_exact_at_every_batch_edge(B):
    _run(_general(2, B, 32))


@pytest.mark.parametrize("S", [1, 2, 5])
def test_exact_rows_at_a_pitch_with_nan_padding_and_nan_rows_between(S):
    _run(_general(S, 33, 10), how="pitch")


@pytest.mark.parametrize("O", [1, 2, 10, 15, 16, 17, 31, 32])
def test_exact_at_every_output_count(O):
    _run(_general(5 if O <= 2 else 2, 33, O))


def test_exact_with_permuted_offsets_and_nan_gaps():
    offsets, P = R.layout(10, order=(7, 2, 9, 0, 5, 4, 1, 8, 3, 6), gap=12)
    _run(_general(2, 17, 10), offsets=offsets, P=P, fill=NAN)
    _run(_general(2, 17, 10), how="pitch", offsets=offsets, P=P, fill=NAN)


def test_exact_logits_inside_a_larger_buffer():
    """Every _launch writes into a slice with 64 sentinels on either side; this is
    the ragged O = 7, B = 17 shape, whose last rows end off any 16-byte boundary."""
    _run(_general(2, 17, 7))


def test_every_conv2_tap_and_channel():
    """150 models, one conv2 tap each (weight co + 1 in channel co), five per launch."""
    for g in range(30):
        _run(f"conv2-taps-{5 * g}", entries=(False,))


def test_every_conv1_tap_and_channel():
    for g in range(5):
        _run(f"conv1-taps-{5 * g}", entries=(False,))


@pytest.mark.parametrize("O", [32, 17])
def test_fc_tail_step_and_each_accumulator_alone(O):
    """fc3 fed by its k = 80..83 only; the fc layers with only even, only odd k steps."""
    _run(f"fc-steps-O{O}")


REAL = [(0, 10), (1, 10), (2, 10), (3, 10), (1, 32)]


@pytest.mark.parametrize("idx,O", REAL)
def test_real_weights_within_the_derived_bound(idx, O):
    """The models of tests/test_gpu_lenet.py on 64 of its images: every logit within
    lenet_ref.bound of fp64, nothing added to the bound.  Worst |kernel - fp64| /
    bound measured on an MI355X: 3.05e-6, 2.52e-6, 1.92e-6, 2.45e-6 (O = 10) and
    3.00e-6 (O = 32); torch's CPU fp32 forward has 2.1e-6 .. 3.6e-6.  The bound
    carries a worst case through five layers and is loose by that much: it rules
    out a wrong element of the size of a logit, the exact cases rule out the rest."""
    from tests.test_gpu_lenet import _data, _model
    m = _model(idx, O)
    x = _data(1)[0][:64].numpy()
    params = [q.detach().numpy() for _, q in m.named_parameters()]
    offsets, P = R.layout(O)
    row = R.pack(params, offsets, P)
    ref, _ = R.forward(row, offsets, x, O)
    bnd = R.bound(row, offsets, x, O)
    labels = R.argmax_torch(ref).astype(np.int64)
    got, correct = _launch(row[None], offsets, x, O, labels)
    ratio = np.abs(got[0].astype(np.float64) - ref) / bnd
    print(f"model {idx} O={O}: worst err/bound {ratio.max():.2e} at {np.unravel_index(ratio.argmax(), ratio.shape)}, "
          f"worst err {np.abs(got[0] - ref).max():.2e}, count {int(correct[0])}/64")
    assert np.isfinite(got).all() and (ratio <= 1.0).all(), np.argwhere(ratio > 1.0)[:4]
    # a prediction can differ from fp64's only where the top two are within the bounds
    top2 = np.sort(ref, axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > 2 * bnd.max(1)
    assert np.array_equal(got[0].argmax(1)[clear], labels[clear]) and int(correct[0]) >= int(clear.sum())


@pytest.mark.parametrize("name", R.SPECIAL_NAMES)
def test_special_values(name):
    """NaN, +-inf pixels, weights and biases, and the argmax rows: the NaN mask, every
    other bit and the count as the reference has them; poisoned launches leave the
    other images and models on the clean launch's bits."""
    got, correct = _run(name)
    _, models, x, O = R.cases()[name]
    if name.startswith("pixel-"):
        clean, _ = _run("pixel-clean-B%d" % x.shape[0], entries=(False,))
        keep = np.isfinite(x).all(axis=(1, 2, 3))
        assert keep.sum() == x.shape[0] - 1
        assert np.array_equal(_bits(got[:, keep]), _bits(clean[:, keep]))
    if name in ("weight-nan", "weight-inf"):
        clean, clean_correct = _run("weight-clean", entries=(False,))
        assert np.array_equal(_bits(got[[0, 2]]), _bits(clean[[0, 2]]))
        assert np.array_equal(correct[[0, 2]], clean_correct[[0, 2]])


def test_subnormals():
    """Pixels of 2^-130 through unit weights (lenet_ref.subnormal_models).  The fp64
    reference keeps subnormals (gradual underflow), and so does the kernel on an
    MI355X, in conv1's fma chains and as MFMA input, product and result of conv2
    and the fc layers: pinned as observed."""
    models = R.subnormal_models()
    x = R.subnormal_images()
    offsets, P = R.layout(4)
    rows = np.stack([R.pack(p, offsets, P) for p in models.values()])
    got, _ = _launch(rows, offsets, x, 4, np.zeros(3, np.int64))
    ref = {n: R.forward_params(p, x)[0] for n, p in models.items()}
    seen = {}
    for s, n in enumerate(models):
        vals = np.unique(got[s])
        assert len(vals) == 1, (n, vals)  # every logit of a model is the same quantity
        seen[n] = float(vals[0]) / 2.0 ** -130
        print(f"subnormal model {n}: kernel {seen[n]:g} x 2^-130, reference {ref[n].max() / 2.0 ** -130:g} x 2^-130")
    assert seen == SUBNORMAL_OBSERVED


# in units of 2^-130, observed on an MI355X; the reference (gradual underflow) has
# the same sub 1, sum 150, fc 1, ctl 16, and a flush anywhere would give 0
SUBNORMAL_OBSERVED = {"sub": 1.0, "sum": 150.0, "fc": 1.0, "ctl": 16.0}
