"""CPU checks of tests/lenet_ref.py, the reference tests/test_gpu_lenet_exact.py
compares dls_lenet5_eval_f32 with: the fp64 forward against models.LeNet5 in
double, special values included; the offset order; the derived bound against
torch's own fp32 forward; and, for every launch of the GPU file, the conditions
that make its comparison mean what it says."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import lenet_ref as R


def _bits64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    """Equal NaN masks, equal bits everywhere else."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(_bits64(a)[~na], _bits64(b)[~nb])


def _torch_forward(params, x, dtype):
    """The module's forward (models.LeNet5.forward) on ten tensors, on the CPU."""
    p = [torch.from_numpy(np.asarray(a, np.float32)).to(dtype) for a in params]
    h = torch.from_numpy(np.asarray(x, np.float32)).to(dtype)
    with torch.no_grad():
        h = F.max_pool2d(F.relu(F.conv2d(h, p[0], p[1])), 2)
        h = F.max_pool2d(F.relu(F.conv2d(h, p[2], p[3])), 2).flatten(1)
        h = F.relu(F.linear(h, p[4], p[5]))
        h = F.relu(F.linear(h, p[6], p[7]))
        return F.linear(h, p[8], p[9]).numpy()


def _module(params, O):
    from distributed_learning_simulator_amd.models import LeNet5
    m = LeNet5(O).double().eval()
    with torch.no_grad():
        for (name, q), a in zip(m.named_parameters(), params):
            q.copy_(torch.from_numpy(np.asarray(a, np.float64)))
    assert tuple(n for n, _ in m.named_parameters()) == R.NAMES
    return m


@pytest.mark.parametrize("O", [1, 7, 10, 17, 32])
def test_forward_equals_the_module_in_double(O):
    """Integer models (every fp64 sum exact in any order, so equality is owed) and
    the same with NaN, +-inf and -0 among pixels, weights and biases."""
    params = R.int_params(O, 50 + O)
    x = R.int_images(6, 50 + O)
    offsets, P = R.layout(O)
    row = R.pack(params, offsets, P)
    m = _module(params, O)
    with torch.no_grad():
        want = m(torch.from_numpy(x).double()).numpy()
    got, pre = R.forward(row, offsets, x, O)
    assert [z.shape for z in pre] == [(6, 6, 28, 28), (6, 16, 10, 10), (6, 120), (6, 84), (6, O)]
    assert np.array_equal(_bits64(got), _bits64(want))
    assert np.array_equal(got, _torch_forward(params, x, torch.float64))
    # special values, one kind per image / tensor
    xs = x.copy()
    xs[0, 0, 3, 4], xs[1, 0, 30, 2], xs[2, 0, 7, 7], xs[3, 0, 0, 0] = np.nan, np.inf, -np.inf, -0.0
    seen_nan = seen_clean = False
    for i, at, v in ((None, None, None), (1, (2,), -np.inf), (3, (5,), np.inf), (4, (9, 11), np.nan),
                     (5, (3,), -np.inf), (6, (0, 0), -0.0), (8, (0, 5), np.inf), (9, (0,), -0.0)):
        q = [np.array(a) for a in params]
        if i is not None:
            q[i][at] = v
        with torch.no_grad():
            want = _module(q, O)(torch.from_numpy(xs).double()).numpy()
        got, _ = R.forward(R.pack(q, offsets, P), offsets, xs, O)
        assert _same(got, want), (i, at, v)
        seen_nan |= bool(np.isnan(got).any())
        seen_clean |= bool(np.isfinite(got).any())
    assert seen_nan and seen_clean


def test_relu_and_pool_special_values():
    z = np.array([-np.inf, -0.0, 0.0, np.nan, 2.0, np.inf])
    got = R.relu(z)
    want = F.relu(torch.from_numpy(z)).numpy()
    # torch's scalar CPU path returns relu(-0) = -0; the kernel's relu_nan and the
    # reference give +0, and the two zeros are equal to everything that follows
    assert _same(got[[0, 2, 3, 4, 5]], want[[0, 2, 3, 4, 5]]) and got[1] == want[1] == 0
    assert not np.signbit(got[:3]).any()
    for pos in range(4):  # a NaN survives the pool at each window position
        a = np.arange(16, dtype=np.float64).reshape(1, 1, 4, 4)
        a[0, 0, pos // 2, pos % 2] = np.nan
        got = R.pool(a)
        assert _same(got, F.max_pool2d(torch.from_numpy(a), 2).numpy())
        assert np.isnan(got[0, 0, 0, 0]) and np.isfinite(got[0, 0, 1:, :]).all()


def test_offsets_are_in_native_order_and_layout_free():
    from distributed_learning_simulator_amd import _native
    from distributed_learning_simulator_amd.models import LeNet5
    assert R.NAMES == _native.LENET5_NAMES and R.shapes(17) == _native.lenet5_shapes(17)
    lay = LeNet5(17).split_layout()
    assert tuple(lay.names) == R.NAMES
    params = R.int_params(17, 3)
    x = R.int_images(4, 3)
    offsets, P = R.layout(17)
    base, _ = R.forward(R.pack(params, offsets, P), offsets, x, 17)
    # the library's own layout of the module
    row = lay.flatten({n: torch.from_numpy(a) for n, a in zip(R.NAMES, params)}).numpy()
    got, _ = R.forward(row, [lay.offset_of(n) for n in R.NAMES], x, 17)
    assert np.array_equal(got, base)
    # tensors in another order with NaN in the gaps between them
    o2, P2 = R.layout(17, order=(7, 2, 9, 0, 5, 4, 1, 8, 3, 6), gap=12)
    assert sorted(o2) != o2 and P2 > P and all(o % 4 == 0 for o in o2)
    row2 = R.pack(params, o2, P2, fill=np.nan)
    assert np.isnan(row2).sum() == P2 - sum(a.size for a in params)
    got, _ = R.forward(row2, o2, x, 17)
    assert np.array_equal(got, base)
    assert all(np.array_equal(a, b) for a, b in zip(R.unpack(row2, o2, 17), params))


def test_argmax_torch():
    rows = np.array(list(R.ARGMAX_ROWS.values()) + [[3, 3, 3, 3, 3, 3, 3, 3], [0, 1, 2, 3, 4, 5, 6, 7]],
                    np.float32)
    want = torch.from_numpy(rows).argmax(-1).numpy()
    assert np.array_equal(R.argmax_torch(rows), want)
    assert dict(zip(R.ARGMAX_ROWS, want[:7])) == dict(tie=1, zeros=1, neg_inf=0, nan_first=0,
                                                      nan_later=2, two_nans=2, inf_then_nan=3)


def test_argmax_counts_name_the_picked_index():
    """The argmax launches' labels ask for class i exactly i + 1 times, so each of
    the 8 possible picks gives another count: the right index differs in count from
    every competitor (the other tied maxima, a later NaN, a larger finite or inf)."""
    per_pick = np.array([(R.ARGMAX_LABELS == i).sum() for i in range(8)])
    assert len(set(per_pick.tolist())) == 8 and len(R.ARGMAX_LABELS) == 36 <= 48
    for case in ("argmax-a", "argmax-b"):
        _, models, x, O = R.cases()[case]
        ref, _, labels = R.reference(case)
        assert O == 8 and x.shape[0] == 36 and labels is R.ARGMAX_LABELS
        for s in range(len(models)):
            assert _same(ref[s], np.broadcast_to(ref[s, 0], ref[s].shape))  # one row, every image
    rows = {n: np.array(v, np.float32) for n, v in R.ARGMAX_ROWS.items()}
    pick = {n: int(R.argmax_torch(v)) for n, v in rows.items()}
    rivals = {"tie": [3, 5, 7], "zeros": [0, 2, 3, 4, 6], "neg_inf": [1, 7], "nan_first": [4, 1],
              "nan_later": [4, 1, 0], "two_nans": [4, 5, 6], "inf_then_nan": [0, 1]}
    assert set(rivals) == set(rows)
    for n, others in rivals.items():
        assert pick[n] not in others
        assert all(per_pick[o] != per_pick[pick[n]] for o in others), n
    # what the named wrong rules would pick: >= (the last of equal maxima), the last
    # NaN, no NaN rule at all
    assert int(np.flatnonzero(rows["tie"] == 5)[-1]) == 5 != pick["tie"]
    assert int(np.flatnonzero(rows["zeros"] == 0)[-1]) == 6 != pick["zeros"]
    assert int(np.flatnonzero(np.isnan(rows["two_nans"]))[-1]) == 4 != pick["two_nans"]
    assert int(np.nanargmax(rows["nan_later"])) == 4 != pick["nan_later"]


def test_case_names_are_the_cases():
    assert tuple(R.cases()) == R.CASE_NAMES
    assert tuple(n for n, c in R.cases().items() if c[0] == "special") == R.SPECIAL_NAMES


REAL = [(0, 10), (1, 10), (2, 10), (3, 10), (1, 32)]


@pytest.mark.parametrize("idx,O", REAL)
def test_torch_fp32_forward_stays_inside_the_bound(idx, O):
    """The models of tests/test_gpu_lenet.py on 64 of its images: torch's CPU fp32
    forward, another correct fp32 evaluation, is inside ``bound`` at every logit.
    Worst |fp32 - fp64| / bound here: 3.6e-6, 3.2e-6, 2.1e-6, 3.0e-6 (O = 10) and
    3.2e-6 (O = 32).  The bound is a worst case carried through five layers (each
    multiplies the incoming error by sum |w|), so it is loose by that much; the
    exact cases are what pins single elements."""
    from tests.test_gpu_lenet import _data, _model
    m = _model(idx, O)
    x = _data(1)[0][:64]
    params = [q.detach().numpy() for _, q in m.named_parameters()]
    offsets, P = R.layout(O)
    row = R.pack(params, offsets, P)
    ref, _ = R.forward(row, offsets, x.numpy(), O)
    bnd = R.bound(row, offsets, x.numpy(), O)
    with torch.no_grad():
        got = m(x).numpy().astype(np.float64)
        dbl = _module(params, O)(x.double()).numpy()
    assert np.abs(ref - dbl).max() <= 1e-12 * np.abs(dbl).max()  # two fp64 orders
    ratio = np.abs(got - ref) / bnd
    print(f"model {idx} O={O}: torch fp32 worst err/bound {ratio.max():.2e}, "
          f"bound {bnd.min():.2e}..{bnd.max():.2e}")
    assert bnd.shape == (64, O) and (bnd > 0).all() and (ratio <= 1.0).all()


@pytest.mark.parametrize("name", R.CASE_NAMES)
def test_every_gpu_case_is_what_it_claims(name):
    """Conditions, not measurements: integers with every layer's certificate below
    2^24 (non-finite entries aside), torch's CPU fp32 forward already on the
    reference's bits, and for the random integer models both ReLU branches in
    every layer and at least 0.9 of a launch's logits distinct."""
    kind, models, x, O = R.cases()[name]
    ref, pre, labels = R.reference(name)
    assert 1 <= len(models) <= 5 and x.shape[0] <= 48 and ref.shape == (len(models), x.shape[0], O)
    for s, params in enumerate(models):
        fin = [np.where(np.isfinite(a), a, 0) for a in params]
        assert R.is_integer_model(fin, np.where(np.isfinite(x), x, 0))
        assert max(R.certificate_params(params, x)) < 2 ** 24
        assert _same(_torch_forward(params, x, torch.float32), ref[s]), s
        assert _same(ref[s].astype(np.float32), ref[s])  # the logits are fp32 values
    assert labels.shape == (x.shape[0],) and labels.min() >= 0 and labels.max() < O
    if kind == "general":
        assert np.isfinite(ref).all()
        for l in range(5):
            share = np.mean(np.concatenate([p[l].ravel() for p in pre]) > 0)
            assert 0.25 <= share <= 0.75, (R.LAYERS[l], share)
        assert len(np.unique(ref)) >= 0.9 * ref.size
        hits = (R.argmax_torch(ref) == labels).sum(-1)
        assert x.shape[0] < 4 or O == 1 or (0 < hits[0] and (hits < x.shape[0]).any())


def test_tap_models_tell_every_tap_and_channel_apart():
    """The 150 conv2 tap models give 150 different logit tensors on the same images,
    the 25 conv1 tap models 25, and moving a tap's weights to other output channels
    changes the logits too."""
    for build, n, i, C in ((R.conv2_tap_model, 150, 2, 16), (R.conv1_tap_model, 25, 0, 6)):
        x = R.int_images(3, 21)
        seen = {R.forward_params(build(k), x)[0].tobytes() for k in range(n)}
        assert len(seen) == n
        for k in (0, n // 2, n - 1):
            p = build(k)
            base = R.forward_params(p, x)[0]
            for a in range(C - 1):  # swap the weights of channels a and a + 1
                q = [np.array(t) for t in p]
                q[i][[a, a + 1]] = q[i][[a + 1, a]]
                assert not np.array_equal(R.forward_params(q, x)[0], base), (k, a)


def test_step_models_exercise_their_steps():
    x = R.int_images(17, 22)
    for which in ("tail", "even", "odd"):
        p = R.fc_step_model(which)
        for i in (4, 6, 8):
            step = np.arange(p[i].shape[1]) // 4
            used = np.unique(step[(p[i] != 0).any(0)])
            if which == "tail":
                assert i != 8 or list(used) == [20]
            else:
                assert (used % 2 == (which == "odd")).all() and len(used) == (step.max() + 1 + (which == "even")) // 2
        ref, pre = R.forward_params(p, x)
        assert len(np.unique(ref)) >= 0.9 * ref.size
        if which == "tail":  # all four inputs of the tail step are active everywhere
            assert (pre[3][:, 80:84] > 0).all() and (p[8][:, 80:84] != 0).all()


def test_special_models_have_the_values_they_are_named_for():
    c = R.cases()
    for O in (10, 32):
        ref, pre, _ = R.reference(f"inf-conv1-channel-O{O}")
        assert np.isinf(ref).all() and (np.signbit(ref[0, 0]) == (np.arange(O) % 2 == 1)).all()
        assert np.isposinf(pre[0][0][:, 0]).all()
    for O in (7, 17):
        ref, pre, _ = R.reference(f"inf-fc2-O{O}")
        assert np.isinf(ref[0]).all() and np.isfinite(ref[1]).all()
    ref, pre, _ = R.reference("neg-inf-preactivations")
    assert np.isfinite(ref).all() and all(np.isneginf(pre[0][l]).any() for l in range(4))
    ref, _, _ = R.reference("nan-corners")
    assert np.isnan(ref[:, :4]).all() and np.isfinite(ref[:, 4]).all()
    for tag in ("nan", "inf"):
        for B, b in ((32, 5), (21, 18)):
            ref, _, _ = R.reference(f"pixel-{tag}-B{B}")
            assert np.isnan(ref[:, b]).all() and np.isfinite(np.delete(ref, b, axis=1)).all()
        ref, _, _ = R.reference(f"weight-{tag}")
        assert np.isnan(ref[1]).all() and np.isfinite(ref[[0, 2]]).all()
    ref, _, _ = R.reference("inf-weight-ragged-fc3")
    assert np.isposinf(ref[0][:, 3]).all() and np.isfinite(np.delete(ref[0], 3, axis=1)).all()
    assert c["inf-weight-ragged-fc3"][2].min() >= 1


def test_subnormal_models_in_the_reference():
    """The reference keeps subnormals (IEEE gradual underflow)."""
    x = R.subnormal_images()
    assert x.dtype == np.float32 and (x == 2.0 ** -130).all() and (x < np.finfo(np.float32).tiny).all()
    want = {"sub": 2.0 ** -130, "sum": 150 * 2.0 ** -130, "fc": 2.0 ** -130, "ctl": 2.0 ** -126}
    for name, p in R.subnormal_models().items():
        ref, pre = R.forward_params(p, x)
        assert (ref == want[name]).all(), name
        assert _same(ref.astype(np.float32), ref)
    _, pre = R.forward_params(R.subnormal_models()["fc"], x)
    assert pre[1].max() == 2.0 ** -126 and pre[2].max() == 2.0 ** -130  # fc1 makes the first
