"""fed_hetero on the GPU: dls_hetero_fedavg_f32 and dls_hetero_extract_f32 bit for bit against
tests/hetero_ref.py, a float64 masked weighted mean as the second opinion, and one
FedHeteroServer round."""
import numpy as np
import pytest
import torch

from tests import hetero_ref as ref

pytestmark = pytest.mark.gpu


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a, np.float32)
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def dev():
    from distributed_learning_simulator_amd import _native
    _native.require_gpu()
    return torch.device("cuda", 0)


def make_plan(which, shift):
    """A: LeNet-like, I_l * R = 75 forces the element path.  B: the vector path, tiles of 1024
    cut the rows of 576.  C: one tensor shorter than a lane's vector.  shift: 0, 1 or -1 (C - 1)."""
    from distributed_learning_simulator_amd.hetero import HeteroPlan, SliceView, vector_view
    if which == "A":
        views = [SliceView("w1", (6, 25), (6, 1, 25), "c1", None), vector_view("b1", 6, "c1"),
                 SliceView("w2", (16, 150), (16, 6, 25), "c2", "c1"), vector_view("b2", 16, "c2"),
                 SliceView("w3", (120, 400), (120, 16, 25), "h1", "c2"), vector_view("b3", 120, "h1"),
                 SliceView("w4", (10, 84), (10, 84, 1), None, "h2")]
        widths = (1.0, 0.5, 0.25)
    elif which == "B":
        views = [SliceView("w", (64, 64, 3, 3), (64, 64, 9), "c", "c"), vector_view("b", 64, "c")]
        widths = (1.0, 0.5, 0.0625)  # 64, 32 and 4 channels
    else:
        views = [vector_view("b", 3, "c")]
        widths = (1.0, 2 / 3, 1 / 3)  # 3, 2 and 1 channels
    plan = HeteroPlan(views, widths)
    plan.set_shifts({g: shift % C for g, C in plan.groups.items()})
    return plan


ASSIGN = {"full": lambda k: 0, "mixed": lambda k: k % 3, "narrow": lambda k: 1 + k % 2}
# the unheld places of prev: -0, a denormal, a NaN with a payload, a number
SPECIAL = np.array([0x80000000, 0x00000123, 0x7FC12345, 0x3F800000], np.uint32).view(np.float32)


def make_case(plan, K, assign, seed=0):
    rng = np.random.default_rng(seed)
    levels = [ASSIGN[assign](k) for k in range(K)]
    rows = [rng.normal(0, 1, plan.level_P[l]).astype(np.float32) for l in levels]
    starts = np.cumsum([0] + [r.size for r in rows])[:-1].tolist()
    prev = np.resize(SPECIAL, plan.P)
    return levels, rows, starts, list(range(1, K + 1)), prev


def run(dev, plan, levels, rows, starts, weights, prev, alias=True):
    from distributed_learning_simulator_amd import _native
    ragged = torch.from_numpy(np.concatenate(rows)).to(dev)
    dprev = torch.from_numpy(prev.copy()).to(dev)
    out = dprev if alias else torch.full((plan.P,), 7.0, device=dev)
    got = _native.hetero_fedavg(plan, levels, starts, weights, ragged, dprev, None if alias else out)
    assert got is out and (alias or np.array_equal(bits(dprev), bits(prev)))
    return out.cpu().numpy()


@pytest.mark.parametrize("assign", list(ASSIGN))
@pytest.mark.parametrize("K", [1, 3, 9, 64])
@pytest.mark.parametrize("shift", [0, 1, -1])
@pytest.mark.parametrize("which", ["A", "B", "C"])
def test_fedavg(dev, which, shift, K, assign):
    plan = make_plan(which, shift)
    levels, rows, starts, weights, prev = make_case(plan, K, assign, seed=K)
    got = run(dev, plan, levels, rows, starts, weights, prev)
    want, count = ref.fedavg(rows, levels, weights, prev, plan.tensors(), plan.slices)
    assert np.array_equal(bits(got), bits(want))
    if assign == "narrow":  # somewhere nobody holds: prev's bits, all four kinds of them
        unheld = (count == 0) & (bits(want) != 0)
        assert unheld.any() and np.array_equal(bits(got)[unheld], bits(prev)[unheld])
    # the second opinion: the float64 masked weighted mean.  A term passes through its product,
    # at most |M| - 1 additions and the quotient, and den's own chain is exact (integers), so
    # |out - exact| <= (|M| + 2) 2^-24 sum w |u| / den to first order
    held = count > 0
    exact, _ = ref.fedavg(rows, levels, weights, prev, plan.tensors(), plan.slices, np.float64)
    mag, _ = ref.fedavg([abs(r) for r in rows], levels, weights, prev, plan.tensors(), plan.slices,
                        np.float64)
    err = abs(got.astype(np.float64) - exact)[held]
    assert (err <= (count[held] + 2) * 2.0 ** -24 * mag[held]).all()


def test_fedavg_out_apart_from_prev(dev):
    plan = make_plan("A", 1)
    case = make_case(plan, 9, "narrow")
    assert np.array_equal(bits(run(dev, plan, *case, alias=False)), bits(run(dev, plan, *case)))


def test_nonfinite_stays_with_its_client(dev):
    plan = make_plan("A", 0)
    levels, rows, starts, weights, prev = make_case(plan, 3, "mixed")
    clean = run(dev, plan, levels, rows, starts, weights, prev)
    loff = plan.slices[2][4][0]  # client 2 is of level 2: two places in its part of w3
    rows[2][loff + 5], rows[2][loff + 80] = np.inf, np.nan
    got = run(dev, plan, levels, rows, starts, weights, prev)
    want, _ = ref.fedavg(rows, levels, weights, prev, plan.tensors(), plan.slices)
    bad = ~np.isfinite(want)
    assert bad.sum() == 2 and np.isinf(want).sum() == 1
    # bit for bit wherever the result is not NaN; a NaN is some NaN
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert np.array_equal(bits(got)[~np.isnan(want)], bits(want)[~np.isnan(want)])
    assert np.array_equal(bits(got)[~bad], bits(clean)[~bad])


@pytest.mark.parametrize("shift", [0, -1])
@pytest.mark.parametrize("which", ["A", "B"])
def test_extract(dev, which, shift):
    from distributed_learning_simulator_amd import _native
    plan = make_plan(which, shift)
    flat = np.random.default_rng(0).normal(0, 1, plan.P).astype(np.float32)
    flat[::5] = np.resize(SPECIAL, flat[::5].size)  # -0, denormals and NaN payloads are copied too
    rows = torch.full((sum(plan.level_P),), 7.0, device=dev)
    got = _native.hetero_extract(plan, torch.from_numpy(flat).to(dev), rows)
    for l, row in enumerate(got):
        want = ref.extract(flat, plan.tensors(), plan.slices[l], plan.level_P[l])
        assert np.array_equal(bits(row), bits(want))


def test_server_round(dev):
    from distributed_learning_simulator_amd import factory
    from distributed_learning_simulator_amd.models import LeNet5
    from distributed_learning_simulator_amd.servers.fed_hetero_server import HeteroUpdate
    torch.manual_seed(0)
    model = LeNet5()
    server = factory.get_server("fed_hetero", sharded=False, tester=None, worker_number=4,
                                synchronous=True, device=dev, widths=(1.0, 0.5), rolling=True,
                                views=model.hetero_views(),
                                initial_model=dict(model.named_parameters()))
    plan, queue = server.plan, server.worker_data_queue
    first = queue.get_result(consumer=0)
    prev = server.flat.cpu().numpy()
    for w, lay in zip(plan.widths, plan.level_layouts):  # the downlink: each level's slices
        want = ref.extract(prev, plan.tensors(), plan.slices[plan.level_of(w)], lay.P)
        assert np.array_equal(bits(lay.flatten(first.for_width(w), device=dev)), bits(want))
    tensors, slices = plan.tensors(), [list(s) for s in plan.slices]
    rng = np.random.default_rng(1)
    levels, ns = [0, 1, 0, 1], [300, 120, 777, 64]
    rows = [rng.normal(0, 1, plan.level_P[l]).astype(np.float32) for l in levels]
    for wid in (2, 0, 3, 1):  # any arrival order: the chain runs in id order
        queue.add_task((wid, ns[wid], HeteroUpdate(plan.widths[levels[wid]],
                                                   torch.from_numpy(rows[wid]).to(dev))))
    want, _ = ref.fedavg(rows, levels, ns, prev, tensors, slices)
    assert server.round == 1 and np.array_equal(bits(server.flat), bits(want))
    assert set(plan.shifts.values()) == {1}  # the second round's plan is rolled on by one
    assert int(plan.words[16 + len(tensors) + 12 + 8 + 3]) == 1  # shO of tensor 0, level 1
    second = queue.get_result(consumer=0).for_width(0.5)
    assert np.array_equal(bits(plan.level_layouts[1].flatten(second, device=dev)),
                          bits(ref.extract(want, tensors, plan.slices[1], plan.level_P[1])))
