"""GPU checks of the loss utilities on the deterministic evaluation path: the shared
per-image cross-entropy (dls_softmax_ce_f32, the epilogue of
dls_lenet5_eval_loss_f32), the fixed-order fp64 sum (dls_sum_rows_f64), the tester's
metrics_many / metrics_async and the Shapley servers' utility_metric="loss"."""
import copy
import functools
import math
import multiprocessing as mp
import pickle

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _bits64(t):
    return t.contiguous().view(torch.int64)


# ---- the seeded models and data of tests/test_gpu_lenet.py
@functools.lru_cache(maxsize=None)
def _model(idx, num_classes=10):
    """Models 0..2: LeNet5() under torch.manual_seed(idx); model 3: seed 3 with
    every parameter x 3 (CPU, eval)."""
    from distributed_learning_simulator_amd.models import LeNet5
    torch.manual_seed(idx)
    m = LeNet5(num_classes).eval()
    if idx == 3:
        with torch.no_grad():
            for p in m.parameters():
                p.mul_(3.0)
    return m


@functools.lru_cache(maxsize=None)
def _data(seed, n=2000):
    from distributed_learning_simulator_amd.models import synthetic_classification
    return synthetic_classification(n, (1, 32, 32), seed=seed)


@functools.lru_cache(maxsize=None)
def _row(idx, num_classes=10):
    """(flat device row, layout) of model idx."""
    m = _model(idx, num_classes)
    lay = m.split_layout()
    return lay.flatten(dict(m.named_parameters()), device=dev), lay


def _offsets(lay):
    from distributed_learning_simulator_amd import _native
    return [lay.offset_of(n) for n in _native.LENET5_NAMES]


# ---- 1. the per-image cross-entropy
@pytest.mark.parametrize("O", [10, 1000])
def test_ce_rows_within_8x_torch_fp32_error_of_fp64(O):
    """2,048 rows of fp32 logits (the first 256 scaled x 1e4, row 256 all equal):
    max |kernel - fp64 CE| <= 8 * max |torch CPU fp32 CE - fp64 CE| on the same rows;
    no overflow at the large scale; equal logits give log O."""
    from distributed_learning_simulator_amd import _native
    g = torch.Generator().manual_seed(O)
    z = torch.randn(2048, O, generator=g) * 3
    z[:256] *= 1e4
    z[256] = 1.25
    y = torch.randint(0, O, (2048,), generator=g)
    ref = F.cross_entropy(z.double(), y, reduction="none")
    t32 = F.cross_entropy(z, y, reduction="none").double()
    got = _native.softmax_ce(z.to(dev), y.to(dev))
    assert got.shape == (1, 2048) and got.dtype == torch.float32
    got = got[0].cpu().double()
    assert bool(torch.isfinite(got).all())
    for name, sl in (("x1e4 rows", slice(0, 256)), ("plain rows", slice(256, None))):
        e, et = float((got - ref)[sl].abs().max()), float((t32 - ref)[sl].abs().max())
        print(f"O={O} {name}: kernel err {e:.3e}, torch fp32 err {et:.3e}, ratio {e / et:.2f}")
        assert e <= 8 * et, (O, name, e, et)  # each scale on its own as well
    err, err_t = float((got - ref).abs().max()), float((t32 - ref).abs().max())
    print(f"O={O} all rows: kernel err {err:.3e}, torch fp32 err {err_t:.3e}, "
          f"ratio {err / err_t:.2f}")
    assert err <= 8 * err_t, (O, err, err_t)
    # equal logits: m - z[label] = 0 and s = O exactly, so the loss is logf(O), which
    # HIP documents within 1 ulp of log O
    print(f"O={O} equal logits: {float(got[256])!r} vs log O {math.log(O)!r}")
    assert abs(float(got[256]) - math.log(O)) <= float(np.spacing(np.float32(math.log(O))))


def test_ce_single_output_is_exactly_zero():
    """O = 1: m = z[0], expf(0) = 1, logf(1) = 0: exactly 0 at any scale."""
    from distributed_learning_simulator_amd import _native
    g = torch.Generator().manual_seed(1)
    z = torch.randn(300, 1, generator=g) * 50
    z[:100] *= 1e4
    got = _native.softmax_ce(z.to(dev), torch.zeros(300, dtype=torch.int64, device=dev))
    assert bool((_bits(got) == 0).all())


def test_ce_nan_inf_and_labels_out_of_range():
    """NaN-ness as torch's CPU fp32 cross_entropy: a NaN logit, +inf at the label and
    an all -inf row give NaN, -inf beside the label does not; labels -1 and O give NaN
    (torch refuses them); +inf beside the label is NaN in both; S = 2 at a row pitch
    > B writes nothing else."""
    from distributed_learning_simulator_amd import _native
    O = 10
    g = torch.Generator().manual_seed(2)
    z = torch.randn(2, 8, O, generator=g)
    y = torch.randint(0, O, (8,), generator=g)
    z[0, 0, 3] = float("nan")
    z[0, 1, y[1]] = float("inf")
    z[0, 4, (y[4] + 1) % O] = float("-inf")
    z[0, 5, :] = float("-inf")
    z[1, 6, (y[6] + 2) % O] = float("inf")  # +inf elsewhere: inf - inf in the sum, NaN too
    want = torch.stack([F.cross_entropy(z[s], y, reduction="none") for s in range(2)])
    assert want[0, :2].isnan().all() and want[0, 5].isnan() and not want[0, 4].isnan()
    yk = y.clone()
    yk[2], yk[3] = -1, O
    buf = torch.full((2, 13), 123.0, device=dev)
    _native.softmax_ce(z.to(dev), yk.to(dev), loss=buf[:, :8])
    got = buf[:, :8].cpu()
    assert bool((buf[:, 8:] == 123.0).all())
    assert got[:, 2:4].isnan().all()
    keep = torch.tensor([0, 1, 4, 5, 6, 7])
    assert torch.equal(got[:, keep].isnan(), want[:, keep].isnan())
    fin = torch.isfinite(want[:, keep])
    assert torch.equal(torch.isfinite(got[:, keep]), fin)
    assert torch.allclose(got[:, keep][fin], want[:, keep][fin], rtol=0, atol=1e-5)


# ---- 2. the fused epilogue is the stand-alone kernel
@pytest.mark.parametrize("O", [10, 7, 32])
def test_fused_loss_equals_softmax_ce_of_the_launch_logits(O):
    """S = 3, B in {1, 5, 16, 17, 33}: one launch with logits, loss and correct; the
    losses are the bits of softmax_ce of that launch's logits, the logits and the
    counts the bits of a launch without loss, and nothing past [S, B] of the loss
    buffer (row pitch B + 3) is written."""
    from distributed_learning_simulator_amd import _native
    lay = _row(0, O)[1]
    M = torch.stack([_row(i, O)[0] for i in range(3)])
    X, y = _data(5)
    off = _offsets(lay)
    for B in (1, 5, 16, 17, 33):
        xb = X[:B].to(dev)
        yb = (y[:B] % O).to(dev)
        if B > 4:
            yb[3], yb[4] = O, -1  # outside [0, O): NaN, no read
        lg = torch.empty((3, B, O), device=dev)
        c = torch.zeros(3, dtype=torch.int64, device=dev)
        buf = torch.full((3, B + 3), 123.0, device=dev)
        _native.lenet5_eval(M, off, xb, labels=yb, logits=lg, correct=c, loss=buf[:, :B])
        lg0 = torch.empty((3, B, O), device=dev)
        c0 = torch.zeros(3, dtype=torch.int64, device=dev)
        _native.lenet5_eval(M, off, xb, labels=yb, logits=lg0, correct=c0)
        assert torch.equal(_bits(lg), _bits(lg0)) and torch.equal(c, c0), (O, B)
        want = _native.softmax_ce(lg, yb)
        assert torch.equal(_bits(buf[:, :B]), _bits(want)), (O, B)
        assert bool((buf[:, B:] == 123.0).all())
        if B > 4:
            assert want[:, 3:5].isnan().all() and not want[:, :3].isnan().any()
        # loss alone, and with the count: the same bits
        only = torch.empty((3, B), device=dev)
        _native.lenet5_eval(M, off, xb, labels=yb, loss=only, num_out=O)
        assert torch.equal(_bits(only), _bits(want)), (O, B)


# ---- 3. end to end against fp64
@functools.lru_cache(maxsize=None)
def _loss_reference(idx, seed):
    """(fp64 CE of the fp64 forward, err_t) of model idx on data `seed`, per image:
    err_t = max |torch CPU fp32 forward + CE - that|."""
    m = _model(idx)
    X, y = _data(seed)
    with torch.no_grad():
        ref = F.cross_entropy(copy.deepcopy(m).double()(X.double()), y, reduction="none")
        err_t = float((F.cross_entropy(m(X), y, reduction="none").double() - ref).abs().max())
    return ref, err_t


def test_fused_loss_within_8x_torch_fp32_error_of_fp64():
    """Per-image losses of the four models on 2,000 images (one S = 4 launch):
    max |kernel - fp64| <= 8 * max |torch CPU fp32 forward + CE - fp64| per model."""
    from distributed_learning_simulator_amd import _native
    lay = _row(0)[1]
    M = torch.stack([_row(i)[0] for i in range(4)])
    X, y = _data(1)
    loss = torch.empty((4, 2000), device=dev)
    _native.lenet5_eval(M, _offsets(lay), X.to(dev), labels=y.to(dev), loss=loss, num_out=10)
    got = loss.cpu().double()
    for i in range(4):
        ref, err_t = _loss_reference(i, 1)
        err = float((got[i] - ref).abs().max())
        print(f"model {i}: fused loss err {err:.3e}, torch fp32 err {err_t:.3e}, "
              f"ratio {err / err_t:.2f}")
        assert err <= 8 * err_t, (i, err, err_t)


# ---- 4. the fixed-order sum
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1000])
def test_sum_rows_f64(n):
    """Within n * 2^-52 relative of numpy's fp64 sum of the same (positive) values;
    the same bits for the same row at S = 1 and in rows 0 and 2 of S = 3 at a row
    pitch > n; a NaN element makes that row NaN and no other."""
    from distributed_learning_simulator_amd import _native
    g = torch.Generator().manual_seed(n)
    a = (torch.randn(n, generator=g).abs() * 10 ** torch.empty(n).uniform_(-3, 3, generator=g))
    b = torch.rand(n, generator=g)
    want = float(a.numpy().astype(np.float64).sum())
    one = _native.sum_rows_f64(a.to(dev).unsqueeze(0))
    assert one.dtype == torch.float64 and one.shape == (1,)
    got = float(one[0])
    print(f"n={n}: kernel {got!r} numpy {want!r}")
    assert abs(got - want) <= n * 2.0 ** -52 * abs(want)
    if n == 0:
        assert got == 0.0
    buf = torch.full((3, n + 7), float("nan"), device=dev)
    buf[0, :n], buf[1, :n], buf[2, :n] = a.to(dev), b.to(dev), a.to(dev)
    three = _native.sum_rows_f64(buf[:, :n])
    assert torch.equal(_bits64(three[0:1]), _bits64(one))
    assert torch.equal(_bits64(three[2:3]), _bits64(one))
    assert abs(float(three[1]) - float(b.double().sum())) <= n * 2.0 ** -52 * float(b.double().sum())
    wide = torch.zeros((2, 2 * n + 64), device=dev)  # another pitch, another row
    wide[1, :n] = a.to(dev)
    assert torch.equal(_bits64(_native.sum_rows_f64(wide[:, :n])[1:2]), _bits64(one))
    if n:
        buf[1, n // 2] = float("nan")
        after = _native.sum_rows_f64(buf[:, :n])
        assert bool(after[1].isnan()) and torch.equal(_bits64(after[[0, 2]]),
                                                      _bits64(three[[0, 2]]))


# ---- 5. the tester: chunking independence
def test_metrics_many_bits_do_not_depend_on_chunking_rows_repeat_or_stream():
    from distributed_learning_simulator_amd.model_util import ModelUtil
    from distributed_learning_simulator_amd.trainer import Inferencer
    X, y = _data(6)
    X, y = X[:301], y[:301]
    inf = Inferencer(copy.deepcopy(_model(1)).to(dev), (X, y), device=dev)
    lay = _row(0)[1]
    assert inf.supports_correct_many(lay)
    rows = torch.stack([_row(i)[0] for i in (2, 0, 3)])
    assert inf.split_batch(301) == 301  # the whole set in one forward
    c, l = inf.metrics_many(rows, lay)
    assert c.dtype == torch.int64 and l.dtype == torch.float64 and l.shape == (3,)
    assert torch.equal(c, inf.correct_many(rows, lay))
    # the loss itself, once: the module's fp32 forward + CE summed in fp64
    with torch.no_grad():
        want = float(F.cross_entropy(_model(2)(X), y, reduction="none").double().sum())
    assert abs(float(l[0]) - want) <= 1e-5 * want
    for chunk in (5, 64):
        inf.split_batch = lambda n, chunk=chunk: chunk
        c2, l2 = inf.metrics_many(rows, lay)
        assert torch.equal(_bits64(l2), _bits64(l)) and torch.equal(c2, c), chunk
        del inf.split_batch
    for s in range(3):
        cs, ls = inf.metrics_many(rows[s], lay)
        assert torch.equal(_bits64(ls), _bits64(l[s:s + 1])) and int(cs) == int(c[s])
    c3, l3 = inf.metrics_many(rows, lay)
    assert torch.equal(_bits64(l3), _bits64(l)) and torch.equal(c3, c)
    st = torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(st):
        c4, l4 = inf.metrics_many(rows, lay)
    st.synchronize()
    assert torch.equal(_bits64(l4), _bits64(l)) and torch.equal(c4, c)
    for s, idx in enumerate((2, 0, 3)):
        ModelUtil(inf.model).load_parameter_dict(dict(_model(idx).named_parameters()))
        ca, la = inf.metrics_async()
        assert la.dim() == 0 and la.dtype == torch.float64
        assert torch.equal(_bits64(la.reshape(1)), _bits64(l[s:s + 1])) and int(ca) == int(c[s])
        assert int(ca) == int(inf.correct_async())


# ---- 6. any other model
def test_metrics_async_resnet18():
    """conv="dls" ResNet-18 on 64 CIFAR-shaped images: the mean loss is inference()'s
    within 1e-5 relative (another reduction order), the count correct_async()'s, and
    two calls give the same bits."""
    from distributed_learning_simulator_amd.models import ResNet18, synthetic_classification
    from distributed_learning_simulator_amd.trainer import Inferencer
    torch.manual_seed(4)
    model = ResNet18().to(dev).eval()
    X, y = synthetic_classification(64, (3, 32, 32), seed=3)
    inf = Inferencer(model, (X, y), device=dev, conv="dls")
    assert inf._split_forward() is not None and not hasattr(model, "score_rows")
    loss, acc, _ = inf.inference()
    c, l = inf.metrics_async()
    c2, l2 = inf.metrics_async()
    assert l.dtype == torch.float64 and l.dim() == 0
    assert torch.equal(_bits64(l.reshape(1)), _bits64(l2.reshape(1))) and int(c) == int(c2)
    print(f"ResNet-18: metrics_async mean loss {float(l) / 64!r}, inference() {float(loss)!r}")
    assert abs(float(l) / 64 - float(loss)) <= 1e-5 * abs(float(loss))
    assert int(c) == int(inf.correct_async()) and int(c) / 64 == acc


# ---- 7. the servers
def _run_server(cls, N, prepare=None, **kw):
    """One round of N clients (the base model 3 plus seeded noise) on a tester with
    200 images labelled by the base model; `prepare(server)` runs before the
    clients' updates arrive."""
    from distributed_learning_simulator_amd.trainer import Inferencer
    X = _data(9)[0][:200]
    with torch.no_grad():
        y = _model(3)(X).argmax(1)
    tester = Inferencer(copy.deepcopy(_model(1)).to(dev), (X, y), device=dev)
    server = cls(tester=tester, worker_number=N, synchronous=True, **kw)
    if prepare is not None:
        prepare(server)
    base = dict(_model(3).named_parameters())
    g = torch.Generator().manual_seed(77)
    for i in range(N):
        d = {k: (v.detach() + 0.02 * (i + 1) * torch.randn(v.shape, generator=g))
             for k, v in base.items()}
        server.worker_data_queue.add_task((i, 100 + 10 * i, d))
    for w in range(2 * N):
        server.worker_data_queue.get_result(consumer=w % N)
    return server


def _record_rows(server):
    """Keep a copy of every matrix of rows the tester's metrics_many scores."""
    server.seen_rows = []
    many = server.tester.metrics_many

    def wrapped(rows, layout):
        server.seen_rows.append(rows.clone())
        return many(rows, layout)

    server.tester.metrics_many = wrapped


def _slow_loss_route(server):
    """The route without the feature: get_metric replaced by the loss one."""
    from distributed_learning_simulator_amd.servers.fed_server import FedServer
    server.get_metric = lambda model, metric_type="acc": FedServer.get_metric(server, model, "loss")


def test_multiround_server_loss_utilities(tmp_path):
    from distributed_learning_simulator_amd.servers.multiround_shapley_value_server import \
        MultiRoundShapleyValueServer
    N, n = 4, 200
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    a = _run_server(MultiRoundShapleyValueServer, N, _record_rows, utility_metric="loss",
                    metric_dir=str(tmp_path / "a"))
    metrics = pickle.loads((tmp_path / "a" / "metric_1").read_bytes())
    assert len(metrics) == 16 and len(set(metrics.values())) == 16
    # one batch: the 15 non-empty coalitions in power-set order, then the empty one
    assert [r.shape[0] for r in a.seen_rows] == [15, 1]
    lay = a.tester.model.split_layout()
    order = [s for s in a.evaluated_subsets if s] + [()]
    for key, row in zip(order, torch.cat(a.seen_rows)):
        _, l = a.tester.metrics_many(row, lay)  # that coalition alone, S = 1
        assert metrics[key] == float(l[0]) / n, key
    sv = a.shapley_values[1]
    full = tuple(range(N))
    assert abs(sum(sv.values()) - (metrics[full] - metrics[()])) <= 1e-9
    b = _run_server(MultiRoundShapleyValueServer, N, _slow_loss_route,
                    metric_dir=str(tmp_path / "b"))
    slow = pickle.loads((tmp_path / "b" / "metric_1").read_bytes())
    assert a.evaluated_subsets == b.evaluated_subsets
    for key in metrics:
        assert abs(metrics[key] - slow[key]) <= 1e-5 * abs(slow[key]), key
    for i in range(N):
        print(f"SV[{i}] loss utilities: fast {sv[i]!r} slow route {b.shapley_values[1][i]!r}")
        assert abs(sv[i] - b.shapley_values[1][i]) <= 1e-5


def _record_utilities(server):
    server.seen_values, server.seen_utility = {}, []
    evaluate, utility = server.evaluate_subsets, server.utility

    def ev(subsets):
        subsets = [tuple(s) for s in subsets]
        values = evaluate(subsets)
        server.seen_values.update(zip(subsets, values))
        return values

    def ut(model):
        server.seen_utility.append(utility(model))
        return server.seen_utility[-1]

    server.evaluate_subsets, server.utility = ev, ut


def test_gtg_server_loss_utilities():
    from distributed_learning_simulator_amd.servers.GTG_shapley_value_server import \
        GTGShapleyValueServer
    out = []
    for kw in ({}, {"subset_batch": 1}):
        np.random.seed(3)
        out.append(_run_server(GTGShapleyValueServer, 5, _record_utilities,
                               utility_metric="loss", **kw))
    a, b = out
    assert a.evaluated_subsets == b.evaluated_subsets and a.evaluated_subsets
    assert a.seen_values == b.seen_values
    assert a.shapley_values == b.shapley_values
    assert any(v != 0 for v in a.shapley_values[1].values())
    full = tuple(range(5))
    last_round_metric, this_round_metric = a.seen_utility
    assert full in a.seen_values and a.seen_values[full] == this_round_metric
    assert last_round_metric != this_round_metric and a.seen_utility == b.seen_utility


@pytest.mark.parametrize("name", ["multiround", "gtg"])
def test_default_utility_metric_is_the_accuracy_path(name, tmp_path):
    """The keyword left out: the batched path's results are those of the per-coalition
    path and of utility_metric="acc", and the utilities are counts / n."""
    from distributed_learning_simulator_amd.servers.GTG_shapley_value_server import \
        GTGShapleyValueServer
    from distributed_learning_simulator_amd.servers.multiround_shapley_value_server import \
        MultiRoundShapleyValueServer
    cls, N, kw = ((MultiRoundShapleyValueServer, 4, {"metric_dir": None}) if name == "multiround"
                  else (GTGShapleyValueServer, 5, {}))

    def per_coalition(server):
        _record_utilities(server)
        server.tester.supports_correct_many = lambda layout: False

    out = []
    for prepare, extra in ((_record_utilities, {}), (per_coalition, {}),
                           (_record_utilities, {"utility_metric": "acc"})):
        np.random.seed(3)
        out.append(_run_server(cls, N, prepare, **kw, **extra))
    a, b, c = out
    assert a.utility_metric == "acc"
    assert a.evaluated_subsets == b.evaluated_subsets == c.evaluated_subsets
    assert a.seen_values == b.seen_values == c.seen_values and a.seen_values
    assert a.shapley_values == b.shapley_values == c.shapley_values
    assert a.seen_utility == b.seen_utility == c.seen_utility
    assert all(v == round(v * 200) / 200 for v in a.seen_values.values())
    assert a.tester.accuracy_metric.value == b.tester.accuracy_metric.value


# ---- 8. two processes
def _loss_worker(outq):
    torch.cuda.set_device(0)
    from distributed_learning_simulator_amd.models import LeNet5, synthetic_classification
    from distributed_learning_simulator_amd.trainer import Inferencer
    rows = []
    for seed in (7, 8):
        torch.manual_seed(seed)
        m = LeNet5()
        rows.append(m.split_layout().flatten(dict(m.named_parameters()), device="cuda:0"))
    X, y = synthetic_classification(64, (1, 32, 32), seed=11)
    inf = Inferencer(m.to("cuda:0"), (X, y), device=torch.device("cuda", 0))
    c, l = inf.metrics_many(torch.stack(rows), m.split_layout())
    outq.put((l.cpu().numpy().tobytes(), c.tolist()))


def test_loss_sums_byte_identical_across_processes():
    """Two fresh spawned processes, one after the other, score the same two seeded
    LeNet-5 models on the same 64 images: byte-identical loss sums."""
    from tests.test_gpu_distributed import _collect
    ctx = mp.get_context("spawn")
    res = []
    for _ in range(2):
        q = ctx.Queue()
        p = ctx.Process(target=_loss_worker, args=(q,))
        p.start()
        res.extend(_collect([p], q, 1, 120))
        p.join(60)
        assert p.exitcode == 0
    (la, ca), (lb, cb) = res
    assert len(la) == 16 and la == lb and ca == cb
    sums = np.frombuffer(la, dtype=np.float64)
    assert np.isfinite(sums).all() and sums[0] != sums[1]
