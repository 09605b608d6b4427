"""GPU checks of the batched deterministic LeNet-5 utility evaluation
(dls_lenet5_eval_f32, csrc/lenet.hip): accuracy against fp64, ragged shapes,
bit-determinism, the correct counts, the tester and the Shapley servers."""
import functools
import multiprocessing as mp
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)


def _bits(t):
    return t.contiguous().view(torch.int32)


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
def _reference(idx, seed):
    """(fp64 logits, err_t) of model idx on data `seed`: err_t = max |torch CPU fp32
    forward - fp64 forward|, the yardstick of another fp32 ordering of the sums."""
    import copy
    m = _model(idx)
    X, _ = _data(seed)
    with torch.no_grad():
        ref = copy.deepcopy(m).double()(X.double())
        err_t = float((m(X).double() - ref).abs().max())
    return ref, err_t


@functools.lru_cache(maxsize=None)
def _row(idx, num_classes=10):
    """(flat device row, layout) of model idx."""
    m = _model(idx, num_classes)
    lay = m.split_layout()
    return lay.flatten(dict(m.named_parameters()), device=dev), lay


def _offsets(lay):
    from distributed_learning_simulator_amd import _native
    return [lay.offset_of(n) for n in _native.LENET5_NAMES]


def _eval(models, lay, X, O=10, labels=None, correct=None, want_logits=True, stream=None):
    from distributed_learning_simulator_amd import _native
    S = 1 if models.dim() == 1 else models.shape[0]
    logits = torch.empty((S, X.shape[0], O), device=dev) if want_logits else None
    _native.lenet5_eval(models, _offsets(lay), X, labels=labels, logits=logits, correct=correct,
                        num_out=O, stream=stream)
    return logits


def _check_against_fp64(got, idx, seed):
    ref, err_t = _reference(idx, seed)
    got = got.cpu().double()
    err = float((got - ref).abs().max())
    print(f"model {idx} data {seed}: kernel err {err:.3e}, torch fp32 err {err_t:.3e}, "
          f"ratio {err / err_t:.2f}")
    assert err <= 8 * err_t, (idx, err, err_t)
    top2 = ref.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > 16 * err_t
    assert (~clear).sum() <= 0.01 * ref.shape[0]
    assert torch.equal(got.argmax(1)[clear], ref.argmax(1)[clear])


@pytest.mark.parametrize("idx", [0, 1, 2, 3])
def test_single_model_within_8x_torch_fp32_error_of_fp64(idx):
    """S = 1: max |kernel - fp64| <= 8 * max |torch CPU fp32 - fp64| on 2,000 images,
    and the fp64 prediction wherever its top-two margin exceeds 16 * err_t."""
    row, lay = _row(idx)
    X, _ = _data(idx + 1)
    _check_against_fp64(_eval(row, lay, X.to(dev))[0], idx, idx + 1)


def test_four_models_batched_within_8x_torch_fp32_error_of_fp64():
    """The four models as S = 4 rows at ldm > P, on the first model's images: each
    row meets the same bound, and row 0 is the S = 1 launch's bits."""
    lay = _row(0)[1]
    M = torch.full((4, lay.P + 192), float("nan"), device=dev)
    for i in range(4):
        M[i, :lay.P] = _row(i)[0]
    X = _data(1)[0].to(dev)
    got = _eval(M, lay, X)
    for i in range(4):
        _check_against_fp64(got[i], i, 1)
    assert torch.equal(_bits(got[0]), _bits(_eval(_row(0)[0], lay, X)[0]))


@pytest.mark.parametrize("O", [10, 7])
@pytest.mark.parametrize("B", [1, 37, 301])
def test_ragged_batches_equal_rows_of_a_larger_batch(B, O):
    """B a multiple of no tile, O = 10 and 7: the logits are the same images' rows
    of a 320-image launch, and nothing past [S, B, O] is written."""
    from distributed_learning_simulator_amd import _native
    row, lay = _row(1, O)
    X = _data(5)[0][:320].to(dev)
    big = _eval(row, lay, X, O)[0]
    if O == 7:  # the function itself, once: the module's fp32 forward
        ref = _model(1, 7)(X.cpu()).detach()
        assert (big.cpu() - ref).abs().max() < 1e-5
    buf = torch.full((B * O + 64,), 123.0, device=dev)
    out = buf[:B * O].view(1, B, O)
    _native.lenet5_eval(row, _offsets(lay), X[:B].contiguous(), logits=out)
    assert torch.equal(_bits(out[0]), _bits(big[:B]))
    assert bool((buf[B * O:] == 123.0).all())


def test_bits_do_not_depend_on_batching_position_row_pitch_repeat_or_stream():
    row, lay = _row(2)
    X = _data(6)[0][:301].to(dev)
    whole = _eval(row, lay, X)[0]
    for chunk in (5, 64):
        parts = torch.cat([_eval(row, lay, X[i:i + chunk].contiguous())[0]
                           for i in range(0, 301, chunk)])
        assert torch.equal(_bits(whole), _bits(parts)), chunk
    # an image moved to another batch position (another tile, another column)
    perm = torch.roll(torch.arange(301, device=dev), 23)
    moved = _eval(row, lay, X[perm].contiguous())[0]
    assert torch.equal(_bits(moved), _bits(whole[perm]))
    # the same model in row 0 and in row 4 of S = 5, different neighbours
    for pitch in (lay.P, lay.P + 64):
        M = torch.zeros((5, pitch), device=dev)
        for r, i in enumerate((2, 0, 1, 3, 2)):
            M[r, :lay.P] = _row(i)[0]
        got = _eval(M, lay, X)
        assert torch.equal(_bits(got[0]), _bits(whole)), pitch
        assert torch.equal(_bits(got[4]), _bits(whole)), pitch
        assert torch.equal(_bits(got[2]), _bits(_eval(_row(1)[0], lay, X)[0]))
    # a repeated launch, and one on a non-default stream
    assert torch.equal(_bits(_eval(row, lay, X)[0]), _bits(whole))
    st = torch.cuda.Stream(dev)
    st.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(st):
        other = _eval(row, lay, X, stream=st)[0]
    st.synchronize()
    assert torch.equal(_bits(other), _bits(whole))


def test_correct_counts():
    lay = _row(0)[1]
    M = torch.stack([_row(i)[0] for i in range(3)])
    X, y = _data(7)
    X, y = X[:301].to(dev), y[:301].to(dev)
    correct = torch.zeros(3, dtype=torch.int64, device=dev)
    logits = _eval(M, lay, X, labels=y, correct=correct)
    want = (logits.argmax(-1) == y).sum(-1)
    assert torch.equal(correct, want)
    only = torch.zeros(3, dtype=torch.int64, device=dev)
    assert _eval(M, lay, X, labels=y, correct=only, want_logits=False) is None
    assert torch.equal(only, want)
    _eval(M, lay, X, labels=y, correct=only, want_logits=False)  # accumulates
    assert torch.equal(only, 2 * want)
    # an all-zero model: all logits equal, argmax 0, so exactly the images labelled 0
    zero = torch.zeros((1, lay.P), device=dev)
    c0 = torch.zeros(1, dtype=torch.int64, device=dev)
    lz = _eval(zero, lay, X, labels=y, correct=c0)
    assert bool((lz == 0).all()) and int(c0) == int((y == 0).sum()) > 0
    # a NaN logit is a maximum, as torch.argmax has it
    nan = _row(0)[0].clone()
    nan[lay.offset_of("fc3.bias") + 4] = float("nan")
    cn = torch.zeros(1, dtype=torch.int64, device=dev)
    ln = _eval(nan, lay, X, labels=y, correct=cn)
    assert int(cn) == int((ln[0].argmax(-1) == y).sum()) == int((y == 4).sum())


def test_tester_runs_the_library_forward():
    """The default CUDA Inferencer on LeNet-5 leaves torch's cudnn flags alone, scores
    forward_split's bits, and its accuracy is the counted one; conv="miopen" and a
    28 x 28 dataset run the module's forward as before."""
    import copy
    from distributed_learning_simulator_amd.trainer import Inferencer
    model = copy.deepcopy(_model(1)).to(dev)
    X, y = _data(8)
    X, y = X[:777], y[:777]
    flags = (torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)
    a = Inferencer(model, (X, y), device=dev)
    assert a.conv == "dls" and a._split_forward() is not None
    la = a.logits()
    _, acc, _ = a.inference()
    assert (torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark) == flags
    with torch.no_grad():
        direct = model.forward_split(X.to(dev), model.pack_split())
    assert torch.equal(_bits(la), _bits(direct))
    assert acc == int(a.correct_async()) / 777
    assert acc == int((la.argmax(1).cpu() == y).sum()) / 777
    lay = model.split_layout()
    assert a.supports_correct_many(lay)
    many = a.correct_many(torch.stack([_row(1)[0], _row(0)[0]]), lay)
    assert many.dtype == torch.int64 and int(many[0]) / 777 == acc
    # the module path: conv="miopen", and inputs the kernel does not take
    det = dict(enabled=True, deterministic=True, benchmark=False)  # the module path's flags
    with torch.no_grad(), torch.backends.cudnn.flags(**det):
        module = model(X.to(dev))
    b = Inferencer(model, (X, y), device=dev, conv="miopen")
    assert b._split_forward() is None and not b.supports_correct_many(lay)
    assert torch.equal(_bits(b.logits()), _bits(module))

    class Net28(type(model)):  # LeNet-5 on 28 x 28 images: fc1 takes 16 * 4 * 4
        def __init__(self):
            super().__init__()
            self.fc1 = torch.nn.Linear(256, 120)

    torch.manual_seed(5)
    m28 = Net28().to(dev).eval()
    X28 = X[:, :, 2:30, 2:30].contiguous()
    c = Inferencer(m28, (X28, y), device=dev)
    assert c._split_forward() is None and not c.supports_correct_many(m28.split_layout())
    with torch.no_grad(), torch.backends.cudnn.flags(**det):
        want = m28(X28.to(dev))
    assert torch.equal(_bits(c.logits()), _bits(want))


def _run_server(cls, N, tmp, batched, **kw):
    import copy
    from distributed_learning_simulator_amd.trainer import Inferencer
    # 500 images labelled by the clients' common base model (seed 0): the base scores
    # 1.0, the noisy clients and their coalitions anything below, the tester's own
    # initial model (seed 1, the empty coalition) something else again
    X = _data(9)[0][:500]
    with torch.no_grad():
        y = _model(0)(X).argmax(1)
    tester = Inferencer(copy.deepcopy(_model(1)).to(dev), (X, y), device=dev)
    if not batched:
        tester.supports_correct_many = lambda layout: False
    calls = []
    many = tester.correct_many
    tester.correct_many = lambda rows, layout: (calls.append(rows.shape[0]), many(rows, layout))[1]
    server = cls(tester=tester, worker_number=N, synchronous=True, **kw)
    base = dict(_model(0).named_parameters())
    g = torch.Generator().manual_seed(77)
    for i in range(N):
        d = {k: (v.detach() + 0.02 * (i + 1) * torch.randn(v.shape, generator=g))
             for k, v in base.items()}
        server.worker_data_queue.add_task((i, 100 + 10 * i, d))
    for w in range(2 * N):
        server.worker_data_queue.get_result(consumer=w % N)
    return server, calls


def test_multiround_server_same_results_on_the_batched_path(tmp_path):
    from distributed_learning_simulator_amd.servers.multiround_shapley_value_server import \
        MultiRoundShapleyValueServer
    out = []
    for batched in (True, False):
        d = tmp_path / str(batched)
        d.mkdir()
        server, calls = _run_server(MultiRoundShapleyValueServer, 4, d, batched,
                                    metric_dir=str(d))
        assert bool(calls) == batched
        out.append((server, (d / "metric_1").read_bytes()))
    (a, pa), (b, pb) = out
    metrics = pickle.loads(pa)
    assert len(metrics) == 16 and len(set(metrics.values())) > 1, metrics
    assert metrics == pickle.loads(pb) and pa == pb
    assert a.evaluated_subsets == b.evaluated_subsets and len(a.evaluated_subsets) == 16
    assert a.shapley_values == b.shapley_values
    assert a.tester.accuracy_metric.value == b.tester.accuracy_metric.value


def test_gtg_server_same_results_on_the_batched_path(tmp_path):
    from distributed_learning_simulator_amd.servers.GTG_shapley_value_server import \
        GTGShapleyValueServer
    out = []
    for batched in (True, False):
        np.random.seed(3)
        server, calls = _run_server(GTGShapleyValueServer, 5, tmp_path, batched)
        assert bool(calls) == batched
        out.append(server)
    a, b = out
    assert a.evaluated_subsets == b.evaluated_subsets and a.evaluated_subsets
    assert a.shapley_values == b.shapley_values
    assert any(v != 0 for v in a.shapley_values[1].values())


def _lenet_worker(seed, outq):
    torch.cuda.set_device(0)
    from distributed_learning_simulator_amd.models import LeNet5, synthetic_classification
    from distributed_learning_simulator_amd.trainer import Inferencer
    torch.manual_seed(seed)
    model = LeNet5().to("cuda:0")
    X, y = synthetic_classification(256, (1, 32, 32), seed=11)
    inf = Inferencer(model, (X, y), device=torch.device("cuda", 0))
    assert inf._split_forward() is not None
    lg = inf.logits()
    _, acc, _ = inf.inference()
    outq.put((lg.cpu().numpy(), acc))


def test_lenet_utility_bit_identical_across_processes():
    """Two fresh spawned processes, one after the other, evaluate the same seeded
    LeNet-5 on the same 256 images through the default Inferencer: identical
    logit bits and accuracy."""
    from tests.test_gpu_distributed import _collect
    ctx = mp.get_context("spawn")
    res = []
    for _ in range(2):
        q = ctx.Queue()
        p = ctx.Process(target=_lenet_worker, args=(7, q))
        p.start()
        res.extend(_collect([p], q, 1, 120))
        p.join(60)
        assert p.exitcode == 0
    (la, acc_a), (lb, acc_b) = res
    assert la.shape == (256, 10)
    assert np.array_equal(la.view(np.uint32), lb.view(np.uint32))
    assert acc_a == acc_b
