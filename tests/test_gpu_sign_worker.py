"""GPU: the signSGD device path bit for bit — dls_sign_sgd_direction (momentum buffer,
sign and the packed planes a worker sends), dls_sign_sgd_apply, SignSGDWorker and
SignSGDServer as shipped, and one whole round.  The references are oracle.sign
(C oracle / numpy), checked against torch's CPU ops at these inputs by
tests/test_sign_worker_host.py."""
import threading

import numpy as np
import pytest
import torch

from oracle import sign as osign
from tests import golden as G
from tests import sign_worker_ref as R

pytestmark = pytest.mark.gpu

dev = torch.device("cuda", 0)


def words(t):
    return t.cpu().numpy().view(np.uint64)


def to_dev(a, dtype=None):
    t = torch.from_numpy(np.array(a))  # a C-ordered copy; keeps a 0-d shape
    return (t if dtype is None else t.view(dtype)).to(dev)


# ------------------------------------------------------------ dls_sign_sgd_direction
def run_direction(st, cfg, W, word_off, with_sign_out):
    """One launch on fresh device copies of the step's inputs; returns
    (buf, sign_out, the whole plane buffer) as numpy."""
    from distributed_learning_simulator_amd import _native
    P = st["grad"].size
    grad = to_dev(st["grad"])
    buf = None
    if cfg["momentum"] != 0:
        # on a first step the kernel must not read the buffer: poison it
        buf = torch.full((P,), float("nan"), device=dev) if st["first"] else to_dev(st["buf_in"])
    big = torch.full((word_off + W + 16,), R.FILL, dtype=torch.int64, device=dev)
    sout = torch.full((P,), 7.0, device=dev) if with_sign_out else None
    _native.sign_sgd_direction(grad, buf, cfg["momentum"], 1 - cfg["dampening"], cfg["nesterov"],
                               st["first"], big[word_off:], sout)
    return (None if buf is None else buf.cpu().numpy(),
            None if sout is None else sout.cpu().numpy(), words(big))


@pytest.mark.parametrize("P", R.SIZES)
def test_direction_buffer_sign_and_planes(P):
    from distributed_learning_simulator_amd import _native
    W = _native.sign_words(P)
    nw = 2 * ((P + 63) // 64)  # the words the tensor owns; the rest of its last tile is not its
    fill = np.uint64(0xABABABABABABABAB)
    for ci, cfg in enumerate(R.CONFIGS):
        for s, st in enumerate(R.trajectory(P, ci)):
            tag = (P, ci, s)
            want = osign.pack_planes(st["sign"])
            assert want.size == W
            for word_off, with_sign_out in ((0, True), (0, False), (2, False), (6, True)):
                buf, sout, got = run_direction(st, cfg, W, word_off, with_sign_out)
                if cfg["momentum"] != 0:
                    assert R.same_bits(buf, st["buf"]), tag
                if with_sign_out:
                    assert R.same_bits(sout, st["sign"]), tag
                assert np.all(got[:word_off] == fill), (tag, word_off)  # before the slice
                mine = got[word_off:word_off + nw]
                assert np.array_equal(mine, want[:nw]), (tag, word_off)
                assert np.all(got[word_off + nw:] == fill), (tag, word_off)  # every later word
                # a NaN direction sets neither bit (dls_sign_pack_f32 would set both)
                back = osign.unpack_planes(mine, P)
                assert not np.isnan(back).any() and np.all(back[np.isnan(st["d"])] == 0), tag
                assert R.same_bits(back, st["sign"]), tag


def test_direction_rejects_misaligned_and_strided_inputs():
    from distributed_learning_simulator_amd import _native
    planes = torch.zeros(_native.sign_words(64), dtype=torch.int64, device=dev)
    g = torch.zeros(65, device=dev)
    with pytest.raises(RuntimeError):
        _native.sign_sgd_direction(g[1:], None, 0.0, 1.0, False, False, planes)  # 4-byte aligned
    with pytest.raises(RuntimeError):
        _native.sign_sgd_direction(torch.zeros(8, 8, device=dev).t(), None, 0.0, 1.0, False, False,
                                   planes)
    with pytest.raises(RuntimeError):
        _native.sign_sgd_direction(torch.zeros(64, device=dev), torch.zeros(8, 8, device=dev).t(),
                                   0.9, 1.0, False, False, planes)


# ---------------------------------------------------------------- dls_sign_sgd_apply
@pytest.mark.parametrize("P", R.SIZES)
def test_apply_vote_planes(P):
    from distributed_learning_simulator_amd import _native
    p0 = R.edge_vector(P, seed=(P, 77))
    vote, planes = R.ternary_vote(P, seed=P, nan_code_at=sorted({0, P // 2, P - 1}))
    assert planes.size == _native.sign_words(P)
    for wd in (0.0, 1e-4, 5e-4):
        for lr in (0.01, 0.1):
            want = osign.worker_apply(p0, vote, lr, wd)  # the NaN-coded votes as 0.0
            for word_off in (0, 2):
                # the parameter at a 4-byte-aligned address inside a larger buffer
                big = torch.full((P + 2,), 12345.0, device=dev)
                big[1:1 + P] = to_dev(p0)
                vbuf = torch.full((word_off + planes.size,), R.FILL, dtype=torch.int64, device=dev)
                vbuf[word_off:] = to_dev(planes, torch.int64)
                _native.sign_sgd_apply(big[1:1 + P], vbuf[word_off:], -lr, wd)
                got = big.cpu().numpy()
                assert got[0] == 12345.0 and got[-1] == 12345.0, (P, wd, lr)
                assert R.same_bits(got[1:1 + P], want), (P, wd, lr, word_off)


def test_apply_rejects_memory_not_in_logical_order():
    """A silently permuted update was the bug: dls_sign_sgd_apply walks memory, so a
    parameter whose memory is not in logical order is rejected (SignSGDWorker steps a
    contiguous copy and writes it back)."""
    from distributed_learning_simulator_amd import _native
    w = torch.zeros(8, 4, 3, 3, device=dev).to(memory_format=torch.channels_last)
    vote = torch.zeros(_native.sign_words(w.numel()), dtype=torch.int64, device=dev)
    with pytest.raises(RuntimeError, match="contiguous"):
        _native.sign_sgd_apply(w, vote, -0.1, 0.0)
    with pytest.raises(RuntimeError, match="contiguous"):
        _native.sign_sgd_apply(torch.zeros(8, 8, device=dev).t(), vote, -0.1, 0.0)
    with pytest.raises(RuntimeError):  # too few vote words for the parameter
        _native.sign_sgd_apply(torch.zeros(65, device=dev), vote[:2], -0.1, 0.0)


# ------------------------------------------------------------------- SignSGDWorker
class StubTrainer:
    def __init__(self, optimizer):
        self.optimizer = optimizer
        self.callbacks = {}

    def get_optimizer(self):
        return self.optimizer

    def add_named_callback(self, point, name, fn):
        self.callbacks[name] = fn


class StubQueue:
    """Records add_task; answers get_result with the packed vote ``reply(task)``."""

    def __init__(self, reply):
        self.sent = []
        self.reply = reply

    def add_task(self, task):
        self.sent.append(task)

    def get_result(self):
        return self.reply(self.sent[-1])


WORKER_SHAPES = ((8, 3, 3, 3), (7,), (1,), (), (64,), (300, 70), (10, 72))
WORKER_CONFIGS = (
    dict(momentum=0.9, dampening=0.0, nesterov=True, weight_decay=1e-4, lr=0.05),
    dict(momentum=0.0, dampening=0.0, nesterov=False, weight_decay=1e-3, lr=0.01),
)


def numel(shape):
    return int(np.prod(shape)) if shape else 1


def make_worker(params, cfg, queue):
    from distributed_learning_simulator_amd.workers.sign_sgd_worker import SignSGDWorker
    opt = torch.optim.SGD(params, **cfg)
    trainer = StubTrainer(opt)
    SignSGDWorker(worker_id=0, trainer=trainer, worker_data_queue=queue, round=1)
    return opt, trainer.callbacks["sign"]


class OracleWorker:
    """The reference worker's state per tensor, advanced with oracle.sign."""

    def __init__(self, p0, cfg):
        self.p = [np.array(p, np.float32).reshape(-1) for p in p0]
        self.buf = [None] * len(p0)
        self.cfg = cfg

    def direction(self, i, g):
        cfg = self.cfg
        first = cfg["momentum"] != 0 and self.buf[i] is None
        d, b = osign.worker_direction(np.asarray(g, np.float32).reshape(-1), self.buf[i], first,
                                      cfg["momentum"], cfg["dampening"], cfg["nesterov"])
        if cfg["momentum"] != 0:
            self.buf[i] = b
        return osign.worker_sign(d)

    def apply(self, i, vote):
        self.p[i] = osign.worker_apply(self.p[i], vote, self.cfg["lr"], self.cfg["weight_decay"])


def packed_reply(votes):
    """get_result's answer: SignVoteResult with the pack of ``votes`` (one flat array
    per sent tensor) at the offsets of the sent layout."""
    from distributed_learning_simulator_amd.layout import ParameterLayout
    from distributed_learning_simulator_amd.servers.sign_sgd_server import SignVoteResult

    def reply(task):
        layout = ParameterLayout((str(i), s) for i, s in enumerate(task.shapes))
        res = SignVoteResult()
        res.vote_planes = to_dev(osign.pack_planes(R.layout_row(layout, votes)), torch.int64)
        return res
    return reply


@pytest.mark.parametrize("ci", range(len(WORKER_CONFIGS)))
def test_worker_sends_planes_and_steps_like_the_reference(ci):
    from distributed_learning_simulator_amd import _native
    from distributed_learning_simulator_amd.layout import ParameterLayout
    from distributed_learning_simulator_amd.servers.sign_sgd_server import PackedSigns
    cfg = WORKER_CONFIGS[ci]
    p0 = [R.edge_vector(numel(s), seed=(ci, i, 1)).reshape(s) for i, s in enumerate(WORKER_SHAPES)]
    params = [torch.nn.Parameter(to_dev(p)) for p in p0]
    queue = StubQueue(None)
    opt, step = make_worker(params, cfg, queue)
    ref = OracleWorker(p0, cfg)
    rng = np.random.default_rng(ci)
    for s in range(3):
        # step 1: one tensor without a gradient, as the golden generator has it; a
        # middle one, so that every later tensor's plane offset moves
        live = [i for i in range(len(params)) if not (s == 1 and i == 1)]
        grads = {i: R.edge_vector(numel(WORKER_SHAPES[i]), seed=(ci, i, s, 2), shift=s + i)
                 for i in live}
        for i, p in enumerate(params):
            p.grad = to_dev(grads[i].reshape(WORKER_SHAPES[i])) if i in grads else None
        signs = [ref.direction(i, grads[i]) for i in live]
        votes = [rng.integers(-1, 2, numel(WORKER_SHAPES[i])).astype(np.float32) for i in live]
        queue.reply = packed_reply(votes)
        step(opt)
        sent = queue.sent[-1]
        assert isinstance(sent, PackedSigns)
        assert sent.shapes == [tuple(WORKER_SHAPES[i]) for i in live]
        layout = ParameterLayout((str(j), WORKER_SHAPES[i]) for j, i in enumerate(live))
        want = osign.pack_planes(R.layout_row(layout, signs))
        assert want.size == _native.sign_words(layout.P)
        assert np.array_equal(words(sent.planes), want), (ci, s)  # word for word, padding zero
        for j, i in enumerate(live):
            ref.apply(i, votes[j])
        for i, p in enumerate(params):
            if cfg["momentum"] != 0 and ref.buf[i] is not None:
                got = opt.state[p]["momentum_buffer"]
                assert got.shape == p.shape
                assert R.same_bits(got.cpu().numpy().reshape(-1), ref.buf[i]), (ci, s, i)
            else:
                assert "momentum_buffer" not in opt.state[p]
            assert R.same_bits(p.detach().cpu().numpy().reshape(-1), ref.p[i]), (ci, s, i)


@pytest.mark.parametrize("grad_channels_last", [False, True])
def test_worker_steps_a_channels_last_weight_in_logical_order(grad_channels_last):
    """A (8, 4, 3, 3) weight whose memory is channels_last (Inferencer's
    model.to(memory_format=...)) takes the reference's step on the logical tensor:
    the worker steps a contiguous copy and writes it back; its momentum buffer is
    kept in logical order."""
    cfg = WORKER_CONFIGS[0]
    shapes = ((8, 4, 3, 3), (5,))
    p0 = [R.edge_vector(numel(s), seed=(9, i)).reshape(s) for i, s in enumerate(shapes)]
    w = to_dev(p0[0]).to(memory_format=torch.channels_last)
    assert not w.is_contiguous() and w.is_contiguous(memory_format=torch.channels_last)
    params = [torch.nn.Parameter(w), torch.nn.Parameter(to_dev(p0[1]))]
    assert not params[0].is_contiguous()
    queue = StubQueue(None)
    opt, step = make_worker(params, cfg, queue)
    ref = OracleWorker(p0, cfg)
    rng = np.random.default_rng(3)
    for s in range(3):
        grads = [R.edge_vector(numel(sh), seed=(9, i, s), shift=s).reshape(sh)
                 for i, sh in enumerate(shapes)]
        for p, g in zip(params, grads):
            p.grad = to_dev(g)
        if grad_channels_last:
            params[0].grad = params[0].grad.to(memory_format=torch.channels_last)
        signs = [ref.direction(i, g) for i, g in enumerate(grads)]
        votes = [rng.integers(-1, 2, numel(sh)).astype(np.float32) for sh in shapes]
        queue.reply = packed_reply(votes)
        step(opt)
        from distributed_learning_simulator_amd.layout import ParameterLayout
        layout = ParameterLayout((str(i), sh) for i, sh in enumerate(shapes))
        assert np.array_equal(words(queue.sent[-1].planes),
                              osign.pack_planes(R.layout_row(layout, signs))), s
        for i, v in enumerate(votes):
            ref.apply(i, v)
        for i, p in enumerate(params):
            buf = opt.state[p]["momentum_buffer"]
            # .cpu().numpy() of the logical tensor: reshape(-1) walks logical order
            assert R.same_bits(buf.cpu().contiguous().numpy().reshape(-1), ref.buf[i]), (s, i)
            assert R.same_bits(p.detach().cpu().contiguous().numpy().reshape(-1), ref.p[i]), (s, i)
        # the parameter keeps its memory format
        assert params[0].is_contiguous(memory_format=torch.channels_last)


# ------------------------------------------------------------------- SignSGDServer
def golden_vote_cases():
    z = G.load("sign_vote.npz")
    return [(c, z[f"{c['key']}_signs"], z[f"{c['key']}_vote"]) for c in G.meta(z)]


def check_broadcast(res, vote_flat, shapes):
    """The broadcast list equals the vote bit for bit, and vote_planes is its pack."""
    from distributed_learning_simulator_amd.layout import ParameterLayout
    assert [tuple(t.shape) for t in res] == [tuple(s) for s in shapes]
    got = np.concatenate([t.cpu().numpy().reshape(-1) for t in res])
    assert R.same_bits(got, vote_flat)
    layout = ParameterLayout((str(i), s) for i, s in enumerate(shapes))
    parts = np.split(np.asarray(vote_flat, np.float32), np.cumsum(layout.numels)[:-1])
    assert np.array_equal(words(res.vote_planes), osign.pack_planes(R.layout_row(layout, parts)))


@pytest.mark.parametrize("packed", [False, True])
def test_server_golden_votes_on_the_gpu(packed):
    """tests/golden/sign_vote.npz through the real SignSGDServer: 128-byte row pitch,
    one-row dls_sign_pack_f32 calls (fp32 lists) or PackedSigns rows, dls_sign_vote."""
    from distributed_learning_simulator_amd import _native
    from distributed_learning_simulator_amd.layout import ParameterLayout
    from distributed_learning_simulator_amd.servers.sign_sgd_server import PackedSigns, SignSGDServer
    for case, S, vote in golden_vote_cases():
        shapes = [tuple(s) for _, s in case["layout"]]
        layout = ParameterLayout((str(i), s) for i, s in enumerate(shapes))
        server = SignSGDServer(tester=None, worker_number=case["K"], synchronous=True, device=dev)
        for k in range(case["K"]):
            tensors = list(G.split(S[k], case["layout"]).values())
            if packed:
                planes = osign.pack_planes(R.layout_row(layout, tensors))
                server.worker_data_queue.add_task(PackedSigns(to_dev(planes, torch.int64), shapes))
            else:  # CPU fp32 tensors, as the reference worker sends them
                server.worker_data_queue.add_task([torch.from_numpy(t.copy()) for t in tensors])
        res = server.worker_data_queue.get_result(consumer=0)
        check_broadcast(res, vote, shapes)
        assert server._planes.stride(0) == _native.sign_row_pitch(layout.P)
        assert server._planes.stride(0) % 16 == 0
        server.stop()


def client_lists(S, shapes):
    out, off = [], 0
    for s in shapes:
        n = numel(s)
        out.append(torch.from_numpy(S[off:off + n].reshape(s).copy()))
        off += n
    return out


def test_server_nonternary_resets_and_tensor_list_may_change():
    from distributed_learning_simulator_amd.servers.sign_sgd_server import SignSGDServer
    shapes = [(8, 3, 3, 3), (7,), (300,), (1,)]
    n = sum(numel(s) for s in shapes)
    K = 3
    rng = np.random.default_rng(5)
    server = SignSGDServer(tester=None, worker_number=K, synchronous=True, device=dev)
    q = server.worker_data_queue

    def vote_of(S, shp):
        for k in range(K):
            q.add_task(client_lists(S[k], shp))
        return q.get_result(consumer=0)

    S = rng.integers(-1, 2, (K, n)).astype(np.float32)
    check_broadcast(vote_of(S, shapes), osign.majority_vote(S), shapes)
    # a nonternary client: the completing add_task raises, and the next vote is clean
    bad = S.copy()
    bad[1, 5] = 0.5
    with pytest.raises(ValueError, match="outside"):
        vote_of(bad, shapes)
    S2 = rng.integers(-1, 2, (K, n)).astype(np.float32)
    check_broadcast(vote_of(S2, shapes), osign.majority_vote(S2), shapes)
    # a vote with another tensor list (one tensor had no gradient on this step; all
    # clients agree) is legal in the reference, which keeps no layout
    dropped = [shapes[0]] + shapes[2:]
    n3 = sum(numel(s) for s in dropped)
    S3 = rng.integers(-1, 2, (K, n3)).astype(np.float32)
    check_broadcast(vote_of(S3, dropped), osign.majority_vote(S3), dropped)
    # ... and back
    S4 = rng.integers(-1, 2, (K, n)).astype(np.float32)
    check_broadcast(vote_of(S4, shapes), osign.majority_vote(S4), shapes)
    # a client that disagrees within a vote still raises
    q.add_task(client_lists(S4[0], shapes))
    with pytest.raises(ValueError, match="differ"):
        q.add_task(client_lists(S3[1], dropped))
    # the broken vote is dropped; the next complete one is correct
    check_broadcast(vote_of(S2, shapes), osign.majority_vote(S2), shapes)
    server.stop()


# ------------------------------------------------------------------ one whole round
def test_one_round_three_workers_against_the_server():
    """Three worker threads against the real server's queue, wired as simulator.run
    wires them; after one optimizer step every parameter is the reference's step with
    the majority vote of the three oracles' signs."""
    from distributed_learning_simulator_amd.servers.sign_sgd_server import SignSGDServer
    cfg = WORKER_CONFIGS[0]
    K = 3
    shapes = WORKER_SHAPES
    p0 = [R.edge_vector(numel(s), seed=(21, i)).reshape(s) for i, s in enumerate(shapes)]
    grads = [[R.edge_vector(numel(s), seed=(21, k, i), shift=k + i).reshape(s)
              for i, s in enumerate(shapes)] for k in range(K)]
    server = SignSGDServer(tester=None, worker_number=K, device=dev)
    params = [[torch.nn.Parameter(to_dev(p)) for p in p0] for _ in range(K)]
    errors = []

    def create_worker_and_train(k):
        try:
            torch.cuda.set_device(dev)
            opt, step = make_worker(params[k], cfg, server.worker_data_queue)
            for p, g in zip(params[k], grads[k]):
                p.grad = to_dev(g)
            step(opt)
            torch.cuda.synchronize()
        except BaseException as e:
            errors.append(e)
            raise

    threads = [threading.Thread(target=create_worker_and_train, args=(k,), daemon=True)
               for k in range(K)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(120)
    server.stop()
    assert not errors, errors
    assert not any(t.is_alive() for t in threads)
    refs = [OracleWorker(p0, cfg) for _ in range(K)]
    for i, s in enumerate(shapes):
        signs = np.stack([refs[k].direction(i, grads[k][i]) for k in range(K)])
        vote = osign.majority_vote(signs)
        want = osign.worker_apply(p0[i].reshape(-1), vote, cfg["lr"], cfg["weight_decay"])
        for k in range(K):
            assert R.same_bits(params[k][i].detach().cpu().numpy().reshape(-1), want), (i, k)
