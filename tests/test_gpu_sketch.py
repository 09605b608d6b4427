"""GPU: dls_sketch_f32 and dls_unsketch_f32 against tests/sketch_ref.py, bit for bit (in the
sketch a NaN equals any NaN: which one arithmetic gives is not in the contract; the inverse
moves bits, payloads included); FedSketchWorker and FedSketchServer on the device."""
import ctypes

import numpy as np
import pytest
import torch

from tests import sketch_ref as ref
from tests.sketch_ref import bits
from tests.test_topk_host import FakeTrainer, initial_model, make_model

pytestmark = pytest.mark.gpu

F32 = np.float32
SEED, STREAM = 0x1234567890ABCDEF, 3
SHAPES = [(64, 1, 1024),                 # a single partial block
          (33 * 1024 + 4, 3, 1024),      # one tile, segment boundary at q = 32, ragged tail
          (65 * 4096 + 1028, 5, 4096),   # high mask bits select tiles, three segments
          (3 * 2048, 7, 2048)]           # the maximum R
# 1280 tiles: two segments walked by one workgroup, not spread through the workspace
ONE_PASS = (33 * (1 << 18) + 4, 5, 1 << 18)


def _dev():
    return torch.device("cuda", 0)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


def same(got, want):
    return bool(np.all((bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))))


def run_sketch(w, base, P, R, C, stream=None):
    from distributed_learning_simulator_amd import _native
    buf = torch.full((R * C + 64,), 7.0, device=_dev())
    stats = torch.full((4,), -1, dtype=torch.int32, device=_dev())
    ws = _native.sketch_workspace(P, R, C, _dev())
    tw, tb = _t(w), None if base is None else _t(base)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream or torch.cuda.current_stream()):
        _native.sketch(tw, tb, P, R, C, SEED, STREAM, buf[:R * C].view(R, C), stats, ws,
                       stream=stream)
    torch.cuda.synchronize()
    assert bool((buf[R * C:] == 7.0).all()) and stats[1:].tolist() == [-1] * 3  # the canaries
    return buf[:R * C].view(R, C).cpu().numpy(), int(stats[0])


@pytest.mark.parametrize("with_base", [False, True])
@pytest.mark.parametrize("P,R,C", SHAPES + [ONE_PASS])
def test_sketch(P, R, C, with_base):
    """Random normal rows; then planted inf / NaN are counted once, not once per row, and the
    table is still the reference's; a second HIP stream gives the same bits."""
    rng = np.random.default_rng(P + R)
    w = rng.standard_normal(P).astype(F32)
    base = rng.standard_normal(P).astype(F32) if with_base else None
    want, bad = ref.sketch(w, base, P, R, C, SEED, STREAM)
    got = run_sketch(w, base, P, R, C)
    assert same(got[0], want) and got[1] == bad == 0
    if (P, R, C) == ONE_PASS:
        return
    again = run_sketch(w, base, P, R, C, stream=torch.cuda.Stream(_dev()))
    assert np.array_equal(bits(again[0]), bits(got[0])) and again[1] == 0
    w[0], w[P // 2], w[P - 1] = np.inf, -np.inf, np.nan
    if with_base:
        base[P - 1], base[1] = np.inf, np.nan
    want, bad = ref.sketch(w, base, P, R, C, SEED, STREAM)
    got = run_sketch(w, base, P, R, C)
    assert same(got[0], want) and got[1] == bad == 3 + with_base


@pytest.mark.parametrize("P,R,C", SHAPES)
def test_unsketch(P, R, C):
    """Tables of +-0, +-inf, NaNs of both signs and few distinct values, so that ranks tie."""
    from distributed_learning_simulator_amd import _native
    rng = np.random.default_rng(P * R)
    special = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00001, 0xFFC00002,
                        0x3F800000, 0xBF800000, 0x40200000, 0x00000001, 0x80000001], np.uint32)
    T = rng.choice(np.concatenate([special, bits(rng.standard_normal(5).astype(F32))]), (R, C))
    est = torch.full((P + 64,), 7.0, device=_dev())
    _native.unsketch(_t(T.view(F32)), P, R, C, SEED, STREAM, est)
    est = est.cpu().numpy()
    assert np.array_equal(bits(est[:P]), bits(ref.unsketch(T.view(F32), P, R, C, SEED, STREAM)))
    assert np.all(est[P:] == 7.0)


REFUSALS = [  # the operand, then the status and the message
    ({"w": None}, -1, "null pointer"), ({"table": None}, -1, "null pointer"),
    ({"stats": None}, -1, "null pointer"), ({"ws": None}, -1, "null pointer"),
    ({"R": 0}, -1, "R=0"), ({"R": 4}, -1, "R=4"), ({"R": 9}, -1, "R=9"), ({"C": 512}, -1, "C=512"),
    ({"C": 1536}, -1, "C=1536"), ({"C": 1 << 25}, -1, "C="), ({"P": 0}, -1, "P=0"),
    ({"P": 1 << 31}, -1, "P="), ({"P": 126}, -2, "multiple of 4"), ({"w": "off"}, -2, "alignment"),
    ({"base": "off"}, -2, "alignment"), ({"table": "off"}, -2, "alignment"),
    ({"table": "w"}, -1, "alias"), ({"stats": "base"}, -1, "alias"), ({"ws": "w"}, -1, "alias"),
    ({"ws": "table"}, -1, "alias")]


@pytest.mark.parametrize("change,status,message", REFUSALS)
def test_refusals(change, status, message):
    """Both entry points refuse the operand with the documented status; nothing is written."""
    from distributed_learning_simulator_amd import _native
    L, dev, u64 = _native.lib(), _dev(), ctypes.c_uint64
    t = {"w": torch.zeros(128, device=dev), "base": torch.zeros(128, device=dev),
         "table": torch.full((1024,), 5.0, device=dev), "ws": torch.full((8,), 5.0, device=dev),
         "stats": torch.full((4,), 5, dtype=torch.int32, device=dev)}
    t["off"] = t["table"][1:]
    a = {"P": 128, "R": 1, "C": 1024, **{k: k for k in ("w", "base", "table", "stats", "ws")}, **change}
    p = {k: None if a[k] is None else ctypes.c_void_p(t[a[k]].data_ptr())
         for k in ("w", "base", "table", "stats", "ws")}
    assert L.dls_sketch_f32(p["w"], p["base"], a["P"], a["R"], a["C"], u64(0), u64(1), p["table"],
                            p["stats"], p["ws"], None) == status
    assert message in L.dls_last_error().decode()
    if not {"base", "stats", "ws"} & set(change):  # unsketch: w plays est
        assert L.dls_unsketch_f32(p["table"], a["P"], a["R"], a["C"], u64(0), u64(1), p["w"],
                                  None) == status
        assert message in L.dls_last_error().decode()
    torch.cuda.synchronize()
    assert not t["w"].any() and not t["base"].any() and bool((t["table"] == 5.0).all())
    assert bool((t["ws"] == 5.0).all()) and t["stats"].tolist() == [5] * 4


def _pair(model0, **options):
    from distributed_learning_simulator_amd.servers.fed_sketch_server import FedSketchServer
    from distributed_learning_simulator_amd.workers.fed_sketch_worker import FedSketchWorker
    K = options.pop("K")
    table = {name: options[name] for name in ("rows", "cols", "seed", "stream_id")}
    server = FedSketchServer(initial_model=model0, tester=None, worker_number=K, synchronous=True,
                             device=_dev(), **options)
    workers = [FedSketchWorker(worker_id=i, trainer=FakeTrainer(make_model(10 + i).to(_dev()), 100),
                               worker_data_queue=server.worker_data_queue, round=2, **table)
               for i in range(K)]
    return server, workers


def test_three_workers_two_rounds():
    """Every table and both broadcast models are the reference's; u and v carry over."""
    R, C, k, rho, ns = 3, 1024, 8, 0.9, [300, 120, 777]
    server, workers = _pair(initial_model(), K=3, rows=R, cols=C, k=k, momentum=rho, seed=SEED,
                            stream_id=STREAM)
    for i, wk in enumerate(workers):
        wk.load_model(server.worker_data_queue.get_result(consumer=i))
    lay, dev = server.layout, _dev()
    P = lay.P
    real = np.zeros(P, bool)  # the layout's padding slots may move too, and are dropped
    for a, n in zip(lay.offsets, lay.numels):
        real[a:a + n] = True
    u = v = np.zeros((R, C), F32)
    g = torch.Generator().manual_seed(4)
    for order in ([2, 0, 1], [1, 2, 0]):
        prev = lay.flatten(server.prev_model, device=dev).cpu().numpy()
        sent = {}
        for i in order:
            with torch.no_grad():
                for p in workers[i].trainer.model.parameters():
                    p += (0.05 * torch.randn(p.shape, generator=g)).to(dev)
            w = lay.flatten(dict(workers[i].trainer.model.named_parameters()), device=dev).cpu().numpy()
            sent[i] = ref.sketch(w, prev, P, R, C, SEED, STREAM)[0]
            up = workers[i].sketch_update()
            assert np.array_equal(bits(up.table.cpu().numpy()), bits(sent[i]))
            server.worker_data_queue.add_task((i, ns[i], up))
        u, v, want = ref.server_round(u, v, [sent[i] for i in order], [ns[i] for i in order], prev,
                                      P, R, C, k, rho, SEED, STREAM)
        assert np.array_equal(bits(server.u.cpu().numpy()), bits(u))
        assert np.array_equal(bits(server.v.cpu().numpy()), bits(v))
        for i in order:
            model = server.worker_data_queue.get_result(consumer=i)
            got = lay.flatten(model, device=dev).cpu().numpy()
            assert np.array_equal(bits(got)[real], bits(want)[real]) and not got[~real].any()
            workers[i].load_model(model)
    assert server.round == 2 and server.payload_bytes[0] == {i: 4 * R * C for i in order}
    with torch.no_grad():
        next(workers[0].trainer.model.parameters())[0, 0] = float("inf")
    with pytest.raises(ValueError, match="not finite"):
        workers[0].sketch_update()


def test_recovers_planted_coordinates():
    """P = 65536, R = 5, C = 4096, k = 32, no momentum: N(0, 0.01^2) noise and 32 planted
    coordinates of magnitude 1..2.  After one round the model has moved on exactly those (the
    reference recovers all 32, its worst error on them 0.049: the noise of 15 colliding
    coordinates, |error| <~ 4 sigma sqrt(15) 0.01 = 0.15)."""
    P, rng = 1 << 16, np.random.default_rng(0)
    x = (rng.standard_normal(P) * 0.01).astype(F32)
    planted = rng.choice(P, 32, replace=False)
    x[planted] = (rng.uniform(1, 2, 32) * rng.choice([-1, 1], 32)).astype(F32)
    server, (worker,) = _pair({"weight": torch.zeros(256, 256)}, K=1, rows=5, cols=4096, k=32,
                              momentum=0.0, seed=7, stream_id=3)
    worker.trainer.model = torch.nn.Linear(256, 256, bias=False).to(_dev())
    worker.load_model(server.worker_data_queue.get_result(consumer=0))
    with torch.no_grad():
        worker.trainer.model.weight += _t(x).view(256, 256)
    server.worker_data_queue.add_task((0, 100, worker.sketch_update()))
    moved = server.worker_data_queue.get_result(consumer=0)["weight"].reshape(-1).cpu().numpy()
    assert sorted(np.nonzero(moved)[0]) == sorted(planted)
    assert np.abs(moved[planted] - x[planted]).max() < 0.15
