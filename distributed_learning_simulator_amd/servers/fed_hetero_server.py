"""Width-heterogeneous FedAvg server: HeteroFL (Diao, Ding & Tarokh 2021) and FedRolex (Alam,
Liu, Yan & Zhang 2022).

Every worker trains the model at its own width ratio (``widths`` is dealt to the workers
round-robin by id).  The server keeps the full-width model as one flat row.  Its downlink is a
``HeteroBroadcast``: one ``dls_hetero_extract_f32`` launch makes the compact row of every width
level and each worker takes its level's parameter dict, views of that row.  The uplink is a
``HeteroUpdate``, the worker's flat compact row, copied on arrival into the worker's place in
one ragged buffer; when all K have arrived one ``dls_hetero_fedavg_f32`` launch averages every
coordinate over the clients that hold it, in worker-id order, weighted by their sample counts
(a coordinate nobody holds keeps its value).  With ``rolling`` the window of every channel
group then moves on by one (shift = round mod C, FedRolex); without, the windows are prefixes
(HeteroFL).  The full-width model is evaluated with the tester as in ``FedServer``.

Only ``named_parameters`` travel, as in ``fed``: batch-norm running statistics stay local and
HeteroFL's Scaler, static batch norm and masked cross-entropy are not part of this server.
"""
import logging
import math

import torch

from .. import _native
from ..hetero import MAX_K, HeteroPlan, check_width
from ..task_queue import RepeatedResult
from .fed_server import FedServer
from .server import Server

log = logging.getLogger("distributed_learning_simulator_amd")


class HeteroUpdate:
    """A client's uplink payload: its ``width`` ratio and ``row``, its parameters flat in its
    own ``ParameterLayout`` (fp32 [P_level])."""

    __slots__ = ("width", "row")

    def __init__(self, width, row):
        self.width, self.row = float(width), row


class HeteroBroadcast:
    """The server's downlink: {width ratio: parameter dict of that level}, views of one row."""

    __slots__ = ("models",)

    def __init__(self, models):
        self.models = models

    def for_width(self, width):
        if float(width) not in self.models:
            raise ValueError(f"width {width!r} is not one of the server's levels "
                             f"{sorted(self.models, reverse=True)}")
        return self.models[float(width)]


def worker_width(widths, worker_id):
    """The width ratio of worker ``worker_id``: ``widths`` dealt round-robin by id."""
    return float(widths[worker_id % len(widths)])


class FedHeteroServer(Server):
    """``widths``: the width ratios dealt to the workers round-robin by id (their distinct
    values are the plan's levels, at most ``hetero.MAX_LEVELS``); ``rolling``: FedRolex's
    rolling windows instead of HeteroFL's prefixes; ``views``: the global model's
    ``hetero.SliceView``s (default: the tester model's ``hetero_views()``); ``initial_model``:
    the full-width parameter dict the first round starts from (default: the tester's model).
    Any FedServer option other than ``aggregation_mode="exact"`` raises ``ValueError``:
    combining the widths with the robust rules, the attacks, the server optimizers or DP is
    out of scope here."""

    get_metric = FedServer.get_metric

    def __init__(self, widths=(1.0,), rolling=False, views=None, initial_model=None,
                 aggregation_mode="exact", **kwargs):
        base = {k: kwargs.pop(k) for k in ("tester", "worker_number", "multi_process", "device",
                                           "synchronous") if k in kwargs}
        if aggregation_mode != "exact" or kwargs:
            raise ValueError("FedHeteroServer has one arithmetic (aggregation_mode='exact') and "
                             "does not support " + ", ".join(
                                 [f"aggregation_mode={aggregation_mode!r}"] * (aggregation_mode != "exact")
                                 + sorted(kwargs)) + ": one fused launch averages every "
                             "coordinate over the clients that hold it")
        try:
            widths = tuple(check_width(w) for w in widths)
        except TypeError:
            raise ValueError(f"widths must be a sequence of width ratios, not {widths!r}")
        if not widths:
            raise ValueError("widths must name at least one width ratio")
        workers, tester = base.get("worker_number"), base.get("tester")
        if isinstance(workers, bool) or not isinstance(workers, int) or not 1 <= workers <= MAX_K:
            raise ValueError(f"FedHeteroServer takes 1..MAX_K={MAX_K} clients, not "
                             f"worker_number={workers!r}")
        if views is None:
            if tester is None or not hasattr(tester.model, "hetero_views"):
                raise ValueError("FedHeteroServer needs the model's slice views: views=, or a "
                                 "tester whose model has hetero_views()")
            views = tester.model.hetero_views()
        if tester is None and not initial_model:
            raise ValueError("FedHeteroServer needs a full-width model to start from: a tester "
                             "or initial_model=")
        self.widths, self.rolling = widths, bool(rolling)
        self.plan = HeteroPlan(views, tuple(dict.fromkeys(widths)))  # > MAX_LEVELS: ValueError
        super().__init__(**base)
        if initial_model is None:
            initial_model = dict(tester.model.named_parameters())
        if not self.plan.layout.matches(initial_model):
            raise ValueError("FedHeteroServer: the initial model's names and shapes are not the "
                             "slice views'")
        self.round = 0
        self.flat = self.plan.layout.flatten(
            {k: v.detach() for k, v in initial_model.items()}, device=self.device)
        # worker id -> its level and the start of its row in the ragged buffer
        self._levels = [self.plan.level_of(worker_width(widths, w)) for w in range(workers)]
        self._starts, at = [], 0
        for lvl in self._levels:
            self._starts.append(at)
            at += self.plan.level_P[lvl]
        self._ragged = torch.zeros(at, dtype=torch.float32, device=self.device)
        self._counts = {}  # worker id -> sample count, of the round's arrivals
        self.worker_data_queue.put_result(
            RepeatedResult(data=self._broadcast(), num=self.worker_number))

    @property
    def clients_per_round(self):
        return self.worker_number

    @property
    def prev_model(self):
        """The full-width global model, views of the flat row."""
        return self.plan.layout.views(self.flat)

    def _broadcast(self):
        """One extract launch: every level's parameter dict as views of its compact row."""
        rows = _native.hetero_extract(self.plan, self.flat)
        return HeteroBroadcast({w: lay.views(row) for w, lay, row in
                                zip(self.plan.widths, self.plan.level_layouts, rows)})

    def _check_payload(self, worker_id, size, payload):
        who = f"worker {worker_id}"
        if isinstance(worker_id, bool) or not isinstance(worker_id, int) \
                or not 0 <= worker_id < self.worker_number:
            raise ValueError(f"{who}: not a worker id in 0..{self.worker_number - 1}")
        if not isinstance(payload, HeteroUpdate):
            raise ValueError(f"{who}: the payload must be a HeteroUpdate, not "
                             f"{type(payload).__name__}")
        lvl = self._levels[worker_id]
        if payload.width != self.plan.widths[lvl]:
            raise ValueError(f"{who}: sent width {payload.width}, the server dealt it "
                             f"{self.plan.widths[lvl]}")
        row, P = payload.row, self.plan.level_P[lvl]
        if not torch.is_tensor(row) or row.dtype != torch.float32 or row.dim() != 1:
            raise ValueError(f"{who}: the row must be an fp32 vector")
        if row.numel() != P:
            raise ValueError(f"{who}: the row has {row.numel()} elements, level {lvl} (width "
                             f"{payload.width}) has P={P}")
        if isinstance(size, bool) or not isinstance(size, (int, float)) \
                or not math.isfinite(_native.fl32(size)) or not _native.fl32(size) > 0.0:
            raise ValueError(f"{who}: the sample count {size!r} must be finite and > 0 in fp32")

    def _process_worker_data(self, data, __):
        worker_id, size, payload = data
        self._check_payload(worker_id, size, payload)
        start = self._starts[worker_id]
        self._ragged[start:start + payload.row.numel()].copy_(payload.row)
        self._counts[worker_id] = size
        if len(self._counts) != self.worker_number:
            log.debug("%s %s,skip", len(self._counts), self.worker_number)
            return None
        log.info("begin aggregating")
        ids = sorted(self._counts)
        _native.hetero_fedavg(self.plan, [self._levels[w] for w in ids],
                              [self._starts[w] for w in ids], [self._counts[w] for w in ids],
                              self._ragged, self.flat)
        self.round += 1
        if self.rolling:  # FedRolex: shift = round mod C for every channel group
            self.plan.set_shifts({g: self.round for g in self.plan.groups})
        acc = self.get_metric(self.prev_model)
        log.info("end aggregating, test accuracy is %s", acc)
        self._counts.clear()
        return RepeatedResult(data=self._broadcast(), num=self.worker_number)
