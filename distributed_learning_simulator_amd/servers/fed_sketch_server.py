"""FetchSGD server (Rothchild et al. 2020, "FetchSGD: Communication-Efficient Federated
Learning with Sketching").

Client payloads are ``SketchUpdate(table, P)``: a Count Sketch, ``rows`` x ``cols`` fp32
buckets, of the client's update, a difference to the model this server broadcast.  The
sketch is linear, so the server never holds a dense client row: it averages the tables and
keeps momentum ``u`` and the error accumulation ``v`` in sketch space, both fp32 [R, C] and
zero at the start.  One round, every step fp32 and rounded once (tests/sketch_ref.py restates
it):

1. ``S`` = ``dls_fedavg_f32`` over the clients' tables as rows of R * C, in arrival order,
   weighted by the sample counts;
2. ``u = fl(fl(momentum * u) + S)``, ``v = fl(v + u)``;
3. ``est = dls_unsketch_f32(v)``, the median-of-rows estimate of every coordinate;
4. the ``k`` coordinates of the largest ``|est|`` by ``dls_topk_compress_f32``'s selection
   rule (ties to the lowest index);
5. the new model = ``dls_sparse_fedavg_f32`` of that one sparse row onto the previous model;
6. ``D = dls_sketch_f32(new model, previous model)``, the sketch of what the model moved by;
7. ``v = fl(v - D)``;
8. ``u = +0.0`` where ``D != 0`` (FetchSGD's momentum masking).

The hash (seed, stream id) is the run's, the same in every round.  The rest of the round is
FedServer's; the downlink stays dense.
"""
import copy
import logging

import torch

from .. import _native
from ..layout import ParameterLayout
from ..task_queue import RepeatedResult
from ..workers.fed_sketch_worker import SketchUpdate, check_sketch_options
from .fed_server import FedServer

log = logging.getLogger("distributed_learning_simulator_amd")


class FedSketchServer(FedServer):
    """``rows``, ``cols``, ``seed``, ``stream_id``: the table's shape and the run's hash, the
    ones the workers were given (``cols`` None: the largest power of two <= P / 32, clamped to
    1024..2^24).  ``k``: the coordinates the model moves on per round (None: ``ratio`` * P, at
    least 1).  ``momentum``: rho of step 2.  ``initial_model``: the parameter dict the first
    round starts from (default: the tester's model); one of ``tester`` and ``initial_model`` is
    needed, because the workers' updates are differences to the broadcast model.

    ``payload_bytes`` holds, per round, the bytes each worker sent.

    ``aggregation_rule`` other than "mean", ``attack``, ``server_optimizer`` and ``dp_clip`` raise
    ``ValueError``: composing the sketch with them is out of scope here."""

    _robust_unsupported = "it holds the clients' Count Sketch tables, not fp32 rows"
    _attack_unsupported = "it holds the clients' Count Sketch tables, not fp32 rows"
    _server_opt_unsupported = "it holds the clients' Count Sketch tables, not fp32 rows"
    _dp_unsupported = "it holds the clients' Count Sketch tables, not fp32 rows"

    def __init__(self, rows=5, cols=None, k=None, ratio=0.01, momentum=0.9, seed=0, stream_id=0,
                 initial_model=None, **kwargs):
        if kwargs.get("tester") is None and not initial_model:
            raise ValueError("FedSketchServer needs a model to start from, a tester or "
                             "initial_model=: the workers' updates are differences to the "
                             "broadcast model")
        if kwargs.get("aggregation_mode", "exact") != "exact":
            raise ValueError("FedSketchServer has one arithmetic (aggregation_mode='exact'), not "
                             f"{kwargs['aggregation_mode']!r}")
        check_sketch_options("FedSketchServer", rows, cols, seed, stream_id)
        if k is not None and (isinstance(k, bool) or not isinstance(k, int) or k < 1):
            raise ValueError(f"FedSketchServer: k={k!r} must be a positive integer")
        if not 0.0 < float(ratio) <= 1.0:
            raise ValueError(f"FedSketchServer: ratio={ratio!r} must lie in (0, 1]")
        if not 0.0 <= float(momentum) < 1.0:
            raise ValueError(f"FedSketchServer: momentum={momentum!r} must lie in [0, 1)")
        self.rows, self.cols, self.seed, self.stream_id = rows, cols, seed, stream_id
        self.momentum = float(momentum)
        self.__initial = initial_model
        self._payloads = {}  # worker id -> (n, SketchUpdate), in arrival order
        self.payload_bytes = []  # per round: worker id -> bytes it sent
        super().__init__(**kwargs)
        self.layout = ParameterLayout.from_dict(self.prev_model)
        P, dev = self.layout.P, self.device
        if self.cols is None:
            self.cols = _native.sketch_default_cols(P)
        self.k = min(P, max(1, int(float(ratio) * P))) if k is None else k
        if self.k > P:
            raise ValueError(f"FedSketchServer: k={k} exceeds the row's P={P} coordinates")
        self.u = torch.zeros((self.rows, self.cols), dtype=torch.float32, device=dev)
        self.v = torch.zeros_like(self.u)
        self._scratch = None

    def _initial_model(self):
        if self.__initial:
            return {k: v.detach().clone().to(self.device) for k, v in self.__initial.items()}
        return super()._initial_model()

    def _check_payload(self, worker_id, payload):
        who = f"worker {worker_id}"
        if not isinstance(payload, SketchUpdate):
            raise ValueError(f"{who}: the payload must be a SketchUpdate, not "
                             f"{type(payload).__name__}")
        if payload.P != self.layout.P:
            raise ValueError(f"{who}: the payload is over rows of P={payload.P} elements, the "
                             f"server's model has P={self.layout.P}")
        table = payload.table
        if not torch.is_tensor(table) or table.dtype != torch.float32 \
                or tuple(table.shape) != (self.rows, self.cols):
            raise ValueError(f"{who}: table must be an fp32 [{self.rows}, {self.cols}] tensor")
        if not bool(torch.isfinite(table).all()):
            raise ValueError(f"{who}: table must be finite")
        return SketchUpdate(table.contiguous().to(self.device), payload.P)

    def _buffers(self):
        """The round's P-sized vectors and workspaces, allocated once."""
        if self._scratch is None:
            P, dev = self.layout.P, self.device
            f32 = dict(dtype=torch.float32, device=dev)
            self._scratch = {
                "est": torch.empty(P, **f32), "zero": torch.zeros(P, **f32),
                "resid": torch.empty(P, **f32), "out": torch.empty(P, **f32),
                "idx": torch.empty(self.k, dtype=torch.int32, device=dev),
                "val": torch.empty(self.k, **f32),
                "stats": torch.empty(4, dtype=torch.int32, device=dev),
                "off": torch.tensor([0, self.k], dtype=torch.int64).to(dev),
                "one": torch.ones(1, **f32),
                "D": torch.empty((self.rows, self.cols), **f32),
                "topk_ws": _native.topk_workspace(P, dev),
                "sketch_ws": _native.sketch_workspace(P, self.rows, self.cols, dev)}
        return self._scratch

    def _sketch_flat(self, ids):
        """Steps 1-8 over the clients ``ids``, in that order: the new model as a flat row."""
        ns = [int(self._payloads[i][0]) for i in ids]
        dev, P, R, C = self.device, self.layout.P, self.rows, self.cols
        b = self._buffers()
        tables = torch.stack([self._payloads[i][1].table for i in ids]).reshape(len(ids), R * C)
        S = torch.empty(R * C, dtype=torch.float32, device=dev)
        _native.fedavg(tables, torch.arange(len(ids), dtype=torch.int32).to(dev),
                       torch.tensor(ns, dtype=torch.float32).to(dev), float(sum(ns)), R * C, S)
        self.u = self.u * self.momentum + S.view(R, C)
        self.v = self.v + self.u
        _native.unsketch(self.v, P, R, C, self.seed, self.stream_id, b["est"])
        b["resid"].zero_()
        _native.topk_compress(b["est"], b["zero"], b["resid"], self.k, P, b["idx"], b["val"],
                              b["stats"], b["topk_ws"])
        prev = self.layout.flatten(self.prev_model, device=dev)
        _native.sparse_fedavg(prev, b["idx"], b["val"], b["off"], b["one"], 1.0, P, b["out"])
        _native.sketch(b["out"], prev, P, R, C, self.seed, self.stream_id, b["D"], b["stats"],
                       b["sketch_ws"])
        self.v = self.v - b["D"]
        self.u = torch.where(b["D"] != 0, torch.zeros_like(self.u), self.u)
        return b["out"].clone()

    def _process_worker_data(self, data, __):
        worker_id, training_dataset_size, payload = data
        self._payloads[worker_id] = (training_dataset_size, self._check_payload(worker_id, payload))
        if len(self._payloads) != self.clients_per_round:
            log.debug("%s %s,skip", len(self._payloads), self.clients_per_round)
            return None
        log.info("begin aggregating")
        self.payload_bytes.append({w: u.nbytes for w, (_, u) in self._payloads.items()})
        sent = sum(u.nbytes for _, u in self._payloads.values())
        dense = 4 * self.layout.numel * len(self._payloads)
        log.info("round %s: uplink %s bytes against %s dense, ratio %s", self.round + 1, sent,
                 dense, float(sent) / float(dense))
        flat = self._sketch_flat(list(self._payloads.keys()))
        data = self._process_aggregated_parameter(self.layout.views(flat))
        self.round += 1
        self._set_prev_model(copy.deepcopy(data))
        acc = self.get_metric(self.prev_model)
        log.info("end aggregating, test accuracy is %s", acc)
        self._payloads.clear()
        return RepeatedResult(data=data, num=self.clients_per_round)

    def get_subset_model(self, client_subset):
        raise RuntimeError("FedSketchServer keeps momentum and the error accumulation across "
                           "rounds: a subset's model is not a function of the round's payloads")
