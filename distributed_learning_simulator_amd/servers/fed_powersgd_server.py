"""Low-rank FedAvg server (Vogels, Karimireddy & Jaggi 2019, "PowerSGD").

Client payloads are ``LowRankUpdate(payload, P, rank)``: per weight matrix the factors P^ and Q
of the client's update, a difference to the model this server broadcast, and the values of the
tensors too small to compress.  The server holds the round's payloads as they are and never a
dense client row; when all have arrived one ``dls_powersgd_fedavg_f32`` launch adds the FedAvg
of the products P^_i Q_i^T, one GEMM per tensor with contraction length K x rank, to the
previous global model and takes the exact FedAvg of the dense tensors.  The rest of the round
is FedServer's; the downlink stays dense.
"""
import copy
import logging

import torch

from .. import _native
from ..layout import ParameterLayout
from ..task_queue import RepeatedResult
from ..workers.fed_powersgd_worker import LowRankUpdate, check_powersgd_options, sent_floats
from .fed_server import FedServer

log = logging.getLogger("distributed_learning_simulator_amd")


class FedPowerSGDServer(FedServer):
    """``rank``: the workers'.  ``initial_model``: the parameter dict the first round starts
    from (default: the tester's model); one of ``tester`` and ``initial_model`` is needed,
    because the workers' updates are differences to the broadcast model.

    ``payload_floats`` holds, per round, the floats each worker sent.

    ``aggregation_rule`` other than "mean", ``attack``, ``server_optimizer`` and ``dp_clip`` raise
    ``ValueError``: composing the low-rank compressor with them is out of scope here."""

    _robust_unsupported = "it holds the clients' low-rank factors, not fp32 rows"
    _attack_unsupported = "it holds the clients' low-rank factors, not fp32 rows"
    _server_opt_unsupported = "it holds the clients' low-rank factors, not fp32 rows"
    _dp_unsupported = "it holds the clients' low-rank factors, not fp32 rows"

    def __init__(self, rank=4, initial_model=None, **kwargs):
        check_powersgd_options("FedPowerSGDServer", rank)
        if kwargs.get("tester") is None and not initial_model:
            raise ValueError("FedPowerSGDServer needs a model to start from, a tester or "
                             "initial_model=: the workers' updates are differences to the "
                             "broadcast model")
        if kwargs.get("aggregation_mode", "exact") != "exact":
            raise ValueError("FedPowerSGDServer has one arithmetic (aggregation_mode='exact'), "
                             f"not {kwargs['aggregation_mode']!r}")
        self.rank = rank
        self.__initial = initial_model
        self._payloads = {}  # worker id -> (n, LowRankUpdate), in arrival order
        self.payload_floats = []  # per round: worker id -> floats it sent
        super().__init__(**kwargs)
        self.layout = ParameterLayout.from_dict(self.prev_model)
        self._plan = None

    def _initial_model(self):
        if self.__initial:
            return {k: v.detach().clone().to(self.device) for k, v in self.__initial.items()}
        return super()._initial_model()

    @property
    def plan(self):
        if self._plan is None:
            self._plan = _native.powersgd_layout_plan(self.layout, self.rank, self.device)
        return self._plan

    def _check_payload(self, worker_id, update):
        who = f"worker {worker_id}"
        if not isinstance(update, LowRankUpdate):
            raise ValueError(f"{who}: the payload must be a LowRankUpdate, not "
                             f"{type(update).__name__}")
        if update.P != self.layout.P or update.rank != self.rank:
            raise ValueError(f"{who}: the payload is over rows of P={update.P} elements at rank "
                             f"{update.rank}, the server's model has P={self.layout.P} at rank "
                             f"{self.rank}")
        payload, L = update.payload, self.plan.L
        if not torch.is_tensor(payload) or payload.dtype != torch.float32 or payload.dim() != 1 \
                or payload.numel() != L:
            raise ValueError(f"{who}: payload must be an fp32 vector of L = {L} elements")
        return LowRankUpdate(payload.contiguous().to(self.device), update.P, update.rank,
                             sent_floats(self.plan))

    def _lowrank_flat(self, ids):
        """prev_model + the low-rank FedAvg of the clients ``ids``, in that order, as a flat row."""
        ns = [int(self._payloads[i][0]) for i in ids]
        dev = self.device
        base = self.layout.flatten(self.prev_model, device=dev)
        out = torch.empty(self.layout.P, dtype=torch.float32, device=dev)
        return _native.powersgd_fedavg(base, torch.stack([self._payloads[i][1].payload for i in ids]),
                                       self.plan, torch.tensor(ns, dtype=torch.float32).to(dev),
                                       float(sum(ns)), out)

    def get_subset_model(self, client_subset):
        """The model the subset's updates alone would have given, in the subset's order
        (empty subset -> previous model)."""
        ids = list(client_subset)
        if not ids:
            return self.prev_model
        missing = [i for i in ids if i not in self._payloads]
        if missing:
            raise ValueError(f"workers {missing} sent no update this round")
        return self.layout.views(self._lowrank_flat(ids))

    def _process_worker_data(self, data, __):
        worker_id, training_dataset_size, update = data
        self._payloads[worker_id] = (training_dataset_size, self._check_payload(worker_id, update))
        if len(self._payloads) != self.clients_per_round:
            log.debug("%s %s,skip", len(self._payloads), self.clients_per_round)
            return None
        self.round += 1
        log.info("begin aggregating")
        self.payload_floats.append({w: u.floats for w, (_, u) in self._payloads.items()})
        sent = sum(u.floats for _, u in self._payloads.values())
        log.info("round %s: uplink %s payload floats per client against P = %s (%s real), ratio %s",
                 self.round, sent // len(self._payloads), self.layout.P, self.layout.numel,
                 float(sent) / float(self.layout.numel * len(self._payloads)))
        data = self._process_aggregated_parameter(self.get_subset_model(self._payloads.keys()))
        self._set_prev_model(copy.deepcopy(data))
        acc = self.get_metric(self.prev_model)
        log.info("end aggregating, test accuracy is %s", acc)
        self._payloads.clear()
        return RepeatedResult(data=data, num=self.clients_per_round)
