"""SCAFFOLD / FedProx server (Karimireddy et al. 2020, "SCAFFOLD: stochastic controlled
averaging for federated learning").

Client payloads are ``ScaffoldUpdate(delta, steps, lr)``: the dense difference of a client's
local model to the model this server broadcast, and how many optimizer steps of which
learning rate made it.  With the paper's option II a client's control variate changes by
-c - delta / (steps * lr), a function of delta and the server control variate c alone, so
the uplink is one row, not two.  When all K have arrived one
``dls_scaffold_server_step_f32`` launch reads every row once, in arrival order, and makes
both the new model, x += global_lr * FedAvg(delta), and the new control variate, c +=
sum_k (-c - delta_k / (steps_k * lr_k)) / N with N = ``worker_number``.  The downlink is a
``ScaffoldBroadcast`` of the model and c; the rest of the round is FedServer's.

``control=False`` keeps no control variate: with workers of ``mu > 0`` that is FedProx.
"""
import copy
import logging
import math

import torch

from .. import _native
from ..layout import ParameterLayout
from ..task_queue import RepeatedResult
from ..workers.fed_scaffold_worker import ScaffoldBroadcast, ScaffoldUpdate
from .fed_server import FedServer

log = logging.getLogger("distributed_learning_simulator_amd")


class FedScaffoldServer(FedServer):
    """``global_lr``: the server's step on the averaged delta (1.0: the average becomes the
    model); ``control``: SCAFFOLD's control variates on or off, as the workers were told.
    ``initial_model``: the parameter dict the first round starts from (default: the
    tester's model); one of ``tester`` and ``initial_model`` is needed, because the workers'
    updates are differences to the broadcast model.

    ``aggregation_rule`` other than "mean", ``attack``, ``server_optimizer`` and ``dp_clip`` raise
    ``ValueError``: composing the control variates with them is out of scope here."""

    _robust_unsupported = "its one fused step averages the deltas and moves the control variate"
    _attack_unsupported = "its one fused step averages the deltas and moves the control variate"
    _server_opt_unsupported = "its one fused step averages the deltas and moves the control variate"
    _dp_unsupported = "its one fused step averages the deltas and moves the control variate"

    def __init__(self, global_lr=1.0, control=True, initial_model=None, **kwargs):
        if kwargs.get("tester") is None and not initial_model:
            raise ValueError("FedScaffoldServer needs a model to start from, a tester or "
                             "initial_model=: the workers' updates are differences to the "
                             "broadcast model")
        if kwargs.get("aggregation_mode", "exact") != "exact":
            raise ValueError("FedScaffoldServer has one arithmetic (aggregation_mode='exact'), not "
                             f"{kwargs['aggregation_mode']!r}")
        if isinstance(global_lr, bool) or not isinstance(global_lr, (int, float)) \
                or not math.isfinite(global_lr) or global_lr <= 0:
            raise ValueError(f"FedScaffoldServer: global_lr={global_lr!r} must be a positive "
                             "finite number")
        workers = kwargs.get("worker_number")
        if workers is not None and not 1 <= workers <= _native.SCAFFOLD_MAX_K:
            raise ValueError(f"FedScaffoldServer takes 1..SCAFFOLD_MAX_K={_native.SCAFFOLD_MAX_K} "
                             f"clients, not worker_number={workers}")
        self.global_lr, self.use_control = float(global_lr), bool(control)
        self.__initial = initial_model
        self._payloads = {}  # worker id -> (n, ScaffoldUpdate), in arrival order
        super().__init__(**kwargs)
        self.layout = ParameterLayout.from_dict(self.prev_model)
        self.control = torch.zeros(self.layout.P, dtype=torch.float32, device=self.device) \
            if self.use_control else None

    def _initial_model(self):
        if self.__initial:
            return {k: v.detach().clone().to(self.device) for k, v in self.__initial.items()}
        return super()._initial_model()

    def _check_payload(self, worker_id, payload):
        who = f"worker {worker_id}"
        if not isinstance(payload, ScaffoldUpdate):
            raise ValueError(f"{who}: the payload must be a ScaffoldUpdate, not "
                             f"{type(payload).__name__}")
        P, delta = self.layout.P, payload.delta
        if not torch.is_tensor(delta) or delta.dtype != torch.float32 or delta.dim() != 1:
            raise ValueError(f"{who}: delta must be an fp32 vector")
        if delta.numel() != P:
            raise ValueError(f"{who}: the payload is over rows of P={delta.numel()} elements, the "
                             f"server's model has P={P}")
        if payload.steps < 1 or not math.isfinite(payload.lr) or payload.lr <= 0:
            raise ValueError(f"{who}: steps={payload.steps} and lr={payload.lr} must be positive")
        return payload

    def _process_worker_data(self, data, __):
        worker_id, training_dataset_size, payload = data
        self._payloads[worker_id] = (training_dataset_size, self._check_payload(worker_id, payload))
        if len(self._payloads) != self.clients_per_round:
            log.debug("%s %s,skip", len(self._payloads), self.clients_per_round)
            return None
        log.info("begin aggregating")
        dev, P, N = self.device, self.layout.P, self.worker_number
        ns = [int(n) for n, _ in self._payloads.values()]
        ups = [u for _, u in self._payloads.values()]
        K = len(ups)
        U = torch.stack([u.delta.to(dev) for u in ups])
        rows = torch.arange(K, dtype=torch.int32, device=dev)
        weight = torch.tensor(ns, dtype=torch.float32).to(dev)
        b = torch.tensor([_native.scaffold_coeff(u.steps, u.lr, N) for u in ups],
                         dtype=torch.float32).to(dev) if self.use_control else None
        x = self.layout.flatten(self.prev_model, device=dev)
        _native.scaffold_server_step(U, rows, weight, b, float(sum(ns)), P, self.global_lr,
                                     float(K) / float(N), x, self.control)
        model = self._process_aggregated_parameter(self.layout.views(x))
        self.round += 1
        self._set_prev_model(copy.deepcopy(model))
        acc = self.get_metric(self.prev_model)
        log.info("end aggregating, test accuracy is %s", acc)
        self._payloads.clear()
        data = ScaffoldBroadcast(model, self.control.clone() if self.use_control else None)
        return RepeatedResult(data=data, num=self.clients_per_round)
