"""Multi-bit rotated FedAvg server (Vargaftik et al. 2022, "EDEN: communication-efficient and
robust distributed mean estimation for federated learning").

Client payloads are ``EDENUpdate(codes, scales, P, bits)``: a ``bits``-bit Lloyd-Max code per
rotated coordinate and one fp32 scale per block of 4096 of the client's update, a difference
to the model this server broadcast, under the round's rotation (seed ``seed``, stream id the
round's number, counted from 1: every round gets a fresh rotation and all its clients share
it).  The server holds the round's payloads as they are, NB * 512 * bits + 4 NB bytes per
client and never a dense client row; because the rotation is shared it stays linear: when all
have arrived one ``dls_eden_fedavg_f32`` launch decodes and sums the clients' levels in the
rotated domain in arrival order, rotates back once and adds the result to the previous global
model.  The rest of the round is FedServer's; the downlink stays dense.
"""
import copy
import logging

import torch

from .. import _native
from ..layout import ParameterLayout
from ..task_queue import RepeatedResult
from ..workers.fed_eden_worker import EDENUpdate
from .fed_server import FedServer

log = logging.getLogger("distributed_learning_simulator_amd")


class FedEDENServer(FedServer):
    """``bits``: the width of the workers' codes (2 or 4); a payload of another width is
    refused.  ``seed``: the rotation's, the one the workers were given.  ``initial_model``: the
    parameter dict the first round starts from (default: the tester's model); one of ``tester``
    and ``initial_model`` is needed, because the workers' updates are differences to the
    broadcast model.

    ``payload_bytes`` holds, per round, the bytes each worker sent.

    ``aggregation_rule`` other than "mean", ``attack``, ``server_optimizer`` and ``dp_clip`` raise
    ``ValueError``: composing the rotated compressor with them is out of scope here."""

    _robust_unsupported = "it holds the clients' rotated codes and scales, not fp32 rows"
    _attack_unsupported = "it holds the clients' rotated codes and scales, not fp32 rows"
    _server_opt_unsupported = "it holds the clients' rotated codes and scales, not fp32 rows"
    _dp_unsupported = "it holds the clients' rotated codes and scales, not fp32 rows"

    def __init__(self, bits=4, seed=0, initial_model=None, **kwargs):
        if kwargs.get("tester") is None and not initial_model:
            raise ValueError("FedEDENServer needs a model to start from, a tester or "
                             "initial_model=: the workers' updates are differences to the "
                             "broadcast model")
        if kwargs.get("aggregation_mode", "exact") != "exact":
            raise ValueError("FedEDENServer has one arithmetic (aggregation_mode='exact'), not "
                             f"{kwargs['aggregation_mode']!r}")
        if isinstance(bits, bool) or bits not in _native.EDEN_BITS:
            raise ValueError(f"FedEDENServer: bits={bits!r} must be one of {_native.EDEN_BITS}")
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64:
            raise ValueError(f"FedEDENServer: seed={seed!r} must be an integer in 0..2^64 - 1")
        self.bits, self.seed = bits, seed
        self.__initial = initial_model
        self._payloads = {}  # worker id -> (n, EDENUpdate), in arrival order
        self.payload_bytes = []  # per round: worker id -> bytes it sent
        super().__init__(**kwargs)
        self.layout = ParameterLayout.from_dict(self.prev_model)

    def _initial_model(self):
        if self.__initial:
            return {k: v.detach().clone().to(self.device) for k, v in self.__initial.items()}
        return super()._initial_model()

    def _check_payload(self, worker_id, payload):
        who = f"worker {worker_id}"
        if not isinstance(payload, EDENUpdate):
            raise ValueError(f"{who}: the payload must be an EDENUpdate, not "
                             f"{type(payload).__name__}")
        P = self.layout.P
        if payload.P != P:
            raise ValueError(f"{who}: the payload is over rows of P={payload.P} elements, the "
                             f"server's model has P={P}")
        if payload.bits != self.bits:
            raise ValueError(f"{who}: the payload has bits={payload.bits!r}, the server decodes "
                             f"bits={self.bits}")
        NB, words = _native.drive_blocks(P), _native.eden_code_words(P, self.bits)
        codes, scales = payload.codes, payload.scales
        if not torch.is_tensor(codes) or codes.dtype != torch.int32 or codes.dim() != 1 \
                or codes.numel() != words:
            raise ValueError(f"{who}: codes must be an int32 vector of NB * 128 * bits = {words} "
                             "words")
        if not torch.is_tensor(scales) or scales.dtype != torch.float32 or scales.dim() != 1 \
                or scales.numel() != NB:
            raise ValueError(f"{who}: scales must be an fp32 vector of NB = {NB} elements, one "
                             "per block")
        if not bool((torch.isfinite(scales) & (scales >= 0)).all()):
            raise ValueError(f"{who}: scales must be finite and non-negative")
        return EDENUpdate(codes.contiguous().to(self.device), scales.contiguous().to(self.device),
                          P, self.bits)

    def _eden_flat(self, ids):
        """prev_model + the decoded FedAvg of the clients ``ids``, in that order, as a flat
        row."""
        ns = [int(self._payloads[i][0]) for i in ids]
        ups = [self._payloads[i][1] for i in ids]
        dev = self.device
        base = self.layout.flatten(self.prev_model, device=dev)
        out = torch.empty(self.layout.P, dtype=torch.float32, device=dev)
        return _native.eden_fedavg(base, torch.stack([u.codes for u in ups]),
                                   torch.stack([u.scales for u in ups]),
                                   torch.tensor(ns, dtype=torch.float32).to(dev), float(sum(ns)),
                                   self.layout.P, self.bits, self.seed, self.round + 1, out)

    def get_subset_model(self, client_subset):
        """The model the subset's updates alone would have given, in the subset's order
        (empty subset -> previous model)."""
        ids = list(client_subset)
        if not ids:
            return self.prev_model
        missing = [i for i in ids if i not in self._payloads]
        if missing:
            raise ValueError(f"workers {missing} sent no update this round")
        return self.layout.views(self._eden_flat(ids))

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
        data = self._process_aggregated_parameter(self.get_subset_model(self._payloads.keys()))
        self.round += 1
        self._set_prev_model(copy.deepcopy(data))
        acc = self.get_metric(self.prev_model)
        log.info("end aggregating, test accuracy is %s", acc)
        self._payloads.clear()
        return RepeatedResult(data=data, num=self.clients_per_round)
