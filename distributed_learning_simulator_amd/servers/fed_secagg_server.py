"""Secure-aggregation server (Bonawitz et al. 2017, "Practical Secure Aggregation for
Privacy-Preserving Machine Learning"), as simulated: single server, honest but curious.

Client payloads are ``MaskedUpdate``s: a client's quantised update times its weight, plus
its self mask and one pair mask per other participant, in the ring Z_2^32.  The server
copies each into a row of one int32 ``[K, P]`` device buffer and never holds an update in
the clear.  When all payloads of the round are in, one ``dls_secagg_unmask_f32`` launch sums
the survivors' rows, takes off the survivors' self masks and the pair masks the dropped
workers left uncancelled, decodes the integer sum and adds its weighted mean to the previous
global model.  The masked sum is commutative and every step is integer arithmetic until the
decode, so the round's model is bit-identical for any arrival order, weighted or not.

What is simulated: one ``secagg_seed`` stands for every agreed pair key and self-mask seed,
and the server regenerates a mask from it where the protocol would reconstruct the seed from
the surviving clients' Shamir shares.  Key agreement, the shares, a malicious server and
clients that lie about the dropout set are outside this simulation.
"""
import copy
import logging

import torch

from .. import _native
from ..aggregation import secagg_check_capacity, secagg_server_streams
from ..layout import ParameterLayout
from ..task_queue import RepeatedResult
from ..workers.fed_secagg_worker import (SECAGG_DEFAULTS, MaskedUpdate, check_secagg_format,
                                         to_stream_table)
from .fed_server import FedServer

log = logging.getLogger("distributed_learning_simulator_amd")

_REASON = "it never holds an individual update, only masked payloads and their sum"


class FedSecAggServer(FedServer):
    """``secagg_dropouts``: the worker ids that drop out of every round after the masks were
    agreed: their payloads are never read and the server recovers the pair masks they leave
    in the survivors' payloads; ``secagg_threshold``: the survivors a round needs, as the
    shares of a dropped client's key could not be reconstructed from fewer (default
    ``worker_number // 2 + 1``); ``secagg_seed``, ``secagg_bits``, ``secagg_frac_bits``: the
    workers' (``FedSecAggWorker``); ``initial_model``: the parameter dict the first round
    starts from (default: the tester's model); one of ``tester`` and ``initial_model`` is
    needed, because the workers' updates are differences to the broadcast model.

    The clients' weights are all 1 or all their reported sample counts, and ``L * sum of the
    survivors' weights < 2^31`` with L = 2^(secagg_bits-1) - 1 must hold, or the sum could
    wrap: both are checked before anything is launched.  At most ``_native.ROBUST_MAX_K``
    workers.

    ``get_subset_model`` returns the previous model for an empty subset and the round's
    aggregate for exactly the round's survivors; any other subset raises ``ValueError``: the
    aggregate of fewer clients is what the protocol exists to prevent.  ``last_secagg`` holds
    the latest round's ``survivors``, ``dropped``, ``total`` (the survivors' weights summed),
    ``saturated`` (coordinates the survivors reported at the end of the range) and
    ``streams_removed`` (the masks the server regenerated).

    ``aggregation_rule`` other than "mean", ``aggregation_mode="fma"``, ``attack``,
    ``server_optimizer`` and ``dp_clip`` raise ``ValueError``: robust rules on masked data and
    distributed DP are out of scope here."""

    _robust_unsupported = _REASON
    _attack_unsupported = _REASON
    _server_opt_unsupported = _REASON
    _dp_unsupported = _REASON

    def __init__(self, initial_model=None, secagg_dropouts=(), secagg_threshold=None,
                 secagg_seed=SECAGG_DEFAULTS["secagg_seed"],
                 secagg_bits=SECAGG_DEFAULTS["secagg_bits"],
                 secagg_frac_bits=SECAGG_DEFAULTS["secagg_frac_bits"], **kwargs):
        if kwargs.get("tester") is None and not initial_model:
            raise ValueError("FedSecAggServer needs a model to start from, a tester or "
                             "initial_model=: the workers' updates are differences to the "
                             "broadcast model")
        if kwargs.get("aggregation_mode", "exact") != "exact":
            raise ValueError("FedSecAggServer has one arithmetic (aggregation_mode='exact'), not "
                             f"{kwargs['aggregation_mode']!r}: {_REASON}")
        check_secagg_format(secagg_bits, secagg_frac_bits, secagg_seed)
        workers = kwargs.get("worker_number")
        if workers > _native.ROBUST_MAX_K:
            raise ValueError(f"fed_secagg takes at most ROBUST_MAX_K={_native.ROBUST_MAX_K} "
                             f"workers, not worker_number={workers}")
        self.secagg_dropouts = self._check_dropouts(secagg_dropouts, workers)
        if secagg_threshold is None:
            secagg_threshold = workers // 2 + 1
        if isinstance(secagg_threshold, bool) or not isinstance(secagg_threshold, int) \
                or not 1 <= secagg_threshold <= workers:
            raise ValueError(f"secagg_threshold must be an integer in 1..worker_number = "
                             f"{workers}, not {secagg_threshold!r}")
        alive = workers - len(self.secagg_dropouts)
        if alive < secagg_threshold:
            raise ValueError(f"secagg_dropouts={list(self.secagg_dropouts)} leaves {alive} of "
                             f"{workers} workers, fewer than secagg_threshold={secagg_threshold}: "
                             "the dropped workers' shares could not be reconstructed")
        self.secagg_threshold, self.secagg_seed = secagg_threshold, secagg_seed
        self.secagg_bits, self.secagg_frac_bits = secagg_bits, secagg_frac_bits
        self.__initial = initial_model
        self._arrived = {}  # worker id -> (n, weight, saturated, row or None), arrival order
        self._Y = None  # int32 [worker_number, P]: the round's masked rows
        self._aggregate = None  # (the round's survivors, its model)
        self.last_secagg = {}
        super().__init__(**kwargs)
        self.layout = ParameterLayout.from_dict(self.prev_model)

    @staticmethod
    def _check_dropouts(dropouts, worker_number):
        """The sorted tuple of dropped worker ids; ValueError for ids no worker has."""
        try:
            ids = list(dropouts)
        except TypeError:
            raise ValueError(f"secagg_dropouts must be a collection of worker ids, not "
                             f"{dropouts!r}")
        if any(isinstance(w, bool) or not isinstance(w, int) or w < 0 for w in ids):
            raise ValueError(f"secagg_dropouts must be non-negative integer worker ids, not "
                             f"{ids!r}")
        if len(set(ids)) != len(ids):
            raise ValueError(f"secagg_dropouts must be distinct worker ids, not {ids!r}")
        if ids and max(ids) >= worker_number:
            raise ValueError(f"secagg_dropouts={ids} must be worker ids in 0..worker_number - 1 "
                             f"= {worker_number - 1}")
        return tuple(sorted(ids))

    def _initial_model(self):
        if self.__initial:
            return {k: v.detach().clone().to(self.device) for k, v in self.__initial.items()}
        return super()._initial_model()

    def _check_payload(self, worker_id, n, payload):
        who = f"worker {worker_id}"
        if isinstance(worker_id, bool) or not isinstance(worker_id, int) \
                or not 0 <= worker_id < self.worker_number:
            raise ValueError(f"{who}: not a worker id in 0..worker_number - 1 = "
                             f"{self.worker_number - 1}")
        if worker_id in self._arrived:
            raise ValueError(f"{who}: a second payload in round {self.round + 1}")
        if not isinstance(payload, MaskedUpdate):
            raise ValueError(f"{who}: the payload must be a MaskedUpdate, not "
                             f"{type(payload).__name__}")
        P = self.layout.P
        if payload.P != P:
            raise ValueError(f"{who}: the payload is over rows of P={payload.P} elements, the "
                             f"server's model has P={P}")
        if payload.round != self.round + 1:
            raise ValueError(f"{who}: the payload is masked for round {payload.round}, the "
                             f"server is in round {self.round + 1}")
        if (payload.bits, payload.frac_bits) != (self.secagg_bits, self.secagg_frac_bits):
            raise ValueError(f"{who}: the payload's format (bits {payload.bits}, frac_bits "
                             f"{payload.frac_bits}) is not the server's (secagg_bits "
                             f"{self.secagg_bits}, secagg_frac_bits {self.secagg_frac_bits})")
        if payload.weight != 1 and payload.weight != n:
            raise ValueError(f"{who}: weight {payload.weight} is neither 1 nor the reported "
                             f"sample count {n}")
        y = payload.y
        if not torch.is_tensor(y) or y.dtype != torch.int32 or y.dim() != 1 or y.numel() != P:
            raise ValueError(f"{who}: y must be an int32 vector of P={P} elements")

    def _unmask(self, survivors):
        """The round's model as a flat row: prev_model + the decoded mean of the survivors'
        updates.  Books ``last_secagg``."""
        dev, P = self.device, self.layout.P
        dropped = [w for w in self._arrived if w in set(self.secagg_dropouts)]
        weights = [self._arrived[w][1] for w in survivors]
        ns = [int(self._arrived[w][0]) for w in survivors]
        if any(wt != 1 for wt in weights) and weights != ns:
            raise ValueError(f"the survivors' weights {dict(zip(survivors, weights))} are neither "
                             f"all 1 nor all the reported sample counts {dict(zip(survivors, ns))}")
        total = secagg_check_capacity(self.secagg_bits, weights)
        add, sub = secagg_server_streams(survivors, dropped, self.round)
        rows = torch.tensor([self._arrived[w][3] for w in survivors], dtype=torch.int32).to(dev)
        base = self.layout.flatten(self.prev_model, device=dev)
        out = torch.empty(P, dtype=torch.float32, device=dev)
        _native.secagg_unmask(self._Y, rows, to_stream_table(add, dev), to_stream_table(sub, dev),
                              self.secagg_seed, base, self.secagg_frac_bits, float(total), P, out)
        saturated = sum(self._arrived[w][2] for w in survivors)
        self.last_secagg = {"round": self.round, "survivors": tuple(sorted(survivors)),
                            "dropped": tuple(sorted(dropped)), "total": total,
                            "saturated": saturated, "streams_removed": len(add) + len(sub)}
        log.info("secagg round %s: survivors %s, dropped %s, %s masks removed, total weight %s, "
                 "saturated share %s", self.round, sorted(survivors), sorted(dropped),
                 len(add) + len(sub), total,
                 float(saturated) / float(max(self.layout.numel * len(survivors), 1)))
        return out

    def get_subset_model(self, client_subset):
        """The previous model for an empty subset, the round's aggregate for exactly the
        round's survivors; ValueError for any other subset."""
        ids = list(client_subset)
        if not ids:
            return self.prev_model
        if self._aggregate is not None and len(set(ids)) == len(ids) \
                and set(ids) == set(self._aggregate[0]):
            return self._aggregate[1]
        raise ValueError(f"FedSecAggServer holds the sum of the round's survivors "
                         f"{sorted(self._aggregate[0]) if self._aggregate else []} alone, not "
                         f"the aggregate of {ids}: a smaller subset is what secure aggregation "
                         "exists to prevent")

    def _process_worker_data(self, data, __):
        worker_id, n, payload = data
        self._check_payload(worker_id, n, payload)
        row = None
        if worker_id not in self.secagg_dropouts:  # a dropped worker's payload is never read
            if self._Y is None:
                self._Y = torch.empty((self.worker_number, self.layout.P), dtype=torch.int32,
                                      device=self.device)
            row = sum(1 for r in self._arrived.values() if r[3] is not None)
            self._Y[row].copy_(payload.y)
        self._arrived[worker_id] = (n, payload.weight, payload.saturated, row)
        if len(self._arrived) != self.clients_per_round:
            log.debug("%s %s,skip", len(self._arrived), self.clients_per_round)
            return None
        self.round += 1
        log.info("begin aggregating")
        survivors = [w for w, r in self._arrived.items() if r[3] is not None]
        try:
            self._aggregate = (tuple(survivors), self.layout.views(self._unmask(survivors)))
        finally:
            self._arrived = {}
        data = self._process_aggregated_parameter(self.get_subset_model(survivors))
        self._set_prev_model(copy.deepcopy(data))
        acc = self.get_metric(self.prev_model)
        log.info("end aggregating, test accuracy is %s", acc)
        return RepeatedResult(data=data, num=self.clients_per_round)
