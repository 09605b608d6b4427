"""Low-rank FedAvg worker with error feedback (Vogels, Karimireddy & Jaggi 2019, "PowerSGD:
practical low-rank gradient compression").

Where the update is a set of weight matrices, rank-``rank`` factors carry most of it: after
each ``trainer.train()`` the update ``u = (w - base) + e`` (w the trained model, base the model
the worker last loaded, e what the factors of earlier rounds did not carry) goes through one
``dls_powersgd_compress_f32``: per weight matrix one power-iteration step, P^ = orth(U Q0) and
Q = U^T P^, sent as ``(worker_id, n, LowRankUpdate(payload, P, rank))``; vectors and matrices
too small to gain are sent as they are; e keeps u - P^ Q^T for the next round.  Each worker
does its own power step (PowerSGD's all-reduce of P is a data-centre device, not a federated
one).  Q0 of round 1 is drawn from the library's Philox stream under ``seed``, one stream id per
tensor; afterwards the worker starts from its own last Q (``warm_start``) or draws a fresh Q0
with the round in the counter.  The downlink is the dense model the ``FedPowerSGDServer``
broadcasts.
"""
import logging

import torch

from .. import _native
from ..layout import ParameterLayout
from ..model_util import ModelUtil
from ..trainer import ModelExecutorCallbackPoint
from .fed_worker import FedWorker, dataset_size

log = logging.getLogger("distributed_learning_simulator_amd")


def check_powersgd_options(who, rank, seed=0):
    """The options the worker and the server share."""
    if isinstance(rank, bool) or not isinstance(rank, int) \
            or not 1 <= rank <= _native.POWERSGD_MAX_RANK:
        raise ValueError(f"{who}: rank={rank!r} must be an integer in "
                         f"1..{_native.POWERSGD_MAX_RANK}")
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64:
        raise ValueError(f"{who}: seed={seed!r} must be an integer in 0..2^64 - 1")


class LowRankUpdate:
    """A client's uplink payload: ``payload`` (fp32 [L]), per tensor of the flat
    ``ParameterLayout`` row of ``P`` coordinates the factors P^ [n, rank] and Q [m, rank] or
    the tensor's values, at the offsets of ``_native.powersgd_plan``; ``floats`` counts what
    is sent: the blocks without their padding."""

    __slots__ = ("payload", "P", "rank", "floats")

    def __init__(self, payload, P, rank, floats):
        self.payload, self.P, self.rank, self.floats = payload, int(P), int(rank), int(floats)

    @property
    def nbytes(self):
        return 4 * self.floats


def sent_floats(plan):
    """The floats of a payload under ``plan`` that carry data."""
    r = plan.r
    return sum((n + m) * r if kind else n * m for _, n, m, kind, *_ in plan.rows[:plan.T])


class FedPowerSGDWorker(FedWorker):
    """``error_feedback=False`` drops the residual, so a client sampled once needs no state
    beyond the base; ``warm_start=False`` draws a fresh Q0 every round."""

    def __init__(self, rank=4, seed=0, warm_start=True, error_feedback=True, **kwargs):
        check_powersgd_options("FedPowerSGDWorker", rank, seed)
        self.rank, self.seed = rank, seed
        self.warm_start, self.error_feedback = bool(warm_start), bool(error_feedback)
        super().__init__(**kwargs)
        # replaces FedWorker's dense send (same callback name)
        self.trainer.add_named_callback(ModelExecutorCallbackPoint.AFTER_EXECUTE,
                                        "send_parameter", self.__send_factors)
        self.layout = self.plan = self.base = self.residual = self.q0 = self._workspace = None
        self.rounds_sent = 0

    def train(self, device):
        self.trainer.set_device(device)
        self.load_model(self.worker_data_queue.get_result())
        log.info("end load initial parameter_dict")
        for _ in range(self.round):
            self.trainer.train()

    def load_model(self, parameter_dict):
        """Load the server's dense model; its bits become the base of the next update."""
        model = self.trainer.model
        ModelUtil(model).load_parameter_dict(parameter_dict)
        params = ModelUtil(model).get_parameter_dict(detach=True)
        if self.layout is None:
            dev = next(iter(params.values())).device
            self.layout = ParameterLayout.from_dict(params)
            self.plan = _native.powersgd_layout_plan(self.layout, self.rank, dev)
            self.base = torch.zeros(self.layout.P, dtype=torch.float32, device=dev)
            if self.error_feedback:
                self.residual = torch.zeros(self.layout.P, dtype=torch.float32, device=dev)
            self._workspace = _native.powersgd_workspace(self.plan, dev)
        self.layout.copy_into(params, self.base)

    def draw_q0(self):
        """A Gaussian Q0 in the payload's layout: tensor t's Q block from stream id t, its
        counter starting at round x block length, so no two rounds share a value."""
        q0 = torch.zeros(self.plan.L, dtype=torch.float32, device=self.base.device)
        for t in range(self.plan.T):
            if self.plan.kind(t):
                qoff, m = self.plan.blocks(t)[1], self.plan.rows[t][2]
                n = (m * self.rank + 63) // 64 * 64
                _native.philox_normal(n, self.seed, t, first=self.rounds_sent * n,
                                      out=q0[qoff:qoff + n])
        return q0

    def lowrank_update(self):
        """Compress the model as it stands against the base: the round's LowRankUpdate; the
        residual keeps what the factors did not carry.  ValueError when the update is not
        finite."""
        if self.layout is None:
            raise RuntimeError("FedPowerSGDWorker: no model loaded yet (the update is a "
                               "difference to the server's broadcast model)")
        dev = self.base.device
        w = self.layout.flatten(ModelUtil(self.trainer.model).get_parameter_dict(detach=True),
                                device=dev)
        if self.q0 is None or not self.warm_start:
            self.q0 = self.draw_q0()
        payload = torch.empty(self.plan.L, dtype=torch.float32, device=dev)
        stats = torch.empty(4, dtype=torch.int32, device=dev)
        _native.powersgd_compress(w, self.base, self.residual, self.plan, self.q0, payload, stats,
                                  self._workspace)
        nonfinite = int(stats[0])
        if nonfinite:
            raise ValueError(f"worker {self.worker_id}: {nonfinite} coordinates of the update are "
                             "not finite (training diverged); nothing is sent")
        self.rounds_sent += 1
        if self.warm_start:
            self.q0 = payload  # the next round's Q0 is read at the Q blocks alone
        return LowRankUpdate(payload, self.layout.P, self.rank, sent_floats(self.plan))

    def __send_factors(self, **kwargs):
        trainer = kwargs["model_executor"]
        update = self.lowrank_update()
        dense = 4 * self.layout.numel
        log.warning("parameter_size is %s, lowrank_parameter_size is %s, compression ratio is %s",
                    dense, update.nbytes, float(update.nbytes) / float(dense))
        self.worker_data_queue.add_task((self.worker_id, dataset_size(trainer.dataset), update))
        self.load_model(self.worker_data_queue.get_result())
        log.info("end load_parameter_dict")
