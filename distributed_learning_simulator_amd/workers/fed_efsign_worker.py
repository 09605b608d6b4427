"""Scaled-sign FedAvg worker with error feedback (Karimireddy, Rebjock, Stich & Jaggi 2019,
"Error feedback fixes SignSGD"; the compressor of 1-bit SGD / 1-bit Adam).

The reference simulator's sign_SGD votes on signs and does not converge under heterogeneous
clients; this worker keeps the FedAvg protocol on the task queue and sends one bit per
coordinate: after each ``trainer.train()`` the update ``u = (w - base) + e`` (w the trained
model, base the model the worker last loaded, e what the bits of earlier rounds did not
carry) goes through one ``dls_efsign_compress_f32``: per tensor the scale s = mean |u|, per
coordinate the bit u < 0, sent as ``(worker_id, n, SignUpdate(bits, scales, P))``; e keeps
u -+ s for the next round.  The downlink is the dense model the ``FedEFSignServer``
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


class SignUpdate:
    """A client's uplink payload: ``bits`` (int64 [P / 64] words, bit j % 64 of word j / 64
    set where coordinate j of the flat ``ParameterLayout`` row is negative) and ``scales``
    (fp32 [T], one per tensor), on the worker's device."""

    __slots__ = ("bits", "scales", "P")

    def __init__(self, bits, scales, P):
        self.bits, self.scales, self.P = bits, scales, int(P)

    @property
    def nbytes(self):
        return self.P // 8 + 4 * int(self.scales.numel())


class FedEFSignWorker(FedWorker):
    """``error_feedback=False`` zeroes the residual before every compress: the plain scaled
    sign, the baseline the literature compares against."""

    def __init__(self, error_feedback=True, **kwargs):
        self.error_feedback = bool(error_feedback)
        super().__init__(**kwargs)
        # replaces FedWorker's dense send (same callback name)
        self.trainer.add_named_callback(ModelExecutorCallbackPoint.AFTER_EXECUTE,
                                        "send_parameter", self.__send_signs)
        self.layout = self.segments = None
        self.base = self.residual = self._workspace = None

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
            self.segments = _native.efsign_layout_segments(self.layout, dev)
            self.base = torch.zeros(self.layout.P, dtype=torch.float32, device=dev)
            self.residual = torch.zeros(self.layout.P, dtype=torch.float32, device=dev)
            self._workspace = _native.efsign_workspace(self.layout.P, len(self.layout), dev)
        self.layout.copy_into(params, self.base)

    def sign_update(self):
        """Compress the model as it stands against the base: the round's SignUpdate; the
        residual keeps what the bits did not carry.  ValueError when the update is not
        finite."""
        if self.layout is None:
            raise RuntimeError("FedEFSignWorker: no model loaded yet (the update is a "
                               "difference to the server's broadcast model)")
        dev = self.base.device
        w = self.layout.flatten(ModelUtil(self.trainer.model).get_parameter_dict(detach=True),
                                device=dev)
        if not self.error_feedback:
            self.residual.zero_()
        bits = torch.empty(self.layout.P // 64, dtype=torch.int64, device=dev)
        scales = torch.empty(len(self.layout), dtype=torch.float32, device=dev)
        stats = torch.empty(4, dtype=torch.int32, device=dev)
        _native.efsign_compress(w, self.base, self.residual, self.segments, bits, scales, stats,
                                self._workspace)
        nonfinite = int(stats[0])
        if nonfinite:
            raise ValueError(f"worker {self.worker_id}: {nonfinite} coordinates of the update are "
                             "not finite (training diverged); nothing is sent")
        return SignUpdate(bits, scales, self.layout.P)

    def __send_signs(self, **kwargs):
        trainer = kwargs["model_executor"]
        payload = self.sign_update()
        dense = 4 * self.layout.numel
        log.warning("parameter_size is %s, sign_parameter_size is %s, compression ratio is %s",
                    dense, payload.nbytes, float(payload.nbytes) / float(dense))
        self.worker_data_queue.add_task((self.worker_id, dataset_size(trainer.dataset), payload))
        self.load_model(self.worker_data_queue.get_result())
        log.info("end load_parameter_dict")
