"""Microscaling FP8 / FP4 FedAvg worker (Rouhani et al. 2023, "Microscaling Data Formats for
Deep Learning"; the OCP MX v1.0 specification; Wang et al. 2024, "Towards Federated Learning
with On-device Training and Communication in 8-bit Floating Point").

After each ``trainer.train()`` the update ``u = (w - base) + r`` (w the trained model, base the
model the worker last loaded, r what the codes of earlier rounds did not carry; without error
feedback ``u = w - base``) goes through one ``dls_mx_compress_f32``: per block of 32
coordinates one power-of-two scale byte, per coordinate an E4M3, E5M2 or E2M1 code, sent as
``(worker_id, n, MXUpdate(codes, scales, P, format))``.  ``rounding="nearest"`` is deterministic
and pairs with the residual; ``rounding="stochastic"`` is unbiased and needs none: its noise is
the library's Philox stream under ``seed`` and the stream id ``round * 2^32 + worker_id``
(rounds counted from 1).  The downlink is the dense model the ``FedMXServer`` broadcasts.
"""
import logging

import torch

from .. import _native
from ..layout import ParameterLayout
from ..model_util import ModelUtil
from ..trainer import ModelExecutorCallbackPoint
from .fed_worker import FedWorker, dataset_size

log = logging.getLogger("distributed_learning_simulator_amd")


class MXUpdate:
    """A client's uplink payload: ``codes`` (int32 holding uint32 words: code j is byte j at 8
    bits, nibble j & 1 of byte j >> 1 at 4; whole groups of 512 coordinates) and ``scales``
    (uint8, the E8M0 byte of each block of 32; 16 per group)."""

    __slots__ = ("codes", "scales", "P", "format")

    def __init__(self, codes, scales, P, format):
        self.codes, self.scales, self.P, self.format = codes, scales, int(P), format

    @property
    def nbytes(self):
        return 4 * _native.mx_code_words(self.P, self.format) + _native.mx_scale_bytes(self.P)


class FedMXWorker(FedWorker):
    """``format``: "e4m3", "e5m2" or "e2m1"; ``rounding``: "nearest" or "stochastic";
    ``error_feedback``: keep what the codes did not carry for the next round (default: on for
    "nearest", off for "stochastic")."""

    def __init__(self, format="e4m3", rounding="nearest", error_feedback=None, seed=0, **kwargs):
        if format not in _native.MX_FORMATS:
            raise ValueError(f"FedMXWorker: format={format!r} must be one of "
                             f"{sorted(_native.MX_FORMATS)}")
        if rounding not in _native.MX_ROUNDINGS:
            raise ValueError(f"FedMXWorker: rounding={rounding!r} must be one of "
                             f"{sorted(_native.MX_ROUNDINGS)}")
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64:
            raise ValueError(f"FedMXWorker: seed={seed!r} must be an integer in 0..2^64 - 1")
        self.format, self.rounding, self.seed = format, rounding, seed
        self.error_feedback = (rounding == "nearest") if error_feedback is None \
            else bool(error_feedback)
        super().__init__(**kwargs)
        if not 0 <= int(self.worker_id) < 1 << 32:
            raise ValueError(f"FedMXWorker: worker_id={self.worker_id!r} must lie in 0..2^32 - 1 "
                             "(the low half of the noise's stream id)")
        # replaces FedWorker's dense send (same callback name)
        self.trainer.add_named_callback(ModelExecutorCallbackPoint.AFTER_EXECUTE,
                                        "send_parameter", self.__send_codes)
        self.layout = self.base = self.residual = None
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
            self.base = torch.zeros(self.layout.P, dtype=torch.float32, device=dev)
            if self.error_feedback:
                self.residual = torch.zeros(self.layout.P, dtype=torch.float32, device=dev)
        self.layout.copy_into(params, self.base)

    def mx_update(self, round):
        """Compress the model as it stands against the base with the noise of (``round``, this
        worker): that round's MXUpdate; the residual, if kept, takes what the codes did not
        carry.  ValueError when the update is not finite."""
        if self.layout is None:
            raise RuntimeError("FedMXWorker: no model loaded yet (the update is a difference to "
                               "the server's broadcast model)")
        round = int(round)
        if not 0 <= round < 1 << 32:
            raise ValueError(f"FedMXWorker: round={round} must lie in 0..2^32 - 1")
        dev, P = self.base.device, self.layout.P
        w = self.layout.flatten(ModelUtil(self.trainer.model).get_parameter_dict(detach=True),
                                device=dev)
        codes = torch.empty(_native.mx_code_words(P, self.format), dtype=torch.int32, device=dev)
        scales = torch.empty(_native.mx_scale_bytes(P), dtype=torch.uint8, device=dev)
        stats = torch.empty(4, dtype=torch.int32, device=dev)
        _native.mx_compress(w, self.base, self.residual, P, self.format, self.rounding, self.seed,
                            (round << 32) + int(self.worker_id), codes, scales, stats)
        nonfinite = int(stats[0])
        if nonfinite:
            raise ValueError(f"worker {self.worker_id}: {nonfinite} coordinates of the update are "
                             "not finite (training diverged); nothing is sent")
        return MXUpdate(codes, scales, P, self.format)

    def __send_codes(self, **kwargs):
        trainer = kwargs["model_executor"]
        payload = self.mx_update(self.rounds_sent + 1)
        self.rounds_sent += 1
        dense = 4 * self.layout.numel
        log.warning("parameter_size is %s, mx_parameter_size is %s, compression ratio is %s",
                    dense, payload.nbytes, float(payload.nbytes) / float(dense))
        self.worker_data_queue.add_task((self.worker_id, dataset_size(trainer.dataset), payload))
        self.load_model(self.worker_data_queue.get_result())
        log.info("end load_parameter_dict")
