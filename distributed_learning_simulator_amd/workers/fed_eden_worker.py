"""Multi-bit rotated FedAvg worker without client state (Vargaftik et al. 2022, "EDEN:
communication-efficient and robust distributed mean estimation for federated learning"),
``FedDriveWorker``'s successor at 2 or 4 bits per coordinate.

The worker keeps the base model alone: after each ``trainer.train()`` the update ``u = w -
base`` goes through one ``dls_eden_compress_f32``: per block of 4096 coordinates the
randomised Hadamard rotation that every client of the round shares (seed ``seed``, stream id
the round's number, counted from 1), per rotated coordinate the nearest level of the Lloyd-Max
quantizer of the normal distribution and one scale per block, sent as ``(worker_id, n,
EDENUpdate(codes, scales, P, bits))``.  The downlink is the dense model the ``FedEDENServer``
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


class EDENUpdate:
    """A client's uplink payload: ``codes`` (int32 [NB * 128 * bits] holding uint32 words in the
    layout of dls_eden_compress_f32; NB = ceil(P / 4096)) and ``scales`` (fp32 [NB], one per
    block)."""

    __slots__ = ("codes", "scales", "P", "bits")

    def __init__(self, codes, scales, P, bits):
        self.codes, self.scales, self.P, self.bits = codes, scales, int(P), bits

    @property
    def nbytes(self):
        return 4 * _native.eden_code_words(self.P, self.bits) + 4 * _native.drive_blocks(self.P)


class FedEDENWorker(FedWorker):
    """``bits``: 2 or 4 per coordinate; ``scale``: "unbiased" (EDEN's sum y^2 / sum |y| cent:
    the decoded update is right in expectation over the rotation) or "mse" (the least squared
    error of one decode)."""

    def __init__(self, bits=4, scale="unbiased", seed=0, **kwargs):
        if isinstance(bits, bool) or bits not in _native.EDEN_BITS:
            raise ValueError(f"FedEDENWorker: bits={bits!r} must be one of {_native.EDEN_BITS}")
        if scale not in _native.EDEN_SCALES:
            raise ValueError(f"FedEDENWorker: scale={scale!r} must be one of "
                             f"{sorted(_native.EDEN_SCALES)}")
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64:
            raise ValueError(f"FedEDENWorker: seed={seed!r} must be an integer in 0..2^64 - 1")
        self.bits, self.scale, self.seed = bits, scale, seed
        super().__init__(**kwargs)
        # replaces FedWorker's dense send (same callback name)
        self.trainer.add_named_callback(ModelExecutorCallbackPoint.AFTER_EXECUTE,
                                        "send_parameter", self.__send_codes)
        self.layout = self.base = None
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
        self.layout.copy_into(params, self.base)

    def eden_update(self, round):
        """Compress the model as it stands against the base under the rotation of
        ``round``: that round's EDENUpdate.  ValueError when the update is not finite."""
        if self.layout is None:
            raise RuntimeError("FedEDENWorker: no model loaded yet (the update is a "
                               "difference to the server's broadcast model)")
        dev, P = self.base.device, self.layout.P
        w = self.layout.flatten(ModelUtil(self.trainer.model).get_parameter_dict(detach=True),
                                device=dev)
        codes = torch.empty(_native.eden_code_words(P, self.bits), dtype=torch.int32, device=dev)
        scales = torch.empty(_native.drive_blocks(P), dtype=torch.float32, device=dev)
        stats = torch.empty(4, dtype=torch.int32, device=dev)
        _native.eden_compress(w, self.base, P, self.bits, self.seed, int(round), self.scale, codes,
                              scales, stats)
        nonfinite = int(stats[0])
        if nonfinite:
            raise ValueError(f"worker {self.worker_id}: {nonfinite} coordinates of the update are "
                             "not finite (training diverged); nothing is sent")
        return EDENUpdate(codes, scales, P, self.bits)

    def __send_codes(self, **kwargs):
        trainer = kwargs["model_executor"]
        payload = self.eden_update(self.rounds_sent + 1)
        self.rounds_sent += 1
        dense = 4 * self.layout.numel
        log.warning("parameter_size is %s, eden_parameter_size is %s, compression ratio is %s",
                    dense, payload.nbytes, float(payload.nbytes) / float(dense))
        self.worker_data_queue.add_task((self.worker_id, dataset_size(trainer.dataset), payload))
        self.load_model(self.worker_data_queue.get_result())
        log.info("end load_parameter_dict")
