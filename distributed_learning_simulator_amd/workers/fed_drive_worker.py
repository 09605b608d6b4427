"""Rotated one-bit FedAvg worker without client state (Suresh, Yu, Kumar & McMahan 2017,
"Distributed mean estimation with limited communication"; Vargaftik et al. 2021, "DRIVE:
one-bit distributed mean estimation").

``FedEFSignWorker`` is accurate because it carries a residual from round to round; a client
that is sampled once has nowhere to keep one.  This worker keeps the base model alone: after
each ``trainer.train()`` the update ``u = w - base`` goes through one
``dls_drive_compress_f32``: per block of 4096 coordinates a randomised Hadamard rotation
that every client of the round shares (seed ``seed``, stream id the round's number, counted
from 1), one bit per rotated coordinate and one scale per block, sent as ``(worker_id, n,
DriveUpdate(bits, scales, P, round))``.  The downlink is the dense model the
``FedDriveServer`` broadcasts.
"""
import logging

import torch

from .. import _native
from ..layout import ParameterLayout
from ..model_util import ModelUtil
from ..trainer import ModelExecutorCallbackPoint
from .fed_worker import FedWorker, dataset_size

log = logging.getLogger("distributed_learning_simulator_amd")


class DriveUpdate:
    """A client's uplink payload: ``bits`` (int64 [Pd / 64] words, bit j % 64 of word j / 64
    set where rotated coordinate j is negative; Pd = 4096 NB, NB = ceil(P / 4096)), ``scales``
    (fp32 [NB], one per block) and the ``round`` whose rotation they are in."""

    __slots__ = ("bits", "scales", "P", "round")

    def __init__(self, bits, scales, P, round):
        self.bits, self.scales, self.P, self.round = bits, scales, int(P), int(round)

    @property
    def nbytes(self):
        NB = _native.drive_blocks(self.P)
        return NB * _native.DRIVE_BLOCK // 8 + 4 * NB


class FedDriveWorker(FedWorker):
    """``scale``: "unbiased" (DRIVE's sum y^2 / sum |y|: the decoded update is right in
    expectation over the rotation) or "mse" (mean |y|: the least squared error of one
    decode)."""

    def __init__(self, seed=0, scale="unbiased", **kwargs):
        if scale not in _native.DRIVE_SCALES:
            raise ValueError(f"FedDriveWorker: scale={scale!r} must be one of "
                             f"{sorted(_native.DRIVE_SCALES)}")
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64:
            raise ValueError(f"FedDriveWorker: seed={seed!r} must be an integer in 0..2^64 - 1")
        self.seed, self.scale = seed, scale
        super().__init__(**kwargs)
        # replaces FedWorker's dense send (same callback name)
        self.trainer.add_named_callback(ModelExecutorCallbackPoint.AFTER_EXECUTE,
                                        "send_parameter", self.__send_bits)
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

    def drive_update(self, round):
        """Compress the model as it stands against the base under the rotation of
        ``round``: that round's DriveUpdate.  ValueError when the update is not finite."""
        if self.layout is None:
            raise RuntimeError("FedDriveWorker: no model loaded yet (the update is a "
                               "difference to the server's broadcast model)")
        dev, P = self.base.device, self.layout.P
        NB = _native.drive_blocks(P)
        w = self.layout.flatten(ModelUtil(self.trainer.model).get_parameter_dict(detach=True),
                                device=dev)
        bits = torch.empty(NB * _native.DRIVE_BLOCK // 64, dtype=torch.int64, device=dev)
        scales = torch.empty(NB, dtype=torch.float32, device=dev)
        stats = torch.empty(4, dtype=torch.int32, device=dev)
        _native.drive_compress(w, self.base, P, self.seed, int(round), self.scale, bits, scales,
                               stats)
        nonfinite = int(stats[0])
        if nonfinite:
            raise ValueError(f"worker {self.worker_id}: {nonfinite} coordinates of the update are "
                             "not finite (training diverged); nothing is sent")
        return DriveUpdate(bits, scales, P, round)

    def __send_bits(self, **kwargs):
        trainer = kwargs["model_executor"]
        payload = self.drive_update(self.rounds_sent + 1)
        self.rounds_sent += 1
        dense = 4 * self.layout.numel
        log.warning("parameter_size is %s, drive_parameter_size is %s, compression ratio is %s",
                    dense, payload.nbytes, float(payload.nbytes) / float(dense))
        self.worker_data_queue.add_task((self.worker_id, dataset_size(trainer.dataset), payload))
        self.load_model(self.worker_data_queue.get_result())
        log.info("end load_parameter_dict")
