"""Stochastically quantized FedAvg worker without client state (Alistarh et al. 2017, "QSGD:
communication-efficient SGD via gradient quantization and encoding"; Wen et al. 2017,
"TernGrad", the ``bits=2, norm="max"`` case).

The worker keeps the base model alone: after each ``trainer.train()`` the update ``u = w -
base`` goes through one ``dls_qsgd_compress_f32``: per bucket of 512 coordinates one fp32
scale, per coordinate a signed level of ``bits`` bits, rounded up or down at random so that the
decode is ``u`` in expectation, sent as ``(worker_id, n, QSGDUpdate(codes, scales, P, bits))``.
The rounding noise comes from the library's Philox stream under ``seed`` and the stream id
``round * 2^32 + worker_id`` (rounds counted from 1): no two (round, worker) pairs share it,
and the server needs neither.  The downlink is the dense model the ``FedQSGDServer``
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


class QSGDUpdate:
    """A client's uplink payload: ``codes`` (int32 [NB * 16 * bits] holding uint32 words, the
    field of coordinate j at bit (j % (32 / bits)) * bits of word j / (32 / bits); NB = ceil(P /
    512)) and ``scales`` (fp32 [NB], the decode step of each bucket)."""

    __slots__ = ("codes", "scales", "P", "bits")

    def __init__(self, codes, scales, P, bits):
        self.codes, self.scales, self.P, self.bits = codes, scales, int(P), bits

    @property
    def nbytes(self):
        return 4 * _native.qsgd_code_words(self.P, self.bits) + 4 * _native.qsgd_buckets(self.P)


class FedQSGDWorker(FedWorker):
    """``bits``: 2 (ternary), 4 or 8 per coordinate; ``norm``: "l2" (QSGD's) or "max"
    (TernGrad's) per bucket of 512 coordinates."""

    def __init__(self, bits=4, norm="l2", seed=0, **kwargs):
        if isinstance(bits, bool) or bits not in _native.QSGD_BITS:
            raise ValueError(f"FedQSGDWorker: bits={bits!r} must be one of {_native.QSGD_BITS}")
        if norm not in _native.QSGD_NORMS:
            raise ValueError(f"FedQSGDWorker: norm={norm!r} must be one of "
                             f"{sorted(_native.QSGD_NORMS)}")
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 1 << 64:
            raise ValueError(f"FedQSGDWorker: seed={seed!r} must be an integer in 0..2^64 - 1")
        self.bits, self.norm, self.seed = bits, norm, seed
        super().__init__(**kwargs)
        if not 0 <= int(self.worker_id) < 1 << 32:
            raise ValueError(f"FedQSGDWorker: worker_id={self.worker_id!r} must lie in 0..2^32 - 1 "
                             "(the low half of the noise's stream id)")
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

    def qsgd_update(self, round):
        """Quantize the model as it stands against the base with the noise of (``round``, this
        worker): that round's QSGDUpdate.  ValueError when the update is not finite."""
        if self.layout is None:
            raise RuntimeError("FedQSGDWorker: no model loaded yet (the update is a "
                               "difference to the server's broadcast model)")
        round = int(round)
        if not 0 <= round < 1 << 32:
            raise ValueError(f"FedQSGDWorker: round={round} must lie in 0..2^32 - 1")
        dev, P = self.base.device, self.layout.P
        w = self.layout.flatten(ModelUtil(self.trainer.model).get_parameter_dict(detach=True),
                                device=dev)
        codes = torch.empty(_native.qsgd_code_words(P, self.bits), dtype=torch.int32, device=dev)
        scales = torch.empty(_native.qsgd_buckets(P), dtype=torch.float32, device=dev)
        stats = torch.empty(4, dtype=torch.int32, device=dev)
        _native.qsgd_compress(w, self.base, P, self.bits, self.norm, self.seed,
                              (round << 32) + int(self.worker_id), codes, scales, stats)
        nonfinite = int(stats[0])
        if nonfinite:
            raise ValueError(f"worker {self.worker_id}: {nonfinite} coordinates of the update are "
                             "not finite (training diverged); nothing is sent")
        return QSGDUpdate(codes, scales, P, self.bits)

    def __send_codes(self, **kwargs):
        trainer = kwargs["model_executor"]
        payload = self.qsgd_update(self.rounds_sent + 1)
        self.rounds_sent += 1
        dense = 4 * self.layout.numel
        log.warning("parameter_size is %s, qsgd_parameter_size is %s, compression ratio is %s",
                    dense, payload.nbytes, float(payload.nbytes) / float(dense))
        self.worker_data_queue.add_task((self.worker_id, dataset_size(trainer.dataset), payload))
        self.load_model(self.worker_data_queue.get_result())
        log.info("end load_parameter_dict")
