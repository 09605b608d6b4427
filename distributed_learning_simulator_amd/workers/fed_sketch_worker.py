"""FetchSGD worker (Rothchild et al. 2020, "FetchSGD: Communication-Efficient Federated
Learning with Sketching"): sparsification without client state.

``FedTopKWorker`` is accurate because it carries a residual from round to round; a client
that is sampled once has nowhere to keep one.  This worker keeps the base model alone: after
each ``trainer.train()`` the update ``u = w - base`` goes through one ``dls_sketch_f32`` and
is sent as ``(worker_id, n, SketchUpdate(table, P))``, a Count Sketch of ``rows`` x ``cols``
fp32 buckets under the run's hash (seed ``seed``, stream id ``stream_id``: the same in every
round, because the ``FedSketchServer`` keeps momentum and the error accumulation in sketch
space).  The downlink is the dense model the server broadcasts.
"""
import logging

import torch

from .. import _native
from ..layout import ParameterLayout
from ..model_util import ModelUtil
from ..trainer import ModelExecutorCallbackPoint
from .fed_worker import FedWorker, dataset_size

log = logging.getLogger("distributed_learning_simulator_amd")


def check_sketch_options(who, rows, cols, seed, stream_id):
    """The options the worker and the server share (``cols`` None: chosen from P later)."""
    if isinstance(rows, bool) or rows not in _native.SKETCH_ROWS:
        raise ValueError(f"{who}: rows={rows!r} must be one of {_native.SKETCH_ROWS}")
    if cols is not None and (isinstance(cols, bool) or not isinstance(cols, int)
                             or not _native.SKETCH_MIN_COLS <= cols <= _native.SKETCH_MAX_COLS
                             or cols & (cols - 1)):
        raise ValueError(f"{who}: cols={cols!r} must be a power of two in 1024..2^24")
    for name, v in (("seed", seed), ("stream_id", stream_id)):
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v < 1 << 64:
            raise ValueError(f"{who}: {name}={v!r} must be an integer in 0..2^64 - 1")


class SketchUpdate:
    """A client's uplink payload: ``table`` (fp32 [R, C]), the Count Sketch of its update over
    rows of ``P`` coordinates."""

    __slots__ = ("table", "P")

    def __init__(self, table, P):
        self.table, self.P = table, int(P)

    @property
    def nbytes(self):
        return 4 * self.table.numel()


class FedSketchWorker(FedWorker):
    """``rows`` x ``cols``: the table's shape (``cols`` None: the largest power of two <= P /
    32, clamped to 1024..2^24); ``seed`` and ``stream_id``: the run's hash, the server's."""

    def __init__(self, rows=5, cols=None, seed=0, stream_id=0, **kwargs):
        check_sketch_options("FedSketchWorker", rows, cols, seed, stream_id)
        self.rows, self.cols, self.seed, self.stream_id = rows, cols, seed, stream_id
        super().__init__(**kwargs)
        # replaces FedWorker's dense send (same callback name)
        self.trainer.add_named_callback(ModelExecutorCallbackPoint.AFTER_EXECUTE,
                                        "send_parameter", self.__send_sketch)
        self.layout = self.base = self.workspace = None

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
            if self.cols is None:
                self.cols = _native.sketch_default_cols(self.layout.P)
            self.workspace = _native.sketch_workspace(self.layout.P, self.rows, self.cols, dev)
        self.layout.copy_into(params, self.base)

    def sketch_update(self):
        """Sketch the model as it stands against the base: the SketchUpdate to send.
        ValueError when the update is not finite."""
        if self.layout is None:
            raise RuntimeError("FedSketchWorker: no model loaded yet (the update is a "
                               "difference to the server's broadcast model)")
        dev, P = self.base.device, self.layout.P
        w = self.layout.flatten(ModelUtil(self.trainer.model).get_parameter_dict(detach=True),
                                device=dev)
        table = torch.empty((self.rows, self.cols), dtype=torch.float32, device=dev)
        stats = torch.empty(4, dtype=torch.int32, device=dev)
        _native.sketch(w, self.base, P, self.rows, self.cols, self.seed, self.stream_id, table,
                       stats, self.workspace)
        nonfinite = int(stats[0])
        if nonfinite:
            raise ValueError(f"worker {self.worker_id}: {nonfinite} coordinates of the update are "
                             "not finite (training diverged); nothing is sent")
        return SketchUpdate(table, P)

    def __send_sketch(self, **kwargs):
        trainer = kwargs["model_executor"]
        payload = self.sketch_update()
        dense = 4 * self.layout.numel
        log.warning("parameter_size is %s, sketch_parameter_size is %s, compression ratio is %s",
                    dense, payload.nbytes, float(payload.nbytes) / float(dense))
        self.worker_data_queue.add_task((self.worker_id, dataset_size(trainer.dataset), payload))
        self.load_model(self.worker_data_queue.get_result())
        log.info("end load_parameter_dict")
