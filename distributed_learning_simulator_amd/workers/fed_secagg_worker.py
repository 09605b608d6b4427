"""Secure-aggregation worker (Bonawitz et al. 2017, "Practical Secure Aggregation for
Privacy-Preserving Machine Learning"), as simulated.

The reference simulator has no secure aggregation; this worker keeps the FedAvg protocol on
the task queue and hides its update from the server: after each ``trainer.train()`` the
update ``w - base`` (w the trained model, base the model the worker last loaded) is quantised
to ``secagg_bits`` bits of fixed point, multiplied by the worker's weight and masked in the
ring Z_2^32 by one ``dls_secagg_mask_f32``: its self mask and one pair mask per other
participant of the round, all drawn from the library's Philox stream.  What it sends,
``(worker_id, n, MaskedUpdate(...))``, is uniformly random to anyone who does not hold the
masks; the pair masks cancel in the sum the ``FedSecAggServer`` forms.

Key agreement is simulated: one ``secagg_seed`` stands for every pair's agreed key and every
worker's self-mask seed.  A deployment derives them per pair (Diffie-Hellman) and per client
and secret-shares them; a seed that is published protects nothing.
"""
import logging

import torch

from .. import _native
from ..aggregation import secagg_client_streams
from ..layout import ParameterLayout
from ..model_util import ModelUtil
from ..trainer import ModelExecutorCallbackPoint
from .fed_worker import FedWorker, dataset_size

log = logging.getLogger("distributed_learning_simulator_amd")

SECAGG_DEFAULTS = {"secagg_bits": 20, "secagg_frac_bits": 16, "secagg_seed": 0,
                   "secagg_weighted": False}


class MaskedUpdate:
    """A client's uplink payload: ``y`` (int32 [P], the uint32 bit patterns of the masked,
    quantised update over the flat ``ParameterLayout`` row), the ``round`` its masks belong
    to, the fixed-point format (``frac_bits``, ``bits``), the integer ``weight`` the update
    was multiplied by, and ``saturated``, the number of coordinates that hit the range."""

    __slots__ = ("y", "P", "round", "frac_bits", "bits", "weight", "saturated")

    def __init__(self, y, P, round, frac_bits, bits, weight, saturated):
        self.y, self.P, self.round = y, int(P), int(round)
        self.frac_bits, self.bits, self.weight = int(frac_bits), int(bits), int(weight)
        self.saturated = int(saturated)

    @property
    def nbytes(self):
        return self.P * 4


def check_secagg_format(bits, frac_bits, seed):
    """ValueError unless 2 <= bits <= 31, 0 <= frac_bits <= 126 and 0 <= seed < 2^64."""
    for name, v, lo, hi, text in (("secagg_bits", bits, 2, 31, "31"),
                                  ("secagg_frac_bits", frac_bits, 0, 126, "126"),
                                  ("secagg_seed", seed, 0, (1 << 64) - 1, "2^64 - 1")):
        if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
            raise ValueError(f"{name} must be an integer in {lo}..{text}, not {v!r}")


def to_stream_table(ids, device):
    """The device table of the uint64 stream ids ``ids`` (held as int64 bit patterns), or None
    for none."""
    if not ids:
        return None
    return torch.tensor([i - (1 << 64) if i >= 1 << 63 else i for i in ids],
                        dtype=torch.int64).to(device)


class FedSecAggWorker(FedWorker):
    """``secagg_bits`` (default 20) and ``secagg_frac_bits`` (default 16): an update
    coordinate is sent as round(d * 2^frac_bits) clamped to +-(2^(bits-1) - 1), so the
    defaults cover +-8 at a resolution of 1.5e-5; ``secagg_seed``: the simulation's stand-in
    for all agreed keys (the server's must equal it); ``secagg_weighted``: False (default)
    weights every worker 1, as DP-FedAvg and the robust rules do, True by its sample count;
    ``participants``: the worker ids of the round's key agreement, this worker's among them
    (every round of this simulation has the same)."""

    def __init__(self, participants, secagg_bits=SECAGG_DEFAULTS["secagg_bits"],
                 secagg_frac_bits=SECAGG_DEFAULTS["secagg_frac_bits"],
                 secagg_seed=SECAGG_DEFAULTS["secagg_seed"],
                 secagg_weighted=SECAGG_DEFAULTS["secagg_weighted"], **kwargs):
        check_secagg_format(secagg_bits, secagg_frac_bits, secagg_seed)
        self.secagg_bits, self.secagg_frac_bits = secagg_bits, secagg_frac_bits
        self.secagg_seed, self.secagg_weighted = secagg_seed, bool(secagg_weighted)
        worker_id = kwargs.get("worker_id")
        secagg_client_streams(worker_id, participants, 0)  # the ids' ValueError, if any
        self.participants = tuple(sorted(participants))
        if len(self.participants) > _native.ROBUST_MAX_K:
            raise ValueError(f"fed_secagg takes at most ROBUST_MAX_K={_native.ROBUST_MAX_K} "
                             f"participants, not {len(self.participants)}")
        super().__init__(**kwargs)
        # replaces FedWorker's dense send (same callback name)
        self.trainer.add_named_callback(ModelExecutorCallbackPoint.AFTER_EXECUTE,
                                        "send_parameter", self.__send_masked)
        self.layout = None
        self.base = None
        self.sent_rounds = 0  # the masks of round r are used once: r = sent_rounds + 1

    def train(self, device):
        self.trainer.set_device(device)
        self.load_model(self.worker_data_queue.get_result())
        log.info("end load initial parameter_dict")
        for _ in range(self.round):
            self.trainer.train()

    def load_model(self, parameter_dict):
        """Load the server's model; its bits become the base of the next update."""
        model = self.trainer.model
        ModelUtil(model).load_parameter_dict(parameter_dict)
        params = ModelUtil(model).get_parameter_dict(detach=True)
        if self.layout is None:
            dev = next(iter(params.values())).device
            self.layout = ParameterLayout.from_dict(params)
            self.base = torch.zeros(self.layout.P, dtype=torch.float32, device=dev)
        self.layout.copy_into(params, self.base)

    def masked_update(self, samples):
        """Encode and mask the model as it stands against the base: the MaskedUpdate of the
        next round.  ValueError, and the round is not consumed, when the update is not
        finite."""
        if self.layout is None:
            raise RuntimeError("FedSecAggWorker: no model loaded yet (the update is a difference "
                               "to the server's broadcast model)")
        dev, P = self.base.device, self.layout.P
        weight = int(samples) if self.secagg_weighted else 1
        if not 1 <= weight < 1 << 32:
            raise ValueError(f"worker {self.worker_id}: secagg_weighted needs a sample count in "
                             f"1..2^32 - 1, not {samples!r}")
        round_ = self.sent_rounds + 1
        add, sub = secagg_client_streams(self.worker_id, self.participants, round_)
        w = self.layout.flatten(ModelUtil(self.trainer.model).get_parameter_dict(detach=True),
                                device=dev)
        y = torch.empty(P, dtype=torch.int32, device=dev)
        stats = torch.zeros(2, dtype=torch.int32, device=dev)
        _native.secagg_mask(w, self.base, P, self.secagg_frac_bits, self.secagg_bits, weight,
                            to_stream_table(add, dev), to_stream_table(sub, dev),
                            self.secagg_seed, y, stats)
        saturated, nonfinite = stats.tolist()
        if nonfinite:
            raise ValueError(f"worker {self.worker_id}: {nonfinite} coordinates of the update are "
                             "not finite (training diverged); nothing is sent")
        self.sent_rounds = round_
        log.info("worker %s round %s: %s of %s coordinates saturated at +-%s (share %s)",
                 self.worker_id, round_, saturated, self.layout.numel,
                 float((1 << (self.secagg_bits - 1)) - 1) / float(1 << self.secagg_frac_bits),
                 float(saturated) / float(max(self.layout.numel, 1)))
        return MaskedUpdate(y, P, round_, self.secagg_frac_bits, self.secagg_bits, weight,
                            saturated)

    def __send_masked(self, **kwargs):
        trainer = kwargs["model_executor"]
        n = dataset_size(trainer.dataset)
        payload = self.masked_update(n)
        self.worker_data_queue.add_task((self.worker_id, n, payload))
        self.load_model(self.worker_data_queue.get_result())
        log.info("end load_parameter_dict")
