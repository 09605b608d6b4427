"""FedAvg server (reference: servers/fed_server.py:11-91).

Same hooks, same round protocol, same return objects; ``get_subset_model`` is
one ``dls_fedavg_f32`` launch over the clients' HBM rows instead of a Python
loop of K x (#tensors) torch ops, bit-exact with the reference's op order.
"""
import copy
import logging
import math

from .. import _native
from ..aggregation import ClientParameters, ClientUpdateStore
from ..layout import ParameterLayout
from ..model_util import ModelUtil
from ..task_queue import RepeatedResult
from .server import Server

log = logging.getLogger("distributed_learning_simulator_amd")

_MODES = {"exact": _native.FEDAVG_EXACT, "fma": _native.FEDAVG_FMA}
_RULES = ("mean", "median", "trimmed_mean", "multi_krum", "geometric_median", "centered_clip",
          "mean_around_median", "bulyan")
_BYZANTINE_RULES = ("multi_krum", "bulyan", "mean_around_median")
_GM_ITERS, _GM_NU = 3, 1e-6  # the defaults of RFA (Pillutla et al.)
_CC_TAU, _CC_ITERS = 10.0, 3


class FedServer(Server):
    """``aggregation_rule`` selects what a round (and ``get_subset_model``) computes
    from the clients' rows:

    * ``"mean"`` (default): the reference's weighted mean, ``aggregation_mode``
      "exact" or "fma" (dls_fedavg_f32);
    * ``"trimmed_mean"``: per coordinate, the ``trim`` lowest and ``trim`` highest
      client values are dropped and the rest averaged (Yin et al. 2018;
      dls_trimmed_mean_f32); ``"median"``: the coordinate-wise median;
    * ``"multi_krum"``: whole updates are scored by the sum of their squared
      distances to their K - ``byzantine`` - 2 nearest neighbours
      (dls_pairwise_sqdist_f32) and the ``krum_select`` best-scored ones (default
      K - ``byzantine``) are averaged unweighted (Blanchard et al. 2017);
      ``krum_select=1`` is classic Krum.  ``last_selection`` / ``last_scores``
      hold the latest choice;
    * ``"geometric_median"``: the point that minimises the sum of Euclidean
      distances to the updates, by ``gm_iters`` smoothed Weiszfeld steps
      (smoothing ``gm_nu``, in the units of the parameters) from the coordinate-wise
      median (RFA, Pillutla et al.; dls_weiszfeld_step_f32): an outlier is
      down-weighted by 1 / distance instead of dropped, a client with a non-finite
      update is rejected.  ``last_distances`` / ``last_rejected`` hold the latest
      call's distances to the aggregate and rejected workers;
    * ``"centered_clip"``: centered clipping (Karimireddy, He & Jaggi 2021;
      dls_centered_clip_step_f32): ``cc_iters`` times the aggregate moves from where
      it is by the mean of the clients' differences to it, every difference longer
      than ``cc_tau`` shortened to ``cc_tau`` first, so a client pulls a step by at
      most cc_tau / K however far away it sits and the clients inside the radius
      count as in the plain mean.  It starts from the previous global model
      (``prev_model``; from the coordinate-wise median while there is none, as in
      round 1 of a server without a tester); ``cc_iters=1`` is norm clipping (Sun
      et al. 2019).  ``cc_tau`` is in the units of the parameters:
      ``last_distances`` of a trial round shows the scale to choose it from.  Like
      the other robust rules it ignores the sample counts; a client with a
      non-finite update is rejected.  ``last_clip_scales`` holds the last step's
      scale per worker (1.0: not clipped) beside ``last_distances`` /
      ``last_rejected``;
    * ``"mean_around_median"``: per coordinate, the K - ``byzantine`` consecutive
      sorted values closest to the median are averaged (MeaMed, Xie, Koyejo & Gupta
      2018; dls_mean_around_median_f32): unlike the trimmed mean the kept window is
      not centred, it slides to where the values cluster.  2*``byzantine`` < K;
    * ``"bulyan"``: Bulyan (El Mhamdi, Guerraoui & Rouault 2018): K - 2*``byzantine``
      whole updates are chosen by iterated Krum on the squared distances
      (dls_pairwise_sqdist_f32), then every coordinate is the mean of the K -
      4*``byzantine`` chosen values closest to their median
      (dls_mean_around_median_f32), so a single poisoned coordinate cannot hide
      inside a small Euclidean distance.  4*``byzantine`` + 3 <= K.
      ``last_selection`` (in pick order) / ``last_scores`` hold the latest choice.

    The robust rules ignore the clients' sample counts n_i (every client counts
    once), take at most ``_native.ROBUST_MAX_K`` clients and are bit-identical for
    any arrival order.  Hooks, ``prev_model``, ``get_metric`` and the round protocol
    are the same for every rule."""

    # why a subclass cannot run the robust rules (None: it can)
    _robust_unsupported = None

    def __init__(self, aggregation_mode="exact", aggregation_rule="mean", trim=0, byzantine=0,
                 krum_select=None, gm_iters=_GM_ITERS, gm_nu=_GM_NU, cc_tau=_CC_TAU,
                 cc_iters=_CC_ITERS, **kwargs):
        if aggregation_mode not in _MODES:
            raise ValueError(f"aggregation_mode must be one of {sorted(_MODES)}, not {aggregation_mode!r}")
        self._check_rule(aggregation_rule, trim, aggregation_mode, kwargs.get("worker_number"),
                         byzantine, krum_select, gm_iters, gm_nu, cc_tau, cc_iters)
        super().__init__(**kwargs)
        _native.require_gpu()
        self.round = 0
        self.aggregation_mode = aggregation_mode
        self.aggregation_rule = aggregation_rule
        self.trim = int(trim)
        self.byzantine = int(byzantine)
        self.krum_select = None if krum_select is None else int(krum_select)
        self.last_selection = ()
        self.last_scores = {}
        self.gm_iters = gm_iters
        self.gm_nu = float(gm_nu)
        self.last_distances = {}
        self.last_rejected = ()
        self.cc_tau = float(cc_tau)
        self.cc_iters = cc_iters
        self.last_clip_scales = {}
        self.parameters: ClientParameters = ClientParameters(self._make_store)
        self.__prev_model = copy.deepcopy(
            ModelUtil(self.tester.model).get_parameter_dict()) if self.tester is not None else {}
        self.worker_data_queue.put_result(
            RepeatedResult(data=self.prev_model, num=self.clients_per_round))

    @classmethod
    def _check_rule(cls, rule, trim, mode, worker_number, byzantine=0, krum_select=None,
                    gm_iters=_GM_ITERS, gm_nu=_GM_NU, cc_tau=_CC_TAU, cc_iters=_CC_ITERS):
        if rule not in _RULES:
            raise ValueError(f"aggregation_rule must be one of {list(_RULES)}, not {rule!r}")
        if isinstance(trim, bool) or not isinstance(trim, int) or trim < 0:
            raise ValueError(f"trim must be a non-negative integer, not {trim!r}")
        if rule != "trimmed_mean" and trim != 0:
            raise ValueError(f"trim={trim} needs aggregation_rule='trimmed_mean', not {rule!r}")
        if isinstance(byzantine, bool) or not isinstance(byzantine, int) or byzantine < 0:
            raise ValueError(f"byzantine must be a non-negative integer, not {byzantine!r}")
        if krum_select is not None and (isinstance(krum_select, bool)
                                        or not isinstance(krum_select, int)):
            raise ValueError(f"krum_select must be an integer or None, not {krum_select!r}")
        if (rule not in _BYZANTINE_RULES and byzantine != 0) or (rule != "multi_krum"
                                                                  and krum_select is not None):
            raise ValueError(f"byzantine={byzantine} / krum_select={krum_select} needs "
                             f"aggregation_rule='multi_krum', not {rule!r}")
        if isinstance(gm_iters, bool) or not isinstance(gm_iters, int) or gm_iters < 1:
            raise ValueError(f"gm_iters must be a positive integer, not {gm_iters!r}")
        if (isinstance(gm_nu, bool) or not isinstance(gm_nu, (int, float))
                or not math.isfinite(gm_nu) or gm_nu <= 0):
            raise ValueError(f"gm_nu must be a positive finite number, not {gm_nu!r}")
        if rule != "geometric_median" and (gm_iters != _GM_ITERS or gm_nu != _GM_NU):
            raise ValueError(f"gm_iters={gm_iters} / gm_nu={gm_nu} needs "
                             f"aggregation_rule='geometric_median', not {rule!r}")
        if isinstance(cc_iters, bool) or not isinstance(cc_iters, int) or cc_iters < 1:
            raise ValueError(f"cc_iters must be a positive integer, not {cc_iters!r}")
        if (isinstance(cc_tau, bool) or not isinstance(cc_tau, (int, float))
                or not math.isfinite(cc_tau) or cc_tau <= 0):
            raise ValueError(f"cc_tau must be a positive finite number, not {cc_tau!r}")
        if rule != "centered_clip" and (cc_tau != _CC_TAU or cc_iters != _CC_ITERS):
            raise ValueError(f"cc_tau={cc_tau} / cc_iters={cc_iters} needs "
                             f"aggregation_rule='centered_clip', not {rule!r}")
        if rule == "mean":
            return
        if cls._robust_unsupported is not None:
            raise ValueError(
                f"{cls.__name__} does not support aggregation_rule={rule!r} "
                f"({cls._robust_unsupported}); the one-process FedServer "
                "(factory.get_server('fed', ...)) is the server that runs the median and "
                "trimmed-mean rules")
        if mode != "exact":
            raise ValueError(f"aggregation_mode={mode!r} applies to aggregation_rule='mean' only; "
                             f"{rule!r} has one arithmetic")
        if worker_number is not None:
            if worker_number > _native.ROBUST_MAX_K:
                raise ValueError(f"aggregation_rule={rule!r} takes at most ROBUST_MAX_K="
                                 f"{_native.ROBUST_MAX_K} clients, not worker_number={worker_number}")
            if 2 * trim >= worker_number:
                raise ValueError(f"trim={trim} leaves nothing of worker_number={worker_number} "
                                 "clients (2*trim < worker_number is needed)")
            if rule == "multi_krum":
                if 2 * byzantine + 3 > worker_number:
                    raise ValueError(f"byzantine={byzantine} is too many for worker_number="
                                     f"{worker_number} (2*byzantine + 3 <= worker_number is needed)")
                if krum_select is not None and not 1 <= krum_select <= worker_number - byzantine:
                    raise ValueError(f"krum_select={krum_select} must be in 1..worker_number - "
                                     f"byzantine = {worker_number - byzantine}")
            if rule == "mean_around_median" and 2 * byzantine >= worker_number:
                raise ValueError(f"byzantine={byzantine} leaves no majority of worker_number="
                                 f"{worker_number} clients (2*byzantine < worker_number is "
                                 "needed)")
            if rule == "bulyan" and 4 * byzantine + 3 > worker_number:
                raise ValueError(f"byzantine={byzantine} is too many for worker_number="
                                 f"{worker_number} (4*byzantine + 3 <= worker_number is needed)")
        elif rule == "multi_krum" and krum_select is not None and krum_select < 1:
            raise ValueError(f"krum_select={krum_select} must be at least 1")

    @property
    def clients_per_round(self):
        """Clients whose updates this process receives per round (all of them here;
        the sharded servers in ``distributed.py`` override it)."""
        return self.worker_number

    @property
    def store_capacity(self):
        """Client rows this process holds per round: its own clients (the sharded
        servers receive only their local ones; the sharded Shapley servers
        override this, they all-gather every client)."""
        return self.clients_per_round

    def _make_store(self, parameter_dict):
        return ClientUpdateStore(ParameterLayout.from_dict(parameter_dict), self.device,
                                 capacity=self.store_capacity)

    def get_metric(self, model, metric_type="acc"):
        """servers/fed_server.py:26-32 — load, run the tester, top-1 accuracy or loss."""
        if self.tester is None:
            return None
        ModelUtil(self.tester.model).load_parameter_dict(model)
        self.tester.inference()
        if metric_type == "acc":
            return self.tester.accuracy_metric.get_accuracy(1)
        return self.tester.loss_metric.get_loss(1).data.item()

    @property
    def prev_model(self):
        return self.__prev_model

    def _set_prev_model(self, model):
        self.__prev_model = model

    def _process_client_parameter(self, client_parameter: dict):
        return client_parameter

    def _before_aggregate(self):
        """Hook when this process has all its clients of the round (sharded servers)."""

    def _process_aggregated_parameter(self, aggregated_parameter: dict):
        return aggregated_parameter

    def get_subset_model(self, client_subset):
        """servers/fed_server.py:44-66 (empty subset -> previous model)."""
        if not client_subset:
            return self.__prev_model
        ids = list(client_subset)
        store = self.parameters.store
        # multi-Krum, Bulyan, the geometric median and centered clipping report, break ties and
        # order by worker id (no subclass that overrides _aggregate runs those rules)
        extra = {"ids": ids} if self.aggregation_rule in ("multi_krum", "geometric_median",
                                                          "centered_clip", "bulyan") else {}
        flat = self._aggregate(store, [self.parameters.row_of(i) for i in ids],
                               [self.parameters.n_of(i) for i in ids], **extra)
        return store.layout.views(flat)

    def _aggregate(self, store, rows, ns, total=None, ids=None):
        if self.aggregation_rule == "mean":
            return store.fedavg(rows, ns, mode=_MODES[self.aggregation_mode], total=total)
        K = len(rows)
        if K > _native.ROBUST_MAX_K:
            raise ValueError(f"aggregation_rule={self.aggregation_rule!r} takes at most "
                             f"ROBUST_MAX_K={_native.ROBUST_MAX_K} clients, not {K}")
        if self.aggregation_rule == "median":
            return store.median(rows)
        if self.aggregation_rule == "multi_krum":
            return self._multi_krum(store, rows, list(range(K)) if ids is None else ids)
        if self.aggregation_rule == "geometric_median":
            return self._geometric_median(store, rows, list(range(K)) if ids is None else ids)
        if self.aggregation_rule == "centered_clip":
            return self._centered_clip(store, rows, list(range(K)) if ids is None else ids)
        if self.aggregation_rule == "bulyan":
            return self._bulyan(store, rows, list(range(K)) if ids is None else ids)
        if self.aggregation_rule == "mean_around_median":
            if 2 * self.byzantine >= K:
                raise ValueError(f"byzantine={self.byzantine} leaves no majority of a subset of "
                                 f"{K} clients (2*byzantine < len(subset) is needed)")
            return store.mean_around_median(rows, K - self.byzantine)
        if 2 * self.trim >= K:
            raise ValueError(f"trim={self.trim} leaves nothing of a subset of {K} clients "
                             "(2*trim < len(subset) is needed)")
        return store.trimmed_mean(rows, self.trim)

    def _multi_krum(self, store, rows, ids):
        K, f = len(rows), self.byzantine
        if 2 * f + 3 > K:
            raise ValueError(f"byzantine={f} is too many for a subset of {K} clients "
                             "(2*byzantine + 3 <= len(subset) is needed)")
        select = K - f if self.krum_select is None else self.krum_select
        if select > K - f:
            raise ValueError(f"krum_select={select} exceeds len(subset) - byzantine = {K - f}")
        flat, selected, scores = store.multi_krum(rows, ids, f, select)
        self.last_selection = tuple(selected)
        self.last_scores = dict(zip(ids, scores))
        chosen = set(selected)
        log.info("multi_krum: kept %s of %s clients, rejected workers %s", len(selected), K,
                 [i for i in ids if i not in chosen])
        return flat

    def _bulyan(self, store, rows, ids):
        K, f = len(rows), self.byzantine
        if 4 * f + 3 > K:
            raise ValueError(f"byzantine={f} is too many for a subset of {K} clients "
                             "(4*byzantine + 3 <= len(subset) is needed)")
        flat, selected, scores = store.bulyan(rows, ids, f)
        self.last_selection = tuple(selected)
        self.last_scores = scores
        chosen = set(selected)
        log.info("bulyan: kept %s of %s clients, rejected workers %s", len(selected), K,
                 [i for i in ids if i not in chosen])
        return flat

    def _geometric_median(self, store, rows, ids):
        flat, info = store.geometric_median(rows, ids, self.gm_iters, self.gm_nu)
        self.last_distances = info["distances"]
        self.last_rejected = tuple(info["rejected"])
        log.info("geometric_median: %s of %s clients, rejected workers %s, objective %s -> %s",
                 len(info["distances"]), len(rows), list(self.last_rejected),
                 info["objective"][0], info["objective"][-1])
        return flat

    def _centered_clip(self, store, rows, ids):
        # from the model the clients started from; the coordinate-wise median of the
        # subset while there is none (round 1 of a server without a tester)
        prev = self.__prev_model
        if prev and store.accepts(prev):
            start = store.layout.flatten(prev, device=store.U.device)
        else:
            start = store.median(rows)
        flat, info = store.centered_clip(rows, ids, start, self.cc_tau, self.cc_iters)
        self.last_distances = info["distances"]
        self.last_rejected = tuple(info["rejected"])
        self.last_clip_scales = info["scales"]
        log.info("centered_clip: %s of %s clients, %s clipped in the last step (tau %s), "
                 "rejected workers %s, steps of length %s",
                 len(info["distances"]), len(rows),
                 sum(1 for s in info["scales"].values() if s < 1.0), self.cc_tau,
                 list(self.last_rejected), info["moved"])
        return flat

    def _process_worker_data(self, data, __):
        worker_id, training_dataset_size, parameter_dict = data
        self.parameters[worker_id] = (
            training_dataset_size,
            self._process_client_parameter(parameter_dict),
        )
        if len(self.parameters) != self.clients_per_round:
            log.debug("%s %s,skip", len(self.parameters), self.clients_per_round)
            return None
        self._before_aggregate()
        self.round += 1
        log.info("begin aggregating")
        avg_parameter = self.get_subset_model(self.parameters.keys())
        data = self._process_aggregated_parameter(avg_parameter)
        self.__prev_model = copy.deepcopy(data)
        acc = self.get_metric(self.prev_model)
        log.info("end aggregating, test accuracy is %s", acc)
        self.parameters.clear()
        # one copy per client that feeds this process (its local clients when sharded)
        return RepeatedResult(data=data, num=self.clients_per_round)
