"""FedAvg server (reference: servers/fed_server.py:11-91).

Same hooks, same round protocol, same return objects; ``get_subset_model`` is
one ``dls_fedavg_f32`` launch over the clients' HBM rows instead of a Python
loop of K x (#tensors) torch ops, bit-exact with the reference's op order.
"""
import collections
import copy
import logging

import torch

from .. import _native
from ..aggregation import (ATTACKS, ClientParameters, ClientUpdateStore, attack_coefficients,
                           dp_epsilon, finite_number)
from ..layout import ParameterLayout
from ..model_util import ModelUtil
from ..task_queue import RepeatedResult
from .server import Server

log = logging.getLogger("distributed_learning_simulator_amd")

_MODES = {"exact": _native.FEDAVG_EXACT, "fma": _native.FEDAVG_FMA}
SERVER_OPTIMIZERS = tuple(_native.SERVER_OPT_KINDS)  # sgd: FedAvgM; the others: Reddi et al.


# Every constructor option, declared once, in the order a feature's options are checked:
# its default (gm_*: RFA's, Pillutla et al.; fg_kappa: the paper's confidence; None is
# resolved later), its kind (_check_kinds: the type it is held as, and an integer's minimum
# or which reals), its feature and who takes it (a misplaced option is told the first).
_Option = collections.namedtuple("_Option", "default kind feature owners")
OPTIONS = {
    "trim": _Option(0, (int, 0), "rule", ("trimmed_mean",)),
    "byzantine": _Option(0, (int, 0), "rule", ("multi_krum", "mean_around_median", "bulyan")),
    "krum_select": _Option(None, (int, None), "rule", ("multi_krum",)),
    "gm_iters": _Option(3, (int, 1), "rule", ("geometric_median",)),
    "gm_nu": _Option(1e-6, (float, "positive"), "rule", ("geometric_median",)),
    "cc_iters": _Option(3, (int, 1), "rule", ("centered_clip",)),
    "cc_tau": _Option(10.0, (float, "positive"), "rule", ("centered_clip",)),
    "fg_kappa": _Option(1.0, (float, "positive"), "rule", ("foolsgold",)),
    "attack_z": _Option(None, (float, "finite"), "attack", ("alie",)),
    "attack_eps": _Option(0.1, (float, "finite"), "attack", ("ipm",)),
    "attack_scale": _Option(1.0, (float, "finite"), "attack", ("sign_flip",)),
    "server_lr": _Option(None, (float, "positive"), "server_opt", SERVER_OPTIMIZERS),
    "server_momentum": _Option(None, (float, "in [0, 1)"), "server_opt", SERVER_OPTIMIZERS),
    "server_beta2": _Option(0.99, (float, "in [0, 1)"), "server_opt", ("adam", "yogi")),
    "server_tau": _Option(1e-3, (float, "positive"), "server_opt", ("adagrad", "adam", "yogi")),
    # differentially private FedAvg: on when dp_clip is set, which the others need
    "dp_clip": _Option(None, (float, "positive"), "dp", ("dp_clip",)),
    "dp_noise_multiplier": _Option(1.0, (float, "non-negative"), "dp", ("dp_clip",)),
    "dp_seed": _Option(0, (int, 0), "dp", ("dp_clip",)),
    "dp_delta": _Option(1e-5, (float, "in (0, 1)"), "dp", ("dp_clip",)),
}
DEFAULTS, ATTACK_DEFAULTS, SERVER_OPT_DEFAULTS, DP_DEFAULTS = (
    {name: o.default for name, o in OPTIONS.items() if o.feature == feature}
    for feature in ("rule", "attack", "server_opt", "dp"))
# Every robust rule needs 2*trim < K (trim is 0 under all but the trimmed mean).
_TRIM_FITS = (lambda K, p: 2 * p["trim"] < K,
              "trim={trim} leaves nothing of {clients} (2*trim < {n} is needed)")
# The rules, in the order they are listed to the user.  ids: whether get_subset_model
# hands the rule the worker ids (it reports, breaks ties and orders by them); count: its
# condition on the number of clients K, a predicate of (K, parameters) and the message
# when it fails (_count_error fills in {group}, {clients} and {n}); run: the FedServer
# method (store, rows, ids) -> flat; owns: the options of OPTIONS the rule takes.
RULES = {
    "mean": dict(ids=False, count=None, run=None),  # store.fedavg, with the n_i
    "median": dict(ids=False, count=None, run="_median"),
    "trimmed_mean": dict(ids=False, count=None, run="_trimmed_mean"),
    "multi_krum": dict(ids=True, run="_multi_krum", count=(
        lambda K, p: 2 * p["byzantine"] + 3 <= K,
        "byzantine={byzantine} is too many for {group} (2*byzantine + 3 <= {n} is needed)")),
    "geometric_median": dict(ids=True, count=None, run="_geometric_median"),
    "centered_clip": dict(ids=True, count=None, run="_centered_clip"),
    "mean_around_median": dict(ids=False, run="_mean_around_median", count=(
        lambda K, p: 2 * p["byzantine"] < K,
        "byzantine={byzantine} leaves no majority of {clients} (2*byzantine < {n} is needed)")),
    "bulyan": dict(ids=True, run="_bulyan", count=(
        lambda K, p: 4 * p["byzantine"] + 3 <= K,
        "byzantine={byzantine} is too many for {group} (4*byzantine + 3 <= {n} is needed)")),
    "foolsgold": dict(ids=True, count=None, run="_foolsgold"),
}
# The rule options that are checked, and listed to a rule that takes none of them, together.
_LISTED = (("trim",), ("byzantine", "krum_select"), ("gm_iters", "gm_nu"), ("cc_tau", "cc_iters"),
           ("fg_kappa",))
for _rule, _row in RULES.items():
    _row["owns"] = tuple(n for names in _LISTED for n in names if _rule in OPTIONS[n].owners)


def _count_error(rule, K, p, subset):
    """The message for K clients that robust ``rule`` with the parameters ``p`` cannot
    take, or None; K is the constructor's worker_number, or a subset's length."""
    if K > _native.ROBUST_MAX_K:
        return (f"aggregation_rule={rule!r} takes at most ROBUST_MAX_K={_native.ROBUST_MAX_K} "
                f"clients, not {K if subset else f'worker_number={K}'}")
    group = f"a subset of {K} clients" if subset else f"worker_number={K}"
    for fits, text in filter(None, (_TRIM_FITS, RULES[rule]["count"])):
        if not fits(K, p):
            return text.format(group=group, clients=group if subset else group + " clients",
                               n="len(subset)" if subset else "worker_number",
                               trim=p["trim"], byzantine=p["byzantine"])
    return None


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
      ``last_selection`` (in pick order) / ``last_scores`` hold the latest choice;
    * ``"foolsgold"``: FoolsGold (Fung, Yoon & Beschastnikh 2020), the defence against
      sybils: clients whose accumulated updates keep pointing the same way are
      down-weighted, whatever their number; no count of bad clients is needed.  Every
      round each client's update, taken from the previous global model (from the
      coordinate-wise median of the round's rows while there is none, as in round 1 of
      a server without a tester), is added to that worker's history row and the cosines
      of the histories come out of the same visit (dls_history_gram_f32), exactly once
      per round, when all updates have arrived and after the attack;
      ``aggregation.foolsgold_weights`` turns them into a weight alpha in [0, 1] per
      client (``fg_kappa`` is the paper's confidence: larger pushes the weights towards
      0 and 1) and the aggregate is the alpha-weighted mean of the updates (one
      dls_centered_clip_step_f32).  ``get_subset_model`` weights a subset from the
      round's cached similarities and folds nothing.  ``last_weights`` /
      ``last_similarity`` hold each worker's alpha and maximum cosine after pardoning,
      ``last_rejected`` the workers whose history is not finite; ``reset_history``
      forgets one worker's history or all.

    ``attack`` makes the workers listed in ``attackers`` Byzantine: once a round's
    updates have all arrived, their rows are rewritten in place before anything reads
    them, so hooks, ``self.parameters[w]``, Shapley coalitions and every rule above see
    the attacker exactly as if the worker had sent the crafted update.

    * ``"alie"``: "a little is enough" (Baruch, Baruch & Goldberg 2019): every attacker
      sends, per coordinate, mean - z * std of the honest updates
      (dls_craft_rows_f32); z = ``attack_z``, by default ``aggregation.alie_z`` of the
      worker and attacker counts;
    * ``"ipm"``: inner product manipulation (Xie, Koyejo & Gupta 2019): every attacker
      sends -``attack_eps`` times the honest mean update, taken relative to the
      previous global model (relative to zero while there is none);
    * ``"sign_flip"``: every attacker sends its own update mirrored at the previous
      global model and scaled by ``attack_scale``.

    ``last_attack`` holds the latest round's attack, attackers and coefficients.

    ``server_optimizer`` turns the round's aggregate, of whichever rule, into the next
    global model through a server optimizer instead of storing it as it is (None, the
    default and the reference's behaviour: server learning rate 1, no momentum).  The
    pseudo-gradient is d = aggregate - previous model and one fused launch
    (dls_server_opt_step_f32) updates the moments and the model:

    * ``"sgd"``: server momentum, FedAvgM (Hsu et al. 2019): m <- ``server_momentum`` *
      m + d, model += ``server_lr`` * m;
    * ``"adagrad"``, ``"adam"``, ``"yogi"``: FedAdagrad, FedAdam and FedYogi (Reddi et al.
      2021, without bias correction, as in the paper): m <- beta1 * m + (1 - beta1) * d
      with beta1 = ``server_momentum``; v <- v + d^2 (adagrad), beta2 * v + (1 - beta2) *
      d^2 (adam) or v - (1 - beta2) * d^2 * sign(v - d^2) (yogi) with beta2 =
      ``server_beta2``; model += ``server_lr`` * m / (sqrt(v) + ``server_tau``).  m starts at
      zero and v at ``server_tau``^2.

    ``server_lr`` defaults to 1.0 for sgd and to 0.01 for the adaptive optimizers (this
    project's choice: Reddi et al. tune it per task between 1e-3 and 1), ``server_momentum``
    to 0.0 for sgd (with ``server_lr`` 1.0 that is plain FedAvg again, up to one rounding)
    and 0.9 for the adaptive ones, ``server_beta2`` to 0.99 and ``server_tau`` to 1e-3.  A
    parameter given to an optimizer that does not use it raises.  While there is no
    previous model (round 1 of a server without a tester) the aggregate becomes the model
    as it is and the state is created.  An aggregate that is not finite raises
    ``ValueError`` before the step and leaves the state alone: a poisoned m or v would
    never recover.  ``get_subset_model`` stays the pure aggregate of the subset (what the
    subset would have averaged to).  ``server_opt_state`` holds the step count and the
    views of m and v, ``last_server_step`` the Euclidean norms of the latest
    pseudo-gradient and applied update, ``reset_server_optimizer()`` starts the state
    over.

    ``dp_clip`` turns the round into client-level differentially private FedAvg (McMahan,
    Ramage, Talwar & Zhang 2018; None, the default: off).  Every client's update, taken
    from the previous global model, is clipped to the Euclidean norm ``dp_clip`` (in the
    units of the parameters), the clipped updates are averaged, every client counting once
    (the sample counts are ignored, as the robust rules ignore them), and Gaussian noise of
    standard deviation ``dp_noise_multiplier`` * ``dp_clip`` / K is added to every
    coordinate: one distance pass and one fused launch that reads the rows once
    (dls_dp_clip_noise_step_f32, ``ClientUpdateStore.dp_mean``).  The noise is the
    library's Philox4x32-10 stream under the key ``dp_seed`` (an integer in 0..2^64 - 1)
    with the round number as the stream id, so a run is reproducible bit for bit and no two
    rounds share noise; its normals are truncated at sqrt(48 ln 2) ~ 5.768 standard
    deviations (probability 8e-9 per coordinate), and a ``dp_seed`` that is published is no
    secret: a deployment draws it from the operating system.  It needs
    ``aggregation_rule="mean"`` and ``aggregation_mode="exact"`` and at most
    ``_native.ROBUST_MAX_K`` clients, and a previous global model to clip against: a round
    without one (round 1 of a server without a tester) raises ``ValueError``.  A client with
    a non-finite update is rejected and K counts the others.  ``dp_noise_multiplier`` (z,
    default 1.0; 0 clips without noise and guarantees nothing) and ``dp_delta`` (default
    1e-5) set the guarantee: after T rounds the released models are (epsilon, dp_delta)-DP
    with epsilon = ``aggregation.dp_epsilon(z, T, dp_delta)`` under the adjacency "one
    client's clipped update replaced by zero, K fixed, every client in every round".  A
    ``dp_*`` option without ``dp_clip`` raises.  A ``server_optimizer``, if set, steps on the
    noised aggregate: post-processing, which keeps the guarantee.  ``last_dp`` holds the
    latest round's ``norms`` (each client's update norm), ``scales`` (1.0: not clipped),
    ``rejected``, ``sigma``, ``clipped_fraction``, ``releases`` and ``epsilon``.
    ``get_subset_model`` of such a server returns the clipped mean of the subset WITHOUT
    noise (the same entry point with sigma = 0): an analysis hook for Shapley-style callers,
    reproducible for any call order, and not a release: its result is not private and is
    not counted in ``epsilon``.

    The robust rules ignore the clients' sample counts n_i (every client counts
    once), take at most ``_native.ROBUST_MAX_K`` clients and are bit-identical for
    any arrival order.  Hooks, ``prev_model``, ``get_metric`` and the round protocol
    are the same for every rule."""

    # why a subclass cannot run a feature (None: it can); _check_runs words the refusal
    _robust_unsupported = None  # the robust rules
    _attack_unsupported = None  # the Byzantine client attacks
    _server_opt_unsupported = None  # a server optimizer
    _dp_unsupported = None  # differentially private FedAvg

    def __init__(self, aggregation_mode="exact", aggregation_rule="mean",
                 trim=DEFAULTS["trim"], byzantine=DEFAULTS["byzantine"],
                 krum_select=DEFAULTS["krum_select"], gm_iters=DEFAULTS["gm_iters"],
                 gm_nu=DEFAULTS["gm_nu"], cc_tau=DEFAULTS["cc_tau"], cc_iters=DEFAULTS["cc_iters"],
                 attack=None, attackers=(), attack_z=ATTACK_DEFAULTS["attack_z"],
                 attack_eps=ATTACK_DEFAULTS["attack_eps"],
                 attack_scale=ATTACK_DEFAULTS["attack_scale"], fg_kappa=DEFAULTS["fg_kappa"],
                 server_optimizer=None, server_lr=SERVER_OPT_DEFAULTS["server_lr"],
                 server_momentum=SERVER_OPT_DEFAULTS["server_momentum"],
                 server_beta2=SERVER_OPT_DEFAULTS["server_beta2"],
                 server_tau=SERVER_OPT_DEFAULTS["server_tau"], dp_clip=DP_DEFAULTS["dp_clip"],
                 dp_noise_multiplier=DP_DEFAULTS["dp_noise_multiplier"],
                 dp_seed=DP_DEFAULTS["dp_seed"], dp_delta=DP_DEFAULTS["dp_delta"], **kwargs):
        # the options by name (the first statement: only the arguments are bound yet)
        given = {name: v for name, v in locals().items() if name in OPTIONS}
        if aggregation_mode not in _MODES:
            raise ValueError(f"aggregation_mode must be one of {sorted(_MODES)}, not {aggregation_mode!r}")
        workers = kwargs.get("worker_number")
        self._check_rule(aggregation_rule, aggregation_mode, workers,
                         **{name: given[name] for name in DEFAULTS})
        attackers = self._check_attack(attack, attackers, worker_number=workers,
                                       **{name: given[name] for name in ATTACK_DEFAULTS})
        server_opt = self._check_server_opt(
            server_optimizer, **{name: given[name] for name in SERVER_OPT_DEFAULTS})
        self._check_dp(aggregation_rule, aggregation_mode, workers,
                       **{name: given[name] for name in DP_DEFAULTS})
        super().__init__(**kwargs)
        _native.require_gpu()
        self.round = 0
        self.dp_clip = None if dp_clip is None else float(dp_clip)
        self.dp_noise_multiplier = float(dp_noise_multiplier)
        self.dp_seed, self.dp_delta = dp_seed, float(dp_delta)
        self.last_dp = {}
        self._dp_releases = 0  # the rounds released so far: what epsilon is composed over
        self.server_optimizer = server_optimizer
        # the resolved lr, momentum, beta2, tau, and the fp32 values the kernel is handed
        self.server_lr, self.server_momentum, self.server_beta2, self.server_tau = \
            server_opt if server_opt else (None,) * 4
        self._server_opt_coeffs = _native.server_opt_coeffs(*server_opt) if server_opt else None
        self.last_server_step = {}
        self._server_opt_adopted = False  # "no previous model" is logged once
        self.aggregation_mode = aggregation_mode
        self.aggregation_rule = aggregation_rule
        self.attack = attack
        self.attackers = attackers
        for name in (*DEFAULTS, *ATTACK_DEFAULTS):  # held as the type of their kind
            v, o = given[name], OPTIONS[name]
            setattr(self, name, v if v is None and o.default is None else o.kind[0](v))
        self.last_selection = ()
        self.last_scores = {}
        self.last_distances = {}
        self.last_rejected = ()
        self.last_clip_scales = {}
        self.last_weights = {}
        self.last_similarity = {}
        self._fg_round = None  # the folded round: its worker ids, their G and the base
        self.last_attack = {}
        self.parameters: ClientParameters = ClientParameters(self._make_store)
        self.__prev_model = self._initial_model()
        self.worker_data_queue.put_result(
            RepeatedResult(data=self.prev_model, num=self.clients_per_round))

    @staticmethod
    def _check_kinds(p):
        """ValueError for an option in ``p`` that is not of its kind; a default None passes."""
        for name, v in p.items():
            default, (held, which) = OPTIONS[name][:2]
            if v is None and default is None:
                continue
            if held is float:
                finite_number(name, v, positive=which == "positive")
                if (which == "in [0, 1)" and not 0.0 <= v < 1.0) \
                        or (which == "in (0, 1)" and not 0.0 < v < 1.0) \
                        or (which == "non-negative" and v < 0.0):
                    raise ValueError(f"{name} must be {which}, not {v!r}")
            elif isinstance(v, bool) or not isinstance(v, int) or (which is not None and v < which):
                what = ("an integer or None" if which is None
                        else f"a {'positive' if which else 'non-negative'} integer")
                raise ValueError(f"{name} must be {what}, not {v!r}")

    @classmethod
    def _check_runs(cls, what, reason, runs):
        """ValueError if ``reason``, a ``_*_unsupported`` of this class, says it cannot run the
        feature ``what``; ``runs`` names the servers that do."""
        if reason is not None:
            raise ValueError(f"{cls.__name__} does not support {what} ({reason}); the one-process "
                             f"FedServer (factory.get_server('fed', ...)) {runs}")

    @classmethod
    def _check_rule(cls, rule, mode, worker_number, **parameters):
        """ValueError for a rule, or rule parameters (keywords of ``DEFAULTS``, the rest
        at their defaults), that no round could run."""
        if rule not in RULES:
            raise ValueError(f"aggregation_rule must be one of {list(RULES)}, not {rule!r}")
        p = {**DEFAULTS, **parameters}
        for names in _LISTED:
            cls._check_kinds({n: p[n] for n in DEFAULTS if n in names})
            if any(p[n] != DEFAULTS[n] and rule not in OPTIONS[n].owners for n in names):
                raise ValueError(" / ".join(f"{n}={p[n]}" for n in names) + " needs "
                                 f"aggregation_rule={OPTIONS[names[0]].owners[0]!r}, not {rule!r}")
        if rule == "mean":
            return
        cls._check_runs(f"aggregation_rule={rule!r}", cls._robust_unsupported,
                        "is the server that runs the median and trimmed-mean rules")
        if mode != "exact":
            raise ValueError(f"aggregation_mode={mode!r} applies to aggregation_rule='mean' only; "
                             f"{rule!r} has one arithmetic")
        if worker_number is not None:
            error = _count_error(rule, worker_number, p, subset=False)
            if error:
                raise ValueError(error)
        select = p["krum_select"]
        if rule == "multi_krum" and select is not None:
            if worker_number is None:
                if select < 1:
                    raise ValueError(f"krum_select={select} must be at least 1")
            elif not 1 <= select <= worker_number - p["byzantine"]:
                raise ValueError(f"krum_select={select} must be in 1..worker_number - "
                                 f"byzantine = {worker_number - p['byzantine']}")

    @classmethod
    def _check_attack(cls, attack, attackers, attack_z=ATTACK_DEFAULTS["attack_z"],
                      attack_eps=ATTACK_DEFAULTS["attack_eps"],
                      attack_scale=ATTACK_DEFAULTS["attack_scale"], worker_number=None):
        """The sorted tuple of attacker ids; ValueError for what no round could run."""
        if attack is not None and attack not in ATTACKS:
            raise ValueError(f"attack must be None or one of {list(ATTACKS)}, not {attack!r}")
        try:
            ids = list(attackers)
        except TypeError:
            raise ValueError(f"attackers must be a collection of worker ids, not {attackers!r}")
        if any(isinstance(w, bool) or not isinstance(w, int) or w < 0 for w in ids):
            raise ValueError(f"attackers must be non-negative integer worker ids, not {ids!r}")
        if len(set(ids)) != len(ids):
            raise ValueError(f"attackers must be distinct worker ids, not {ids!r}")
        p = {"attack_z": attack_z, "attack_eps": attack_eps, "attack_scale": attack_scale}
        # a None that is not the default passes here too: float() refuses it in __init__
        cls._check_kinds({name: v for name, v in p.items() if v is not None})
        if attack is None and ids:
            raise ValueError(f"attackers={ids} needs an attack, one of {list(ATTACKS)}")
        for name, v in p.items():
            if v != ATTACK_DEFAULTS[name] and attack not in OPTIONS[name].owners:
                raise ValueError(f"{name}={v} needs attack={OPTIONS[name].owners[0]!r}, "
                                 f"not {attack!r}")
        if attack is None:
            return ()
        cls._check_runs(f"attack={attack!r}", cls._attack_unsupported,
                        "and the one-process Shapley servers are the servers that run the "
                        "Byzantine client attacks")
        if not ids:
            raise ValueError(f"attack={attack!r} needs attackers, a non-empty collection of "
                             "worker ids")
        if len(ids) > _native.ROBUST_MAX_K:
            raise ValueError(f"attack={attack!r} takes at most ROBUST_MAX_K="
                             f"{_native.ROBUST_MAX_K} attackers, not {len(ids)}")
        if worker_number is not None:
            if max(ids) >= worker_number:
                raise ValueError(f"attackers={ids} must be worker ids in 0..worker_number - 1 = "
                                 f"{worker_number - 1}")
            if attack != "sign_flip":
                honest = worker_number - len(ids)
                if honest < 1:
                    raise ValueError(f"attack={attack!r} needs at least one honest worker, "
                                     f"attackers={ids} leaves none of worker_number="
                                     f"{worker_number}")
                if honest > _native.ROBUST_MAX_K:
                    raise ValueError(f"attack={attack!r} takes at most ROBUST_MAX_K="
                                     f"{_native.ROBUST_MAX_K} honest workers, not {honest}")
                if attack == "alie" and attack_z is None:
                    attack_coefficients("alie", worker_number, len(ids))  # alie_z's ValueError
        return tuple(sorted(ids))

    @classmethod
    def _check_server_opt(cls, optimizer, server_lr=SERVER_OPT_DEFAULTS["server_lr"],
                          server_momentum=SERVER_OPT_DEFAULTS["server_momentum"],
                          server_beta2=SERVER_OPT_DEFAULTS["server_beta2"],
                          server_tau=SERVER_OPT_DEFAULTS["server_tau"]):
        """The resolved (server_lr, server_momentum, server_beta2, server_tau) of a server
        optimizer, or None without one; ValueError for what no round could run."""
        if optimizer is not None and optimizer not in SERVER_OPTIMIZERS:
            raise ValueError(f"server_optimizer must be None or one of {list(SERVER_OPTIMIZERS)}, "
                             f"not {optimizer!r}")
        p = {"server_lr": server_lr, "server_momentum": server_momentum,
             "server_beta2": server_beta2, "server_tau": server_tau}
        cls._check_kinds(p)
        for name, v in p.items():
            owners = OPTIONS[name].owners
            if v != SERVER_OPT_DEFAULTS[name] and optimizer not in owners:
                raise ValueError(f"{name}={v} needs server_optimizer "
                                 + (f"in {list(owners)}" if len(owners) < len(SERVER_OPTIMIZERS)
                                    else f"set, one of {list(owners)}") + f", not {optimizer!r}")
        if optimizer is None:
            return None
        cls._check_runs(f"server_optimizer={optimizer!r}", cls._server_opt_unsupported,
                        "is the server that runs the server optimizers")
        sgd = optimizer == "sgd"
        lr = float(server_lr) if server_lr is not None else (1.0 if sgd else 0.01)
        beta1 = float(server_momentum) if server_momentum is not None else (0.0 if sgd else 0.9)
        try:
            _native.server_opt_coeffs(lr, beta1, server_beta2, server_tau)
        except RuntimeError as e:
            raise ValueError(str(e))
        if _native.fl32(lr) == 0.0 or _native.fl32(server_tau) == 0.0 or _native.fl32(beta1) >= 1.0 \
                or _native.fl32(server_beta2) >= 1.0:
            raise ValueError(f"server_lr={lr} and server_tau={server_tau} must be positive and "
                             f"server_momentum={beta1} and server_beta2={server_beta2} below 1 "
                             "when rounded to fp32")
        return lr, beta1, float(server_beta2), float(server_tau)

    @classmethod
    def _check_dp(cls, rule, mode, worker_number, dp_clip=DP_DEFAULTS["dp_clip"],
                  dp_noise_multiplier=DP_DEFAULTS["dp_noise_multiplier"],
                  dp_seed=DP_DEFAULTS["dp_seed"], dp_delta=DP_DEFAULTS["dp_delta"]):
        """ValueError for differential-privacy options that no round could run."""
        p = {"dp_clip": dp_clip, "dp_noise_multiplier": dp_noise_multiplier, "dp_seed": dp_seed,
             "dp_delta": dp_delta}
        cls._check_kinds(p)
        if dp_seed >= 1 << 64:
            raise ValueError(f"dp_seed must be an integer in 0..2^64 - 1, not {dp_seed!r}")
        if dp_clip is None:
            for name, v in p.items():
                if v != DP_DEFAULTS[name]:
                    raise ValueError(f"{name}={v} needs dp_clip set, the clipping norm of "
                                     "differentially private FedAvg, not None")
            return
        cls._check_runs(f"dp_clip={dp_clip}", cls._dp_unsupported,
                        "is the server that runs differentially private FedAvg")
        if rule != "mean" or mode != "exact":
            raise ValueError(f"dp_clip={dp_clip} needs aggregation_rule='mean' and "
                             "aggregation_mode='exact' (DP-FedAvg is the clipped mean plus noise, "
                             f"with one arithmetic), not {rule!r} and {mode!r}")
        if worker_number is not None and worker_number > _native.ROBUST_MAX_K:
            raise ValueError(f"dp_clip={dp_clip} takes at most ROBUST_MAX_K={_native.ROBUST_MAX_K} "
                             f"clients, not worker_number={worker_number}")

    def _initial_model(self):
        """The model the first round starts from: the tester's; none without a tester."""
        return copy.deepcopy(
            ModelUtil(self.tester.model).get_parameter_dict()) if self.tester is not None else {}

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

    def _prev_flat(self, store):
        """The previous global model as a flat vector on the store's device, or None while
        there is none the store accepts (round 1 of a server without a tester)."""
        prev = self.__prev_model
        if prev and store.accepts(prev):
            return store.layout.flatten(prev, device=store.U.device)
        return None

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
        store = self.parameters.store
        return store.layout.views(self._subset_flat(store, list(client_subset)))

    def _subset_flat(self, store, ids):
        """The aggregate of the clients ``ids`` under the server's rule, as a flat vector."""
        if self.dp_clip is not None:
            return self._dp_flat(store, ids, release=False)
        # the rules that report, break ties and order by worker id are handed the ids (no
        # subclass that overrides _aggregate runs those rules)
        extra = {"ids": ids} if RULES[self.aggregation_rule]["ids"] else {}
        return self._aggregate(store, [self.parameters.row_of(i) for i in ids],
                               [self.parameters.n_of(i) for i in ids], **extra)

    def _aggregate(self, store, rows, ns, total=None, ids=None):
        if self.aggregation_rule == "mean":
            return store.fedavg(rows, ns, mode=_MODES[self.aggregation_mode], total=total)
        K = len(rows)
        error = _count_error(self.aggregation_rule, K, vars(self), subset=True)
        if error:
            raise ValueError(error)
        run = getattr(self, RULES[self.aggregation_rule]["run"])
        return run(store, rows, list(range(K)) if ids is None else ids)

    def _median(self, store, rows, ids):
        return store.median(rows)

    def _trimmed_mean(self, store, rows, ids):
        return store.trimmed_mean(rows, self.trim)

    def _mean_around_median(self, store, rows, ids):
        return store.mean_around_median(rows, len(rows) - self.byzantine)

    def _multi_krum(self, store, rows, ids):
        K, f = len(rows), self.byzantine
        select = K - f if self.krum_select is None else self.krum_select
        if select > K - f:
            raise ValueError(f"krum_select={select} exceeds len(subset) - byzantine = {K - f}")
        flat, selected, scores = store.multi_krum(rows, ids, f, select)
        self._keep_selection("multi_krum", ids, selected, dict(zip(ids, scores)))
        return flat

    def _bulyan(self, store, rows, ids):
        flat, selected, scores = store.bulyan(rows, ids, self.byzantine)
        self._keep_selection("bulyan", ids, selected, scores)
        return flat

    def _keep_selection(self, rule, ids, selected, scores):
        """Record and log what a selecting rule chose of the clients ``ids``."""
        self.last_selection = tuple(selected)
        self.last_scores = scores
        chosen = set(selected)
        log.info("%s: kept %s of %s clients, rejected workers %s", rule, len(selected), len(ids),
                 [i for i in ids if i not in chosen])

    def _geometric_median(self, store, rows, ids):
        flat, info = store.geometric_median(rows, ids, self.gm_iters, self.gm_nu)
        self.last_distances = info["distances"]
        self.last_rejected = tuple(info["rejected"])
        log.info("geometric_median: %s of %s clients, rejected workers %s, objective %s -> %s",
                 len(info["distances"]), len(rows), list(self.last_rejected),
                 info["objective"][0], info["objective"][-1])
        return flat

    def _start_flat(self, store, rows):
        """(The model the clients started from, flat, True); while there is none (round 1 of a
        server without a tester), (the coordinate-wise median of ``rows``, False)."""
        prev = self._prev_flat(store)
        return (store.median(rows), False) if prev is None else (prev, True)

    def _centered_clip(self, store, rows, ids):
        start, _ = self._start_flat(store, rows)
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

    def _dp_flat(self, store, ids, release):
        """DP-FedAvg over the clients ``ids`` from the previous global model
        (``store.dp_mean``).  ``release``: the round's aggregate, with the noise of stream
        ``self.round``, booked in ``last_dp``; otherwise the clipped mean without noise (sigma
        = 0 through the same entry point), which books nothing."""
        start = self._prev_flat(store)
        if start is None:
            raise ValueError(f"dp_clip={self.dp_clip}: no previous global model in round "
                             f"{self.round}: an update cannot be clipped without the model it "
                             "started from (a server with a tester starts from the tester's)")
        if len(ids) > _native.ROBUST_MAX_K:
            raise ValueError(f"dp_clip={self.dp_clip} takes at most ROBUST_MAX_K="
                             f"{_native.ROBUST_MAX_K} clients, not {len(ids)}")
        flat, info = store.dp_mean([self.parameters.row_of(i) for i in ids], ids, start,
                                   self.dp_clip, self.dp_noise_multiplier if release else 0.0,
                                   self.dp_seed, self.round)
        if not release:
            return flat
        # the padding between the tensors drew noise like any coordinate: back to zero
        ends = [o + n for o, n in zip(store.layout.offsets, store.layout.numels)]
        for a, b in zip(ends, store.layout.offsets[1:] + [store.layout.P]):
            flat[a:b] = 0.0
        self._dp_releases += 1
        self.last_dp = dict(info, round=self.round, releases=self._dp_releases,
                            epsilon=dp_epsilon(self.dp_noise_multiplier, self._dp_releases,
                                               self.dp_delta), delta=self.dp_delta)
        log.info("dp: round %s, %s of %s clients, %s clipped to %s, rejected workers %s, sigma %s, "
                 "(epsilon %s, delta %s) over %s releases", self.round, len(info["norms"]),
                 len(ids), sum(1 for s in info["scales"].values() if s < 1.0), self.dp_clip,
                 info["rejected"], info["sigma"], self.last_dp["epsilon"], self.dp_delta,
                 self._dp_releases)
        return flat

    def _fold_round(self):
        """FoolsGold: add the round's updates to the workers' histories, once (all
        clients have arrived, the attack has run), and cache what the round's
        ``get_subset_model`` calls share: the Gram matrix of the histories and the base."""
        store = self.parameters.store
        ids = list(self.parameters.keys())
        if len(ids) > _native.ROBUST_MAX_K:
            raise ValueError(f"aggregation_rule='foolsgold' takes at most ROBUST_MAX_K="
                             f"{_native.ROBUST_MAX_K} clients, not {len(ids)}")
        if any(isinstance(w, bool) or not isinstance(w, int) or w < 0 for w in ids):
            raise ValueError("aggregation_rule='foolsgold' keeps one history row per worker id: "
                             f"the ids must be non-negative integers, not {ids!r}")
        rows = [self.parameters.row_of(w) for w in ids]
        base, previous = self._start_flat(store, rows)  # what the updates are taken from
        if not previous:
            log.info("foolsgold: no previous model in round %s, updates are taken from the "
                     "coordinate-wise median of the round's %s rows", self.round, len(rows))
        G = store.fold_history(rows, ids, base).cpu().tolist()
        self._fg_round = {"ids": ids, "G": G, "base": base}

    def _foolsgold(self, store, rows, ids):
        fr = self._fg_round
        if fr is None:
            raise ValueError("aggregation_rule='foolsgold': no folded round: the histories are "
                             "folded once per round when all of its updates have arrived, and "
                             "get_subset_model weights subsets of that round only")
        pos = {w: i for i, w in enumerate(fr["ids"])}
        missing = [w for w in ids if w not in pos]
        if missing:
            raise ValueError(f"aggregation_rule='foolsgold': workers {missing} are not part of "
                             "the folded round")
        sub = [[fr["G"][pos[a]][pos[b]] for b in ids] for a in ids]
        flat, info = store.foolsgold(rows, ids, sub, fr["base"], self.fg_kappa)
        self.last_weights = info["weights"]
        self.last_similarity = info["similarity"]
        self.last_rejected = tuple(info["rejected"])
        log.info("foolsgold: %s of %s clients weighted above 0 (kappa %s), weights %s, rejected "
                 "workers %s", sum(1 for a in info["weights"].values() if a > 0.0), len(rows),
                 self.fg_kappa, info["weights"], list(self.last_rejected))
        return flat

    def reset_history(self, worker_id=None):
        """Forget the FoolsGold history of one worker, or of all (None)."""
        if self.parameters.store is not None:
            self.parameters.store.reset_history(worker_id)

    def _apply_attack(self):
        """Rewrite the attackers' rows of the round in place (all clients have arrived)."""
        if self.attack is None:
            return
        store = self.parameters.store
        bad = [w for w in self.attackers if w in self.parameters]
        honest = [w for w in self.parameters.keys() if w not in set(self.attackers)]
        if len(bad) != len(self.attackers):
            raise ValueError(f"attack={self.attack!r}: attackers "
                             f"{[w for w in self.attackers if w not in self.parameters]} sent no "
                             "update this round")
        # relative to the model the clients started from; while there is none, to zero
        base = None if self.attack == "alie" else self._prev_flat(store)
        info = {"attack": self.attack, "attackers": self.attackers}
        if self.attack == "sign_flip":
            store.sign_flip([self.parameters.row_of(w) for w in bad], self.attack_scale,
                            base=base)
            info.update(a=-self.attack_scale, b=0.0, scale=self.attack_scale)
        else:
            if not honest:
                raise ValueError(f"attack={self.attack!r} needs at least one honest worker")
            a, b, _ = attack_coefficients(self.attack, len(self.parameters), len(bad),
                                          z=self.attack_z, eps=self.attack_eps)
            store.craft([self.parameters.row_of(w) for w in honest],
                        [self.parameters.row_of(w) for w in bad], a, b, base=base)
            info.update(a=a, b=b)
            if self.attack == "alie":
                info["z"] = -b
            else:
                info["eps"] = self.attack_eps
        self.last_attack = info
        log.info("attack %s: workers %s rewritten from %s honest ones (a %s, b %s, %s)",
                 self.attack, list(self.attackers), len(honest), info["a"], info["b"],
                 "relative to the previous model" if base is not None else "no base")

    @property
    def server_opt_state(self):
        """None without a server optimizer; else {"step": the steps taken, "m": the first
        moment as a dict of views (None before the state exists, and for sgd without
        momentum), "v": the second moment likewise (None for sgd)}."""
        if self.server_optimizer is None:
            return None
        store = self.parameters.store
        st = store.server_opt if store is not None else None
        if st is None:
            return {"step": 0, "m": None, "v": None}
        views = store.layout.views
        return {"step": st["step"], "m": None if st["m"] is None else views(st["m"]),
                "v": None if st["v"] is None else views(st["v"])}

    def reset_server_optimizer(self):
        """Start the server optimizer's state over: step 0, m zero, v = server_tau^2."""
        if self.parameters.store is not None:
            self.parameters.store.reset_server_opt()

    def _server_opt_round(self, store, flat):
        """The round's model from its aggregate ``flat``: one server-optimizer step from
        the previous global model; the aggregate itself while there is none."""
        kind = _native.SERVER_OPT_KINDS[self.server_optimizer]
        if not bool(torch.isfinite(flat).all()):
            raise ValueError(f"server_optimizer={self.server_optimizer!r}: the aggregate of round "
                             f"{self.round} is not finite; the optimizer state is left as it was")
        prev = self._prev_flat(store)
        if prev is None:
            if not self._server_opt_adopted:
                log.info("server_optimizer %s: no previous model in round %s, the aggregate "
                         "becomes the model and the state starts from it",
                         self.server_optimizer, self.round)
                self._server_opt_adopted = True
            if store.server_opt is None:
                store.reset_server_opt(kind, self._server_opt_coeffs)
            store.set_model(flat)
            self.last_server_step = {}
            return flat
        store.set_model(prev)
        out = store.server_opt_step(flat, kind, self._server_opt_coeffs)
        norms = torch.stack([torch.linalg.vector_norm(flat - prev, dtype=torch.float64),
                             torch.linalg.vector_norm(out - prev, dtype=torch.float64)]).tolist()
        self.last_server_step = {"pseudo_gradient_norm": norms[0], "update_norm": norms[1]}
        log.info("server_optimizer %s: step %s, pseudo-gradient norm %s, update norm %s",
                 self.server_optimizer, store.server_opt["step"], norms[0], norms[1])
        return out

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
        self._apply_attack()
        if self.aggregation_rule == "foolsgold":
            self._fold_round()
        log.info("begin aggregating")
        if self.server_optimizer is None and self.dp_clip is None:
            avg_parameter = self.get_subset_model(self.parameters.keys())
        else:
            store = self.parameters.store
            ids = list(self.parameters.keys())
            flat = self._subset_flat(store, ids) if self.dp_clip is None \
                else self._dp_flat(store, ids, release=True)
            if self.server_optimizer is not None:  # on the noised aggregate: post-processing
                flat = self._server_opt_round(store, flat)
            avg_parameter = store.layout.views(flat)
        data = self._process_aggregated_parameter(avg_parameter)
        self.__prev_model = copy.deepcopy(data)
        acc = self.get_metric(self.prev_model)
        log.info("end aggregating, test accuracy is %s", acc)
        self.parameters.clear()
        self._fg_round = None
        # one copy per client that feeds this process (its local clients when sharded)
        return RepeatedResult(data=data, num=self.clients_per_round)
