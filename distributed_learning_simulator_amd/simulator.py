"""Simulator entry point (reference: simulator.py:18-72, config.py:6-25, simulator.sh).

    python -m distributed_learning_simulator_amd.simulator --dataset_name MNIST \\
        --model_name LeNet5 --distributed_algorithm fed --worker_number 10 --round 5 \\
        --epoch 1 --learning_rate 0.01 --log_level INFO [--aggregation_mode fma]
        [--aggregation_rule median | --aggregation_rule trimmed_mean --trim 2 |
         --aggregation_rule multi_krum --byzantine 2 [--krum_select 1] |
         --aggregation_rule geometric_median [--gm_iters 3] [--gm_nu 1e-6] |
         --aggregation_rule centered_clip [--cc_tau 10.0] [--cc_iters 3] |
         --aggregation_rule mean_around_median --byzantine 2 |
         --aggregation_rule bulyan --byzantine 2 |
         --aggregation_rule foolsgold [--fg_kappa 1.0]]
        [--server_optimizer sgd [--server_lr 1.0] [--server_momentum 0.9] |
         --server_optimizer adagrad|adam|yogi [--server_lr 0.01] [--server_momentum 0.9]
             [--server_beta2 0.99] [--server_tau 1e-3]]
        [--attack alie --attackers 3,7 [--attack_z 1.0] |
         --attack ipm --attackers 3,7 [--attack_eps 0.1] |
         --attack sign_flip --attackers 3,7 [--attack_scale 1.0]]
        [--dp_clip 1.0 [--dp_noise_multiplier 1.0] [--dp_seed 0] [--dp_delta 1e-5]]
    python -m distributed_learning_simulator_amd.simulator --distributed_algorithm fed_topk \\
        --worker_number 10 --round 5 [--topk_ratio 0.01] [--topk_error_feedback 1]
    python -m distributed_learning_simulator_amd.simulator --distributed_algorithm fed_secagg \\
        --worker_number 10 --round 5 [--secagg_bits 20] [--secagg_frac_bits 16] [--secagg_seed 0]
        [--secagg_weighted 1] [--secagg_dropouts 3,7] [--secagg_threshold 6]

Same flags and flow as the reference: IID split of the training set over the
workers (:48-50), a tester on the test split (:51), ``factory.get_server``
(:52-57), one thread per worker placed on GPU ``worker_id % ngpu`` (:59-69),
per-run log file ``log/<algo>/<dataset>/<model>/<date>.log`` (:38-46).
Datasets are synthetic of the named shape (no network: MNIST-shaped 1x32x32 /
CIFAR-shaped 3x32x32, 10 classes, learnable class templates + noise).
"""
import argparse
import datetime
import logging
import os
import threading

import torch

from .aggregation import ATTACKS
from .factory import get_server, get_worker
from .models import MODELS, synthetic_classification
from .servers.fed_server import (ATTACK_DEFAULTS, DEFAULTS, DP_DEFAULTS, RULES,
                                 SERVER_OPT_DEFAULTS, SERVER_OPTIMIZERS)
from .trainer import Inferencer, Trainer
from .workers.fed_secagg_worker import SECAGG_DEFAULTS

TOPK_DEFAULTS = {"topk_ratio": 0.01, "topk_error_feedback": 1}
# the fed_secagg flags and what they hold when not given (threshold None: a majority)
SECAGG_FLAGS = {**{name: int(v) for name, v in SECAGG_DEFAULTS.items()},
                "secagg_dropouts": (), "secagg_threshold": None}
DATASETS = {"MNIST": (1, 32, 32), "CIFAR10": (3, 32, 32)}


def get_config(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--distributed_algorithm", type=str, required=True)
    ap.add_argument("--worker_number", type=int, required=True)
    ap.add_argument("--round", type=int, required=True)
    ap.add_argument("--dataset_name", type=str, default="MNIST")
    ap.add_argument("--model_name", type=str, default="LeNet5")
    ap.add_argument("--epoch", type=int, default=1)
    ap.add_argument("--learning_rate", type=float, default=0.01)
    ap.add_argument("--optimizer_name", type=str, default="SGD")
    ap.add_argument("--momentum", type=float, default=0.0)
    ap.add_argument("--weight_decay", type=float, default=0.0)
    ap.add_argument("--batch_size", type=int, default=64)
    ap.add_argument("--log_level", type=str, default="INFO")
    ap.add_argument("--train_size", type=int, default=10000)
    ap.add_argument("--test_size", type=int, default=2000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--log_dir", type=str, default="log")
    # the FedAvg arithmetic of the fed / fed_quant / Shapley servers: "exact" (the
    # reference's op order, bit for bit) or "fma" (one fused multiply-add per
    # element and client, within the north star's normwise 1e-6 FedAvg tolerance;
    # the fed_quant path that meets the 80 % HBM bar)
    ap.add_argument("--aggregation_mode", type=str, default="exact", choices=("exact", "fma"))
    # the tester's convolutions (trainer.Inferencer): "dls", the library's
    # deterministic bf16x3 ones (a coalition's utility the same bits in every
    # process), or "miopen", torch's fp32 forward with MIOpen's deterministic
    # algorithms (the reference tester's arithmetic, ~4x slower)
    ap.add_argument("--tester_conv", type=str, default="dls", choices=("dls", "miopen"))
    # the utility the two Shapley servers score coalitions with: the tester's top-1
    # accuracy ("acc", the reference's) or its mean cross-entropy ("loss",
    # get_metric(model, "loss"), unnegated), both on the deterministic evaluation path
    ap.add_argument("--utility_metric", type=str, default="acc", choices=("acc", "loss"))
    # what the fed server computes from a round's client updates: the reference's
    # weighted mean, or a robust coordinate-wise rule (FedServer): the median, or the
    # trimmed mean that drops the --trim lowest and highest values of every
    # coordinate, or multi-Krum, which scores whole updates by their squared
    # distances to their nearest neighbours, assuming --byzantine bad clients, and
    # averages the --krum_select best-scored ones (default: all but --byzantine;
    # 1 is classic Krum), or the mean around the median, which averages per coordinate
    # the all-but---byzantine values closest to the median, or Bulyan, which chooses all
    # but 2 x --byzantine updates by iterated Krum and then averages per coordinate the
    # chosen values closest to their median, all but another 2 x --byzantine (it needs
    # 4 x --byzantine + 3 clients).  The robust rules ignore the clients' sample counts.
    ap.add_argument("--aggregation_rule", type=str, default="mean", choices=tuple(RULES))
    # geometric_median: --gm_iters smoothed Weiszfeld steps from the coordinate-wise
    # median, smoothing --gm_nu in the units of the parameters (RFA's defaults)
    # centered_clip: --cc_iters clipped steps from the previous global model, each
    # client's difference to the aggregate shortened to at most --cc_tau (in the units
    # of the parameters); --cc_iters 1 is norm clipping
    # foolsgold: clients whose accumulated updates keep pointing the same way (sybils,
    # e.g. --attack alie --attackers 3,7) are down-weighted; --fg_kappa is the paper's
    # confidence parameter (larger pushes the weights towards 0 and 1)
    for name, default in DEFAULTS.items():  # the counts are integers, the rest real numbers
        ap.add_argument("--" + name, type=float if isinstance(default, float) else int,
                        default=default)
    # Byzantine clients: the workers listed in --attackers (comma-separated ids) have
    # their update of every round rewritten on the server before anything reads it:
    # "alie" (a little is enough) sends mean - z * std of the honest updates per
    # coordinate, z = --attack_z (default: from the worker and attacker counts), "ipm"
    # (inner product manipulation) -(--attack_eps) times the honest mean update,
    # "sign_flip" the attacker's own update mirrored and scaled by --attack_scale
    ap.add_argument("--attack", type=str, default=None, choices=ATTACKS)
    ap.add_argument("--attackers", type=_worker_ids, default=())
    for name, default in ATTACK_DEFAULTS.items():
        ap.add_argument("--" + name, type=float, default=default)
    # the server optimizer that turns the round's aggregate (of any rule) into the next
    # model, with aggregate - previous model as its pseudo-gradient: "sgd" is server
    # momentum (FedAvgM), "adagrad" / "adam" / "yogi" are FedAdagrad / FedAdam / FedYogi
    # (Reddi et al. 2021); none given: the aggregate is the next model.  --server_lr
    # defaults to 1.0 for sgd and 0.01 for the adaptive ones, --server_momentum (beta1) to
    # 0.0 and 0.9; --server_beta2 and --server_tau belong to the adaptive ones
    ap.add_argument("--server_optimizer", type=str, default=None, choices=SERVER_OPTIMIZERS)
    for name in SERVER_OPT_DEFAULTS:
        ap.add_argument("--" + name, type=float, default=None)
    # client-level differentially private FedAvg on the fed server: every client's update is
    # clipped to the norm --dp_clip, the clipped updates are averaged and Gaussian noise of
    # standard deviation --dp_noise_multiplier x --dp_clip / workers is added (default
    # multiplier 1.0), drawn from the library's Philox stream under --dp_seed (default 0);
    # --dp_delta (default 1e-5) is the delta of the reported (epsilon, delta)
    ap.add_argument("--dp_clip", type=float, default=None)
    ap.add_argument("--dp_noise_multiplier", type=float, default=None)
    ap.add_argument("--dp_seed", type=int, default=None)
    ap.add_argument("--dp_delta", type=float, default=None)
    # fed_topk: every worker sends the ceil(--topk_ratio x parameters) largest-magnitude
    # coordinates of its update and keeps the rest in a residual that is added back next
    # round (--topk_error_feedback 0: the residual is dropped, plain top-k)
    ap.add_argument("--topk_ratio", type=float, default=None)
    ap.add_argument("--topk_error_feedback", type=int, default=None, choices=(0, 1))
    # fed_secagg: every worker sends its update quantised to --secagg_bits bits with
    # --secagg_frac_bits fractional ones (defaults 20 and 16: +-8 at 1.5e-5) and masked in
    # Z_2^32 with the pair and self masks of the Philox stream under --secagg_seed;
    # --secagg_weighted 1 weights a worker by its sample count (default 0: every worker 1);
    # the workers in --secagg_dropouts (comma-separated ids) drop out of every round after the
    # masks were agreed, and a round needs --secagg_threshold survivors (default: a majority)
    ap.add_argument("--secagg_bits", type=int, default=None)
    ap.add_argument("--secagg_frac_bits", type=int, default=None)
    ap.add_argument("--secagg_seed", type=int, default=None)
    ap.add_argument("--secagg_weighted", type=int, default=None, choices=(0, 1))
    ap.add_argument("--secagg_dropouts", type=_worker_ids, default=None)
    ap.add_argument("--secagg_threshold", type=int, default=None)
    config = ap.parse_args(argv)
    if config.distributed_algorithm != "fed_secagg" and any(
            getattr(config, name) is not None for name in SECAGG_FLAGS):
        ap.error("--secagg_bits, --secagg_frac_bits, --secagg_seed, --secagg_weighted, "
                 "--secagg_dropouts and --secagg_threshold apply to --distributed_algorithm "
                 "fed_secagg alone")
    for name, default in SECAGG_FLAGS.items():
        if getattr(config, name) is None:
            setattr(config, name, default)
    if config.distributed_algorithm != "fed_topk" and (
            config.topk_ratio is not None or config.topk_error_feedback is not None):
        ap.error("--topk_ratio and --topk_error_feedback apply to --distributed_algorithm "
                 "fed_topk alone")
    if config.topk_ratio is None:
        config.topk_ratio = TOPK_DEFAULTS["topk_ratio"]
    if config.topk_error_feedback is None:
        config.topk_error_feedback = TOPK_DEFAULTS["topk_error_feedback"]
    if config.distributed_algorithm != "fed" and any(
            getattr(config, name) is not None for name in DP_DEFAULTS):
        ap.error("--dp_clip and its parameters apply to --distributed_algorithm fed alone, the "
                 "server that holds fp32 client rows and releases one model per round")
    if config.distributed_algorithm == "sign_SGD" and any(
            getattr(config, name) is not None
            for name in ("server_optimizer",) + tuple(SERVER_OPT_DEFAULTS)):
        ap.error("--server_optimizer and its parameters apply to the fed server, whose round "
                 "ends in a model; sign_SGD broadcasts a vote")
    if config.distributed_algorithm == "sign_SGD" and config.aggregation_rule != "mean":
        ap.error("--aggregation_rule applies to the FedAvg-based servers; sign_SGD votes")
    if config.distributed_algorithm == "sign_SGD" and config.attack is not None:
        ap.error("--attack applies to the servers that hold fp32 client rows; sign_SGD holds "
                 "sign planes")
    return config


def _worker_ids(text):
    """"3,7" -> (3, 7)."""
    try:
        return tuple(int(t) for t in text.split(",") if t.strip())
    except ValueError:
        raise argparse.ArgumentTypeError(f"comma-separated worker ids expected, not {text!r}")


def server_kwargs(config):
    """The keyword arguments run() passes to factory.get_server beside tester /
    worker_number / multi_process: the aggregation mode for the FedAvg-based
    servers (sign_SGD votes; it has no FedAvg), the utility metric for the two
    Shapley servers, the aggregation rule and its trim count when the rule is not the
    default mean, multi-Krum's byzantine / krum_select, byzantine for Bulyan and the
    mean around the median, the geometric median's
    gm_iters / gm_nu, centered clipping's cc_tau / cc_iters and FoolsGold's fg_kappa for
    those rules alone, and
    the attack with its attackers and parameters when --attack is given (the server
    rejects a parameter that belongs to another attack), and --server_optimizer and
    each of its parameters that was given, and likewise --dp_clip and each of its."""
    if config.distributed_algorithm == "sign_SGD":
        return {}
    kwargs = {"aggregation_mode": config.aggregation_mode}
    if config.distributed_algorithm in ("GTG_shapley_value", "multiround_shapley_value"):
        kwargs["utility_metric"] = getattr(config, "utility_metric", "acc")
    if getattr(config, "aggregation_rule", "mean") != "mean":
        kwargs["aggregation_rule"] = config.aggregation_rule
        for name in ("trim",) + RULES[config.aggregation_rule]["owns"]:
            kwargs[name] = getattr(config, name, DEFAULTS[name])
    if getattr(config, "attack", None) is not None:
        kwargs["attack"] = config.attack
        kwargs["attackers"] = tuple(getattr(config, "attackers", ()))
        for name, default in ATTACK_DEFAULTS.items():
            kwargs[name] = getattr(config, name, default)
    for name in ("server_optimizer",) + tuple(SERVER_OPT_DEFAULTS) + tuple(DP_DEFAULTS):
        if getattr(config, name, None) is not None:  # only the ones given
            kwargs[name] = getattr(config, name)
    if config.distributed_algorithm == "fed_secagg":  # the format and the seed the workers use
        for name in ("secagg_bits", "secagg_frac_bits", "secagg_seed", "secagg_threshold"):
            kwargs[name] = getattr(config, name, SECAGG_FLAGS[name])
        kwargs["secagg_dropouts"] = tuple(getattr(config, "secagg_dropouts", ()))
    return kwargs


def worker_kwargs(config):
    """The keyword arguments run() passes to factory.get_worker beside trainer / queue /
    round / worker_id: the sparsifier's for fed_topk, the mask format, seed, weighting and
    the round's participants (every worker) for fed_secagg, none for the other algorithms."""
    if config.distributed_algorithm == "fed_secagg":
        return {"secagg_bits": getattr(config, "secagg_bits", SECAGG_FLAGS["secagg_bits"]),
                "secagg_frac_bits": getattr(config, "secagg_frac_bits",
                                            SECAGG_FLAGS["secagg_frac_bits"]),
                "secagg_seed": getattr(config, "secagg_seed", SECAGG_FLAGS["secagg_seed"]),
                "secagg_weighted": bool(getattr(config, "secagg_weighted",
                                                SECAGG_FLAGS["secagg_weighted"])),
                "participants": tuple(range(config.worker_number))}
    if config.distributed_algorithm != "fed_topk":
        return {}
    return {"topk_ratio": getattr(config, "topk_ratio", TOPK_DEFAULTS["topk_ratio"]),
            "error_feedback": bool(getattr(config, "topk_error_feedback",
                                           TOPK_DEFAULTS["topk_error_feedback"]))}


def get_cuda_devices():
    return [torch.device("cuda", i) for i in range(torch.cuda.device_count())]


def run(config, devices=None, sharded=None):
    """simulator.py:33-72.  ``devices``: the GPUs the worker threads use (default all
    visible); ``sharded``: get_server's (default: sharded servers when
    torch.distributed is initialised with more than one rank) — a caller that runs
    a one-process simulation inside a multi-rank job passes False."""
    log = logging.getLogger("distributed_learning_simulator_amd")
    log.setLevel(config.log_level)
    if config.log_dir:
        path = os.path.join(config.log_dir, config.distributed_algorithm, config.dataset_name,
                            config.model_name,
                            "{date:%Y-%m-%d_%H:%M:%S}.log".format(date=datetime.datetime.now()))
        os.makedirs(os.path.dirname(path), exist_ok=True)
        log.addHandler(logging.FileHandler(path))
    shape = DATASETS[config.dataset_name]
    X, y = synthetic_classification(config.train_size, shape, seed=config.seed)
    Xt, yt = synthetic_classification(config.test_size, shape, seed=config.seed + 1)
    torch.manual_seed(config.seed)
    model_cls = MODELS[config.model_name]
    devices = list(devices) if devices else get_cuda_devices()
    server_device = devices[0]
    tester = Inferencer(model_cls().to(server_device), (Xt, yt), device=server_device,
                        conv=getattr(config, "tester_conv", "dls"))
    server = get_server(config.distributed_algorithm, sharded=sharded, tester=tester,
                        worker_number=config.worker_number, multi_process=False,
                        **server_kwargs(config))
    # IID split (simulator.py:48-50)
    perm = torch.randperm(X.shape[0], generator=torch.Generator().manual_seed(config.seed))
    shards = torch.chunk(perm, config.worker_number)
    errors = []

    def create_worker_and_train(worker_id, device):
        try:
            torch.cuda.set_device(device)
            idx = shards[worker_id]
            trainer = Trainer(model_cls(), (X[idx], y[idx]), (Xt, yt), epoch=config.epoch,
                              batch_size=config.batch_size, learning_rate=config.learning_rate,
                              momentum=config.momentum, weight_decay=config.weight_decay,
                              optimizer_name=config.optimizer_name, device=device,
                              seed=config.seed + worker_id)
            worker = get_worker(config.distributed_algorithm, trainer=trainer,
                                worker_data_queue=server.worker_data_queue, round=config.round,
                                worker_id=worker_id, **worker_kwargs(config))
            worker.train(device=device)
        except BaseException as e:  # surfaced after join
            errors.append(e)
            raise

    threads = [threading.Thread(target=create_worker_and_train,
                                args=(i, devices[i % len(devices)]), daemon=True)
               for i in range(config.worker_number)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    server.stop()
    if errors:
        raise RuntimeError("worker failed") from errors[0]
    return server


def main(argv=None):
    logging.basicConfig(format="%(asctime)s %(levelname)s %(message)s")
    config = get_config(argv)
    server = run(config)
    acc = None
    if hasattr(server, "prev_model") and server.tester is not None and server.prev_model:
        acc = server.get_metric(server.prev_model)
    print(f"finished {config.distributed_algorithm}: rounds={getattr(server, 'round', None)} "
          f"test_accuracy={acc}")
    return server


if __name__ == "__main__":
    main()
