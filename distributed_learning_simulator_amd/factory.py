"""Plugin factory (reference: factory.py:14-35) — same algorithm names and errors."""
from .servers.fed_drive_server import FedDriveServer
from .servers.fed_eden_server import FedEDENServer
from .servers.fed_efsign_server import FedEFSignServer
from .servers.fed_hetero_server import FedHeteroServer
from .servers.fed_mx_server import FedMXServer
from .servers.fed_powersgd_server import FedPowerSGDServer
from .servers.fed_qsgd_server import FedQSGDServer
from .servers.fed_quant_server import FedQuantServer
from .servers.fed_scaffold_server import FedScaffoldServer
from .servers.fed_secagg_server import FedSecAggServer
from .servers.fed_sketch_server import FedSketchServer
from .servers.fed_server import FedServer
from .servers.fed_topk_server import FedTopKServer
from .servers.GTG_shapley_value_server import GTGShapleyValueServer
from .servers.multiround_shapley_value_server import MultiRoundShapleyValueServer
from .servers.server import Server
from .servers.sign_sgd_server import SignSGDServer
from .workers.fed_drive_worker import FedDriveWorker
from .workers.fed_eden_worker import FedEDENWorker
from .workers.fed_efsign_worker import FedEFSignWorker
from .workers.fed_hetero_worker import FedHeteroWorker
from .workers.fed_mx_worker import FedMXWorker
from .workers.fed_powersgd_worker import FedPowerSGDWorker
from .workers.fed_qsgd_worker import FedQSGDWorker
from .workers.fed_quant_worker import FedQuantWorker
from .workers.fed_scaffold_worker import FedScaffoldWorker
from .workers.fed_secagg_worker import FedSecAggWorker
from .workers.fed_sketch_worker import FedSketchWorker
from .workers.fed_topk_worker import FedTopKWorker
from .workers.fed_worker import FedWorker
from .workers.sign_sgd_worker import SignSGDWorker
from .workers.worker import Worker


def get_server(algorithm, sharded=None, **kwargs) -> Server:
    """factory.py:14-25.  ``sharded`` (default: torch.distributed initialised with
    more than one rank) returns the one-process-per-GPU servers of distributed.py."""
    if sharded is None:
        import torch.distributed as dist
        sharded = dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1
    if sharded:
        from .distributed import get_sharded_server
        return get_sharded_server(algorithm, **kwargs)
    if algorithm == "sign_SGD":
        return SignSGDServer(**kwargs)
    if algorithm == "fed_quant":
        return FedQuantServer(**kwargs)
    if algorithm == "fed":
        return FedServer(**kwargs)
    if algorithm == "fed_topk":
        return FedTopKServer(**kwargs)
    if algorithm == "fed_secagg":
        return FedSecAggServer(**kwargs)
    if algorithm == "fed_efsign":
        return FedEFSignServer(**kwargs)
    if algorithm == "fed_drive":
        return FedDriveServer(**kwargs)
    if algorithm == "fed_eden":
        return FedEDENServer(**kwargs)
    if algorithm == "fed_sketch":
        return FedSketchServer(**kwargs)
    if algorithm == "fed_powersgd":
        return FedPowerSGDServer(**kwargs)
    if algorithm == "fed_qsgd":
        return FedQSGDServer(**kwargs)
    if algorithm == "fed_mx":
        return FedMXServer(**kwargs)
    if algorithm == "fed_scaffold":
        return FedScaffoldServer(**kwargs)
    if algorithm == "fed_hetero":
        return FedHeteroServer(**kwargs)
    if algorithm == "multiround_shapley_value":
        return MultiRoundShapleyValueServer(**kwargs)
    if algorithm == "GTG_shapley_value":
        return GTGShapleyValueServer(**kwargs)
    raise RuntimeError("unknown algorithm:" + algorithm)


def get_worker(algorithm, **kwargs) -> Worker:
    if algorithm == "sign_SGD":
        return SignSGDWorker(**kwargs)
    if algorithm == "fed_quant":
        return FedQuantWorker(**kwargs)
    if algorithm == "fed_topk":
        return FedTopKWorker(**kwargs)
    if algorithm == "fed_secagg":
        return FedSecAggWorker(**kwargs)
    if algorithm == "fed_efsign":
        return FedEFSignWorker(**kwargs)
    if algorithm == "fed_drive":
        return FedDriveWorker(**kwargs)
    if algorithm == "fed_eden":
        return FedEDENWorker(**kwargs)
    if algorithm == "fed_sketch":
        return FedSketchWorker(**kwargs)
    if algorithm == "fed_powersgd":
        return FedPowerSGDWorker(**kwargs)
    if algorithm == "fed_qsgd":
        return FedQSGDWorker(**kwargs)
    if algorithm == "fed_mx":
        return FedMXWorker(**kwargs)
    if algorithm == "fed_scaffold":
        return FedScaffoldWorker(**kwargs)
    if algorithm == "fed_hetero":
        return FedHeteroWorker(**kwargs)
    if algorithm in ("fed", "multiround_shapley_value", "GTG_shapley_value"):
        return FedWorker(**kwargs)
    raise RuntimeError("unknown algorithm:" + algorithm)
