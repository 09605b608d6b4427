"""Width-heterogeneous FedAvg worker (HeteroFL / FedRolex): ``FedWorker`` with a ``width``.

Its trainer's model is the model class built at ``width`` (``LeNet5(width=r)``); the downlink is
the server's ``HeteroBroadcast``, of which it loads its level's parameter dict, and the uplink
``(worker_id, n, HeteroUpdate(width, row))`` is its parameters flat in its own
``ParameterLayout``: P_level elements, not the global P.  Which global channels its local ones
stand for is the server's plan alone; the worker never sees a shift.
"""
import logging

from ..hetero import check_width
from ..layout import ParameterLayout
from ..model_util import ModelUtil
from ..servers.fed_hetero_server import HeteroBroadcast, HeteroUpdate
from ..trainer import ModelExecutorCallbackPoint
from .fed_worker import FedWorker, dataset_size

log = logging.getLogger("distributed_learning_simulator_amd")


class FedHeteroWorker(FedWorker):
    def __init__(self, width=1.0, **kwargs):
        self.width = check_width(width)
        super().__init__(**kwargs)
        # replaces FedWorker's dense send (same callback name)
        self.trainer.add_named_callback(ModelExecutorCallbackPoint.AFTER_EXECUTE,
                                        "send_parameter", self.__send_row)
        self.layout = ParameterLayout((n, tuple(p.shape))
                                      for n, p in self.trainer.model.named_parameters())

    def train(self, device):
        self.trainer.set_device(device)
        self.load_model(self.worker_data_queue.get_result())
        log.info("end load initial parameter_dict")
        for _ in range(self.round):
            self.trainer.train()

    def load_model(self, broadcast):
        """Load this worker's level of the server's broadcast."""
        if not isinstance(broadcast, HeteroBroadcast):
            raise ValueError(f"worker {self.worker_id}: the broadcast must be a HeteroBroadcast, "
                             f"not {type(broadcast).__name__}")
        model = broadcast.for_width(self.width)
        if not self.layout.matches(model):
            raise ValueError(f"worker {self.worker_id}: the server's width-{self.width} model is "
                             "not this trainer's (build the trainer's model with width=)")
        ModelUtil(self.trainer.model).load_parameter_dict(model)

    def hetero_update(self):
        """The round's HeteroUpdate: the model as it stands, flat."""
        params = ModelUtil(self.trainer.model).get_parameter_dict(detach=True)
        return HeteroUpdate(self.width, self.layout.flatten(params))

    def __send_row(self, **kwargs):
        trainer = kwargs["model_executor"]
        self.worker_data_queue.add_task((self.worker_id, dataset_size(trainer.dataset),
                                         self.hetero_update()))
        self.load_model(self.worker_data_queue.get_result())
        log.info("end load_parameter_dict")
