"""Shapley-value server base (reference: servers/shapley_value_server.py:9-14).

Adds, on top of the reference's ``powerset``, the batched coalition evaluator
both Shapley servers use: a batch of S coalitions becomes S subset models in
one kernel launch (``dls_subset_fedavg_f32``, bit-exact reference order — the
default, because accuracy utilities are discontinuous — or the fp32 MFMA
contraction ``dls_subset_gemm_f32`` with ``subset_method="gemm"``), then each
model is scored with ``get_metric`` (servers/fed_server.py:26-32).  Under
``torch.distributed`` with several ranks the coalitions are dealt round-robin
over the ranks and the utilities are summed with one all-reduce (each rank
fills only its own entries), so every rank ends with the full table.

``subset_method="gemm"`` is a dense product over the union of a batch's clients:
every element of a subset model is within (K+1) 2^-24 of the magnitude sum of its
terms (K clients in the batch; ``include/dls_hip.h``), but a client row that holds an
inf or NaN (a diverged or attacking client) makes those parameters non-finite in
EVERY coalition of the batch, the ones without that client included, because 0 * inf
is NaN.  The exact kernels read only a coalition's members: with clients that may
diverge, keep the default.

``utility_metric="loss"`` makes the utility the tester's mean cross-entropy
(``get_metric(model, "loss")``, unnegated: the sign convention is the caller's)
instead of the top-1 accuracy, on the same fast paths: every image's loss is
computed in fp32 by one lane and the mean is one fixed-order fp64 sum
(``Inferencer.metrics_many`` / ``metrics_async``), so a coalition's loss is a
function of the coalition, the same bits in any batch, chunking or process.
"""
import inspect
from itertools import chain, combinations

import torch
import torch.distributed as dist

from ..model_util import ModelUtil
from .fed_server import FedServer


class ShapleyValueServer(FedServer):
    _robust_unsupported = "coalition models come from the batched subset-mean kernels"
    _server_opt_unsupported = ("its round hook picks or records the round model among the "
                               "coalitions' plain means")
    _dp_unsupported = ("every coalition model it scores would be a release of its own, which "
                       "the accountant does not cover")

    def __init__(self, subset_method="exact", subset_batch=None, eval_streams=1,
                 utility_metric="acc", **kwargs):
        if utility_metric not in ("acc", "loss"):
            raise ValueError(f"utility_metric must be 'acc' or 'loss', not {utility_metric!r}")
        super().__init__(**kwargs)
        self.utility_metric = utility_metric
        self.subset_method = subset_method
        self.subset_batch = subset_batch
        # queued utility forwards in flight at once, one HIP stream each (1: all
        # on the current stream); the utilities are the same bits either way.
        # Two or three in flight measured no faster (31.58 vs 31.66 evals/s, each
        # layer's grid fills the chip, profiles/r06_stream_eval_probe.txt)
        self.eval_streams = eval_streams
        self._streams = None
        self.evaluated_subsets = []  # coalitions evaluated this round, in evaluation order

    def powerset(self, iterable):
        "powerset([1,2,3]) --> () (1,) (2,) (3,) (1,2) (1,3) (2,3) (1,2,3)"
        s = list(iterable)
        return chain.from_iterable(combinations(s, r) for r in range(len(s) + 1))

    def _batch_size(self):
        if self.subset_batch:
            return self.subset_batch
        P = self.parameters.store.layout.P
        return max(1, min(64, (2 << 30) // (4 * P)))  # <= 2 GiB of subset models

    def _eval_stream_list(self):
        """The streams the queued forwards rotate over, or None (one stream)."""
        dev = getattr(self.tester, "device", None) or self.device
        dev = torch.device(dev) if dev is not None else None
        if (self.eval_streams is None or self.eval_streams < 2 or dev is None
                or dev.type != "cuda"
                or "stream" not in inspect.signature(self.tester.correct_async).parameters):
            return None
        if self._streams is None or len(self._streams) != self.eval_streams:
            self._streams = [torch.cuda.Stream(dev) for _ in range(self.eval_streams)]
        return self._streams

    def _metrics_tester(self):
        """Whether the loss utility runs on the tester's deterministic entries: a GPU
        tester with metrics_async, and get_metric not replaced by a subclass or on
        the instance (a replaced get_metric is the user's own utility)."""
        t = self.tester
        return (getattr(self.get_metric, "__func__", None) is FedServer.get_metric
                and t is not None and hasattr(t, "metrics_async")
                and torch.device(getattr(t, "device", None) or "cpu").type == "cuda")

    def _set_tester_metrics(self, acc, loss):
        """The tester's state as get_metric leaves it: the last evaluated model's."""
        self.tester.accuracy_metric.value = acc
        self.tester.loss_metric.value = torch.tensor(loss, dtype=torch.float64)

    def utility(self, model):
        """The utility of one model (the round metrics of the GTG and multiround
        servers): get_metric(model) for "acc"; for "loss" the mean loss, from the
        tester's metrics_async when it has one (the same float evaluate_subsets
        returns for that model), else get_metric(model, "loss")."""
        if self.utility_metric == "acc":
            return self.get_metric(model)
        if not self._metrics_tester():
            return self.get_metric(model, "loss")
        ModelUtil(self.tester.model).load_parameter_dict(model)
        correct, loss_sum = self.tester.metrics_async()
        n = self.tester.dataset[0].shape[0]
        c, l = torch.stack([correct.double(), loss_sum]).tolist()  # one synchronisation
        self._set_tester_metrics(int(c) / n, l / n)
        return l / n

    def evaluate_subsets(self, subsets):
        """Utilities of coalitions (tuples of worker ids) -> list of floats, in order.

        With a tester that scores a matrix of flat rows in one launch
        (``Inferencer.correct_many``: models.LeNet5) a batch's subset models are
        evaluated in place, ``int(count) / n`` each, and the tester module's
        parameters are NOT overwritten per coalition.  Nothing depends on them:
        ``FedServer.get_metric`` loads its model before every evaluation, and the
        only other reader in the package is ``FedServer.__init__`` (the initial
        ``prev_model`` copy)."""
        subsets = [tuple(s) for s in subsets]
        world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        rank = dist.get_rank() if world > 1 else 0
        mine = [i for i in range(len(subsets)) if i % world == rank]
        values = [0.0] * len(subsets)
        store = self.parameters.store
        bs = self._batch_size()
        # the default accuracy metric on a tester that can count without a host
        # synchronisation: the batch's evaluations are queued back to back and
        # their counts read once (int(count) / n: the same floats as get_metric)
        # (not when a subclass or the instance replaces get_metric)
        # utility_metric="loss": the same two paths through the tester's metrics_many /
        # metrics_async, which return (count, fp64 loss sum); the utility is
        # float(sum) / n
        loss = self.utility_metric == "loss"
        queued = (getattr(self.get_metric, "__func__", None) is FedServer.get_metric
                  and self.tester is not None and hasattr(self.tester, "correct_async"))
        if loss:
            queued = self._metrics_tester()
        # a tester that scores a whole matrix of flat rows in one launch
        # (Inferencer.correct_many: models.LeNet5): the batch's subset models are
        # read in place from the matrix subset_models returned, the empty coalition
        # (prev_model) from one more flattened row.  The tester module's parameters
        # are not overwritten on this path: get_metric always loads a model before
        # it evaluates (fed_server.get_metric) and nothing else in the package reads
        # the tester's parameters after construction (FedServer.__init__ copies them
        # into prev_model once), so no caller sees the difference.
        many = (queued and hasattr(self.tester, "correct_many")
                and getattr(self.tester, "supports_correct_many", None) is not None
                and self.tester.supports_correct_many(store.layout)
                and (not self.prev_model or store.layout.matches(self.prev_model)))
        if loss:
            many = many and hasattr(self.tester, "metrics_many")
        streams = self._eval_stream_list() if queued and not many and not loss else None
        for b0 in range(0, len(mine), bs):
            idx = mine[b0:b0 + bs]
            nonempty = [i for i in idx if subsets[i]]
            out = None
            if nonempty:
                rows = [[self.parameters.row_of(w) for w in subsets[i]] for i in nonempty]
                out = store.subset_models(rows, self.parameters.n_of_row(), method=self.subset_method)
            pos = {i: k for k, i in enumerate(nonempty)}
            if many:
                n = self.tester.dataset[0].shape[0]
                counts = []
                score = self.tester.metrics_many if loss else self.tester.correct_many
                if nonempty:
                    counts.append(score(out[:len(nonempty)], store.layout))
                empty = [i for i in idx if not subsets[i]]
                if empty:
                    row = store.layout.flatten(self.prev_model, device=store.device)
                    counts.append(score(row.unsqueeze(0), store.layout))
                if loss:
                    both = torch.stack([torch.cat([c for c, _ in counts]).double(),
                                        torch.cat([l for _, l in counts])]).tolist()  # one sync
                    for i in idx:
                        k = pos[i] if subsets[i] else -1
                        values[i] = both[1][k] / n
                        self.evaluated_subsets.append(subsets[i])
                    k = pos[idx[-1]] if subsets[idx[-1]] else -1
                    self._set_tester_metrics(int(both[0][k]) / n, both[1][k] / n)
                    continue
                counts = torch.cat(counts).tolist()  # one synchronisation
                for i in idx:
                    c = counts[pos[i]] if subsets[i] else counts[-1]
                    values[i] = int(c) / n
                    self.evaluated_subsets.append(subsets[i])
                self.tester.accuracy_metric.value = values[idx[-1]]
                continue
            pending = []
            for i in idx:
                model = store.layout.views(out[pos[i]]) if subsets[i] else self.prev_model
                if queued:
                    ModelUtil(self.tester.model).load_parameter_dict(model)
                    if loss:
                        c = torch.stack([t.double() for t in self.tester.metrics_async()])
                    elif streams:
                        c = self.tester.correct_async(stream=streams[len(pending) % len(streams)])
                    else:
                        c = self.tester.correct_async()
                    pending.append((i, c))
                else:
                    values[i] = float(self.utility(model))
                self.evaluated_subsets.append(subsets[i])
            if pending:
                if streams:
                    cur = torch.cuda.current_stream(streams[0].device)
                    for st in streams:
                        cur.wait_stream(st)
                n = self.tester.dataset[0].shape[0]
                counts = torch.stack([c for _, c in pending]).tolist()  # one synchronisation
                if loss:
                    for (i, _), (c, l) in zip(pending, counts):
                        values[i] = l / n
                    self._set_tester_metrics(int(counts[-1][0]) / n, counts[-1][1] / n)
                    continue
                for (i, _), c in zip(pending, counts):
                    values[i] = int(c) / n
                # the tester's state as get_metric leaves it: its accuracy metric holds
                # the last evaluated coalition's (the queued path counts top-1 only;
                # loss_metric keeps the last full inference()'s value)
                self.tester.accuracy_metric.value = values[pending[-1][0]]
        if world > 1:
            t = torch.tensor(values, dtype=torch.float64, device=self.device)
            dist.all_reduce(t)
            values = t.tolist()
        return values
