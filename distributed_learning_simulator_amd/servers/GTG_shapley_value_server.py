"""GTG-Shapley server (reference: servers/GTG_shapley_value_server.py:7-100).

Same constants (:12-18), same round truncation (:21-31), same permutation
sampling from the global ``np.random`` stream (:42-49: one
``np.random.permutation`` per worker per while-pass, in worker order), same
in-round truncation (:54), same ``contribution_records`` aliasing (D6: each
permutation's list object appended N times, :64-65), same convergence test
(:79-100) and the same SV mean (:68).

What changes is the evaluation schedule.  The reference walks one permutation
at a time and evaluates each cache-missing prefix sequentially.  Within one
while-pass the N permutations are independent (the cache only skips repeats
and utilities are deterministic), so this server draws the pass's N
permutations first and advances them in lockstep over the prefix length j:
all cache-missing prefixes of one "j-wave" become ONE batched subset-model
launch (``ShapleyValueServer.evaluate_subsets``) and, on several ranks, one
fan-out of utility evaluations.  The set of evaluated coalitions, every
truncation decision and the Shapley values are identical to the reference.
"""
import logging

import numpy as np

from .shapley_value_server import ShapleyValueServer

log = logging.getLogger("distributed_learning_simulator_amd")


class GTGShapleyValueServer(ShapleyValueServer):
    def __init__(self, **kwargs):
        super().__init__(**kwargs)
        self.shapley_values = dict()
        # trunc paras
        self.eps = 0.001
        self.round_trunc_threshold = 0.01
        # converge paras
        self.converge_min = max(30, self.worker_number)
        self.last_k = 10
        self.converge_criteria = 0.05

    def _process_aggregated_parameter(self, aggregated_parameter: dict):
        N = self.worker_number
        self.evaluated_subsets = []
        last_round_metric = self.utility(self.prev_model)
        this_round_metric = self.utility(aggregated_parameter)
        log.info("last_round_metric %s ,this_round_metric %s, round_trunc_threshold %s",
                 last_round_metric, this_round_metric, self.round_trunc_threshold)
        if abs(last_round_metric - this_round_metric) <= self.round_trunc_threshold:
            self.shapley_values[self.round] = {i: 0 for i in range(N)}
            return aggregated_parameter
        metrics = dict()
        index = 0
        contribution_records: list = []
        while self.not_convergent(index, contribution_records):
            perms = []
            for worker_id in range(N):  # RNG consumption order of the reference (:37-49)
                index += 1
                perms.append(np.concatenate((
                    np.array([worker_id]),
                    np.random.permutation([i for i in range(N) if i != worker_id]),
                )).astype(int))
            v = [[last_round_metric] + [0] * N for _ in perms]
            mc = [[0 for _ in range(N)] for _ in perms]
            for j in range(1, N + 1):
                wave, live = [], []
                for p, perm in enumerate(perms):
                    subset = tuple(sorted(perm[:j].tolist()))
                    live.append(abs(this_round_metric - v[p][j - 1]) >= self.eps)  # (:54)
                    if live[-1] and subset not in metrics and subset not in wave:
                        wave.append(subset)
                if wave:
                    for subset, value in zip(wave, self.evaluate_subsets(wave)):
                        metrics[subset] = value
                for p, perm in enumerate(perms):
                    if live[p]:
                        v[p][j] = metrics[tuple(sorted(perm[:j].tolist()))]
                    else:
                        v[p][j] = v[p][j - 1]
                    mc[p][perm[j - 1]] = v[p][j] - v[p][j - 1]
            for p in range(len(perms)):
                contribution_records.extend([mc[p]] * N)  # D6: N aliases per permutation
        shapley_value = np.sum(contribution_records, 0) / len(contribution_records)
        assert len(shapley_value) == N
        self.shapley_values[self.round] = {key: sv for key, sv in enumerate(shapley_value)}
        log.info("shapley_value %s", self.shapley_values[self.round])
        return aggregated_parameter

    def not_convergent(self, index, contribution_records):
        """servers/GTG_shapley_value_server.py:79-100."""
        if index <= self.converge_min:
            return True
        all_vals = (np.cumsum(contribution_records, 0) / np.reshape(
            np.arange(1, len(contribution_records) + 1), (-1, 1)))[-self.last_k:]
        errors = np.mean(np.abs(all_vals[-self.last_k:] - all_vals[-1:]) /
                         (np.abs(all_vals[-1:]) + 1e-12), -1)
        if np.max(errors) > self.converge_criteria:
            return True
        log.info("not convergent for index %s and converge_min %s max error %s converge_criteria %s",
                 index, self.converge_min, np.max(errors), self.converge_criteria)
        return False
