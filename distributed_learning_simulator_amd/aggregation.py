"""Device-resident client-update stores and the aggregation calls on them.

HBM layout:

* ``ClientUpdateStore.U``  fp32 [capacity, P]: one row per client, the flat
  parameter layout of ``layout.ParameterLayout`` (tensors in dict order, each
  64-element aligned).  A FedAvg round is one ``dls_fedavg_f32`` launch over K
  rows: K*P*4 bytes read once, P*4 written.
* ``ClientParameters`` keeps the reference's ``self.parameters`` mapping
  (servers/fed_server.py:15,69-73,87) — ``{worker_id: (n_i, dict)}`` in arrival
  order — but the dict values are views of the client's row in ``U``, so the
  reference hooks and user code still see per-tensor dicts.
"""
import heapq
import logging
import math
import statistics
import threading

import torch

from . import _native
from .layout import ParameterLayout

log = logging.getLogger("distributed_learning_simulator_amd")


def _i32(xs, device):
    return torch.tensor(list(xs), dtype=torch.int32).to(device, non_blocking=True)


def _f32(xs, device):
    return torch.tensor(list(xs), dtype=torch.float32).to(device, non_blocking=True)


def finite_number(name, v, positive=False):
    """float(v); ValueError unless v is a finite (``positive``: and positive) int or float."""
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) \
            or (positive and v <= 0):
        raise ValueError(f"{name} must be a {'positive finite' if positive else 'finite'} "
                         f"number, not {v!r}")
    return float(v)


def _finite_distances(dist2):
    """The indices of the squared distances that are finite and not negative."""
    return [k for k, v in enumerate(dist2) if math.isfinite(v) and v >= 0.0]


def union_order(subsets):
    """One client order that lists every subset's clients in that subset's own
    order (a topological merge of the subsets), or None if there is none (two
    subsets order a pair of clients differently, or a subset repeats a client).
    Ties go to the client seen first, so sorted subsets give the sorted union."""
    first, succ, indeg = {}, {}, {}
    for sub in subsets:
        if len(set(sub)) != len(sub):
            return None
        for c in sub:
            if c not in first:
                first[c] = len(first)
                succ[c] = set()
                indeg[c] = 0
        for a, b in zip(sub, sub[1:]):
            if b not in succ[a]:
                succ[a].add(b)
                indeg[b] += 1
    ready = [(first[c], c) for c in first if indeg[c] == 0]
    heapq.heapify(ready)
    order = []
    while ready:
        _, c = heapq.heappop(ready)
        order.append(c)
        for b in succ[c]:
            indeg[b] -= 1
            if indeg[b] == 0:
                heapq.heappush(ready, (first[b], b))
    return order if len(order) == len(first) else None


def union_batch(subsets, n_of_row, device):
    """Tables of dls_subset_fedavg_union_f32 for <= 64 subsets (row lists) over one
    union order: (urows int32, uweight fp32, member int64 masks) on the device and
    the divisors as a host list, or None when no common order exists."""
    order = union_order(subsets)
    if order is None:
        return None
    pos = {r: j for j, r in enumerate(order)}
    member = [0] * len(order)
    for s, sub in enumerate(subsets):
        for r in sub:
            member[pos[r]] |= 1 << s
    member = [m - (1 << 64) if m >= 1 << 63 else m for m in member]  # as int64
    totals = [float(sum(int(n_of_row[r]) for r in sub)) for sub in subsets]
    return (_i32(order, device), _f32([int(n_of_row[r]) for r in order], device),
            torch.tensor(member, dtype=torch.int64).to(device, non_blocking=True), totals)


def multi_krum_select(D, ids, byzantine, select):
    """The multi-Krum choice (Blanchard et al. 2017) from a [K, K] matrix of squared
    distances, on the host: (selected_ids, scores).

    ``D`` is any [K, K] array-like of float64 (row i belongs to client ``ids[i]``);
    non-finite entries count as +inf.  Client i's score is the sum, ascending in
    fp64, of the K - f - 2 smallest off-diagonal entries of row i (f =
    ``byzantine``).  The clients are ordered by (score, id) ascending (the id
    breaks ties, the arrival order never does) and the first ``select`` ids are
    returned with the scores in the order of ``ids``.  ValueError: K < 2f + 3,
    ``select`` outside 1..K - f, or fewer than ``select`` finite scores."""
    ids = list(ids)
    K, f, m = len(ids), int(byzantine), int(select)
    rows = [[float(v) for v in row] for row in D]
    if len(rows) != K or any(len(r) != K for r in rows):
        raise ValueError(f"D must be a [{K}, {K}] matrix for {K} ids")
    if f < 0 or K < 2 * f + 3:
        raise ValueError(f"multi-Krum needs 2*byzantine + 3 <= K (byzantine={f}, K={K})")
    if not 1 <= m <= K - f:
        raise ValueError(f"select={m} must be in 1..K - byzantine = {K - f}")
    scores = []
    for i, row in enumerate(rows):
        near = sorted(v if math.isfinite(v) else math.inf
                      for j, v in enumerate(row) if j != i)[:K - f - 2]
        sc = 0.0
        for v in near:
            sc += v
        scores.append(sc)
    order = sorted(range(K), key=lambda i: (scores[i], ids[i]))
    if not math.isfinite(scores[order[m - 1]]):
        finite = sum(1 for v in scores if math.isfinite(v))
        raise ValueError(f"fewer than select={m} clients have a finite score ({finite} of {K})")
    return [ids[i] for i in order[:m]], scores


def bulyan_select(D, ids, byzantine):
    """Stage 1 of Bulyan (El Mhamdi, Guerraoui & Rouault 2018), iterated Krum, from a
    [K, K] matrix of squared distances, on the host: (selected_ids, scores).

    ``D`` is any [K, K] array-like of float64 (row i belongs to client ``ids[i]``);
    non-finite entries count as +inf.  theta = K - 2f clients are chosen (f =
    ``byzantine``), one at a time from the remaining set R of r clients: client i's
    score is the sum, ascending in fp64, of its max(r - f - 2, 1) smallest D[i][j]
    over j in R, j != i, and the minimum by (score, id) is picked and leaves R (the
    id breaks ties, the arrival order never does).  ``selected_ids`` is in pick
    order, ``scores`` is {id: its score when it was picked}.  f == 0 selects
    everybody: the sorted ids and no scores.  ValueError: D is not [K, K], f < 0,
    K < 4f + 3, or a picked score is not finite."""
    ids = list(ids)
    K, f = len(ids), int(byzantine)
    rows = [[float(v) for v in row] for row in D]
    if len(rows) != K or any(len(r) != K for r in rows):
        raise ValueError(f"D must be a [{K}, {K}] matrix for {K} ids")
    if f < 0 or K < 4 * f + 3:
        raise ValueError(f"Bulyan needs 4*byzantine + 3 <= K (byzantine={f}, K={K})")
    if f == 0:
        return sorted(ids), {}
    rows = [[v if math.isfinite(v) else math.inf for v in row] for row in rows]
    theta = K - 2 * f
    remaining = list(range(K))
    selected, scores = [], {}
    while len(selected) < theta:
        c = max(len(remaining) - f - 2, 1)
        best = None
        for i in remaining:
            sc = 0.0
            for v in sorted(rows[i][j] for j in remaining if j != i)[:c]:
                sc += v
            if best is None or (sc, ids[i]) < (best[0], ids[best[1]]):
                best = (sc, i)
        if not math.isfinite(best[0]):
            raise ValueError(f"Bulyan could select only {len(selected)} of theta={theta} clients "
                             f"with a finite score (K={K}, byzantine={f})")
        scores[ids[best[1]]] = best[0]
        selected.append(ids[best[1]])
        remaining.remove(best[1])
    return selected, scores


def weiszfeld_weights(dist2, nu):
    """The weights of one smoothed Weiszfeld step (Pillutla et al., RFA) from the
    squared distances of the clients to the current iterate, on the host in fp64:
    (kept_indices, weights).

    Indices whose ``dist2`` is non-finite or negative are dropped.  For the others
    beta_i = 1 / max(nu, sqrt(dist2_i)), S = the sum of the beta_i in ascending index
    order, and weights[j] = float32(beta_i / S) (a Python float holding the fp32
    value) for the j-th kept index i.  ValueError: nothing is kept, or ``nu`` is not
    a positive finite number."""
    nu = finite_number("nu", nu, positive=True)
    d2 = [float(v) for v in dist2]
    kept = _finite_distances(d2)
    if not kept:
        raise ValueError(f"no client has a finite distance (0 of {len(d2)})")
    beta = [1.0 / max(nu, math.sqrt(d2[i])) for i in kept]
    total = 0.0
    for b in beta:
        total += b
    return kept, torch.tensor([b / total for b in beta], dtype=torch.float64).float().tolist()


def clip_scales(dist2, tau):
    """The scales of one centered-clipping step (Karimireddy et al. 2021) from the
    squared distances of the clients to the current iterate, on the host in fp64:
    (kept_indices, scales, coeffs).

    Indices whose ``dist2`` is non-finite or negative are dropped.  For the others
    s_i = 1.0 if sqrt(dist2_i) <= tau, else tau / sqrt(dist2_i) (a client inside the
    radius counts in full, one outside is pulled back onto it), and coeffs[j] =
    float32(s_i / n_kept) (a Python float holding the fp32 value) for the j-th kept
    index i: what dls_centered_clip_step_f32 multiplies the client's difference by.
    ValueError: nothing is kept, or ``tau`` is not a positive finite number."""
    tau = finite_number("tau", tau, positive=True)
    d2 = [float(v) for v in dist2]
    kept = _finite_distances(d2)
    if not kept:
        raise ValueError(f"no client has a finite distance (0 of {len(d2)})")
    dist = [math.sqrt(d2[i]) for i in kept]
    scales = [1.0 if d <= tau else tau / d for d in dist]
    n = float(len(kept))
    return kept, scales, torch.tensor([s / n for s in scales],
                                      dtype=torch.float64).float().tolist()


def dp_epsilon(noise_multiplier, rounds, delta):
    """The epsilon of the (epsilon, delta) differential-privacy guarantee of ``rounds``
    Gaussian releases, each of L2 sensitivity C with noise of standard deviation
    ``noise_multiplier`` * C (z * C): what ``ClientUpdateStore.dp_mean`` releases per round.

    Adjacency: two rounds' inputs are neighbours when one client's clipped update is
    replaced by zero, the denominator K (the number of clients averaged) staying fixed,
    with every client taking part in every round (no subsampling, so no amplification).
    The sum of the clipped updates then moves by at most C and its mean, with noise of
    standard deviation z * C / K, is the Gaussian mechanism with multiplier z.  One release
    is (alpha, alpha / (2 z^2))-Renyi DP for every order alpha > 1; T releases compose to
    alpha T / (2 z^2), and Mironov 2017, Prop. 3 converts that to (alpha T / (2 z^2) +
    ln(1 / delta) / (alpha - 1), delta)-DP.  The best order has a closed form and gives
        epsilon = T / (2 z^2) + sqrt(2 T ln(1 / delta)) / z.
    Returns ``inf`` for noise_multiplier == 0 (no noise, no guarantee) and otherwise 0.0 for
    rounds == 0.
    ValueError: delta outside (0, 1), rounds not a non-negative integer, or a
    noise_multiplier that is not a finite number >= 0."""
    z = finite_number("noise_multiplier", noise_multiplier)
    if z < 0:
        raise ValueError(f"noise_multiplier must be >= 0, not {noise_multiplier!r}")
    if isinstance(rounds, bool) or not isinstance(rounds, int) or rounds < 0:
        raise ValueError(f"rounds must be a non-negative integer, not {rounds!r}")
    if isinstance(delta, bool) or not isinstance(delta, (int, float)) or not 0.0 < delta < 1.0:
        raise ValueError(f"delta must be in (0, 1), not {delta!r}")
    if z == 0.0:
        return math.inf
    return rounds / (2.0 * z * z) + math.sqrt(2.0 * rounds * math.log(1.0 / delta)) / z


SECAGG_MAX_WORKER_ID = (1 << 16) - 1  # a stream id holds two worker ids of 16 bits


def secagg_stream_id(round, a, b):
    """The Philox stream id of a secure-aggregation mask: (round << 32) | (a << 16) | b for
    worker ids a <= b <= 65535 and 0 <= round < 2^32.  a < b: the pair mask workers a and b
    share; a == b: worker a's self mask (Bonawitz et al. 2017, double masking).  No two masks
    of a run share an id, and none repeats across rounds."""
    for name, v, top in (("round", round, (1 << 32) - 1), ("a", a, SECAGG_MAX_WORKER_ID),
                         ("b", b, SECAGG_MAX_WORKER_ID)):
        if isinstance(v, bool) or not isinstance(v, int) or not 0 <= v <= top:
            raise ValueError(f"secagg_stream_id: {name}={v!r} must be an integer in 0..{top}")
    if a > b:
        raise ValueError(f"secagg_stream_id: a={a} must not exceed b={b} (a pair is named by its "
                         "smaller id first)")
    return (round << 32) | (a << 16) | b


def _secagg_ids(name, ids):
    """The sorted list of the distinct worker ids ``ids``."""
    try:
        ids = list(ids)
    except TypeError:
        raise ValueError(f"{name} must be a collection of worker ids, not {ids!r}")
    if any(isinstance(w, bool) or not isinstance(w, int) or not 0 <= w <= SECAGG_MAX_WORKER_ID
           for w in ids):
        raise ValueError(f"{name} must be integer worker ids in 0..{SECAGG_MAX_WORKER_ID}, not "
                         f"{ids!r}")
    if len(set(ids)) != len(ids):
        raise ValueError(f"{name} must be distinct worker ids, not {ids!r}")
    return sorted(ids)


def secagg_client_streams(worker_id, participants, round):
    """(add, sub): the stream ids whose masks worker ``worker_id`` adds to and subtracts from
    its encoded update in ``round``, among the round's ``participants`` (which include it).
    add: its self mask and the pair masks with every participant of a larger id; sub: the pair
    masks with every participant of a smaller id.  Summed over all participants, every pair
    mask is added once and subtracted once."""
    ids = _secagg_ids("participants", participants)
    if worker_id not in ids:
        raise ValueError(f"worker {worker_id!r} is not among the participants {ids}")
    add = [secagg_stream_id(round, worker_id, worker_id)]
    add += [secagg_stream_id(round, worker_id, j) for j in ids if j > worker_id]
    sub = [secagg_stream_id(round, j, worker_id) for j in ids if j < worker_id]
    return add, sub


def secagg_server_streams(survivors, dropped, round):
    """(add, sub): the stream ids whose masks the server adds to and subtracts from the sum of
    the ``survivors``' payloads, when the workers in ``dropped`` took part in the key agreement
    of ``round`` and sent nothing that is used.  sub: every survivor's self mask (its shares
    are reconstructed because it survived) and the pair mask (i, d) of each survivor i and
    dropped d with i < d, which i added and d never cancelled; add: the pair mask (d, i) for
    d < i, which i subtracted.  The masks between two survivors cancel in the sum; those
    between two dropped workers never entered it."""
    alive, gone = _secagg_ids("survivors", survivors), _secagg_ids("dropped", dropped)
    both = sorted(set(alive) & set(gone))
    if both:
        raise ValueError(f"workers {both} cannot both survive and drop")
    sub = [secagg_stream_id(round, i, i) for i in alive]
    sub += [secagg_stream_id(round, i, d) for i in alive for d in gone if i < d]
    add = [secagg_stream_id(round, d, i) for i in alive for d in gone if d < i]
    return add, sub


def secagg_check_capacity(bits, weights):
    """The sum of the weights, after checking that a sum of updates quantised to ``bits`` bits
    (|q| <= L = 2^(bits-1) - 1) under these integer ``weights`` cannot wrap the ring:
    L * sum(weights) < 2^31.  The ValueError names the largest ``secagg_bits`` that fits."""
    if isinstance(bits, bool) or not isinstance(bits, int) or not 2 <= bits <= 31:
        raise ValueError(f"secagg_bits must be an integer in 2..31, not {bits!r}")
    weights = list(weights)
    if not weights or any(isinstance(n, bool) or not isinstance(n, int) or not 1 <= n < 1 << 32
                          for n in weights):
        raise ValueError(f"the weights must be integers in 1..2^32 - 1, at least one, not "
                         f"{weights!r}")
    total = sum(weights)
    if ((1 << (bits - 1)) - 1) * total >= 1 << 31:
        fits = max((b for b in range(2, 32) if ((1 << (b - 1)) - 1) * total < 1 << 31),
                   default=None)
        raise ValueError(
            f"secagg_bits={bits} does not fit: (2^{bits - 1} - 1) * {total} (the sum of the "
            f"weights) reaches 2^31 and the masked sum would wrap; "
            + (f"the largest secagg_bits that fits is {fits}" if fits is not None
               else "no secagg_bits fits weights this large"))
    return total


def foolsgold_weights(G, kappa=1.0):
    """The FoolsGold weights (Fung, Yoon & Beschastnikh, RAID 2020) from the [K, K] Gram
    matrix of the clients' accumulated updates, on the host in fp64: (alpha, info).

    ``G`` is any [K, K] array-like of float64 (row i belongs to the i-th client; the
    clients are taken in the order given).  Clients whose updates keep pointing the
    same way (sybils) get a weight near 0, clients unlike every other one a weight of 1:

    1. n_i = sqrt(G_ii).  A client whose G_ii is not finite (or negative) is rejected:
       alpha = 0, and it plays no part in the other clients' similarities.  A client
       with n_i == 0 has cosine 0 to everyone.
    2. cs_ij = G_ij / (n_i n_j) for i != j (n_i n_j taken as sqrt(G_ii G_jj), which makes
       the cosine of two histories of equal contents exactly 1), v_i = max_{j != i}
       cs_ij.  A single client gets alpha = 1.
    3. Pardoning: where v_j > v_i, cs_ij *= v_i / v_j (an honest client that resembles
       a sybil is less like it than the sybil is like its twin).  v_j == 0 has no
       finite ratio and leaves cs_ij as it is.
    4. alpha_i = clip(1 - max_{j != i} cs_ij, 0, 1), then alpha /= max alpha; when the
       maximum is 0 every alpha stays 0.
    5. alpha_i == 1 becomes 0.99; alpha_i = clip(kappa * (ln(alpha_i / (1 - alpha_i))
       + 0.5), 0, 1); alpha_i == 0 stays 0.

    ``alpha`` is a list of K Python floats; ``info`` holds ``similarity`` (per client
    its maximum cosine after pardoning; nan for a rejected or a single client) and
    ``rejected`` (ascending indices).  ValueError: G is not [K, K] with K >= 1, or
    ``kappa`` is not a positive finite number."""
    kappa = finite_number("kappa", kappa, positive=True)
    M = [[float(v) for v in row] for row in G]
    K = len(M)
    if K < 1 or any(len(r) != K for r in M):
        raise ValueError(f"G must be a [K, K] matrix with K >= 1, not {K} rows of lengths "
                         f"{sorted({len(r) for r in M})}")
    live = _finite_distances([M[i][i] for i in range(K)])
    rejected = [i for i in range(K) if i not in live]
    alpha = [0.0] * K
    sim = [math.nan] * K
    info = {"similarity": sim, "rejected": rejected}
    if len(live) <= 1:
        for i in live:
            alpha[i] = 1.0
        return alpha, info
    def cosine(i, j):
        gi, gj = M[i][i], M[j][j]
        if gi == 0.0 or gj == 0.0:
            return 0.0
        # n_i n_j as sqrt(G_ii G_jj): exactly G_ii when the two are equal, so histories
        # of equal contents (G_ij == G_ii == G_jj in bits) have a cosine of exactly 1
        den = math.sqrt(gi * gj)
        return M[i][j] / (den if math.isfinite(den) else math.sqrt(gi) * math.sqrt(gj))

    cs = {i: {j: cosine(i, j) for j in live if j != i} for i in live}
    v = {i: max(cs[i].values()) for i in live}
    for i in live:
        for j in cs[i]:
            if v[j] > v[i] and v[j] != 0.0:
                cs[i][j] *= v[i] / v[j]
        sim[i] = max(cs[i].values())
        # a NaN similarity (a non-finite off-diagonal entry of a finite client) is no
        # evidence of honesty: the weight is 0
        a = 1.0 - sim[i]
        alpha[i] = min(max(a, 0.0), 1.0) if a == a else 0.0
    top = max(alpha)
    if top == 0.0:
        return alpha, info
    for i in live:
        a = alpha[i] / top
        if a == 1.0:
            a = 0.99
        alpha[i] = 0.0 if a == 0.0 else min(max(kappa * (math.log(a / (1.0 - a)) + 0.5), 0.0), 1.0)
    return alpha, info


ATTACKS = ("alie", "ipm", "sign_flip")


def alie_z(n, f):
    """The z of "a little is enough" (Baruch, Baruch & Goldberg 2019) for ``n`` clients of
    which ``f`` are Byzantine, as the authors' code computes it: s = n // 2 + 1 - f
    honest clients must be won over for a majority, p = (n - f - s) / (n - f), and z is
    the standard normal quantile of p, so that mean - z * std still lies among the
    honest values of the s clients farthest out on that side.  The result is negative
    for a small f (p < 1/2: (n, f) = (10, 1) gives about -0.14) and is passed through
    as it is, like the authors' code does.  ValueError unless 1 <= f < n and
    0 < p < 1."""
    if any(isinstance(v, bool) or not isinstance(v, int) for v in (n, f)) or not 1 <= f < n:
        raise ValueError(f"alie_z needs integers 1 <= f < n, not n={n!r}, f={f!r}")
    s = n // 2 + 1 - f
    p = (n - f - s) / (n - f)
    if not 0.0 < p < 1.0:
        raise ValueError(f"alie_z: p = (n - f - s) / (n - f) = {p} with s = n // 2 + 1 - f = {s} "
                         f"is not inside (0, 1) (n={n}, f={f})")
    return statistics.NormalDist().inv_cdf(p)


def attack_coefficients(attack, n, f, z=None, eps=0.1):
    """(a, b, uses_base) of ``ClientUpdateStore.craft`` for the crafted attacks, ``n``
    clients of which ``f`` are Byzantine: "alie" sends mean - z * std of the honest
    updates, (1.0, -z, False), z = ``alie_z(n, f)`` unless given; "ipm" (inner product
    manipulation, Xie, Koyejo & Gupta 2019) sends -eps times the honest mean update
    relative to the previous global model, (-eps, 0.0, True).  ValueError: another
    attack name, or a z / eps that is not a finite number."""
    if attack == "alie":
        z = alie_z(n, f) if z is None else finite_number("z", z)
        return 1.0, -z, False
    if attack == "ipm":
        return -finite_number("eps", eps), 0.0, True
    raise ValueError(f"attack_coefficients: attack must be 'alie' or 'ipm', not {attack!r}")


class ClientUpdateStore:
    """``acquire_range = (lo, hi)``: this process's own clients take rows [lo, hi)
    only (a fixed block; the sharded Shapley servers all-gather every rank's block
    into the rest of ``U`` in place); rows outside it may be lent to other
    ranks' clients and are never put on the free list."""

    def __init__(self, layout: ParameterLayout, device, capacity=1, acquire_range=None):
        self.layout = layout
        self.device = torch.device(device)
        self.U = torch.zeros((max(1, capacity), layout.P), dtype=torch.float32, device=self.device)
        self._range = acquire_range
        lo, hi = acquire_range if acquire_range is not None else (0, self.U.shape[0])
        self._free = list(range(lo, hi))[::-1]
        self._lock = threading.Lock()
        self.history = None  # fp32 [worker ids, P], zeroed on first use (fold_history)
        self.model = None  # the current global model, fp32 [P] (set_model)
        self.server_opt = None  # the server optimizer's state (reset_server_opt)

    @property
    def capacity(self):
        return self.U.shape[0]

    def acquire(self):
        with self._lock:
            if not self._free:
                if self._range is not None:
                    raise RuntimeError(f"all {self._range[1] - self._range[0]} rows of this "
                                       "rank's block are in use")
                old = self.U
                new_cap = max(2 * old.shape[0], 1)
                self.U = torch.zeros((new_cap, self.layout.P), dtype=torch.float32,
                                     device=self.device)
                self.U[: old.shape[0]].copy_(old)
                self._free = list(range(old.shape[0], new_cap))[::-1]
            return self._free.pop()

    def release(self, row):
        with self._lock:
            if self._range is None or self._range[0] <= row < self._range[1]:
                self._free.append(row)

    def write(self, row, parameter_dict):
        self.layout.copy_into(parameter_dict, self.U[row])

    def accepts(self, parameter_dict):
        return self.layout.matches(parameter_dict)

    def row(self, row):
        return self.U[row]

    def views(self, row):
        return self.layout.views(self.U[row])

    # ------------------------------------------------------------ aggregation
    def fedavg(self, rows, ns, mode=_native.FEDAVG_EXACT, out=None, total=None, cols=None):
        """Weighted mean of rows in the given order (servers/fed_server.py:44-66).

        ``total`` (default: sum of ``ns``) is the divisor N; a shard of a sharded
        round passes the global N and gets its partial sum.  ``cols = (c0, c1)``
        (multiples of 4) reduces only flat elements [c0, c1) into ``out`` (of that
        length); rows / ns may then be device int32 / fp32 tensors, reused across
        column ranges."""
        U, r, width = self._reduced(rows, cols)
        if total is None:
            total = sum(int(n) for n in ns)
        w = ns if torch.is_tensor(ns) else _f32([int(n) for n in ns], self.device)
        return _native.fedavg(U, r, w, float(total), width, self._vector(width, out), mode=mode)

    def _reduced(self, rows, cols):
        """What a call over ``cols = (c0, c1)`` (default: every column) of ``rows`` hands
        its kernel: U from column c0 on, the rows as a device int32 tensor, c1 - c0."""
        c0, c1 = cols if cols is not None else (0, self.layout.P)
        r = rows if torch.is_tensor(rows) else _i32(rows, self.device)
        return self.U[:, c0:], r, c1 - c0

    def _vector(self, n, out=None):
        """``out``, or a new fp32 device vector of n elements."""
        return torch.empty(n, dtype=torch.float32, device=self.device) if out is None else out

    def _flat_operand(self, noun, t):
        """P; ValueError unless ``t`` is an fp32 vector of P elements on the store's device."""
        P = self.layout.P
        if (not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 1
                or t.numel() != P or t.device != self.U.device):
            raise ValueError(f"{noun} must be an fp32 vector of P={P} elements on {self.U.device}")
        return P

    def trimmed_mean(self, rows, trim, out=None, cols=None):
        """Coordinate-wise trimmed mean of the given rows (dls_trimmed_mean_f32): per
        flat element the ``trim`` lowest and highest of the K values are dropped and
        the rest averaged in ascending order.  The clients' sample counts play no
        part, and the result is the same bits for any order of ``rows``.  K <=
        _native.ROBUST_MAX_K, 0 <= 2*trim < K; ``cols`` as in ``fedavg``."""
        U, r, width = self._reduced(rows, cols)
        return _native.trimmed_mean(U, r, trim, width, self._vector(width, out))

    def median(self, rows, out=None, cols=None):
        """Coordinate-wise median of the given rows: ``trimmed_mean`` with
        trim = (K-1)//2 (an even K averages the two middle values)."""
        K = rows.numel() if torch.is_tensor(rows) else len(rows)
        return self.trimmed_mean(rows, (K - 1) // 2, out=out, cols=cols)

    def mean_around_median(self, rows, keep, out=None, cols=None):
        """Coordinate-wise mean around the median of the given rows
        (dls_mean_around_median_f32): per flat element the ``keep`` consecutive sorted
        values closest to the median are averaged in ascending order (MeaMed, Xie et al.
        2018; stage 2 of Bulyan).  The sample counts play no part, and the result is the
        same bits for any order of ``rows``.  K <= _native.ROBUST_MAX_K, 1 <= keep <= K;
        ``cols`` as in ``fedavg``."""
        U, r, width = self._reduced(rows, cols)
        return _native.mean_around_median(U, r, keep, width, self._vector(width, out))

    def craft(self, honest_rows, attacker_rows, a, b, base=None, cols=None):
        """Rewrite the attacker rows in place from the honest rows (dls_craft_rows_f32):
        per flat element base + a * (mu - base) + b * sigma, mu the ascending mean and
        sigma the population standard deviation of the honest values (a * mu + b *
        sigma without ``base``; ``attack_coefficients`` has the a, b of ALIE and IPM).
        The sample counts play no part, and the result is the same bits for any order
        of ``honest_rows``.  Both are host lists of row indices, 1..
        _native.ROBUST_MAX_K each; ValueError if one is empty or too long, holds a
        duplicate, or the two share a row.  ``base``: an fp32 device vector of the
        reduced length; ``cols`` as in ``fedavg``.  Returns nothing."""
        honest = [int(r) for r in honest_rows]
        bad = [int(r) for r in attacker_rows]
        for name, rows in (("honest_rows", honest), ("attacker_rows", bad)):
            if not 1 <= len(rows) <= _native.ROBUST_MAX_K:
                raise ValueError(f"craft: {name} holds {len(rows)} rows "
                                 f"(1..ROBUST_MAX_K={_native.ROBUST_MAX_K})")
            if len(set(rows)) != len(rows):
                raise ValueError(f"craft: {name} holds a row twice: {rows}")
            if min(rows) < 0 or max(rows) >= self.U.shape[0]:
                raise ValueError(f"craft: {name} {rows} outside the store's "
                                 f"{self.U.shape[0]} rows")
        both = sorted(set(honest) & set(bad))
        if both:
            raise ValueError(f"craft: rows {both} are both honest and attacker rows")
        c0, c1 = cols if cols is not None else (0, self.layout.P)
        _native.craft_rows(self.U[:, c0:], _i32(honest, self.device), _i32(bad, self.device),
                           a, b, c1 - c0, base=base)

    def sign_flip(self, rows, scale, base=None):
        """Rewrite each listed row in place as x <- base - scale * (x - base), the
        sign-flipping attack on the update relative to ``base`` (an fp32 device vector
        of ``layout.P`` elements, the previous global model); without ``base``, x <-
        -(scale * x).  Three elementwise fp32 operations in this order, each rounded
        once: d = x - base; d *= fl32(scale); x = base - d."""
        scale = finite_number("scale", scale)
        rows = [int(r) for r in rows]
        if len(set(rows)) != len(rows):
            raise ValueError(f"sign_flip: a row is listed twice: {rows}")
        scale = torch.tensor(scale, dtype=torch.float32).item()  # its fp32 value
        for r in rows:
            x = self.U[r]
            if base is None:
                d = x * scale
                torch.neg(d, out=x)
            else:
                d = x - base
                d *= scale
                torch.sub(base, d, out=x)

    def pairwise_sqdist(self, rows, cols=None):
        """Squared Euclidean distances between the given rows (dls_pairwise_sqdist_f32):
        an fp64 [K, K] device tensor, symmetric in bits, +0.0 on the diagonal, the
        same bits under any permutation of ``rows`` (permuted).  K <=
        _native.ROBUST_MAX_K; ``cols`` as in ``fedavg``."""
        U, r, width = self._reduced(rows, cols)
        return _native.pairwise_sqdist(U, r, width)

    def multi_krum(self, rows, ids, byzantine, select, out=None):
        """Multi-Krum over the given rows (client ``ids[i]`` in ``rows[i]``): one distance
        launch, one copy of D to the host, ``multi_krum_select``, then the unweighted
        ascending mean of the selected rows (``trimmed_mean`` with trim 0), which is
        the same bits for any arrival order; ``select == 1`` returns the chosen row's
        own bits.  Returns (flat, selected_ids, scores)."""
        rows = [int(r) for r in rows]
        ids = list(ids)
        D = self.pairwise_sqdist(rows).cpu().tolist()
        selected, scores = multi_krum_select(D, ids, byzantine, select)
        row_of = dict(zip(ids, rows))
        flat = self.trimmed_mean([row_of[i] for i in selected], 0, out=out)
        return flat, selected, scores

    def bulyan(self, rows, ids, byzantine, out=None):
        """Bulyan over the given rows (client ``ids[i]`` in ``rows[i]``, distinct ids): one
        distance launch, one copy of D to the host, ``bulyan_select`` (theta = K - 2f
        clients by iterated Krum), then ``mean_around_median`` over the selected rows
        with keep = theta - 2f = K - 4f.  Stage 2 depends only on the set of selected
        rows, so the result is the same bits for any arrival order.  byzantine == 0
        skips the distance launch: everybody is selected and the result is the ascending
        mean.  Returns (flat, selected_ids, scores)."""
        rows = [int(r) for r in rows]
        ids = list(ids)
        if len(set(ids)) != len(ids) or len(ids) != len(rows):
            raise ValueError("bulyan needs one distinct id per row")
        K, f = len(rows), int(byzantine)
        if f < 0 or K < 4 * f + 3:
            raise ValueError(f"Bulyan needs 4*byzantine + 3 <= K (byzantine={f}, K={K})")
        if f == 0:
            selected, scores = sorted(ids), {}
        else:
            D = self.pairwise_sqdist(rows).cpu().tolist()
            selected, scores = bulyan_select(D, ids, f)
        row_of = dict(zip(ids, rows))
        flat = self.mean_around_median([row_of[i] for i in selected], K - 4 * f, out=out)
        return flat, selected, scores

    def sqdist_to(self, rows, point, cols=None):
        """Squared Euclidean distances of the given rows to ``point`` (an fp32 device
        vector of the reduced length; dls_rows_sqdist_to_f32): an fp64 [K] device
        tensor.  K <= _native.ROBUST_MAX_K; ``cols`` as in ``fedavg``."""
        U, r, width = self._reduced(rows, cols)
        return _native.rows_sqdist_to(U, r, width, point)

    @staticmethod
    def _in_id_order(name, rows, ids, iters):
        """(int(iters), the clients as [(id, row)] in id order) of the iterated rules;
        ValueError unless iters >= 1 and every row has one distinct id."""
        iters = int(iters)
        if iters < 1:
            raise ValueError(f"iters={iters} must be at least 1")
        ids = list(ids)
        if len(set(ids)) != len(ids) or len(ids) != len(rows):
            raise ValueError(f"{name} needs one distinct id per row")
        return iters, sorted(zip(ids, (int(r) for r in rows)))

    def _iterate(self, name, active, iters, flat, step, info, trace):
        """The passes ``geometric_median`` and ``centered_clip`` share: one distance pass of
        the clients ``active`` against the iterate ``flat``, then ``iters`` times
        ``step(it, active, d2)``, which moves ``flat`` from the squared distances d2 of the
        clients that go on and returns (the fp32 coefficients it used, the fp64 device
        tensor of their squared distances to the new iterate), each followed by one copy
        of those distances to the host.  After every pass the clients whose distance is
        not finite are rejected for the rest of the call; ValueError when none is left.
        Fills ``info``: ``rejected`` (sorted ids), ``distances`` {id: distance to the
        last iterate} and, with ``trace``, per pass the (ids, coefficients or None, dist2)
        the pass ran on and gave.  Returns per pass the squared distances that went on."""
        K, passes, settled = len(active), [], []

        def settle(coeffs, d2):
            """Book one pass's distances; the clients that go on."""
            if trace:
                passes.append(([i for i, _ in active], coeffs, list(d2)))
            good = _finite_distances(d2)
            info["rejected"] = sorted(info["rejected"]
                                      + [active[k][0] for k in range(len(d2)) if k not in good])
            if not good:
                raise ValueError(f"{name}: no client is at a finite distance from the "
                                 f"iterate after pass {len(settled)} "
                                 f"({K - len(info['rejected'])} of {K} finite)")
            settled.append([d2[k] for k in good])
            return [active[k] for k in good]

        active = settle(None, self.sqdist_to([r for _, r in active], flat).cpu().tolist())
        for it in range(iters):
            coeffs, dist2 = step(it, active, settled[-1])
            active = settle(coeffs, dist2.cpu().tolist())
        info["distances"] = {i: math.sqrt(v) for (i, _), v in zip(active, settled[-1])}
        if trace:
            info["trace"] = passes
        return settled

    def geometric_median(self, rows, ids, iters, nu, out=None, trace=False):
        """The geometric median of the given rows (client ``ids[i]`` in ``rows[i]``) by
        ``iters`` smoothed Weiszfeld steps (RFA, Pillutla et al.) from the coordinate-wise
        median: the clients are taken in id order (distinct, sortable ids), so the
        result is the same bits for any arrival order.  One distance pass against the
        start, then per step ``weiszfeld_weights`` on the host, one fused
        ``dls_weiszfeld_step_f32`` into ``out`` and one copy of K doubles to the host.  A
        client whose distance is not finite after any pass is rejected for the rest of
        the call; ValueError when none is left.  Returns (flat, info): ``distances``
        {id: distance to the returned aggregate}, ``rejected`` (sorted ids),
        ``objective`` (the sum of distances after the start and after each step, added
        in id order) and, with ``trace``, per pass the (ids, fp32 weights or None,
        dist2) the pass ran on and gave."""
        iters, active = self._in_id_order("geometric_median", rows, ids, iters)
        flat = self.median([r for _, r in active], out=out)
        info = {"distances": {}, "rejected": [], "objective": []}

        def step(it, active, d2):
            _, weights = weiszfeld_weights(d2, nu)
            _, dist2 = _native.weiszfeld_step(self.U, _i32([r for _, r in active], self.device),
                                              _f32(weights, self.device), self.layout.P, flat)
            return weights, dist2

        for d2 in self._iterate("geometric_median", active, iters, flat, step, info, trace):
            obj = 0.0
            for v in d2:
                obj += math.sqrt(v)
            info["objective"].append(obj)
        return flat, info

    def centered_clip(self, rows, ids, start, tau, iters, out=None, trace=False):
        """Centered clipping (Karimireddy, He & Jaggi 2021) of the given rows (client
        ``ids[i]`` in ``rows[i]``) from ``start``: ``iters`` times v <- v + (1 / K) *
        sum_k clip(x_k - v), where a difference longer than ``tau`` is shortened to
        ``tau``, so no client moves a step by more than tau / K however far away it
        sits; ``iters=1`` is norm clipping (Sun et al. 2019).  The clients are taken in
        id order (distinct, sortable ids), so the result is the same bits for any arrival
        order.  ``start`` is an fp32 device vector of ``layout.P`` elements and is never
        modified: the iterate begins as its copy (in ``out`` if given).  One distance
        pass against the start, then per step ``clip_scales`` on the host, one fused
        ``dls_centered_clip_step_f32`` in place and one copy of K doubles to the host.
        A client whose distance is not finite after any pass is rejected for the rest
        of the call; ValueError when none is left.  Returns (flat, info):
        ``distances`` {id: distance to the returned aggregate}, ``rejected`` (sorted
        ids), ``scales`` {id: the scale s of the last step, 1.0 for a client inside the
        radius}, ``moved`` (the Euclidean length of each step: the iterate before the
        step is kept, and one device norm of the fp32 difference per step, summed in
        fp64, is copied to the host once at the end) and, with ``trace``, per pass the
        (ids, fp32 coefficients or None, dist2) the pass ran on and gave."""
        iters, active = self._in_id_order("centered_clip", rows, ids, iters)
        P = self._flat_operand("start", start)
        flat = self._vector(P, out)
        flat.copy_(start)
        prev = torch.empty_like(flat)
        moved = torch.zeros(iters, dtype=torch.float64, device=self.device)
        info = {"distances": {}, "rejected": [], "scales": {}, "moved": []}

        def step(it, active, d2):
            _, scales, coeffs = clip_scales(d2, tau)
            info["scales"] = {i: s for (i, _), s in zip(active, scales)}
            prev.copy_(flat)
            _, dist2 = _native.centered_clip_step(
                self.U, _i32([r for _, r in active], self.device), _f32(coeffs, self.device), P,
                flat)
            moved[it] = torch.linalg.vector_norm(flat - prev, dtype=torch.float64)
            return coeffs, dist2

        self._iterate("centered_clip", active, iters, flat, step, info, trace)
        info["moved"] = moved.cpu().tolist()
        return flat, info

    def dp_mean(self, rows, ids, start, clip, noise_multiplier, seed, stream_id, out=None):
        """One release of client-level DP-FedAvg (McMahan et al. 2018) over the given rows
        (client ``ids[i]`` in ``rows[i]``): every client's update U_k - ``start`` is clipped
        to the norm ``clip`` (C), the clipped updates are averaged and Gaussian noise of
        standard deviation sigma = fl32(noise_multiplier * C / n_kept) is added to every
        coordinate: start + (1 / n) sum_k min(1, C / |U_k - start|) (U_k - start) + N(0,
        sigma^2).  The clients are taken in id order (distinct, sortable ids), so the result
        is the same bits for any arrival order; the sample counts play no part.  One
        distance pass against ``start`` (dls_rows_sqdist_to_f32), one copy of K doubles to
        the host, ``clip_scales``, then one fused launch (dls_dp_clip_noise_step_f32) that
        reads the rows once.  A client whose distance is not finite is rejected (ValueError
        when none is left) and n_kept counts the others.  The noise is the library's
        Philox stream under (``seed``, ``stream_id``), coordinate p of the flat layout
        drawing value p: the caller gives every release a ``stream_id`` of its own (the
        same pair draws the same noise again), and |noise| <= 5.768 sigma (the stream's
        normals are truncated at sqrt(48 ln 2)).  noise_multiplier == 0 draws nothing: the
        result is then ``centered_clip`` with one step and tau = clip, bit for bit.
        ``start`` is an fp32 device vector of ``layout.P`` elements and is never modified.
        ``dp_epsilon`` accounts for the releases and states the adjacency.  Returns (flat,
        info): ``norms`` {id: update norm}, ``scales`` {id: s, 1.0 for a client inside the
        radius}, ``rejected`` (sorted ids), ``sigma`` (the fp32 value used) and
        ``clipped_fraction`` (of the clients kept)."""
        _, active = self._in_id_order("dp_mean", rows, ids, 1)
        P = self._flat_operand("start", start)
        clip = finite_number("clip", clip, positive=True)
        z = finite_number("noise_multiplier", noise_multiplier)
        if z < 0:
            raise ValueError(f"noise_multiplier must be >= 0, not {noise_multiplier!r}")
        d2 = self.sqdist_to([r for _, r in active], start).cpu().tolist()
        kept, scales, coeffs = clip_scales(d2, clip)  # ValueError when nothing is kept
        sigma = _native.fl32(z * clip / len(kept))
        if not math.isfinite(sigma):
            raise ValueError(f"dp_mean: sigma = noise_multiplier * clip / {len(kept)} = {sigma} "
                             "is not finite in fp32")
        flat = self._vector(P, out)
        flat.copy_(start)
        _native.dp_clip_noise_step(self.U, _i32([active[k][1] for k in kept], self.device),
                                   _f32(coeffs, self.device), P, flat, sigma, seed, stream_id)
        info = {"norms": {active[k][0]: math.sqrt(d2[k]) for k in kept},
                "scales": {active[k][0]: s for k, s in zip(kept, scales)},
                "rejected": sorted(active[k][0] for k in range(len(active)) if k not in kept),
                "sigma": sigma,
                "clipped_fraction": sum(1 for s in scales if s < 1.0) / len(kept)}
        return flat, info

    def gram(self, rows, base=None, cols=None):
        """Inner products of the given rows, taken from ``base`` if given
        (dls_rows_gram_f32): an fp64 [K, K] device tensor, symmetric in bits, the same
        bits under any permutation of ``rows`` (permuted); a cosine from it is within
        2^-17 absolute.  ``base``: an fp32 device vector of the reduced length.  K <=
        _native.ROBUST_MAX_K; ``cols`` as in ``fedavg``."""
        U, r, width = self._reduced(rows, cols)
        return _native.rows_gram(U, r, width, base=base)

    def _history_rows(self, n):
        """The history buffer with at least ``n`` rows (one per worker id), zeroed on
        first use and grown with its contents kept."""
        with self._lock:
            old = self.history
            if old is None or old.shape[0] < n:
                cap = max(n, self.U.shape[0], 2 * old.shape[0] if old is not None else 0)
                self.history = torch.zeros((cap, self.layout.P), dtype=torch.float32,
                                           device=self.device)
                if old is not None:
                    self.history[: old.shape[0]].copy_(old)
            return self.history

    def fold_history(self, rows, hrows, base=None):
        """Add the given rows' updates, U[rows[k]] - ``base``, to the history rows
        ``hrows[k]`` in place and return the Gram matrix of those history rows after
        the addition (dls_history_gram_f32: one fused visit; fp64 [K, K] on the device).
        The history is a second fp32 buffer of the store's row length, one row per
        worker id (``hrows`` are worker ids: distinct non-negative integers), allocated
        zeroed on first use; it belongs to the store, not to a round, so releasing the
        rows (``ClientParameters.clear``) leaves it alone.  Both are host lists.  The new
        history is defined bit for bit: fl32(H + fl32(U - base)) per element."""
        rows, hrows = [int(r) for r in rows], [int(h) for h in hrows]
        if len(rows) != len(hrows) or not 1 <= len(rows) <= _native.ROBUST_MAX_K:
            raise ValueError(f"fold_history: {len(rows)} rows and {len(hrows)} history rows "
                             f"(equal, 1..ROBUST_MAX_K={_native.ROBUST_MAX_K})")
        if len(set(hrows)) != len(hrows) or min(hrows) < 0:
            raise ValueError(f"fold_history: hrows must be distinct non-negative worker ids, "
                             f"not {hrows}")
        if len(set(rows)) != len(rows) or min(rows) < 0 or max(rows) >= self.U.shape[0]:
            raise ValueError(f"fold_history: rows {rows} must be distinct rows of the store's "
                             f"{self.U.shape[0]}")
        H = self._history_rows(max(hrows) + 1)
        _, G = _native.history_gram(self.U, _i32(rows, self.device), H, _i32(hrows, self.device),
                                    self.layout.P, base=base)
        return G

    def reset_history(self, hrow=None):
        """Zero the history of one worker id, or of all (None)."""
        if self.history is None:
            return
        if hrow is None:
            self.history.zero_()
        elif 0 <= int(hrow) < self.history.shape[0]:
            self.history[int(hrow)].zero_()

    def foolsgold(self, rows, ids, G, base, kappa=1.0, out=None):
        """The FoolsGold aggregate of the given rows (client ``ids[i]`` in ``rows[i]``)
        from the Gram matrix ``G`` of the clients' histories (row i of G belongs to
        ``ids[i]``; any [K, K] array-like, e.g. what ``fold_history`` returned, copied to
        the host): ``foolsgold_weights`` with the clients in id order (distinct, sortable
        ids), so the result is the same bits for any arrival order, then the
        alpha-weighted mean of the updates taken from ``base``,
            base + sum_k c_k (U_k - base),   c_k = fl32(alpha_k / sum alpha),
        over the clients with alpha > 0 in id order: exactly one
        dls_centered_clip_step_f32 from z = base with those c.  The paper adds sum alpha_k
        * delta_k at a global learning rate; this normalises instead, as the other rules
        return a model and not a step.  When every alpha is 0 the aggregate is ``base``
        unchanged and a warning is logged.  ``base`` is an fp32 device vector of
        ``layout.P`` elements and is never modified.  Returns (flat, info): ``weights``
        {id: alpha}, ``similarity`` {id: maximum cosine after pardoning}, ``rejected``
        (sorted ids whose history is not finite), ``coefficients`` {id: c_k}."""
        ids = list(ids)
        rows = [int(r) for r in rows]
        if len(set(ids)) != len(ids) or len(ids) != len(rows):
            raise ValueError("foolsgold needs one distinct id per row")
        P = self._flat_operand("base", base)
        M = G.cpu().tolist() if torch.is_tensor(G) else [list(r) for r in G]
        order = sorted(range(len(ids)), key=lambda i: ids[i])
        alpha, winfo = foolsgold_weights([[M[i][j] for j in order] for i in order], kappa)
        sids = [ids[i] for i in order]
        info = {"weights": dict(zip(sids, alpha)),
                "similarity": dict(zip(sids, winfo["similarity"])),
                "rejected": [sids[i] for i in winfo["rejected"]], "coefficients": {}}
        flat = self._vector(P, out)
        flat.copy_(base)
        kept = [k for k, a in enumerate(alpha) if a > 0.0]
        total = 0.0
        for k in kept:
            total += alpha[k]
        if not kept:
            log.warning("foolsgold: every client's weight is 0 (%s clients, rejected %s); the "
                        "aggregate is the base", len(ids), info["rejected"])
            return flat, info
        coeffs = torch.tensor([alpha[k] / total for k in kept], dtype=torch.float64).float().tolist()
        info["coefficients"] = {sids[k]: c for k, c in zip(kept, coeffs)}
        _native.centered_clip_step(self.U, _i32([rows[order[k]] for k in kept], self.device),
                                   _f32(coeffs, self.device), P, flat)
        return flat, info

    # ------------------------------------------------------- server optimizer
    def set_model(self, flat):
        """Hold ``flat`` (an fp32 device vector of ``layout.P`` elements, padding zero) as
        the current global model: what the next ``server_opt_step`` steps from."""
        self._flat_operand("the model", flat)
        self.model = flat

    def reset_server_opt(self, kind=None, coeffs=None):
        """The server optimizer's initial state for ``kind`` (a ``_native.SERVER_OPT_*``)
        and ``coeffs`` (``_native.server_opt_coeffs``): step 0, m zero, v = fl32(tau *
        tau) on the tensors' elements (Reddi et al. start from v >= tau^2) and zero on
        the padding between them; SGD has no v, and no m either without momentum.
        Without arguments: the state goes back to its start for the kind and coefficients
        it was made with (nothing happens while there is none)."""
        if kind is None:
            if self.server_opt is None:
                return
            kind, coeffs = self.server_opt["kind"], self.server_opt["coeffs"]
        P = self.layout.P
        _, beta1, _, _, _, tau = coeffs
        sgd = kind == _native.SERVER_OPT_SGD
        m = None if sgd and beta1 == 0.0 else torch.zeros(P, dtype=torch.float32,
                                                            device=self.device)
        v = None
        if not sgd:
            v = torch.zeros(P, dtype=torch.float32, device=self.device)
            v0 = _native.fl32(tau * tau)  # the product of two fp32 is exact in fp64
            for o, n in zip(self.layout.offsets, self.layout.numels):
                v[o:o + n] = v0
        self.server_opt = {"kind": kind, "coeffs": tuple(coeffs), "step": 0, "m": m, "v": v}

    def server_opt_step(self, flat_agg, kind, coeffs):
        """One server-optimizer step (dls_server_opt_step_f32) from the held model
        (``set_model``) towards the aggregate ``flat_agg``, an fp32 device vector of
        ``layout.P`` elements: the pseudo-gradient is flat_agg - model.  ``kind`` is a
        ``_native.SERVER_OPT_*``, ``coeffs`` the fp32 values of
        ``_native.server_opt_coeffs``; the state (``server_opt``: step, m, v) is made by
        ``reset_server_opt`` on first use, or when the kind or the coefficients change,
        and updated in place.  The new model is a new vector: it is returned and held as
        the current model; flat_agg and the old model are left alone.  The padding
        between the tensors stays exactly zero in the model, m and v: there d = 0, m = 0
        and v = 0, so the update is 0 / tau = 0."""
        if self.model is None:
            raise ValueError("server_opt_step: no current model (set_model)")
        coeffs = tuple(coeffs)
        st = self.server_opt
        if st is None or st["kind"] != kind or st["coeffs"] != coeffs:
            self.reset_server_opt(kind, coeffs)
            st = self.server_opt
        lr, beta1, _, beta2, _, tau = coeffs
        out = _native.server_opt_step(kind, flat_agg, self.model, st["m"], st["v"],
                                      self._vector(self.layout.P), self.layout.P, lr, beta1, beta2,
                                      tau)
        st["step"] += 1
        self.model = out
        return out

    def subset_models(self, subsets, n_of_row, method="exact", out=None):
        """S subset models at once.  subsets: list of row lists (non-empty, in order).

        ``method="exact"``: the reference's operation order, bit for bit; only a
        coalition's own rows are read.  ``method="gemm"``: one dls_subset_gemm_f32
        call over the sorted union of the subsets' rows (rows in no subset are not
        read) with c_sr = fl32(n_r / N_s) computed in fp64, whatever the order inside
        a subset; each element within (K+1) 2^-24 of the magnitude sum of its terms.
        It is a dense product: an inf or NaN in one client's row makes that parameter
        non-finite in every subset of the call, the ones without that client included
        (0 * inf is NaN)."""
        S = len(subsets)
        P = self.layout.P
        if out is None:
            out = torch.empty((S, P), dtype=torch.float32, device=self.device)
        if method == "exact" and all(subsets):
            # each client row read once per batch of <= 64 coalitions (the union
            # kernel), when one client order suits every coalition (always for the
            # Shapley servers' sorted tuples); else one coalition per grid row
            tables = [union_batch(subsets[c0:c0 + _native.SUBSET_UNION_MAX], n_of_row, self.device)
                      for c0 in range(0, S, _native.SUBSET_UNION_MAX)]
            if all(t is not None for t in tables):
                for i, t in enumerate(tables):
                    c0 = i * _native.SUBSET_UNION_MAX
                    _native.subset_fedavg_union(self.U, *t, P, out[c0:c0 + len(t[3])])
                return out
        if method == "exact":
            off, flat_rows, flat_w, totals = [0], [], [], []
            for sub in subsets:
                flat_rows.extend(sub)
                ws = [int(n_of_row[r]) for r in sub]
                flat_w.extend(ws)
                totals.append(float(sum(ws)))
                off.append(len(flat_rows))
            _native.subset_fedavg(self.U, _i32(off, self.device), _i32(flat_rows, self.device),
                                  _f32(flat_w, self.device), _f32(totals, self.device), P, out)
        elif method == "gemm":
            rows = sorted({r for sub in subsets for r in sub})
            col = {r: j for j, r in enumerate(rows)}
            C = torch.zeros((S, len(rows)), dtype=torch.float64)
            for s, sub in enumerate(subsets):
                tot = float(sum(int(n_of_row[r]) for r in sub))
                for r in sub:
                    C[s, col[r]] = int(n_of_row[r]) / tot
            _native.subset_gemm(C.float().to(self.device), self.U, _i32(rows, self.device), P, out)
        else:
            raise ValueError(f"unknown subset method {method!r}")
        return out


class SlicedClientUpdateStore:
    """Client rows stored slice-major for the bit-exact sharded FedAvg exchange
    (distributed.ShardedFedServer, exchange="alltoall"): the flat row is cut into
    ``world`` slices of L elements (distributed.slice_bounds) and ``B`` is fp32
    [world, capacity, L], so slice d of every client this rank holds is ONE
    contiguous block B[d] — the all-to-all sends straight from the store, one
    block per peer, with no per-client operation and no staging copy.  A
    client's dict is written tensor by tensor into its slices (a tensor that
    straddles a slice boundary is written in pieces); ``views`` returns views of
    the tensors that lie in one slice and copies of the (at most world - 1)
    straddling ones."""

    def __init__(self, layout: ParameterLayout, device, capacity, world, L):
        self.layout = layout
        self.device = torch.device(device)
        self.world, self.L = world, L
        self.B = torch.zeros((world, max(1, capacity), L), dtype=torch.float32, device=self.device)
        self._free = list(range(self.B.shape[1]))[::-1]
        self._lock = threading.Lock()

    @property
    def capacity(self):
        return self.B.shape[1]

    def acquire(self):
        with self._lock:
            if not self._free:
                old = self.B
                cap = 2 * old.shape[1]
                self.B = torch.zeros((self.world, cap, self.L), dtype=torch.float32,
                                     device=self.device)
                self.B[:, : old.shape[1]].copy_(old)
                self._free = list(range(old.shape[1], cap))[::-1]
            return self._free.pop()

    def release(self, row):
        with self._lock:
            self._free.append(row)

    def accepts(self, parameter_dict):
        return self.layout.matches(parameter_dict)

    def _pieces(self, o, m):
        """(slice, start in slice, start in tensor, length) of flat range [o, o+m)."""
        L, out, e = self.L, [], o
        while e < o + m:
            s, a = divmod(e, L)
            n = min(o + m - e, L - a)
            out.append((s, a, e - o, n))
            e += n
        return out

    def write(self, row, parameter_dict):
        dst, src = [], []
        for name, m, o in zip(self.layout.names, self.layout.numels, self.layout.offsets):
            t = parameter_dict[name].detach().reshape(-1)
            t = t if t.dtype == torch.float32 else t.float()
            for s, a, b, n in self._pieces(o, m):
                dst.append(self.B[s, row, a:a + n])
                src.append(t[b:b + n])
        torch._foreach_copy_(dst, src, non_blocking=True)

    def views(self, row):
        out = {}
        for name, shape, m, o in zip(self.layout.names, self.layout.shapes, self.layout.numels,
                                     self.layout.offsets):
            parts = [self.B[s, row, a:a + n] for s, a, _, n in self._pieces(o, m)]
            out[name] = (parts[0] if len(parts) == 1 else torch.cat(parts)).view(shape)
        return out

    def row(self, row):
        """The client's flat row (a copy: its slices are not contiguous)."""
        return self.B[:, row, :].reshape(-1)[: self.layout.P]


class ClientParameters(dict):
    """``self.parameters`` of the reference FedServer, backed by a ClientUpdateStore.

    ``params[worker_id] = (n, parameter_dict)`` copies the dict into the
    worker's row; ``params[worker_id]`` returns ``(n, dict of row views)``.
    """

    def __init__(self, store_factory):
        """store_factory(first_payload) -> store with acquire/release/write/views/accepts."""
        super().__init__()
        self._store_factory = store_factory
        self.store = None
        self._rows = {}

    def _ensure_store(self, parameter_dict):
        if self.store is None:
            self.store = self._store_factory(parameter_dict)
        elif not self.store.accepts(parameter_dict):
            raise ValueError("client parameter dict does not match the model layout")

    def __setitem__(self, worker_id, value):
        n, parameter_dict = value
        self._ensure_store(parameter_dict)
        row = self._rows.get(worker_id)
        if row is None:
            row = self.store.acquire()
            self._rows[worker_id] = row
        self.store.write(row, parameter_dict)
        super().__setitem__(worker_id, int(n))

    def __getitem__(self, worker_id):
        n = super().__getitem__(worker_id)
        return n, self.store.views(self._rows[worker_id])

    def __delitem__(self, worker_id):
        super().__delitem__(worker_id)
        self.store.release(self._rows.pop(worker_id))

    def items(self):
        return [(k, self[k]) for k in self.keys()]

    def values(self):
        return [self[k] for k in self.keys()]

    def pop(self, worker_id, *default):
        if worker_id not in self and default:
            return default[0]
        v = self[worker_id]
        del self[worker_id]
        return v

    def clear(self):
        for k in list(self.keys()):
            del self[k]

    def row_of(self, worker_id):
        return self._rows[worker_id]

    def adopt(self, entries):
        """Re-register the clients as [(worker_id, n, row)] in that order, for rows
        the store already holds (the sharded Shapley gather lands every rank's
        clients in place): no copy; rows this process did not acquire are never
        released to its free list (ClientUpdateStore.acquire_range)."""
        rows = {w: r for w, _, r in entries}
        for w in list(self.keys()):
            if self._rows[w] != rows.get(w):
                self.store.release(self._rows[w])
        dict.clear(self)
        self._rows = {}
        for w, n, r in entries:
            self._rows[w] = r
            dict.__setitem__(self, w, int(n))

    def n_of(self, worker_id):
        return dict.__getitem__(self, worker_id)

    def n_of_row(self):
        return {r: dict.__getitem__(self, w) for w, r in self._rows.items()}
