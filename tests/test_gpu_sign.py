"""GPU parity: sign pack / vote / worker step vs the oracle and golden vectors (bit-exact)."""
import numpy as np
import pytest
import torch

from oracle import sign as osign
from tests import golden as G

pytestmark = pytest.mark.gpu

dev = torch.device("cuda")


def same_bits(a, b):
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(
        a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


def pack(S):
    from distributed_learning_simulator_amd import _native
    K, P = S.shape
    Pp = (P + 3) // 4 * 4
    X = torch.zeros((K, Pp), dtype=torch.float32)
    X[:, :P] = torch.from_numpy(np.ascontiguousarray(S))
    X = X.to(dev)
    planes = torch.full((K, _native.sign_words(P)), 0xAB, dtype=torch.int64, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    _native.sign_pack(X, P, planes, bad)
    return planes, int(bad.item())


def test_pack_matches_wire_format():
    g = np.random.default_rng(0)
    for P in (1, 63, 64, 255, 256, 1000, 4096 + 68):
        S = np.sign(g.standard_normal((3, P))).astype(np.float32)
        S[:, ::13] = 0
        S[1, P // 2] = np.nan
        planes, bad = pack(S)
        assert bad == 0
        got = planes.cpu().numpy().view(np.uint64)
        for k in range(3):
            assert np.array_equal(got[k], osign.pack_planes(S[k])), (P, k)


def test_pack_flags_nonternary():
    S = np.array([[1.0, 0.5, -1.0, 2.0, 0.0, np.inf, -0.0, np.nan]], np.float32)
    _, bad = pack(S)
    assert bad == 3  # 0.5, 2.0, inf


def test_vote_golden_bit_exact():
    from distributed_learning_simulator_amd import _native
    z = G.load("sign_vote.npz")
    for case in G.meta(z):
        S, vote = z[f"{case['key']}_signs"], z[f"{case['key']}_vote"]
        K, P = S.shape
        planes, _ = pack(S)
        Pp = (P + 3) // 4 * 4
        out = torch.empty(Pp, device=dev)
        counts = torch.empty(Pp, dtype=torch.int32, device=dev)
        _native.sign_vote(planes, None, K, Pp, out, counts)
        assert same_bits(out.cpu().numpy()[:P], vote), case["key"]
        assert np.array_equal(counts.cpu().numpy()[:P], osign.vote_counts(S))
        # two-stage path (what the multi-GPU server uses): counts -> sign + packed vote
        c2 = torch.empty(Pp, dtype=torch.int32, device=dev)
        _native.sign_vote_count(planes, None, K, Pp, c2)
        assert torch.equal(c2, counts)
        s2 = torch.empty(Pp, device=dev)
        vp = torch.zeros(_native.sign_words(Pp), dtype=torch.int64, device=dev)
        _native.sign_from_counts(c2, Pp, s2, vp)
        assert same_bits(s2.cpu().numpy()[:P], vote)
        assert np.array_equal(vp.cpu().numpy().view(np.uint64)[: osign.pack_planes(vote).size],
                              osign.pack_planes(np.pad(vote, (0, Pp - P))))


def gpu_vote_reference(planes, rows, P):
    """(#pos, #neg, any NaN code) per parameter from the plane words themselves: a bit
    unpack with torch ops on the GPU, no loop over the clients.  planes: int64
    [*, >= 2 * ceil(P / 64)]; rows: row indices (repeats count twice) or None."""
    ng = (P + 63) // 64
    sel = planes if rows is None else planes[rows.long()]
    pos, neg = sel[:, 0:2 * ng:2], sel[:, 1:2 * ng:2]  # [K, ng]
    both = pos & neg
    cp = torch.empty((ng, 64), dtype=torch.int32, device=planes.device)
    cn = torch.empty_like(cp)
    nan = torch.empty((ng, 64), dtype=torch.bool, device=planes.device)
    for j in range(64):
        cp[:, j] = ((pos >> j) & 1).sum(0, dtype=torch.int32)
        cn[:, j] = ((neg >> j) & 1).sum(0, dtype=torch.int32)
        nan[:, j] = ((both >> j) & 1).any(0)
    return cp.reshape(-1)[:P], cn.reshape(-1)[:P], nan.reshape(-1)[:P]


def gpu_pack_reference(sign, W):
    """int64 [W] wire planes of a ternary fp32 vote [P] (torch ops, zero padded)."""
    P = sign.numel()
    s = torch.zeros(W * 32, device=sign.device)
    s[:P] = sign
    sh = torch.arange(64, device=sign.device)
    out = torch.empty(W, dtype=torch.int64, device=sign.device)
    out[0::2] = ((s > 0).reshape(-1, 64).long() << sh).sum(1)  # wraps into bit 63
    out[1::2] = ((s < 0).reshape(-1, 64).long() << sh).sum(1)
    return out


def check_vote_against_planes(planes, rows, K, P):
    """dls_sign_vote_count and the fused dls_sign_vote (signs + counts + packed vote)
    against gpu_vote_reference, on every parameter."""
    from distributed_learning_simulator_amd import _native
    cp, cn, nan = gpu_vote_reference(planes, rows, P)
    ref_counts = cp - cn + nan.int() * _native.SIGN_NAN_MARK
    ref_sign = torch.where(nan, torch.zeros((), device=dev), torch.sign((cp - cn).float()))
    W = _native.sign_words(P)
    counts = torch.full((P,), -7, dtype=torch.int32, device=dev)
    _native.sign_vote_count(planes, rows, K, P, counts)
    assert torch.equal(counts, ref_counts)
    c2 = torch.full((P,), -7, dtype=torch.int32, device=dev)
    sign = torch.full((P,), 7.0, device=dev)
    vote = torch.full((W,), 0x55, dtype=torch.int64, device=dev)
    _native.sign_vote(planes, rows, K, P, sign, counts=c2, vote_planes=vote)
    assert torch.equal(c2, ref_counts)
    assert torch.equal(sign.view(torch.int32), ref_sign.view(torch.int32))
    assert torch.equal(vote, gpu_pack_reference(ref_sign, W))
    s3 = torch.full((P,), 7.0, device=dev)  # the server's instance: no counts
    v3 = torch.full((W,), 0x55, dtype=torch.int64, device=dev)
    _native.sign_vote(planes, rows, K, P, s3, vote_planes=v3)
    assert torch.equal(s3.view(torch.int32), ref_sign.view(torch.int32))
    assert torch.equal(v3, vote)
    return cp, cn


def one_sided_planes(K, W, seed, nan_row):
    """Random planes without NaN codes; group 0 all-positive and group 1 all-negative in
    every row, so that the counts reach +K and -K (the only inputs that drive the
    eights counter to its top value); NaN codes in group 2 of one row."""
    g = torch.Generator(device=dev).manual_seed(seed)
    planes = torch.randint(-2**62, 2**62, (K, W), generator=g, device=dev)
    planes[:, 1::2] &= ~planes[:, 0::2]  # no NaN codes
    planes[:, 0], planes[:, 1] = -1, 0
    planes[:, 2], planes[:, 3] = 0, -1
    planes[nan_row, 5] |= planes[nan_row, 4]
    return planes


# vote_dispatch picks the counter width CB from (K + 7) / 8 < 2^CB: the widths change
# between K = 24|25, 120|121, 504|505, 2040|2041 and 32760|32761 (CB = 16 from there)
@pytest.mark.parametrize("K", [1, 2, 15, 16, 255, 256, 1023, 1024, 4100,
                               24, 25, 120, 121, 504, 505, 2040, 2041, 32760, 32761])
def test_vote_counter_widths(K):
    """Every bit-sliced counter width on both sides of each width boundary, with all
    K clients on one side of a parameter."""
    from distributed_learning_simulator_amd import _native
    P = 1024
    planes = one_sided_planes(K, _native.sign_words(P), K, K // 2)
    planes[: K // 2 + 1, 6::2] |= -1  # a majority positive on every other parameter...
    planes[: K // 2 + 1, 7::2] = 0
    cp, cn = check_vote_against_planes(planes, None, K, P)
    assert int((cp - cn)[:64].min()) == K and int((cp - cn)[64:128].max()) == -K
    if K <= 4100:  # the oracle's unpack, client by client
        w = planes.cpu().numpy().view(np.uint64)
        ref = np.zeros(P, np.int64)
        for k in range(K):
            ref += np.nan_to_num(osign.unpack_planes(w[k], P)).astype(np.int64)
        assert np.array_equal((cp - cn).cpu().numpy(), ref)


@pytest.mark.parametrize("K,CB,subset", [(40, 4, True), (130, 6, False), (2048, 12, False)])
def test_vote_wide_layout_counter_widths(K, CB, subset):
    """The wide per-wave layout (G > 1 groups per lane) with the counter widths it had
    never run with: signs, counts and packed vote on every parameter."""
    from distributed_learning_simulator_amd import _native
    P = 4_000_000
    W = _native.sign_words(P)
    # the host's condition for G > 1 (launch_vote), restated so that the case cannot
    # fall back to one group per lane on a part with more CUs
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    vote_groups = W // 2
    assert -(-vote_groups // (4 * cus)) + 7 > 64, cus
    c_max = (K + 7) // 8
    assert c_max < (1 << CB) and c_max >= (1 << {4: 2, 6: 4, 12: 8}[CB])
    rows = None
    nrows = K
    if subset:  # K of K + 10 rows, out of order, one of them twice
        nrows = K + 10
        idx = torch.randperm(nrows, generator=torch.Generator().manual_seed(K))[:K]
        idx[7] = idx[3]
        rows = idx.to(torch.int32).to(dev)
    planes = one_sided_planes(nrows, W, K, nrows // 2 if rows is None else int(rows[0]))
    planes[:, 2 * ((P + 63) // 64):] = 0  # past P: zero, as the packer leaves it
    cp, cn = check_vote_against_planes(planes, rows, K, P)
    assert int((cp - cn)[:64].min()) == K and int((cp - cn)[64:128].max()) == -K


@pytest.mark.parametrize("P", [1000, 4096, 4097, 4352 - 3])
def test_pack_server_geometry(P):
    """dls_sign_pack_f32 as SignSGDServer calls it: padded X rows, plane rows at the
    128-byte pitch, one-row launches into planes[slot:slot + 1], and a nonternary
    counter that the kernel only ever adds to.  16 tiles of 256 make a block: 4096 is
    the last size of one block, 4097 and 4349 have 17 tiles."""
    from distributed_learning_simulator_amd import _native
    K = 5
    ldx = (P + 3) // 4 * 4 + 12  # P + 12 where the library accepts it (ldx % 4 == 0)
    W, pitch = _native.sign_words(P), _native.sign_row_pitch(P)
    g = np.random.default_rng(P)
    S = g.integers(-1, 2, (K, P)).astype(np.float32)
    S[:, ::13] = -0.0
    S[1, P // 2] = S[4, P - 1] = np.nan
    S[2, 0], S[2, P - 1], S[3, P // 3] = 0.5, np.inf, -2.0  # 3 nonternary values
    X = torch.full((K, ldx), 7.0, device=dev)  # the pitch padding is nonternary: never read
    X[:, :P] = torch.from_numpy(S)
    fill = 0xABABABABABABABAB - (1 << 64)
    want = np.stack([osign.pack_planes(S[k]) for k in range(K)])
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    planes = torch.full((K, pitch), fill, dtype=torch.int64, device=dev)
    _native.sign_pack(X, P, planes, bad)
    got = planes.cpu().numpy().view(np.uint64)
    assert np.array_equal(got[:, :W], want)
    assert np.all(got[:, W:] == np.uint64(0xABABABABABABABAB))  # pitch words untouched
    assert int(bad.item()) == 3
    # the server's form: one row per launch; the counter accumulates over launches
    planes2 = torch.full((K, pitch), fill, dtype=torch.int64, device=dev)
    for k in range(K):
        _native.sign_pack(X[k:k + 1], P, planes2[k:k + 1], bad)
    assert torch.equal(planes2, planes)
    assert int(bad.item()) == 6
    if P % 4:  # a row pitch of P + 12 that is no multiple of 4 is rejected before any launch
        Xo = torch.zeros((K, P + 12), device=dev)
        with pytest.raises(RuntimeError):
            _native.sign_pack(Xo, P, planes2, bad)
        assert int(bad.item()) == 6


def test_vote_rows_subset_order_free():
    from distributed_learning_simulator_amd import _native
    K, P = 40, 2048
    g = torch.Generator(device=dev).manual_seed(1)
    S = torch.randint(-1, 2, (K, P), generator=g, device=dev).float()
    planes, _ = pack(S.cpu().numpy())
    rows = torch.tensor([5, 3, 39, 0, 12], dtype=torch.int32, device=dev)
    out = torch.empty(P, device=dev)
    _native.sign_vote(planes, rows, 5, P, out)
    ref = osign.majority_vote(S.cpu().numpy()[[5, 3, 39, 0, 12]])
    assert same_bits(out.cpu().numpy(), ref)


def test_vote_1000_clients_resnet18_sampled():
    """Config 3 at full size: 1000 x 11,173,962 parameters; sampled exact check + linearity."""
    from distributed_learning_simulator_amd import _native
    K, P = 1000, 11173962
    Pp = (P + 3) // 4 * 4
    W = _native.sign_words(P)
    g = torch.Generator(device=dev).manual_seed(7)
    planes = torch.randint(-2**62, 2**62, (K, W), generator=g, device=dev)
    planes[:, 1::2] &= ~planes[:, 0::2]
    counts = torch.empty(Pp, dtype=torch.int32, device=dev)
    _native.sign_vote_count(planes, None, K, Pp, counts)
    # linearity: counts(all) == counts(first half) + counts(second half)
    c1 = torch.empty_like(counts)
    c2 = torch.empty_like(counts)
    _native.sign_vote_count(planes[:500], None, 500, Pp, c1)
    _native.sign_vote_count(planes[500:], None, 500, Pp, c2)
    assert torch.equal(counts, c1 + c2)
    # exact check on 2048 sampled parameters
    idx = torch.randint(0, P, (2048,), generator=g, device=dev)
    words = planes[:, (idx // 64) * 2].cpu().numpy().view(np.uint64)
    nwords = planes[:, (idx // 64) * 2 + 1].cpu().numpy().view(np.uint64)
    bit = (idx % 64).cpu().numpy().astype(np.uint64)
    pos = ((words >> bit) & np.uint64(1)).astype(np.int64).sum(0)
    neg = ((nwords >> bit) & np.uint64(1)).astype(np.int64).sum(0)
    assert np.array_equal(counts[idx].cpu().numpy(), pos - neg)


def test_sign_worker_golden_bit_exact():
    """workers/sign_sgd_worker.py:19-58 fused on device, step by step vs golden."""
    from distributed_learning_simulator_amd import _native
    z = G.load("sign_worker.npz")
    for case in G.meta(z):
        k, cfg, layout = case["key"], case["cfg"], case["layout"]
        p = torch.from_numpy(z[f"{k}_p0"].copy())
        bufs, seen = {}, set()
        for s in range(case["steps"]):
            grad, has = z[f"{k}_s{s}_grad"], z[f"{k}_s{s}_hasgrad"]
            vote = z[f"{k}_s{s}_vote"]
            off = 0
            newp = p.clone()
            for ti, (name, shape) in enumerate(layout):
                m = int(np.prod(shape))
                sl = slice(off, off + m)
                off += m
                if not has[ti]:
                    continue
                first = name not in seen
                gd = torch.from_numpy(grad[sl].copy()).to(dev)
                if name not in bufs:
                    bufs[name] = torch.zeros(m, device=dev)
                planes = torch.zeros(_native.sign_words(m), dtype=torch.int64, device=dev)
                sout = torch.empty(m, device=dev)
                _native.sign_sgd_direction(gd, bufs[name], cfg["momentum"], 1 - cfg["dampening"],
                                           cfg["nesterov"], first, planes, sout)
                if cfg["momentum"] != 0:
                    seen.add(name)
                    assert same_bits(bufs[name].cpu().numpy(), z[f"{k}_s{s}_buf"][sl])
                assert same_bits(sout.cpu().numpy(), z[f"{k}_s{s}_sent"][sl]), (k, s, name)
                vplanes = torch.from_numpy(osign.pack_planes(vote[sl]).view(np.int64)).to(dev)
                pd = p[sl].clone().to(dev)
                _native.sign_sgd_apply(pd, vplanes, -cfg["lr"], cfg["weight_decay"])
                newp[sl] = pd.cpu()
            p = newp
            assert same_bits(p.numpy(), z[f"{k}_s{s}_param"]), (k, s)


@pytest.mark.parametrize("P,K", [(4, 3), (1000, 17), (4096 + 68, 64), (70000, 130)])
def test_fused_vote_planes_match_two_stage(P, K):
    """dls_sign_vote's packed vote (and sign-only mode) == counts -> sign_from_counts."""
    from distributed_learning_simulator_amd import _native
    g = np.random.default_rng(P + K)
    S = np.sign(g.standard_normal((K, P))).astype(np.float32)
    S[:, ::7] = 0
    S[K // 2, 3] = np.nan  # one poisoned parameter
    S[:, 1] = 0  # a tie at zero
    planes, _ = pack(S)
    Pp = (P + 3) // 4 * 4
    Wd = _native.sign_words(Pp)
    s1 = torch.empty(Pp, device=dev)
    v1 = torch.full((Wd,), 0x55, dtype=torch.int64, device=dev)
    _native.sign_vote(planes, None, K, Pp, s1, vote_planes=v1)
    c = torch.empty(Pp, dtype=torch.int32, device=dev)
    _native.sign_vote_count(planes, None, K, Pp, c)
    s2 = torch.empty(Pp, device=dev)
    v2 = torch.zeros(Wd, dtype=torch.int64, device=dev)
    _native.sign_from_counts(c, Pp, s2, v2)
    assert same_bits(s1.cpu().numpy(), s2.cpu().numpy())
    assert torch.equal(v1, v2)
    assert same_bits(s1.cpu().numpy()[:P], osign.majority_vote(S))
    v3 = torch.zeros(Wd, dtype=torch.int64, device=dev)  # packed vote alone
    _native.sign_vote(planes, None, K, Pp, None, vote_planes=v3)
    assert torch.equal(v3, v2)


def test_vote_wide_tiles_rows_and_padding():
    """Large models take the 4-groups-per-lane vote; its last block holds live groups,
    padding groups (ngroups <= g < vote_groups) and groups past the end."""
    from distributed_learning_simulator_amd import _native
    K, P = 20, 9_000_004  # ngroups 140626, vote_groups 140628: 550 blocks of 256 groups
    Wd = _native.sign_words(P)
    g = torch.Generator(device=dev).manual_seed(11)
    planes = torch.randint(-2**62, 2**62, (K, Wd), generator=g, device=dev)
    planes[:, 1::2] &= ~planes[:, 0::2]
    planes[3, 2 * 140620 + 1] |= planes[3, 2 * 140620]  # NaN codes in the tail group
    planes[:, 2 * (P // 64) + 1:] = 0  # bits past P are zero, as the packer leaves them
    planes[:, 2 * (P // 64)] &= (1 << (P % 64)) - 1
    planes[:, 2 * (P // 64) + 1] = 0
    rows = torch.tensor([19, 4, 3, 11, 0, 7, 8, 15, 2, 16, 9, 12, 5], dtype=torch.int32, device=dev)
    counts = torch.empty(P, dtype=torch.int32, device=dev)
    _native.sign_vote_count(planes, rows, len(rows), P, counts)
    w = planes.cpu().numpy().view(np.uint64)
    S = np.stack([osign.unpack_planes(w[r], P) for r in rows.tolist()])
    assert np.array_equal(counts.cpu().numpy(), osign.vote_counts(S))
    sign = torch.empty(P, device=dev)
    vp = torch.full((Wd,), 0x55, dtype=torch.int64, device=dev)
    _native.sign_vote(planes, rows, len(rows), P, sign, vote_planes=vp)
    s2 = torch.empty(P, device=dev)
    v2 = torch.zeros(Wd, dtype=torch.int64, device=dev)
    _native.sign_from_counts(counts, P, s2, v2)
    assert same_bits(sign.cpu().numpy(), s2.cpu().numpy())
    assert torch.equal(vp, v2)
    assert same_bits(sign.cpu().numpy(), osign.majority_vote(S))


def test_vote_signs_packed_1000_clients_resnet18_every_parameter():
    """The instance SignSGDServer and bench.py launch at config 3 (signs + packed
    vote, no counts: k_sign_vote<8, false, 4>) at full size, 1000 x ResNet-18:
    every parameter equal to counts -> sign of the count kernel (<8, true, 4>),
    and 4,096 sampled parameters equal to the oracle's vote."""
    from distributed_learning_simulator_amd import _native
    K, P = 1000, 11173962
    Pp = (P + 3) // 4 * 4
    W = _native.sign_words(Pp)
    g = torch.Generator(device=dev).manual_seed(1234)
    planes = torch.randint(-2**62, 2**62, (K, W), generator=g, device=dev)
    planes[:, 1::2] &= ~planes[:, 0::2]
    # ties: two clients' planes mirrored on a band of groups; NaN codes on a few
    planes[1, 2000:4000:2], planes[1, 2001:4001:2] = planes[0, 2001:4001:2], planes[0, 2000:4000:2]
    planes[17, 2 * 12345 + 1] |= planes[17, 2 * 12345]
    planes[:, 2 * (Pp // 64):] = 0  # past P: zero, as the packer leaves it
    sign = torch.empty(Pp, device=dev)
    vote = torch.full((W,), 0x55, dtype=torch.int64, device=dev)
    _native.sign_vote(planes, None, K, Pp, sign, vote_planes=vote)  # the timed launch
    counts = torch.empty(Pp, dtype=torch.int32, device=dev)
    _native.sign_vote_count(planes, None, K, Pp, counts)
    s2 = torch.empty(Pp, device=dev)
    v2 = torch.zeros(W, dtype=torch.int64, device=dev)
    _native.sign_from_counts(counts, Pp, s2, v2)
    assert torch.equal(sign.view(torch.int32), s2.view(torch.int32))
    assert torch.equal(vote, v2)
    idx = torch.randint(0, P, (4096,), generator=g, device=dev)
    idx[:4] = torch.tensor([64 * 1000 + 3, 64 * 12345 + 5, 64 * 12345 + 63, P - 1], device=dev)
    words = planes[:, (idx // 64) * 2].cpu().numpy().view(np.uint64)
    nwords = planes[:, (idx // 64) * 2 + 1].cpu().numpy().view(np.uint64)
    bit = (idx % 64).cpu().numpy().astype(np.uint64)
    pos = ((words >> bit) & np.uint64(1)).astype(np.float32)
    neg = ((nwords >> bit) & np.uint64(1)).astype(np.float32)
    S = pos - neg
    S[(pos == 1) & (neg == 1)] = np.nan  # the NaN code
    assert same_bits(sign[idx].cpu().numpy(), osign.majority_vote(S))


@pytest.mark.parametrize("P", [5_000_004, 14_000_000])
def test_vote_balanced_wave_ranges(P):
    """The large-model vote gives every wave a contiguous range of R groups so that
    the chip gets a whole number of waves per CU (R = ceil(groups / (4 x CUs)):
    G = ceil(R / 64) = 2 here at P = 5M and 4 at P = 14M, the last 64-group chunk
    of a range partial, ranges not 64-aligned).  Signs, packed vote and counts
    (with a row subset) against torch's sum-of-signs on the same ternary matrix."""
    from distributed_learning_simulator_amd import _native
    K = 13
    g = torch.Generator(device=dev).manual_seed(P % 1000)
    S = torch.randint(-1, 2, (K, P), generator=g, device=dev, dtype=torch.int8).float()
    Wd = _native.sign_words(P)
    planes = torch.zeros((K, Wd), dtype=torch.int64, device=dev)
    _native.sign_pack(S, P, planes)
    ref = torch.sign(S.sum(0))
    sign = torch.empty(P, device=dev)
    vote = torch.full((Wd,), 0x55, dtype=torch.int64, device=dev)
    _native.sign_vote(planes, None, K, P, sign, vote_planes=vote)
    assert torch.equal(sign, ref)
    c = torch.empty(P, dtype=torch.int32, device=dev)
    _native.sign_vote_count(planes, None, K, P, c)
    assert torch.equal(c, S.sum(0).int())
    v2 = torch.zeros(Wd, dtype=torch.int64, device=dev)
    _native.sign_from_counts(c, P, None, v2)
    assert torch.equal(vote, v2)
    rows = torch.tensor([12, 0, 5, 7, 3], dtype=torch.int32, device=dev)
    _native.sign_vote_count(planes, rows, len(rows), P, c)
    assert torch.equal(c, S[rows.long()].sum(0).int())


def test_vote_wide_layout_very_large_model():
    """past 64 x 4 vote groups per wave (P > ~16.7M parameters on 256
    CUs; here P = 70M, VGG-16-scale) the vote keeps the wide per-wave layout with
    a multiple m of the waves per CU, the smallest from ceil(r / 256) up for which
    a range (ceil(groups / waves) + 7 for its aligned start) fits 64 x 4 groups:
    5,120 waves of 4 groups per lane here on 256 CUs.  The signs and packed vote
    equal torch's vote computed from the same planes (bit unpacking on the GPU), on
    every parameter."""
    from distributed_learning_simulator_amd import _native
    K, P = 24, 70_000_000
    W = _native.sign_words(P)
    g = torch.Generator(device=dev).manual_seed(77)
    planes = torch.randint(-2**62, 2**62, (K, W), generator=g, device=dev)
    planes[:, 1::2] &= ~planes[:, 0::2]  # no NaN codes
    planes[:, 2 * ((P + 63) // 64):] = 0
    sign = torch.empty(P, device=dev)
    vote = torch.full((W,), 0x55, dtype=torch.int64, device=dev)
    _native.sign_vote(planes, None, K, P, sign, vote_planes=vote)
    pos, neg = planes[:, 0::2], planes[:, 1::2]  # [K, groups of 64]
    ng = (P + 63) // 64
    counts = torch.empty((ng, 64), dtype=torch.int32, device=dev)
    for j in range(64):
        bp = ((pos[:, :ng] >> j) & 1).sum(0, dtype=torch.int32)
        bn = ((neg[:, :ng] >> j) & 1).sum(0, dtype=torch.int32)
        counts[:, j] = bp - bn
    ref = torch.sign(counts.reshape(-1)[:P].float())
    assert torch.equal(sign.view(torch.int32), ref.view(torch.int32))
    v2 = torch.zeros(W, dtype=torch.int64, device=dev)
    s2 = torch.empty(P, device=dev)
    _native.sign_from_counts(counts.reshape(-1)[:P].contiguous(), P, s2, v2)
    assert torch.equal(vote, v2)


# ------------------------------------------------------- the vote's wave ranges
# launch_vote gives wave w of nwaves a contiguous range of vote groups (64 parameters
# each) and every lane G of them (csrc/sign_geometry.h): a range longer than 64 G
# groups leaves its tail unwritten.  Every size below comes from the geometry query on
# this device's CU count, so the cases sit on the same edges on any part; the
# outputs start as sentinels no vote can equal and carry a guard past P.
SENT_SIGN, SENT_VOTE, SENT_COUNT = 7.0, 0x5555555555555555, -2 ** 31 + 1
GUARD = 256
EDGE_K = 13
EDGE_ROWS = [12, 0, 2, 1, 5]  # 5 of the 13 rows, out of order: the tie's clients 0 and 1, the NaN's client 2


def device_cus():
    return torch.cuda.get_device_properties(dev).multi_processor_count


def parent_vote_groups_per_lane(vote_groups, cus):
    """G as launch_vote sized it before vote_geometry (narrow counters, 4 waves per CU,
    at most 4 groups per lane): 5 in bands of sizes, which ran the G = 4 kernel."""
    waves = 4 * cus
    r = (vote_groups + waves - 1) // waves + 7
    if r > 256:
        waves *= (r + 255) // 256
        r = (vote_groups + waves - 1) // waves + 7
    return ((r + 63) // 64, waves) if r > 64 else (1, (vote_groups + 63) // 64)


_edges = {}


def vote_edges():
    """Sizes (in 256-parameter tiles) on this device: the first and the last tile count
    of the first band in which the old formula asked for G = 5, the tile count in the
    band whose last range it made longest, and below the band the first tile count of
    every new (nwaves, G) the geometry query reports."""
    if _edges:
        return _edges
    from distributed_learning_simulator_amd import _native
    cus = device_cus()
    t = 1
    while parent_vote_groups_per_lane(4 * t, cus)[0] != 5:
        t += 1
        assert t < 2048 * cus, "no band"
    first = last = t
    while parent_vote_groups_per_lane(4 * (last + 1), cus)[0] == 5:
        last += 1

    def parent_tail(t):  # groups past the 256 the G = 4 kernel's last wave covered
        vg, nw = 4 * t, parent_vote_groups_per_lane(4 * t, cus)[1]
        return vg - (((nw - 1) * vg // nw) & ~7) - 256

    longest = max(range(first, last + 1), key=parent_tail)
    assert parent_tail(longest) >= 4
    _edges.update(band_first=first, band_last=last, band_longest=longest,
                  parent_tail=parent_tail(longest), parent_tail_first=parent_tail(first),
                  parent_tail_last=parent_tail(last))
    prev, steps = _native.sign_vote_geometry(256, EDGE_K, cus)[:2], []
    for t in range(2, first):
        cur = _native.sign_vote_geometry(256 * t, EDGE_K, cus)[:2]
        if cur != prev and (cur[1] > 1 or prev[1] > 1):  # G = 1: nwaves is ceil(groups / 64)
            steps.append((t, prev, cur))
        prev = cur
    # 1 -> 2, 2 -> 3, 3 -> 4 groups per lane, the multiplier's first step (more waves,
    # fewer groups per lane) and the next growth of G under it
    kinds = {"g1_2": lambda p, c: (p[1], c[1]) == (1, 2), "g2_3": lambda p, c: (p[1], c[1]) == (2, 3) and p[0] == c[0],
             "g3_4": lambda p, c: (p[1], c[1]) == (3, 4) and p[0] == c[0],
             "multiplier": lambda p, c: c[0] == 2 * p[0] and p[1] == 4 and c[1] < 4}
    for name, want in kinds.items():
        _edges[name] = next(t for t, p, c in steps if want(p, c))
    _edges["g_grows_after_multiplier"] = next(t for t, p, c in steps if t > _edges["multiplier"] and c[1] == p[1] + 1)
    assert len(steps) == 5, steps  # nothing else changes below the band
    return _edges


def edge_case_inputs(P, K, pitch, seed):
    """A ternary matrix S [K, P] on the GPU and its planes [K, pitch], with a tie and a
    NaN code in the last live group, which lies in the last wave's last 64-group chunk:
    the last parameter gets +1 from client 0, -1 from client 1 and 0 from the others
    (one vote each way: a tie that is no sum of zeros); client 2 gets a NaN code (both
    planes, by a plane edit) wherever it is positive in that group, at least on the
    group's first parameter.  Returns S, planes, the NaN client and group."""
    from distributed_learning_simulator_amd import _native
    g = torch.Generator(device=dev).manual_seed(seed)
    S = torch.randint(-1, 2, (K, P), generator=g, device=dev, dtype=torch.int8).float()
    ng = (P + 63) // 64
    S[:, P - 1] = 0
    S[0, P - 1], S[1, P - 1] = 1, -1
    S[2, 64 * (ng - 1)] = 1
    planes = torch.full((K, pitch), SENT_VOTE, dtype=torch.int64, device=dev)
    _native.sign_pack(S, P, planes)
    planes[2, 2 * (ng - 1) + 1] |= planes[2, 2 * (ng - 1)]
    # where they sit: in the last chunk of the last wave's range
    nw, G, _ = _native.sign_vote_geometry(P, K)
    wlo, whi = _native.sign_vote_wave_ranges(P, K, first_wave=nw - 1, count=1)
    chunk = int(wlo[0]) + 64 * ((int(whi[0] - wlo[0]) + 63) // 64 - 1)
    assert chunk <= ng - 1 < int(whi[0]) == _native.sign_words(P) // 2 and whi[0] - wlo[0] <= 64 * G
    return S, planes, 2, ng - 1


def edge_reference(S, rows, nan_client, nan_group):
    """(counts, signs) of the vote over S's rows (all, or the list ``rows``) by torch's
    sum of signs; a NaN code counts once each way and marks the parameter."""
    from distributed_learning_simulator_amd import _native
    P = S.shape[1]
    total = (S if rows is None else S[rows]).sum(0)
    times = 1 if rows is None else rows.count(nan_client)
    nan = torch.zeros(P, dtype=torch.bool, device=dev)
    sl = slice(64 * nan_group, min(64 * nan_group + 64, P))
    if times:
        nan[sl] = S[nan_client, sl] > 0
        total[sl] -= times * nan[sl].float()
        assert bool(nan.any())
    counts = total.int() + nan.int() * _native.SIGN_NAN_MARK
    return counts, torch.where(nan, torch.zeros((), device=dev), torch.sign(total))


def check_edge_vote(planes, rows, K, P, ref_counts, ref_sign):
    """dls_sign_vote_count (<CB, true, G>), the fused dls_sign_vote with counts and the
    server's form without (<CB, false, G>): every parameter bit for bit, no sentinel left
    in [0, P), no write into the guards."""
    from distributed_learning_simulator_amd import _native
    W = _native.sign_words(P)
    ref_vote = gpu_pack_reference(ref_sign, W)
    rows_t = None if rows is None else torch.tensor(rows, dtype=torch.int32, device=dev)

    def outputs():
        return (torch.full((P + GUARD,), SENT_COUNT, dtype=torch.int32, device=dev),
                torch.full((P + GUARD,), SENT_SIGN, device=dev),
                torch.full((W + GUARD,), SENT_VOTE, dtype=torch.int64, device=dev))

    def check(counts=None, sign=None, vote=None):
        if counts is not None:
            assert int((counts[:P] == SENT_COUNT).sum()) == 0, "counts never written"
            assert torch.equal(counts[:P], ref_counts)
            assert bool((counts[P:] == SENT_COUNT).all()), "counts guard"
        if sign is not None:
            assert int((sign[:P] == SENT_SIGN).sum()) == 0, "signs never written"
            assert torch.equal(sign[:P].view(torch.int32), ref_sign.view(torch.int32))
            assert bool((sign[P:] == SENT_SIGN).all()), "sign guard"
        if vote is not None:
            assert int((vote[:W] == SENT_VOTE).sum()) == 0, "packed vote never written"
            assert torch.equal(vote[:W], ref_vote)
            assert bool((vote[W:] == SENT_VOTE).all()), "packed vote guard"

    c, s, v = outputs()
    _native.sign_vote_count(planes, rows_t, K, P, c[:P])
    check(counts=c)
    c, s, v = outputs()
    _native.sign_vote(planes, rows_t, K, P, s[:P], counts=c[:P], vote_planes=v[:W])
    check(c, s, v)
    c, s, v = outputs()
    _native.sign_vote(planes, rows_t, K, P, s[:P], vote_planes=v[:W])
    check(None, s, v)
    assert bool((c == SENT_COUNT).all())
    return s[:P], v[:W]


def run_edge_case(P, pitch=None):
    from distributed_learning_simulator_amd import _native
    S, planes, nan_client, nan_group = edge_case_inputs(
        P, EDGE_K, _native.sign_words(P) if pitch is None else pitch, P % 9973)
    out = None
    for rows in (None, EDGE_ROWS):
        K = EDGE_K if rows is None else len(rows)
        ref_counts, ref_sign = edge_reference(S, rows, nan_client, nan_group)
        assert int(ref_counts[P - 1]) == 0 and float(ref_sign[P - 1]) == 0  # the tie
        got = check_edge_vote(planes, rows, K, P, ref_counts, ref_sign)
        out = out or got
    return out


@pytest.mark.parametrize("where", ["first", "last", "ragged"])
def test_vote_wave_ranges_in_the_old_g5_band(where):
    """The sizes at which the host used to ask for 5 groups per lane and launch 4 (about
    32.6M-33.1M parameters on 256 CUs): the band's first and last size, and the one
    whose last range was longest, cut to P % 256 = 68 so that the last wave's last
    chunk holds live groups, padding groups and groups past the end.  The old launch
    dropped groups only where its last wave's range, not just the host's bound on it,
    passed 256 groups: at the "ragged" size (4 groups, asserted; the tie and the NaN
    code sit in them), but not at the band's first and last size on 64 to 304 CUs,
    where its last range is 252 and 256 groups (these two pin the fixed geometry at
    the band's edges; they passed before)."""
    from distributed_learning_simulator_amd import _native
    e = vote_edges()
    P = 256 * {"first": e["band_first"], "last": e["band_last"], "ragged": e["band_longest"]}[where]
    if e["band_first"] * 256 == 32_637_184:  # 256 CUs: what the docstring says of them
        assert (e["parent_tail_first"], e["parent_tail_last"]) == (-4, 0)
    if where == "ragged":
        P -= 188  # 2 of the last tile's 4 groups are live, the last one 4 parameters long
        assert e["parent_tail"] >= 4 and (P + 63) // 64 == _native.sign_words(P) // 2 - 2
    nw, G, wpb = _native.sign_vote_geometry(P, EDGE_K)
    assert 2 <= G <= 4 and wpb == 4 and nw % (4 * device_cus()) == 0
    run_edge_case(P)


@pytest.mark.parametrize("side", ["below", "at"])
@pytest.mark.parametrize("edge", ["g1_2", "g2_3", "g3_4", "multiplier", "g_grows_after_multiplier"])
def test_vote_wave_ranges_at_every_geometry_step(edge, side):
    """Both sides of every change of (nwaves, G) below the band: the first size of
    2, 3 and 4 groups per lane, of the doubled wave count, and of the next G under
    it, each with the size one 256-parameter tile below."""
    from distributed_learning_simulator_amd import _native
    t = vote_edges()[edge] - (side == "below")
    below, at = (_native.sign_vote_geometry(256 * u, EDGE_K)[:2] for u in (vote_edges()[edge] - 1, vote_edges()[edge]))
    assert below != at
    run_edge_case(256 * t)


def test_vote_wave_ranges_row_pitch():
    """One band size with the rows at the minimal pitch sign_words(P) and at the
    server's 128-byte pitch sign_row_pitch(P): the same signs and packed vote."""
    from distributed_learning_simulator_amd import _native
    P = 256 * vote_edges()["band_longest"] - 188 - 256  # sign_words(P) % 16 = 8: the pitches differ
    if _native.sign_words(P) % 16 == 0:
        P -= 256
    assert _native.sign_row_pitch(P) == _native.sign_words(P) + 8
    assert parent_vote_groups_per_lane(_native.sign_words(P) // 2, device_cus())[0] == 5
    s1, v1 = run_edge_case(P)
    s2, v2 = run_edge_case(P, pitch=_native.sign_row_pitch(P))
    assert torch.equal(s1.view(torch.int32), s2.view(torch.int32)) and torch.equal(v1, v2)


def test_vote_wave_ranges_wide_counters():
    """CB = 16 (K = 32,761 client rows): one group per lane, one wave per block, and
    more blocks than the wide layout launches (4 waves per CU in blocks of 4), the
    last one partial.  32,761 rows are drawn from 48 base rows, so the sums are 48
    weighted bit counts; without ``rows`` the matrix is written out."""
    from distributed_learning_simulator_amd import _native
    K, B = 32_761, 48
    cus = device_cus()
    # cus + 3 one-wave blocks is the smallest grid past the wide layout's cus blocks:
    # P = 1,058,628 on 256 CUs, and the matrix written out below is K x sign_words(P)
    # words = 8.7 GB there (a larger P would only add blocks like the middle ones)
    P = 64 * (64 * (cus + 2) + 24) - 188
    nw, G, wpb = _native.sign_vote_geometry(P, K)
    assert (G, wpb) == (1, 1) and nw == cus + 3 and _native.sign_vote_geometry(P, EDGE_K)[1] == 1
    W, ng = _native.sign_words(P), (P + 63) // 64
    base = one_sided_planes(B, W, 5, 7)
    base[:, 2 * ng:] = 0  # past P: zero, as the packer leaves it
    base[:, 2 * (ng - 1):2 * ng] &= (1 << (P % 64)) - 1
    base[9, 2 * (ng - 2) + 1] |= base[9, 2 * (ng - 2)]  # NaN codes in the last chunk
    gen = torch.Generator(device=dev).manual_seed(3)
    idx = torch.randint(0, B, (K,), generator=gen, device=dev)
    idx[:B] = torch.arange(B, device=dev)
    mult = torch.bincount(idx, minlength=B).int()
    pos, neg = base[:, 0:2 * ng:2], base[:, 1:2 * ng:2]
    cp = torch.empty((ng, 64), dtype=torch.int32, device=dev)
    cn, nan = torch.empty_like(cp), torch.empty((ng, 64), dtype=torch.bool, device=dev)
    for j in range(64):
        cp[:, j] = (((pos >> j) & 1).int() * mult[:, None]).sum(0, dtype=torch.int32)
        cn[:, j] = (((neg >> j) & 1).int() * mult[:, None]).sum(0, dtype=torch.int32)
        nan[:, j] = ((((pos & neg) >> j) & 1) != 0).any(0)
    cp, cn, nan = cp.reshape(-1)[:P], cn.reshape(-1)[:P], nan.reshape(-1)[:P]
    assert int((cp - cn)[:64].min()) == K and int((cp - cn)[64:128].max()) == -K and bool(nan[-68:].any())
    ref_counts = cp - cn + nan.int() * _native.SIGN_NAN_MARK
    ref_sign = torch.where(nan, torch.zeros((), device=dev), torch.sign((cp - cn).float()))
    check_edge_vote(base, idx.tolist(), K, P, ref_counts, ref_sign)
    check_edge_vote(base[idx], None, K, P, ref_counts, ref_sign)


def test_sign_server_votes_every_parameter_at_a_band_size(monkeypatch):
    """SignSGDServer end to end with 8 workers at a band size: the path that hands the
    kernel uninitialised outputs.  While the last client arrives and the vote runs,
    torch.empty returns sentinel-filled tensors (its contents are arbitrary by
    contract), so a parameter the kernel skips keeps a value no vote can have.  The
    returned vote equals the oracle's majority vote on every parameter."""
    from distributed_learning_simulator_amd.servers.sign_sgd_server import SignSGDServer
    from distributed_learning_simulator_amd import _native
    K = 8
    P = 256 * vote_edges()["band_longest"]
    n0 = P - 64 * 1000 - 61  # two tensors; the second starts on the next multiple of 64
    shapes = [(n0,), (1000, 64)]
    gen = torch.Generator(device=dev).manual_seed(8)
    S = torch.randint(-1, 2, (K, P), generator=gen, device=dev, dtype=torch.int8).float()
    S[:, n0:n0 + 61] = 0  # the layout's padding between the tensors
    S[2:, P - 1] = 0
    S[0, P - 1], S[1, P - 1] = 1, -1
    server = SignSGDServer(tester=None, worker_number=K, synchronous=True, device=dev)
    tasks = [[S[k, :n0].clone(), S[k, n0 + 61:].reshape(1000, 64).clone()] for k in range(K)]
    for k in range(K - 1):
        server.worker_data_queue.add_task(tasks[k])
    real_empty, poisoned = torch.empty, []

    def empty(*size, **kw):
        t = real_empty(*size, **kw)
        poisoned.append((tuple(t.shape), t.dtype))
        return t.fill_(SENT_VOTE if t.dtype == torch.int64 else SENT_SIGN)

    with monkeypatch.context() as m:
        m.setattr(torch, "empty", empty)
        server.worker_data_queue.add_task(tasks[K - 1])
    assert ((P,), torch.float32) in poisoned and ((_native.sign_words(P),), torch.int64) in poisoned
    res = server.worker_data_queue.get_result(consumer=0)
    assert server._layout.P == P and [tuple(t.shape) for t in res] == shapes
    got = torch.cat([res[0], torch.zeros(61, device=dev), res[1].reshape(-1)]).cpu().numpy()
    ref = osign.majority_vote(S.cpu().numpy())
    assert same_bits(got, ref)
    assert np.array_equal(res.vote_planes.cpu().numpy().view(np.uint64), osign.pack_planes(ref))
