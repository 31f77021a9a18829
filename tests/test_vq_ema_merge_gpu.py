"""The split EMA codebook update on the GPU (vqvae_vq_ema_stats_f32 / vqvae_vq_ema_apply_f32, functional.vq_ema_stats / vq_ema_apply,
the sync / accumulate options of the EMA quantizers) against vq_ema_update's bits at R = 1 and the fp64 restatement of
tests/vq_ema_merge_ref.py at R = 3 and R = 8.

Tolerances: at R = 1 everything is bit-equal to vq_ema_update.  Counts and candidates of a record are exact; a per-code sum is within
c_k 2^-53 sum_i |z_i[c]| of the reference (the recursive-summation bound, which holds for any order).  At R > 1 ema_cluster_size and
ema_w are within 1 ulp of the fp64 restatement rounded to fp32 and the codebook within 2 ulp (tests/test_vq_ema_gpu.py's own
tolerances: any fixed order of fp64 sums differs from another by ~1e-13 relative, far inside half an fp32 ulp except at a rounding
boundary, where it costs the one ulp allowed); restarted rows are bit-exact."""
import copy
import math

import numpy as np
import pytest
import torch

from tests import vq_ema_merge_ref as M
from tests import vq_ema_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DECAY, EPS, THR = 0.9, 1e-5, 2.0

SHAPES = [(3, 5, 3, 3, 7), (2, 64, 8, 8, 512), (13, 5, 10, 20, 3), (1, 256, 4, 4, 16), (1, 1, 1, 1, 1)]    # (B, D, H, W, K)
IDS = ["ragged", "mostly_empty", "skewed", "wide", "one"]
SKEW = SHAPES[2]
CUTS = [(SKEW, (1, 5, 7)), (SKEW, (1, 1, 1, 1, 2, 2, 2, 3)), (SHAPES[1], (1, 1))]
CUT_IDS = ["skewed_3", "skewed_8", "mostly_empty_2"]

_CASES = {}


def _thr(shape):
    """a threshold that leaves some codes dead and some alive: N_k = 0.9 N_k + 0.1 c_k with N_k drawn from [0, 4).  The skewed shape's
    codes 1 and 2 own ~200 rows each (N_k ~ 20 .. 24) and code 0 over 2100 (N_k > 210)"""
    return 100.0 if shape == SKEW else THR


def _case(shape):
    """-> dict of CPU tensors, drawn once per shape: z (B,D,H,W), idx (N,), state (cs, w), uniforms u (rows) and v (shards)"""
    if shape not in _CASES:
        B, D, H, W, K = shape
        N = B * H * W
        g = torch.Generator().manual_seed(1000 + N + K)
        z = torch.randn(B, D, H, W, generator=g)
        idx = torch.randint(0, K, (N,), generator=g)
        if shape == SKEW:
            # at least 2100 of the 2600 rows on code 0 (five 512-row units: segsum_key_sum's four interleaved sums wrap), and the
            # first image -- the first shard of both cuts -- without code 2
            idx[torch.randperm(N, generator=g)[:2200]] = 0
            first = idx[:H * W]
            first[first == 2] = 1
            assert int((idx == 0).sum()) >= 2100 and not (idx[:H * W] == 2).any() and (idx == 2).any()
        _CASES[shape] = dict(z=z, idx=idx, cs=torch.rand(K, generator=g) * 4, w=torch.randn(K, D, generator=g),
                             u=torch.rand(K, generator=g), v=torch.rand(K, generator=g))
    return _CASES[shape]


def _rows(z):
    return z.permute(0, 2, 3, 1).reshape(-1, z.shape[1])


def _lay(z, rowmajor):
    return (z.permute(0, 2, 3, 1) if rowmajor else z).contiguous().to(DEV)


def _bits(t):
    t = t.detach().cpu().contiguous().numpy()
    return t.view(np.uint64 if t.dtype == np.float64 else np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _ulps(got, ref64):
    """|got - round32(ref)| in units of fp32 spacing at round32(ref)"""
    ref = ref64.float().cpu().numpy()
    got = got.detach().float().cpu().numpy()
    sp = np.spacing(np.maximum(np.abs(ref), np.float32(np.finfo(np.float32).tiny))).astype(np.float64)
    return np.abs(got.astype(np.float64) - ref.astype(np.float64)) / sp


def _state(c):
    cs, w = c["cs"].to(DEV).clone(), c["w"].to(DEV).clone()
    return cs, w, torch.full_like(w, 7.0)


def _shards(shape, sizes):
    """[(z_s (b,D,H,W), idx_s)] cut along B"""
    c = _case(shape)
    HW = shape[2] * shape[3]
    return [(c["z"][lo:hi], c["idx"][lo * HW:hi * HW]) for lo, hi in M.cut(shape[0], sizes)]


def _gpu_stats(shards, K, u, rowmajor=False):
    from vqvae_amd import functional as F
    return torch.stack([F.vq_ema_stats(_lay(z, rowmajor), i.to(DEV), K, row_uniforms=None if u is None else u.to(DEV), rowmajor=rowmajor)
                        for z, i in shards])


# ---- 1. R = 1: the bits of vq_ema_update ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
@pytest.mark.parametrize("rowmajor", [False, True])
@pytest.mark.parametrize("restart", [False, True])
def test_one_shard_has_the_bits_of_the_one_shot_update(shape, rowmajor, restart):
    from vqvae_amd import functional as F
    c, K = _case(shape), shape[4]
    z, idx = _lay(c["z"], rowmajor), c["idx"].to(DEV)
    u = c["u"].to(DEV) if restart else None
    cs1, w1, cb1 = _state(c)
    thr = _thr(shape)
    F.vq_ema_update(z, idx, cs1, w1, cb1, DECAY, EPS, threshold=thr if restart else None, uniforms=u, rowmajor=rowmajor)
    st = F.vq_ema_stats(z, idx, K, row_uniforms=u, rowmajor=rowmajor)
    assert st.shape == (K, (2 if restart else 1) * shape[1] + 1) and st.dtype == torch.float64
    for stats in (st[None], [st]):                                                    # a (R, K, C) tensor, or a list of records
        cs2, w2, cb2 = _state(c)
        out = F.vq_ema_apply(stats, cs2, w2, cb2, DECAY, EPS, threshold=thr if restart else None,
                             shard_uniforms=c["v"].to(DEV) if restart else None)
        torch.cuda.synchronize()
        assert out is cb2
        assert _same(cs1, cs2) and _same(w1, w2) and _same(cb1, cb2)
    if restart and K > 1:
        assert (cs1 < thr).any() and (cs1 >= thr).any()                               # both branches ran


# ---- 2. the record ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_the_record(shape):
    c, (B, D, H, W, K) = _case(shape), shape
    rows, idx = _rows(c["z"]), c["idx"]
    ref = M.stats(rows, idx, K, c["u"])
    got = {rm: _gpu_stats([(c["z"], idx)], K, c["u"], rm)[0] for rm in (False, True)}
    torch.cuda.synchronize()
    assert _same(got[False], got[True])                                               # the same bits in both layouts
    plain = _gpu_stats([(c["z"], idx)], K, None)[0]
    assert _same(plain, got[False][:, :D + 1])                                        # and the candidates change nothing else
    g = got[False].cpu()
    assert torch.equal(g[:, 0], ref[:, 0])                                            # counts exact
    assert _same(g[:, D + 1:], ref[:, D + 1:])                                        # candidates bit-exact
    # sums: |s - ref| <= c_k 2^-53 sum_i |z_i[c]| against the restatement, and against the exactly rounded sum (math.fsum), for which
    # the bound is the textbook one: (c_k - 1) u for the recursive sum in any order plus u / 2 for the reference's one rounding
    absum = torch.zeros(K, D, dtype=torch.float64).index_add_(0, idx, rows.double().abs())
    bound = ref[:, :1] * 2.0 ** -53 * absum
    exact = torch.zeros(K, D, dtype=torch.float64)
    for k in range(K):
        mine = rows[idx == k].double()
        if mine.shape[0]:
            exact[k] = torch.tensor([math.fsum(col) for col in mine.t().tolist()], dtype=torch.float64)
    for name, r in (("restatement", ref[:, 1:D + 1]), ("exact", exact)):
        err = (g[:, 1:D + 1] - r).abs()
        print(f"{shape} sums vs {name}: max err {float(err.max()):.3e}, max err / bound "
              f"{float((err / bound.clamp_min(1e-300)).max()):.3f}")
        assert bool((err <= bound).all()), name


# ---- 3. R = 3 and R = 8 against the restatement on the concatenated batch ---------------------------------------------------------------

@pytest.mark.parametrize("shape,sizes", CUTS, ids=CUT_IDS)
@pytest.mark.parametrize("rowmajor", [False, True])
def test_merged_shards_against_the_restatement(shape, sizes, rowmajor):
    from vqvae_amd import functional as F
    c, (B, D, H, W, K) = _case(shape), shape
    shards = _shards(shape, sizes)
    thr = _thr(shape)
    if shape == SKEW:
        assert not (shards[0][1] == 2).any()                                          # one shard lacks code 2
    st = _gpu_stats(shards, K, c["u"], rowmajor)
    assert st.shape == (len(sizes), K, 2 * D + 1)
    whole = R.ema_update(_rows(c["z"]), c["idx"], c["cs"], c["w"], DECAY, EPS)            # the concatenated batch, at once
    # without restart
    cs, w, cb = _state(c)
    F.vq_ema_apply(st[:, :, :D + 1], cs, w, cb, DECAY, EPS)
    torch.cuda.synchronize()
    print(f"{shape} R={len(sizes)}: ulps N {_ulps(cs, whole['N']).max():.2f} m {_ulps(w, whole['m']).max():.2f} e {_ulps(cb, whole['e']).max():.2f}")
    assert _ulps(cs, whole["N"]).max() <= 1 and _ulps(w, whole["m"]).max() <= 1 and _ulps(cb, whole["e"]).max() <= 2
    # with restart: the rows of the shards the uniforms pick, bit for bit; N and m stay as updated
    ref = M.apply([M.stats(_rows(z), i, K, c["u"]) for z, i in shards], c["cs"], c["w"], DECAY, EPS, thr, c["v"])
    dead = ref["dead"]
    assert dead.any() and (~dead).any()
    cs2, w2, cb2 = _state(c)
    F.vq_ema_apply(st, cs2, w2, cb2, DECAY, EPS, threshold=thr, shard_uniforms=c["v"].to(DEV))
    torch.cuda.synchronize()
    assert _same(cs2, cs) and _same(w2, w)
    assert _same(cb2.cpu()[dead], ref["e"][dead].float())
    assert _same(cb2.cpu()[~dead], cb.cpu()[~dead]) and _ulps(cb2.cpu()[~dead], whole["e"][~dead]).max() <= 2
    bounds = M.cut(B, sizes)
    for k in torch.nonzero(dead).flatten().tolist():                                  # ... and they come from the shard v names
        j = int(ref["shard"][k])
        zs = _rows(shards[j][0])
        assert j == min(int(math.floor(float(c["v"][k].double()) * len(sizes))), len(sizes) - 1)
        assert torch.equal(cb2.cpu()[k], zs[int(M.pick(c["u"][k:k + 1], zs.shape[0]))]), (k, j, bounds[j])
    # a NaN in the candidate a dead code takes stays in that code's row
    k = int(torch.nonzero(dead).flatten()[0])
    bad = st.clone()
    bad[int(ref["shard"][k]), k, D + 1 + (D - 1)] = float("nan")
    cs3, w3, cb3 = _state(c)
    F.vq_ema_apply(bad, cs3, w3, cb3, DECAY, EPS, threshold=thr, shard_uniforms=c["v"].to(DEV))
    torch.cuda.synchronize()
    assert _same(cs3, cs) and _same(w3, w)
    got = cb3.cpu()
    assert torch.isnan(got[k, D - 1]) and int(torch.isnan(got).sum()) == 1
    keep = torch.ones(K, dtype=torch.bool)
    keep[k] = False
    assert _same(got[keep], cb2.cpu()[keep]) and _same(got[k, :D - 1], cb2.cpu()[k, :D - 1])


# ---- 4. determinism, graph replay, errors -------------------------------------------------------------------------------------------------

def _chain(z, idx, u, v, cs, w, cb, pend, ws_s, ws_a, rowmajor):
    from vqvae_amd import functional as F
    K = cs.shape[0]
    for r in range(pend.shape[0]):
        F.vq_ema_stats(z, idx, K, row_uniforms=u, rowmajor=rowmajor, workspace=ws_s, out=pend[r])
    F.vq_ema_apply(pend, cs, w, cb, DECAY, EPS, threshold=THR, shard_uniforms=v, workspace=ws_a)


@pytest.mark.parametrize("shape", [SHAPES[0], SHAPES[2]], ids=[IDS[0], IDS[2]])
@pytest.mark.parametrize("rowmajor", [False, True])
def test_two_runs_and_a_graph_replay_have_the_same_bits(shape, rowmajor):
    from vqvae_amd import functional as F
    c, (B, D, H, W, K) = _case(shape), shape
    real = [_lay(c["z"], rowmajor), c["idx"].to(DEV), c["u"].to(DEV), c["v"].to(DEV)]
    ws_s, ws_a = F.vq_ema_stats_workspace(B * H * W, K, D, DEV), F.vq_ema_apply_workspace(2, K, D, DEV)
    runs = []
    for _ in range(2):
        cs, w, cb = _state(c)
        pend = torch.full((2, K, 2 * D + 1), 7.0, dtype=torch.float64, device=DEV)
        _chain(*real, cs, w, cb, pend, ws_s, ws_a, rowmajor)
        torch.cuda.synchronize()
        runs.append((cs, w, cb, pend))
        ws_s.fill_(7)
        ws_a.fill_(7)
    for a, b in zip(*runs):
        assert _same(a, b)
    # the chain captured on other values, replayed on these
    static = [torch.zeros_like(t) for t in real]
    cs, w, cb = _state(c)
    pend = torch.full((2, K, 2 * D + 1), 7.0, dtype=torch.float64, device=DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _chain(*static, cs, w, cb, pend, ws_s, ws_a, rowmajor)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _chain(*static, cs, w, cb, pend, ws_s, ws_a, rowmajor)
    for st, r in zip(static, real):
        st.copy_(r)
    for i in range(2):
        cs.copy_(c["cs"])
        w.copy_(c["w"])
        cb.fill_(7)
        pend.fill_(7)
        ws_s.fill_(7)
        ws_a.fill_(7)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(runs[0], (cs, w, cb, pend)):
            assert _same(a, b), i


def test_argument_errors_come_back_without_a_launch():
    from vqvae_amd import _lib, functional as F
    L = _lib.load()
    c, (B, D, H, W, K) = _case(SHAPES[0]), SHAPES[0]
    z, idx, u = _lay(c["z"], False), c["idx"].to(DEV), c["u"].to(DEV)
    cs, w, cb = _state(c)
    st = torch.full((2, K, 2 * D + 1), 7.0, dtype=torch.float64, device=DEV)
    odd = torch.full((K * (D + 1) * 8 + 8,), 7, dtype=torch.uint8, device=DEV)
    ws = torch.full((1 << 20,), 7, dtype=torch.uint8, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    S = lambda z_=p(z), idx_=p(idx), D_=D, K_=K, flags=0, out=p(st), ws_=p(ws), n=1 << 20: L.vqvae_vq_ema_stats_f32(
        z_, idx_, B, D_, H, W, K_, p(u), flags, out, ws_, n, stream)
    A = lambda st_=p(st), R_=2, K_=K, D_=D, C=2 * D + 1, v=p(u), cs_=p(cs), ws_=p(ws), n=1 << 20: L.vqvae_vq_ema_apply_f32(
        st_, R_, K_, D_, C, DECAY, EPS, THR, v, cs_, p(w), p(cb), ws_, n, stream)
    assert S(z_=None) == -1 and S(idx_=None) == -1 and S(out=None) == -1 and A(st_=None) == -1 and A(cs_=None) == -1
    assert A(R_=0) == -3 and A(R_=1025) == -3 and A(D_=257, C=515) == -3 and A(K_=16385) == -3
    assert S(D_=257) == -3 and S(K_=16385) == -3 and S(flags=4) == -3 and S(flags=1 | 2) == -3
    assert A(C=D + 1) == -3                                                            # shard_uniforms without candidates
    assert S(out=p(odd) + 4) == -3 and A(st_=p(st) + 4) == -3                           # not 8-byte aligned
    assert S(ws_=None) == -4 and S(n=8) == -4 and A(ws_=None) == -4 and A(n=8) == -4
    assert F.vq_ema_stats_workspace(B * H * W, K, D, DEV).numel() > 0
    with pytest.raises(_lib.VqvaeHipError):
        F.vq_ema_apply_workspace(1025, K, D, DEV)
    with pytest.raises(ValueError):
        F.vq_ema_apply(st, cs, w, cb, DECAY, EPS, threshold=THR)                       # a threshold without uniforms
    with pytest.raises(ValueError):
        F.vq_ema_apply(st[:, :, :D + 1], cs, w, cb, DECAY, EPS, threshold=THR, shard_uniforms=u)
    with pytest.raises(ValueError):
        F.vq_ema_stats(z, idx[:-1], K)
    torch.cuda.synchronize()
    for t in (st, ws):                                                               # nothing was launched: every byte as it was
        assert bool((t == 7).all())
    assert _same(cs, c["cs"]) and _same(w, c["w"]) and bool((cb == 7).all())


# ---- 5. the modules -------------------------------------------------------------------------------------------------------------------------

K_, D_ = 24, 6


def _batches(n, seed=5, C=D_):
    g = torch.Generator().manual_seed(seed)
    return [(torch.randn(2 + i, C, 3, 3, generator=g) * 0.05).to(DEV) for i in range(n)]


def _vq(restart=None, seed=0, **kw):
    from vqvae_amd.modules import VectorQuantizerEMA
    torch.manual_seed(seed)
    gen = torch.Generator(device=DEV).manual_seed(77) if restart is not None else None
    m = VectorQuantizerEMA(K_, D_, 0.25, decay=DECAY, restart_threshold=restart, generator=gen, **kw).to(DEV).train()
    return m


def _snapshot(m):
    return m.ema_cluster_size.clone(), m.ema_w.clone(), m.embedding.weight.detach().clone()


def _hand(state, records, u, restart):
    """one apply of the records (a list of (K, C)) on a copy of the state -> (cs, w, cb)"""
    from vqvae_amd import functional as F
    cs, w, cb = state[0].clone(), state[1].clone(), torch.empty_like(state[2])
    F.vq_ema_apply(records, cs, w, cb, DECAY, 1e-5, threshold=restart, shard_uniforms=None if restart is None else u[0])
    return cs, w, cb


@pytest.mark.parametrize("restart", [None, 0.5])
def test_accumulate_applies_once_per_cycle_and_equals_the_hand_chain(restart):
    from vqvae_amd import functional as F
    m = _vq(restart, accumulate=3)
    w = m.embedding.weight
    before, v0 = _snapshot(m), w._version
    u = torch.rand(2, K_, device=DEV, generator=torch.Generator(device=DEV).manual_seed(77)) if restart is not None else None
    records = []
    with torch.no_grad():
        for i, z in enumerate(_batches(3)):
            idx = m(z)[4]
            records.append(F.vq_ema_stats(z, idx, K_, row_uniforms=None if u is None else u[1]))
            if i < 2:
                assert m.pending_ema_updates == i + 1 and w._version == v0
                assert all(_same(a, b) for a, b in zip(before, _snapshot(m)))
    assert m.pending_ema_updates == 0 and w._version == v0 + 1
    want = _hand(before, records, u, restart)
    assert all(_same(a, b) for a, b in zip(want, _snapshot(m)))
    assert not _same(before[2], w)
    if restart is not None:
        assert (want[0] < restart).any()
    # the next cycle starts afresh, and flush_ema_ applies two records as R = 2
    mid = _snapshot(m)
    records = []
    if restart is not None:
        u = torch.rand(2, K_, device=DEV, generator=torch.Generator(device=DEV).set_state(m.generator.get_state()))
    with torch.no_grad():
        for z in _batches(2, seed=6):
            records.append(F.vq_ema_stats(z, m(z)[4], K_, row_uniforms=None if u is None else u[1]))
    assert m.pending_ema_updates == 2 and all(_same(a, b) for a, b in zip(mid, _snapshot(m)))
    m.flush_ema_()
    assert m.pending_ema_updates == 0 and w._version == v0 + 2
    assert all(_same(a, b) for a, b in zip(_hand(mid, records, u, restart), _snapshot(m)))
    m.flush_ema_()                                                                     # nothing pending: nothing happens
    assert w._version == v0 + 2


def test_factorized_cosine_and_grouped_equal_their_hand_chains():
    from vqvae_amd import functional as F
    from vqvae_amd.modules import FactorizedVectorQuantizerEMA, GroupedVectorQuantizerEMA
    torch.manual_seed(1)
    m = FactorizedVectorQuantizerEMA(K_, 12, D_, 0.25, decay=DECAY, cosine_sim=True, accumulate=2).to(DEV).train()
    before, records = _snapshot(m), []
    with torch.no_grad():
        for z in _batches(2, C=12):
            idx = m.quantize(z)[3]
            y = F.linear_rows(z, m.project_in.weight.detach(), m.project_in.bias.detach())
            records.append(F.vq_ema_stats(F.l2norm_rows(y)[0], idx, K_))              # from y^, where today's update reads
    assert m.pending_ema_updates == 0 and all(_same(a, b) for a, b in zip(_hand(before, records, None, None), _snapshot(m)))
    assert not _same(before[2], m.embedding.weight)

    torch.manual_seed(2)
    G = 2
    m = GroupedVectorQuantizerEMA(G, K_, 12, 0.25, decay=DECAY, accumulate=2).to(DEV).train()
    cs0, w0 = m.ema_cluster_size.clone(), m.ema_w.clone()
    books0 = [b.detach().clone() for b in m.codebooks()]
    versions = [b._version for b in m.codebooks()]
    records = [[] for _ in range(G)]
    with torch.no_grad():
        for i, z in enumerate(_batches(2, C=12)):
            slabs, idx = m._slabs(z, False), m.quantize(z)[3]
            for g in range(G):
                records[g].append(F.vq_ema_stats(slabs[g], idx[g], K_))
            if i == 0:
                assert m.pending_ema_updates == 1 and [b._version for b in m.codebooks()] == versions
    assert m.pending_ema_updates == 0 and [b._version for b in m.codebooks()] == [v + 1 for v in versions]
    for g in range(G):
        want = _hand((cs0[g], w0[g], books0[g]), records[g], None, None)
        assert _same(want[0], m.ema_cluster_size[g]) and _same(want[1], m.ema_w[g]) and _same(want[2], m.codebooks()[g])
        assert not _same(books0[g], m.codebooks()[g])


def test_sync_without_a_group_is_accumulate_and_injected_ranks_are_applied_rank_major():
    from vqvae_amd import functional as F
    a, b = _vq(0.5, accumulate=2), _vq(0.5, accumulate=2, sync=True)
    with torch.no_grad():
        for z in _batches(2):
            a(z), b(z)
    assert a.pending_ema_updates == b.pending_ema_updates == 0
    assert all(_same(x, y) for x, y in zip(_snapshot(a), _snapshot(b)))
    # a second "rank" through the two attributes: its uniforms are the ones every rank uses, its records follow this rank's
    m = _vq(0.5, accumulate=2, sync=True)
    before = _snapshot(m)
    u0 = torch.rand(2, K_, device=DEV, generator=torch.Generator(device=DEV).manual_seed(123))
    g = torch.Generator().manual_seed(9)
    other = []
    for z in _batches(2, seed=8):
        other.append(F.vq_ema_stats(z, torch.randint(0, K_, (z.shape[0] * 9,), generator=g).to(DEV), K_, row_uniforms=u0[1]))
    calls = []

    def gather(stats, group=None):
        calls.append(tuple(stats.shape))
        return torch.cat([stats, torch.stack(other)])

    def broadcast(u, group=None):
        calls.append("broadcast")
        return u.copy_(u0[None])

    m._ema_gather, m._ema_broadcast = gather, broadcast
    mine = []
    with torch.no_grad():
        for z in _batches(2):
            mine.append(F.vq_ema_stats(z, m(z)[4], K_, row_uniforms=u0[1]))
    assert calls == ["broadcast", (2, K_, 2 * D_ + 1)]                                 # one broadcast per cycle, one gather per apply
    want = _hand(before, mine + other, u0, 0.5)
    assert all(_same(x, y) for x, y in zip(want, _snapshot(m)))
    assert not all(_same(x, y) for x, y in zip(_hand(before, other + mine, u0, 0.5), want))     # the order is part of the result


def test_eval_records_nothing_and_load_state_dict_and_invalidate_drop_the_pending_records():
    m = _vq(accumulate=3)
    zs = _batches(3)
    before = _snapshot(m)
    with torch.no_grad():
        m.eval()
        m(zs[0])
        assert m.pending_ema_updates == 0
        m.train()
        m(zs[0])
        m(zs[1])
        assert m.pending_ema_updates == 2
        m.load_state_dict(copy.deepcopy(m.state_dict()))
        assert m.pending_ema_updates == 0 and "ema_pending" not in "".join(m.state_dict())
        m(zs[0])
        m.invalidate()
        assert m.pending_ema_updates == 0
        m(zs[0])
        m.to(DEV)
        assert m.pending_ema_updates == 0
        m(zs[0])
        m.init_codebook_(torch.randn(4, D_, 4, 4, device=DEV), iters=1, generator=torch.Generator(device=DEV).manual_seed(1))
        assert m.pending_ema_updates == 0
        m.flush_ema_()
    assert _same(before[0], torch.zeros(K_))                                           # (and none of it reached the buffers before)


def test_graphed_step_refuses_a_model_with_a_cycle():
    from vqvae_amd import _lib
    from vqvae_amd.graph import GraphedStep
    m = _vq(accumulate=2)
    with pytest.raises(_lib.VqvaeHipError, match="not a cycle"):
        GraphedStep(m, lambda z: m(z), _batches(1)[0])
    assert m.pending_ema_updates == 0                                                  # refused before any step ran
