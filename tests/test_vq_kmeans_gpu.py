"""k-means initialisation of the codebook on the GPU (vqvae_vq_kmeans_seed_f32, vqvae_vq_kmeans_update_f32, functional.vq_kmeans,
init_codebook_ of the modules) against the fp64 restatement of tests/kmeans_ref.py, whose operation order is the kernels' (header of
vqvae_amd/csrc/vq_kmeans.hip).

Seeding: the rows exactly the restatement's and the codes bitwise those rows, in both layouts.  Update: counts exact, means at the
EMA test's tolerance for the same segmented sum (rtol 1e-5, atol 1e-7).  K <= 64 throughout: a seeding is 1 + 2 (K - 1) launches."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from tests import kmeans_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U_TOP = np.float32(1.0) - np.float32(2.0 ** -24)          # the largest fp32 below 1


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _layout(rows, B, H, W, rowmajor):
    """(N, D) numpy rows -> the device tensor whose rows they are: (B,H,W,D), or (B,D,H,W)"""
    z = torch.from_numpy(np.ascontiguousarray(rows)).view(B, H, W, rows.shape[1])
    return (z if rowmajor else z.permute(0, 3, 1, 2)).contiguous().to(DEV)


def _uniforms(K, seed):
    return np.random.default_rng(seed).random(K, dtype=np.float32)


def _seed(rows, B, H, W, K, u, rowmajor):
    from vqvae_amd import functional as F
    cb, r = F.vq_kmeans_seed(_layout(rows, B, H, W, rowmajor), K, torch.from_numpy(u).to(DEV), rowmajor=rowmajor)
    torch.cuda.synchronize()
    return cb, r.cpu().numpy()


# (B, H, W, D, K): the plain case, a ragged one, the narrowest and the widest rows, three selection blocks (two of 256 rows and a
# partial one), more codes than rows
SEED_CASES = [(2, 8, 8, 64, 16), (3, 5, 7, 48, 8), (1, 8, 8, 1, 8), (1, 8, 8, 256, 8), (5, 11, 13, 4, 12), (1, 1, 5, 8, 9)]


@pytest.mark.parametrize("rowmajor", [False, True])
@pytest.mark.parametrize("B,H,W,D,K", SEED_CASES)
def test_seeding_picks_the_restatements_rows(B, H, W, D, K, rowmajor):
    N = B * H * W
    rows = np.random.default_rng(N + D).standard_normal((N, D)).astype(np.float32)
    u = _uniforms(K, K + D)
    if N == 715:
        u[:4] = [0.05, 0.5, 0.97, 0.02]                      # picks in the first, a middle and the last block
    want = R.seed(rows, K, u)
    if N == 715:
        assert set((want // R.BLOCK).tolist()) == {0, 1, 2}
    if K > N:
        trace = []
        R.seed(rows, K, u, trace)
        assert [T for _, T in trace[N - 1:]] == [0.0] * (K - N)      # the surplus codes follow the T = 0 rule
    cb, got = _seed(rows, B, H, W, K, u, rowmajor)
    assert np.array_equal(got, want), (got, want)
    assert np.array_equal(_bits(cb), rows[want].view(np.uint32)), "codebook[k] must be row rows[k] bit for bit"


@pytest.mark.parametrize("rowmajor", [False, True])
def test_repeated_points_are_each_taken_once(rowmajor):
    M, r, D = 16, 8, 64
    rows, which = R.repeated_points(M, r, D, M)
    for u in (np.zeros(M, np.float32), np.full(M, U_TOP, np.float32), _uniforms(M, 1)):
        cb, got = _seed(rows, 2, 8, 8, M, u, rowmajor)
        assert sorted(which[got].tolist()) == list(range(M)), "a zero-weight row (a copy of a chosen centre) was picked"
        assert np.array_equal(got, R.seed(rows, M, u))
    # more codes than distinct points: the surplus takes the rows its uniforms name
    u = _uniforms(M + 4, 2)
    cb, got = _seed(rows, 2, 8, 8, M + 4, u, rowmajor)
    assert sorted(which[got[:M]].tolist()) == list(range(M))
    assert got[M:].tolist() == [R.uniform_row(v, M * r) for v in u[M:]]


def test_same_bits_from_two_runs_and_from_both_layouts():
    B, H, W, D, K = 3, 9, 11, 20, 24                        # 297 rows: two selection blocks
    rows = np.random.default_rng(3).standard_normal((B * H * W, D)).astype(np.float32)
    u = _uniforms(K, 4)
    a = _seed(rows, B, H, W, K, u, False)
    b = _seed(rows, B, H, W, K, u, False)
    c = _seed(rows, B, H, W, K, u, True)
    for other in (b, c):
        assert np.array_equal(a[1], other[1]) and np.array_equal(_bits(a[0]), _bits(other[0]))
    from vqvae_amd import functional as F
    idx = torch.from_numpy(np.random.default_rng(5).integers(0, K - 3, B * H * W)).to(DEV)
    outs = []
    for rowmajor in (False, False, True):
        cb = a[0].clone()
        counts = F.vq_kmeans_update(_layout(rows, B, H, W, rowmajor), idx, cb, rowmajor=rowmajor)
        outs.append((_bits(cb), counts.cpu().numpy()))
    for o in outs[1:]:
        assert np.array_equal(outs[0][0], o[0]) and np.array_equal(outs[0][1], o[1])


def _histograms(N, K):
    g = np.random.default_rng(N + K)
    skew = g.integers(0, K // 2, N)                         # half the codes share the rows ...
    skew[g.permutation(N)[:700]] = 3                        # ... and one owns more than kSegChunk = 512 of them: two units combine
    return {"skewed": skew, "one code": np.full(N, K - 2), "uniform": g.integers(0, K, N)}


@pytest.mark.parametrize("rowmajor", [False, True])
def test_update_against_the_restatement(rowmajor):
    from vqvae_amd import functional as F
    B, H, W, D, K = 4, 16, 16, 24, 16
    N = B * H * W
    g = np.random.default_rng(7)
    rows = (g.standard_normal((N, D)) * 0.3 + 0.1).astype(np.float32)
    cb0 = g.standard_normal((K, D)).astype(np.float32)
    u = _uniforms(K, 8)
    z = _layout(rows, B, H, W, rowmajor)
    for name, idx in _histograms(N, K).items():
        for uu in (None, u):
            cb = torch.from_numpy(cb0).to(DEV)
            counts = F.vq_kmeans_update(z, torch.from_numpy(idx).to(DEV), cb, rowmajor=rowmajor,
                                        uniforms=None if uu is None else torch.from_numpy(uu).to(DEV))
            torch.cuda.synchronize()
            ref, rc = R.update(rows, idx, cb0, uu)
            assert counts.dtype == torch.int32 and np.array_equal(counts.cpu().numpy(), rc), name
            if name == "skewed":
                assert rc[3] > 512 and (rc == 0).sum() >= K // 2
            if name == "one code":
                assert (rc > 0).sum() == 1
            have = rc > 0
            got = cb.cpu().numpy()
            np.testing.assert_allclose(got[have].astype(np.float64), ref[have], rtol=1e-5, atol=1e-7, err_msg=name)
            # a code without rows: its own bits, or with uniforms the row they name, bit for bit
            assert np.array_equal(got[~have].view(np.uint32), ref[~have].astype(np.float32).view(np.uint32)), name
            if uu is not None and (~have).any():
                assert np.array_equal(got[~have], rows[[R.uniform_row(v, N) for v in uu[~have]]])


@pytest.mark.parametrize("rowmajor", [False, True])
def test_kmeans_on_separated_blobs(rowmajor):
    from vqvae_amd import functional as F
    K, n, D = 8, 32, 64
    rows, which, sep = R.blobs(K, n, D, 1)
    assert sep >= 100.0
    z = _layout(rows, 4, 8, 8, rowmajor)
    for iters in (1, 3):
        cb, counts = F.vq_kmeans(z, K, iters, generator=torch.Generator(device=DEV).manual_seed(iters), rowmajor=rowmajor)
        torch.cuda.synchronize()
        assert counts.cpu().tolist() == [n] * K
        got = cb.cpu().numpy().astype(np.float64)
        means = np.stack([rows[which == b].astype(np.float64).mean(0) for b in range(K)])
        owner = ((got[:, None, :] - means[None, :, :]) ** 2).sum(-1).argmin(1)
        assert sorted(owner.tolist()) == list(range(K)), "one code per blob"
        np.testing.assert_allclose(got, means[owner], rtol=1e-5, atol=1e-7)


def test_kmeans_on_gaussian_rows_never_gets_worse():
    """Lloyd's two steps each minimise the mean squared distance J over what they change, so J cannot rise -- in exact arithmetic.
    What is inexact here: (a) the mean is one fp64 division rounded to fp32, which moves a code by at most 2^-24 |e| off the exact
    minimiser of a quadratic: a second-order change, <= 2^-48 |e|^2 per row, negligible; (b) the assignment is the quantizer's
    argmin of the reference's fp32 distance |z|^2 + |e|^2 - 2 z.e.  |z|^2 is one value per row, the same for every code, so the
    choice between codes rests on |e|^2 - 2 z.e; the fp32 dot product of D terms is off by at most D 2^-24 sum|z_c e_c|, doubled by
    the factor 2 and bounded with 2 |z_c e_c| <= z_c^2 + e_c^2: D 2^-24 (|z|^2 + |e|^2); the additions that combine the three terms
    and the rounding of |e|^2 add a few 2^-24 of the same magnitude: (D + 4) 2^-24 (|z|^2 + |e|^2) per row.  A row may therefore be
    given a code that is worse than its old one by no more than that, and the mean over the rows is the tolerance
    (D + 4) 2^-24 mean(|z|^2 + |e|^2) of a round-to-round rise in J.  Also: every round's indices are vq_forward's (and the C
    oracle's) against that round's codebook, exactly."""
    from vqvae_amd import functional as F
    B, H, W, D, K, iters = 8, 8, 8, 64, 32, 5
    rows = (np.random.default_rng(11).standard_normal((B * H * W, D)) * 0.5).astype(np.float32)
    z = _layout(rows, B, H, W, True)
    trace = []
    cb, counts = F.vq_kmeans(z, K, iters, generator=torch.Generator(device=DEV).manual_seed(12), rowmajor=True, trace=trace)
    assert len(trace) == iters
    _, _, _, idx_last, hist = F.vq_forward(z, cb, 0.0, rowmajor=True, want_zq=False)
    torch.cuda.synchronize()
    J = []
    for t, (cb_t, idx_t) in enumerate(trace + [(cb, idx_last)]):
        fresh = F.vq_forward(z, cb_t, 0.25, rowmajor=True, want_zq=False)[3]
        assert torch.equal(idx_t, fresh), f"round {t}: indices"
        assert np.array_equal(idx_t.view(-1).cpu().numpy(), R.assign(rows, cb_t)), f"round {t}: indices against the oracle"
        e = cb_t.cpu().numpy()
        tol = (D + 4) * 2.0 ** -24 * float(((rows.astype(np.float64) ** 2).sum(1)
                                            + (e.astype(np.float64)[idx_t.view(-1).cpu().numpy()] ** 2).sum(1)).mean())
        J.append((R.mean_sq_dist(rows, e, idx_t), tol))
    print("J per round:", [f"{j:.9g}" for j, _ in J], "tolerance:", [f"{t:.3g}" for _, t in J])
    for (j0, _), (j1, tol) in zip(J, J[1:]):
        assert j1 <= j0 + tol, (j0, j1, tol)
    assert J[-1][0] < J[0][0]
    # the counts are those of the last assignment the loop made
    assert np.array_equal(counts.cpu().numpy(), np.bincount(trace[-1][1].view(-1).cpu().numpy(), minlength=K))


def _model(**kw):
    from vqvae_amd import conv
    from vqvae_amd.modules import VQVAE
    conv.set_conv_backend("hip")
    torch.manual_seed(0)
    return VQVAE(128, 32, 2, 64, 64, 0.25, **kw).to(DEV)


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def test_vqvae_init_codebook_writes_the_kmeans_of_the_encoders_rows():
    from vqvae_amd import _lib, conv, functional as F
    m = _model().eval()
    x = torch.randn(8, 3, 32, 32, generator=torch.Generator().manual_seed(1)).to(DEV)
    w = m.vector_quantization.embedding.weight
    with torch.no_grad():
        idx_before = m.encode(x)                            # packs the weights and prepares the old codebook's images
        m(x)
    v0, old = w._version, w.detach().clone()
    m.init_codebook_(x, generator=_gen(2))
    assert w._version > v0 and not torch.equal(w.detach(), old)
    with torch.no_grad():
        z_e = conv.encoder_forward(m.encoder, x, pre_quant=m.pre_quantization_conv)
        want, counts = F.vq_kmeans(z_e, 64, 10, generator=_gen(2), rowmajor=True)
        assert np.array_equal(_bits(w), _bits(want))
        assert int(counts.sum()) == 8 * 64
        # the whole path re-packed: encode() quantizes its own z_e (the encoder entry's bits) against the NEW codebook
        idx = m.encode(x)
        L = _lib.load()
        cw, _keep = m._c_weights()
        ws, stream = m._c_workspace(L, cw, 8, 32, 32, torch.device(DEV))
        z_wp = torch.empty(8, 8, 8, 64, device=DEV)
        _lib.check(L.vqvae_encoder_f32(cw, x.data_ptr(), 8, 32, 32, z_wp.data_ptr(), ws.data_ptr(), ws.numel(), stream))
        ref_idx = F.vq_forward(z_wp, w.detach(), 0.25, rowmajor=True, want_zq=False)[3]
        assert torch.equal(idx, ref_idx) and not torch.equal(idx, idx_before)
        print("distinct codes in use before / after the initialisation:", idx_before.unique().numel(), idx.unique().numel())


def test_second_call_on_a_warm_module_equals_a_fresh_modules():
    m = _model().eval()
    fresh = copy.deepcopy(m)
    g = torch.Generator().manual_seed(3)
    x1, x2 = torch.randn(8, 3, 32, 32, generator=g).to(DEV), torch.randn(4, 3, 32, 32, generator=g).to(DEV)
    with torch.no_grad():
        m.init_codebook_(x1, generator=_gen(4))
        m(x1)
        m.vector_quantization(torch.randn(2, 64, 8, 8, device=DEV))
        m.init_codebook_(x2, iters=3, generator=_gen(5))
        fresh.init_codebook_(x2, iters=3, generator=_gen(5))
        for k, v in m.state_dict().items():
            assert np.array_equal(_bits(v), _bits(fresh.state_dict()[k])), k
        for a, b in zip(m(x1), fresh(x1)):
            assert np.array_equal(_bits(a), _bits(b))


def test_ema_quantizer_continues_from_the_clusters():
    from vqvae_amd import training as T
    m = _model(ema_decay=0.99).train()
    vq = m.vector_quantization
    x = torch.randn(8, 3, 32, 32, generator=torch.Generator().manual_seed(6)).to(DEV)
    cb, counts = m.init_codebook_(x, iters=4, generator=_gen(7))
    assert np.array_equal(_bits(vq.embedding.weight), _bits(cb))
    assert torch.equal(vq.ema_cluster_size, counts.float()) and int(counts.sum()) == 8 * 64
    assert np.array_equal(_bits(vq.ema_w), _bits(counts.float()[:, None] * cb))
    el, xh, pp = m(x)                                       # a training forward: one EMA update from the clusters
    T.step_losses(el, xh, pp, x, 0.06)[1].backward()
    torch.cuda.synchronize()
    assert torch.isfinite(vq.embedding.weight).all() and torch.isfinite(vq.ema_w).all()
    assert float(pp) > 8.0                                  # the codes are in use from the first update on
    torch.testing.assert_close(vq.ema_cluster_size.sum(), torch.tensor(512.0, device=DEV), rtol=1e-5, atol=0)


def test_quantizer_alone_takes_nchw_rows():
    from vqvae_amd import functional as F
    from vqvae_amd.modules import VectorQuantizer
    torch.manual_seed(8)
    vq = VectorQuantizer(16, 32, 0.25).to(DEV)
    z = torch.randn(2, 32, 8, 8, device=DEV)
    vq(z)
    v0 = vq.embedding.weight._version
    vq.init_codebook_(z, iters=2, generator=_gen(9))
    want, _ = F.vq_kmeans(z, 16, 2, generator=_gen(9))
    assert vq.embedding.weight._version > v0 and np.array_equal(_bits(vq.embedding.weight), _bits(want))
    out = vq(z)
    ref = F.vq_forward(z, want, 0.25)
    assert torch.equal(out[4], ref[3]) and np.array_equal(_bits(out[1]), _bits(ref[1]))


def test_a_model_without_the_call_is_todays():
    from oracle import torch_port
    m = _model()
    torch.manual_seed(0)
    ref = torch_port.init_state_dict(n_embeddings=64)
    sd = m.state_dict()
    for k, v in ref.items():
        assert torch.equal(sd[k].cpu(), v), k


def test_envelope_on_the_device():
    from vqvae_amd import _lib
    L = _lib.load()
    z = torch.zeros(4 * 64 * 260, device=DEV)
    u = torch.zeros(16385, device=DEV)
    cb = torch.zeros(16385 * 4, device=DEV)
    out = torch.zeros(16385, dtype=torch.int64, device=DEV)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    a = [t.data_ptr() for t in (z, u, cb, out, ws)]
    for D, K in ((257, 16), (4, 16385), (4, 0)):
        assert L.vqvae_vq_kmeans_workspace_bytes(64, K, D) == 0
        assert L.vqvae_vq_kmeans_seed_f32(a[0], 1, D, 8, 8, K, a[1], 0, a[2], a[3], a[4], ws.numel(), None) == _lib.ERR_UNSUPPORTED
        assert L.vqvae_vq_kmeans_update_f32(a[0], a[3], 1, D, 8, 8, K, None, 0, a[2], a[3], a[4], ws.numel(),
                                            None) == _lib.ERR_UNSUPPORTED
    assert L.vqvae_vq_kmeans_workspace_bytes(64, 16, 4) > 0
    torch.cuda.synchronize()
