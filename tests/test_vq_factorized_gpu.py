"""Factorized (low-dimensional) codes on the GPU: FactorizedVectorQuantizer / FactorizedVectorQuantizerEMA and VQVAE(codebook_dim=...)
against the chain they are built from -- functional.linear_rows, the existing quantizer on the narrow rows (functional.vq_forward,
training.vq_backward, functional.vq_ema_update, functional.l2norm_rows), functional.linear_rows again.  The same kernels on the same
operands: every comparison is bit for bit.  (tests/test_vq_linear_gpu.py holds the projection itself against its CPU restatement.)"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DIMS = (32, 8, 1, 64, 16, 0.25)          # h_dim, res_h_dim, n_res_layers, K, D, beta
K, D, d, BETA = 64, 16, 4, 0.25


def _bits(t):
    return t.detach().contiguous().cpu().numpy().view(np.uint32 if t.dtype == torch.float32 else np.int64)


def _same(a, b, what=""):
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert np.array_equal(_bits(a), _bits(b)), what


def _x(seed=1):
    return torch.rand((4, 3, 32, 32), generator=torch.Generator().manual_seed(seed)).to(DEV)


def _z(rowmajor, seed=2):
    z = torch.randn((4, 8, 8, D), generator=torch.Generator().manual_seed(seed))
    return (z if rowmajor else z.permute(0, 3, 1, 2).contiguous()).to(DEV)


def _quantizer(ema=False, seed=0, **kw):
    """a quantizer whose codebook is wide enough for its codes to be in use"""
    from vqvae_amd.modules import FactorizedVectorQuantizer, FactorizedVectorQuantizerEMA
    torch.manual_seed(seed)
    q = (FactorizedVectorQuantizerEMA(K, D, d, BETA, decay=0.9, **kw) if ema else FactorizedVectorQuantizer(K, D, d, BETA, **kw)).to(DEV)
    with torch.no_grad():
        q.embedding.weight.copy_(torch.randn((K, d), generator=torch.Generator().manual_seed(seed + 5)).to(DEV))
        if ema:
            q.ema_w.copy_(q.embedding.weight)
    return q


def _model(seed=0, **kw):
    from vqvae_amd.modules import VQVAE
    torch.manual_seed(seed)
    m = VQVAE(*DIMS, codebook_dim=d, **kw).to(DEV)
    vq = m.vector_quantization
    with torch.no_grad():
        # an untrained encoder's rows lie close together: every fourth projected row of the test images becomes a code, so that
        # the 256 rows spread over the codebook
        from vqvae_amd import conv as C_hip, functional as F
        z_e = C_hip.encoder_forward(m.encoder, _x(), pre_quant=m.pre_quantization_conv)
        y = F.linear_rows(z_e, vq.project_in.weight.detach(), vq.project_in.bias.detach(), rowmajor=True)
        vq.embedding.weight.copy_(y.reshape(-1, d)[::4])
        if "ema_decay" in kw:
            m.vector_quantization.ema_w.copy_(m.vector_quantization.embedding.weight)
    return m


def _manual_forward(q, z, rowmajor):
    """linear_rows -> (l2norm_rows) -> vq_forward -> linear_rows"""
    from vqvae_amd import functional as F
    from vqvae_amd.modules import VectorQuantizerEMA
    y = F.linear_rows(z, q.project_in.weight.detach(), q.project_in.bias.detach(), rowmajor=rowmajor)
    E = q.embedding.weight.detach()
    if q.cosine_sim:
        y, E = F.l2norm_rows(y, rowmajor=rowmajor)[0], F.l2norm_rows(E)[0]
    ema = isinstance(q, VectorQuantizerEMA)
    loss, zq_low, ppl, idx, hist = F.vq_forward(y, E, 0.0 if ema else q.beta, rowmajor=rowmajor)
    if ema:
        loss = loss * q.beta
    z_q = F.linear_rows(zq_low, q.project_out.weight.detach(), q.project_out.bias.detach(), rowmajor=rowmajor)
    return (loss, z_q, ppl, idx, hist), y, E, zq_low


@pytest.mark.parametrize("rowmajor", [True, False])
@pytest.mark.parametrize("cosine", [False, True])
@pytest.mark.parametrize("ema", [False, True])
def test_quantize_equals_the_manual_chain(rowmajor, cosine, ema):
    q = _quantizer(ema, cosine_sim=cosine).eval()
    z = _z(rowmajor)
    with torch.no_grad():
        got = q.quantize(z, rowmajor=rowmajor)
        idx_only = q.quantize(z, rowmajor=rowmajor, want_zq=False)
        five = q(z) if not rowmajor else None
    want = _manual_forward(q, z, rowmajor)[0]
    for i, (a, b) in enumerate(zip(got, want)):
        _same(a, b, f"output {i}")
    assert idx_only[1] is None
    _same(idx_only[3], want[3])
    assert got[1].shape == z.shape and got[3].shape == (256, 1) and got[4].shape == (K,) and len(torch.unique(got[3])) > 8
    if five is not None:                                         # forward(): the reference's 5-tuple with a LazyOneHot
        from vqvae_amd.modules import LazyOneHot
        assert isinstance(five[3], LazyOneHot) and five[3].shape == (256, K)
        _same(five[1], want[1])
        _same(five[4], want[3])
        assert torch.equal(five[3].materialize().argmax(1, keepdim=True), want[3])


@pytest.mark.parametrize("rowmajor", [True, False])
@pytest.mark.parametrize("rotation", [False, True])
def test_backward_equals_the_manual_chain(rowmajor, rotation):
    from vqvae_amd import functional as F, training as T
    q = _quantizer(rotation_trick=rotation).train()
    z = _z(rowmajor).requires_grad_(True)
    G = torch.randn(z.shape, generator=torch.Generator().manual_seed(9)).to(DEV)
    gl = torch.tensor(0.7, device=DEV)
    loss, z_q, _, idx, _ = q.quantize(z, rowmajor=rowmajor)
    assert z_q.grad_fn is not None and loss.grad_fn is not None
    torch.autograd.backward([z_q, loss], [G, gl])
    with torch.no_grad():
        want, y, E, zq_low = _manual_forward(q, z.detach(), rowmajor)
        _same(z_q, want[1])
        _same(loss, want[0])
        g_low, g_wo, g_bo = F.linear_rows_backward(zq_low, G, q.project_out.weight.detach(), rowmajor=rowmajor)
        g_y, g_E = T.vq_backward(y, E, idx, g_low, gl, q.beta, rowmajor=rowmajor, rotation=rotation)
        g_z, g_wi, g_bi = F.linear_rows_backward(z.detach(), g_y, q.project_in.weight.detach(), rowmajor=rowmajor)
    for name, a, b in (("z", z.grad, g_z), ("W_in", q.project_in.weight.grad, g_wi), ("b_in", q.project_in.bias.grad, g_bi),
                       ("W_out", q.project_out.weight.grad, g_wo), ("b_out", q.project_out.bias.grad, g_bo),
                       ("codebook", q.embedding.weight.grad, g_E)):
        assert a is not None and bool(torch.isfinite(a).all()) and bool(a.abs().sum() > 0), name
        _same(a, b, name)


@pytest.mark.parametrize("cosine", [False, True])
def test_ema_update_runs_from_the_projected_rows_in_training_mode_only(cosine):
    from vqvae_amd import functional as F
    q = _quantizer(True, cosine_sim=cosine).train()
    z = _z(True)
    state = lambda: [t.detach().clone() for t in (q.ema_cluster_size, q.ema_w, q.embedding.weight)]
    before = state()
    with torch.no_grad():
        want, y, _, _ = _manual_forward(q, z, True)              # (against the codebook as it is on entry)
        got = q.quantize(z, rowmajor=True)
    for a, b in zip(got, want):
        _same(a, b)
    cs, ew, cb = before[0].clone(), before[1].clone(), torch.empty_like(before[2])
    F.vq_ema_update(y, got[3], cs, ew, cb, q.decay, q.eps, rowmajor=True)
    after = state()
    for name, a, b in zip(("ema_cluster_size", "ema_w", "embedding.weight"), after, (cs, ew, cb)):
        _same(a, b, name)
    assert not torch.equal(after[2], before[2])
    q.eval()
    with torch.no_grad():
        q.quantize(z, rowmajor=True)
    for a, b in zip(state(), after):
        _same(a, b, "eval mode")


def test_encode_never_updates_an_ema_codebook():
    m = _model(ema_decay=0.9).train()
    vq = m.vector_quantization
    before = [t.detach().clone() for t in (vq.ema_cluster_size, vq.ema_w, vq.embedding.weight)]
    idx = m.encode(_x())
    assert idx.shape == (256, 1) and idx.dtype == torch.int64
    for a, b in zip((vq.ema_cluster_size, vq.ema_w, vq.embedding.weight), before):
        _same(a.detach(), b)


@pytest.mark.parametrize("kw", [{}, dict(cosine_sim=True), dict(ema_decay=0.9, cosine_sim=True)], ids=["plain", "cosine", "ema+cosine"])
def test_decode_of_encode_is_the_eval_forward(kw):
    m = _model(**kw).eval()
    x = _x()
    with torch.no_grad():
        loss, x_hat, ppl = m(x)
        idx = m.encode(x)
        again = m.decode_indices(idx, 4, 8, 8)
    assert x_hat.shape == x.shape and bool(torch.isfinite(x_hat).all()) and len(torch.unique(idx)) > 8
    _same(again, x_hat)
    # ... and the quantizer's own outputs on the encoder's rows
    from vqvae_amd import conv as C_hip
    with torch.no_grad():
        z_e = C_hip.encoder_forward(m.encoder, x, pre_quant=m.pre_quantization_conv)
        q = m.vector_quantization.quantize(z_e, rowmajor=True)
    _same(q[3], idx)
    _same(q[0], loss)
    _same(q[2], ppl)
    with pytest.raises(IndexError):
        m.decode_indices(torch.full_like(idx, K), 4, 8, 8)


@pytest.mark.parametrize("kw", [{}, dict(rotation_trick=True, cosine_sim=True), dict(ema_decay=0.9, restart_threshold=0.5)],
                         ids=["plain", "rotation+cosine", "ema+restart"])
def test_a_training_step_leaves_a_finite_gradient_on_every_parameter(kw):
    from vqvae_amd import training as T
    m = _model(**kw).train()
    x = _x()
    el, x_hat, ppl = m(x)
    T.step_losses(el, x_hat, ppl, x, 0.06)[1].backward()
    names = [n for n, p in m.named_parameters() if p.requires_grad]
    for n in ("project_in.weight", "project_in.bias", "project_out.weight", "project_out.bias"):
        assert "vector_quantization." + n in names
    assert ("vector_quantization.embedding.weight" in names) == ("ema_decay" not in kw)
    for n, p in m.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    for n in ("project_in.weight", "project_out.weight"):
        assert bool(m.get_parameter("vector_quantization." + n).grad.abs().sum() > 0), n


@pytest.mark.parametrize("kw", [{}, dict(cosine_sim=True), dict(ema_decay=0.9)], ids=["plain", "cosine", "ema"])
def test_init_codebook_runs_kmeans_on_the_projected_rows(kw):
    from vqvae_amd import conv as C_hip, functional as F
    m = _model(**kw).train()
    vq = m.vector_quantization
    x = _x()
    before = vq.embedding.weight.detach().clone()
    gen = torch.Generator(device=DEV).manual_seed(11)
    codebook, counts = m.init_codebook_(x, iters=3, generator=gen)
    assert codebook.shape == (K, d) and counts.shape == (K,) and int(counts.sum()) == 256
    _same(vq.embedding.weight.detach(), codebook)
    assert not torch.equal(codebook, before)
    # the same rows and the same uniforms by hand
    with torch.no_grad():
        z_e = C_hip.encoder_forward(m.encoder, x, pre_quant=m.pre_quantization_conv)
        y = F.linear_rows(z_e, vq.project_in.weight.detach(), vq.project_in.bias.detach(), rowmajor=True)
        if vq.cosine_sim:
            y = F.l2norm_rows(y, rowmajor=True)[0]
        want, want_counts = F.vq_kmeans(y, K, 3, generator=torch.Generator(device=DEV).manual_seed(11), rowmajor=True)
    _same(codebook, want)
    assert torch.equal(counts, want_counts)
    if "ema_decay" in kw:
        c = counts.to(torch.float32)
        _same(vq.ema_cluster_size, c)
        _same(vq.ema_w, c[:, None] * codebook)


def test_codebook_cache_and_invalidate():
    from vqvae_amd import functional as F
    m = _model(cosine_sim=True).eval()
    vq = m.vector_quantization
    with torch.no_grad():
        codes = vq.codes()
        _same(codes, F.l2norm_rows(vq.embedding.weight.detach())[0])
        cb = vq.codebook()
        _same(cb, F.linear_rows(codes, vq.project_out.weight.detach(), vq.project_out.bias.detach()))
        assert cb.shape == (K, D) and vq.codebook() is cb                         # cached
        vq.project_out.weight.data.mul_(2.0)                                      # a write through .data: no version moves
        assert vq.codebook() is cb
        m.invalidate_caches()
        new = vq.codebook()
        assert new is not cb and not torch.equal(new, cb)
        _same(new, F.linear_rows(codes, vq.project_out.weight.detach(), vq.project_out.bias.detach()))
        vq.project_out.bias.add_(1.0)                                             # an in-place op moves the version: re-keyed
        assert not torch.equal(vq.codebook(), new)
        x = _x()
        _same(m.decode_indices(m.encode(x), 4, 8, 8), m(x)[1])


@pytest.mark.parametrize("kw", [{}, dict(ema_decay=0.9, cosine_sim=True)], ids=["plain", "ema+cosine"])
def test_the_eval_forward_replays_from_a_graph(kw):
    m = _model(**kw).eval()
    xs = torch.zeros(4, 3, 32, 32, device=DEV)
    x = _x()
    with torch.no_grad():
        want = m(x)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            m(xs)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            got = m(xs)
        xs.copy_(x)
        for _ in range(2):
            graph.replay()
            torch.cuda.synchronize()
            for p, q in zip(got, want):
                _same(p, q)


def test_the_fused_entries_refuse_and_the_prior_tools_work():
    from vqvae_amd._lib import VqvaeHipError
    from vqvae_amd.pixelcnn import GatedPixelCNN, complete_images, sample_images
    m = _model().eval()
    with pytest.raises(VqvaeHipError):
        m._c_weights()
    torch.manual_seed(3)
    prior = GatedPixelCNN(K, 16, 3, 10).eval().to(DEV)
    gen = torch.Generator().manual_seed(4)
    label = torch.randint(0, 10, (4,), generator=gen).to(DEV)
    u = torch.rand((4, 8, 8), generator=gen).to(DEV)
    idx, x_hat = sample_images(prior, m, label, (8, 8), 4, uniforms=u)
    assert idx.shape == (4, 8, 8) and x_hat.shape == (4, 3, 32, 32) and int(idx.min()) >= 0 and int(idx.max()) < K
    with torch.no_grad():
        _same(x_hat, m.decode_indices(idx.reshape(-1, 1), 4, 8, 8))
    idx2, x2 = complete_images(prior, m, _x(), label, 4, uniforms=u)
    assert idx2.shape == (4, 8, 8) and x2.shape == (4, 3, 32, 32) and bool(torch.isfinite(x2).all())


def test_the_training_mode_no_grad_ema_forward_decodes_the_codebook_on_entry():
    """VectorQuantizerEMA's rule -- every output belongs to the codebook BEFORE the update -- holds for x_hat too, although the
    update has moved embedding.weight (and re-keyed codebook()) by the time the indices are decoded"""
    from vqvae_amd import conv as C_hip, functional as F
    m = _model(ema_decay=0.9).train()
    vq = m.vector_quantization
    x = _x()
    with torch.no_grad():
        before, w0 = vq.codebook().clone(), vq.embedding.weight.detach().clone()
        idx = m.encode(x)                                        # (never updates)
        loss, x_hat, ppl = m(x)
        assert not torch.equal(vq.embedding.weight.detach(), w0) and not torch.equal(vq.codebook(), before)
        want = C_hip.decoder_forward(m.decoder, F.vq_decode_indices(idx.view(-1), before, 4, 8, 8, validate=False), rowmajor_in=False)
        _same(x_hat, want)
        assert not torch.equal(m.decode_indices(idx, 4, 8, 8), x_hat)          # the moved codebook decodes to other images
