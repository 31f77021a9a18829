"""The cosine-similarity codebook on the GPU: functional.l2norm_rows / l2norm_rows_backward (vqvae_l2norm_forward_f32 /
vqvae_l2norm_backward_f32) and the modules' cosine_sim option against the CPU restatement tests/vq_cosine_ref.py, whose arithmetic is
the header of vqvae_amd/csrc/vq_cosine.hip.

Tier 1: the restatement's bits in both layouts, in two runs and on the element path (a NaN compares as a NaN).  Tier 2: fp64 torch
(F.normalize and its autograd) within the bounds of vq_cosine_ref.forward_bound / backward_bound.  Then the modules: after the
normalisation the quantizer is the existing one on other bits, so its side of every comparison is the restated rows handed to the
existing entries (functional.vq_forward, training.vq_backward), and on the CPU the C oracle's indices and tests/vq_ema_ref.py."""
import functools

import numpy as np
import pytest
import torch

from tests import vq_cosine_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BETA = 0.25

# (B, D, H, W, K): the rotation tests' shapes -- the smallest call; D = 1; odd everything, no 16-byte path; N = 105, a partial wave and
# HW % 4 != 0; the flagship row, 320 rows; D % 4 == 0 and no power of two; the widest (four chunks of the row-major kernel) -- and
# 4 480 rows: 18 workgroups of the row-major kernels, 5 of the NCHW ones.  The kernels run one item per thread over a grid that
# covers all rows (no capped grid, no stride loop), so there is no "more than one pass" case to add.
SHAPES = [(1, 1, 1, 1, 1), (3, 1, 7, 5, 4), (3, 3, 5, 3, 7), (3, 64, 7, 5, 64), (5, 64, 8, 8, 512), (2, 48, 8, 8, 96), (2, 256, 4, 4, 32),
          (70, 64, 8, 8, 512)]
SCALES = [0.05, 1.0]


def _layout(rows, B, H, W, rowmajor):
    z = torch.from_numpy(np.ascontiguousarray(rows)).view(B, H, W, rows.shape[1])
    return (z if rowmajor else z.permute(0, 3, 1, 2)).contiguous().to(DEV)


def _rows(t, rowmajor):
    t = t.detach().cpu()
    t = t if rowmajor else t.permute(0, 2, 3, 1)
    return np.ascontiguousarray(t.contiguous().numpy().reshape(-1, t.shape[-1]))


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _ulps(got, ref64):
    """|got - round32(ref)| in units of fp32 spacing at round32(ref) (tests/test_vq_ema_gpu.py's measure)"""
    ref = ref64.float().cpu().numpy()
    got = got.detach().float().cpu().numpy()
    sp = np.spacing(np.maximum(np.abs(ref), np.float32(np.finfo(np.float32).tiny))).astype(np.float64)
    return np.abs(got.astype(np.float64) - ref.astype(np.float64)) / sp


def _same_bits_nan_aside(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN positions"
    diff = got.view(np.uint32)[~gn] != want.view(np.uint32)[~wn]
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} elements differ in their bits"


@functools.lru_cache(maxsize=None)
def _case(B, D, H, W, K, scale):
    """rows, codebook, g and the restatement (forward, backward, the composed quantizer), computed once and left unchanged.  With
    N >= 8: a zero row, a row below eps, a NaN and an Inf in x and a NaN in g."""
    N = B * H * W
    x, cb, g = R.draw(N, D, K, scale, 1000 * D + N + int(100 * scale))
    if N >= 8:
        x[0] = 0.0
        x[1] = 1e-20
        x[3, D // 2] = np.nan
        x[4, D - 1] = np.inf
        g[5, 0] = np.nan
    y, d = R.l2norm(x)
    gx = R.l2norm_backward(y, d, g)
    for a in (x, cb, g, y, d, gx):
        a.setflags(write=False)
    return x, cb, g, y, d, gx


def _forward(x, B, H, W, rowmajor):
    from vqvae_amd import functional as F
    y, d = F.l2norm_rows(_layout(x, B, H, W, rowmajor), rowmajor=rowmajor)
    torch.cuda.synchronize()
    return _rows(y, rowmajor), d.cpu().numpy()


def _backward(y, d, g, B, H, W, rowmajor):
    from vqvae_amd import functional as F
    gx = F.l2norm_rows_backward(_layout(y, B, H, W, rowmajor), torch.from_numpy(np.ascontiguousarray(d)).to(DEV),
                                _layout(g, B, H, W, rowmajor), rowmajor=rowmajor)
    torch.cuda.synchronize()
    return _rows(gx, rowmajor)


# ---- 1. bits against the restatement ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("B,D,H,W,K", SHAPES)
def test_bits_against_the_restatement_in_both_layouts(B, D, H, W, K, scale):
    x, cb, g, y, d, gx = _case(B, D, H, W, K, scale)
    if B * H * W >= 8:
        eps = np.float32(R.EPS)
        assert d[0] == eps and d[1] == eps and np.isnan(d[3]) and np.isinf(d[4])
        assert np.isnan(y[3]).all() and np.isnan(gx[5]).all()
        assert np.isfinite(np.delete(y, [3, 4], axis=0)).all() and np.isfinite(np.delete(gx, [3, 4, 5], axis=0)).all()
    for rowmajor in (True, False):
        got_y, got_d = _forward(x, B, H, W, rowmajor)
        _same_bits_nan_aside(got_y, y, f"y rowmajor={rowmajor}")
        _same_bits_nan_aside(got_d, d, f"denom rowmajor={rowmajor}")
        _same_bits_nan_aside(_backward(y, d, g, B, H, W, rowmajor), gx, f"grad_x rowmajor={rowmajor}")
    # a codebook: a 2-D tensor is K row-major rows
    from vqvae_amd import functional as F
    En, dn = R.l2norm(cb)
    e_gpu, d_gpu = F.l2norm_rows(torch.from_numpy(cb).to(DEV))
    assert e_gpu.shape == (K, D) and d_gpu.shape == (K,)
    _same_bits_nan_aside(e_gpu.cpu().numpy(), En, "codebook")
    _same_bits_nan_aside(d_gpu.cpu().numpy(), dn, "codebook denom")


@pytest.mark.parametrize("rowmajor", [True, False])
@pytest.mark.parametrize("B,D,H,W,K", [(5, 64, 8, 8, 512), (2, 256, 4, 4, 32)])
def test_tensors_offset_by_four_bytes_take_the_element_path_with_the_same_bits(B, D, H, W, K, rowmajor):
    from vqvae_amd import functional as F
    x, cb, g, y, d, gx = _case(B, D, H, W, K, 1.0)

    def off(t):                                             # the same values in a tensor that starts 4 bytes past an aligned address
        buf = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)
        v = buf[1:].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v

    got_y, got_d = F.l2norm_rows(off(_layout(x, B, H, W, rowmajor)), rowmajor=rowmajor)
    got_gx = F.l2norm_rows_backward(off(_layout(y, B, H, W, rowmajor)), off(torch.from_numpy(d).to(DEV)), off(_layout(g, B, H, W, rowmajor)),
                                    rowmajor=rowmajor)
    torch.cuda.synchronize()
    _same_bits_nan_aside(_rows(got_y, rowmajor), y, "y, offset tensors")
    _same_bits_nan_aside(got_d.cpu().numpy(), d, "denom, offset tensors")
    _same_bits_nan_aside(_rows(got_gx, rowmajor), gx, "grad_x, offset tensors")


def test_same_bits_in_both_layouts_and_in_two_runs():
    B, D, H, W, K = 70, 64, 8, 8, 512
    x, cb, g, y, d, gx = _case(B, D, H, W, K, 1.0)
    fw = [_forward(x, B, H, W, rm)[0] for rm in (True, False, True, False)]
    bw = [_backward(y, d, g, B, H, W, rm) for rm in (True, False, True, False)]
    for r in fw[1:]:
        _same_bits_nan_aside(r, fw[0], "forward: layouts / runs")
    for r in bw[1:]:
        _same_bits_nan_aside(r, bw[0], "backward: layouts / runs")


# ---- 2. the independent bounds ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("B,D,H,W,K", SHAPES)
def test_within_the_bounds_of_fp64_torch(B, D, H, W, K, scale):
    """forward: |y - y^| <= 4 2^-24 |y^| + one fp32 denormal; backward: |grad_x - ref| <= 2^-20 ||g|| / ||x|| per element on rows off
    the clamp (vq_cosine_ref.backward_bound has the derivation: 6u ||g|| / ||x||, doubled and rounded up to a power of two)."""
    x, cb, g, y, d, gx = _case(B, D, H, W, K, scale)
    ok = np.isfinite(x).all(axis=1) & np.isfinite(g).all(axis=1) & (d > np.float32(R.EPS))
    if not ok.any():
        return
    got_y, _ = _forward(x, B, H, W, True)
    got_gx = _backward(y, d, g, B, H, W, True)
    ref_y, ref_gx = R.torch_normalize(x[ok], g[ok])
    ef, bf = np.abs(got_y[ok].astype(np.float64) - ref_y), R.forward_bound(ref_y)
    eb, bb = np.abs(got_gx[ok].astype(np.float64) - ref_gx), R.backward_bound(x[ok], g[ok])[:, None]
    print(f"forward max err / bound = {(ef / bf).max():.4f}, backward max err / bound = {(eb / bb).max():.4f} over {int(ok.sum())} rows")
    assert (ef <= bf).all()
    assert (eb <= bb).all()


# ---- 3. the quantizer modules ----------------------------------------------------------------------------------------------------

def _quantizer(cls, K, D, **kw):
    torch.manual_seed(3)
    m = cls(K, D, BETA, cosine_sim=True, **kw).to(DEV)
    with torch.no_grad():
        m.embedding.weight.copy_(0.3 * torch.randn(K, D, generator=torch.Generator().manual_seed(4)))
        if hasattr(m, "ema_w"):
            m.ema_w.copy_(m.embedding.weight)
    return m


@pytest.mark.parametrize("rotation", [False, True])
@pytest.mark.parametrize("ema", [False, True])
def test_quantizer_modules_against_the_restatement(ema, rotation):
    """forward: idx the C oracle's on (z^, E^), z_q = z^ + (e^ - z^) in numpy fp32, loss and perplexity the existing entry's on the
    restated bits (and the fp64 values to 1e-5); backward: z.grad and weight.grad = the restated l2norm backward of what the existing
    vq_backward returns for (z^, E^); EMA: the buffers after the training forward = vq_ema_ref on z^ (to test_vq_ema_gpu's ulps);
    eval never updates."""
    from tests import vq_ema_ref
    from vqvae_amd import functional as F, training as T
    from vqvae_amd.modules import VectorQuantizer, VectorQuantizerEMA
    B, D, H, W, K = 4, 16, 8, 8, 64
    N = B * H * W
    m = _quantizer(VectorQuantizerEMA if ema else VectorQuantizer, K, D, rotation_trick=rotation).train()
    g0 = torch.Generator().manual_seed(5)
    z0 = torch.randn(B, D, H, W, generator=g0)
    t = torch.randn(B, D, H, W, generator=g0)
    cb = m.embedding.weight.detach().cpu().numpy().copy()
    cs0, w0 = (m.ema_cluster_size.cpu().clone(), m.ema_w.cpu().clone()) if ema else (None, None)
    zn, En, c = R.quantize(_rows(z0, False), cb, BETA)
    z = z0.to(DEV).requires_grad_(True)
    loss, z_q, ppl, _, idx = m(z)
    ((z_q * t.to(DEV)).sum() + loss).backward()
    torch.cuda.synchronize()
    # forward
    assert np.array_equal(idx.view(-1).cpu().numpy(), c.idx[0])
    _same_bits_nan_aside(_rows(z_q, False), c.z_q, "z_q")
    zn_d, En_d = _layout(zn, B, H, W, False), torch.from_numpy(En).to(DEV)
    l_ref, _, p_ref, idx_ref, _ = F.vq_forward(zn_d, En_d, 0.0 if ema else BETA)
    l_ref = l_ref * BETA if ema else l_ref
    assert torch.equal(idx_ref, idx)
    assert np.array_equal(_bits(loss), _bits(l_ref)) and np.array_equal(_bits(ppl), _bits(p_ref))
    mse = c.loss / (1.0 + BETA)
    np.testing.assert_allclose(float(loss), BETA * mse if ema else c.loss, rtol=1e-5)
    np.testing.assert_allclose(float(ppl), c.perplexity[0], rtol=1e-5)
    assert np.abs(np.linalg.norm(_rows(z_q, False).astype(np.float64), axis=1) - 1.0).max() <= 2.0 ** -22
    # backward: the existing quantizer's gradients for (z^, E^), then the restated normalisation backward
    one = torch.ones((), device=DEV)
    gzn, gEn = T.vq_backward(zn_d, En_d, idx, t.to(DEV), one, BETA, need_codebook=not ema, commitment=ema, rotation=rotation)
    _, dz = R.l2norm(_rows(z0, False))
    want_gz = R.l2norm_backward(zn, dz, _rows(gzn, False))
    _same_bits_nan_aside(_rows(z.grad, False), want_gz, "z.grad")
    if ema:
        assert m.embedding.weight.grad is None
        ref = vq_ema_ref.ema_update(torch.from_numpy(zn), idx.cpu(), cs0, w0, m.decay, m.eps)
        assert _ulps(m.ema_cluster_size, ref["N"]).max() <= 1 and _ulps(m.ema_w, ref["m"]).max() <= 1
        assert _ulps(m.embedding.weight, ref["e"]).max() <= 2
        assert not np.array_equal(m.embedding.weight.detach().cpu().numpy(), cb)
    else:
        _, dE = R.l2norm(cb)
        want_gE = R.l2norm_backward(En, dE, gEn.cpu().numpy())
        _same_bits_nan_aside(m.embedding.weight.grad.cpu().numpy(), want_gE, "weight.grad")
        assert float(m.embedding.weight.grad.abs().max()) > 0
    # eval never updates; without grad the cached normalised codebook serves, with the training forward's bits
    m.eval()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    cb2 = m.embedding.weight.detach().cpu().numpy().copy()
    with torch.no_grad():
        loss2, z_q2, ppl2, _, idx2 = m(z0.to(DEV))
    _, En2, c2 = R.quantize(_rows(z0, False), cb2, BETA)
    assert np.array_equal(idx2.view(-1).cpu().numpy(), c2.idx[0])
    _same_bits_nan_aside(_rows(z_q2, False), c2.z_q, "z_q in eval")
    _same_bits_nan_aside(m.normalized_codebook().cpu().numpy(), En2, "normalized_codebook()")
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k
    kept = m.normalized_codebook()
    assert m.normalized_codebook() is kept
    m.invalidate()
    assert m.normalized_codebook() is not kept and torch.equal(m.normalized_codebook(), kept)


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("B,D,H,W,K", SHAPES)
def test_indices_are_the_argmax_of_cosine_similarity(B, D, H, W, K, seed):
    """on rows whose fp64 top-two cosine gap is at least 1e-4 the index is the fp64 argmax of cosine similarity; at most 2 % of the rows
    may be left out (N(0,1) rows against 0.3 N(0,1) codes: 0 - 0.8 % on the CPU at these shapes and seeds).  D = 1 has no angles:
    every cosine is +1 or -1, so rows tie by construction wherever two codes share a sign, and the cap is not asked of it."""
    from vqvae_amd.modules import VectorQuantizer
    N = B * H * W
    x, cb, _ = R.draw(N, D, K, 1.0, 77 + seed)
    m = VectorQuantizer(K, D, BETA, cosine_sim=True).to(DEV)
    with torch.no_grad():
        m.embedding.weight.copy_(torch.from_numpy(cb))
        idx = m.quantize(_layout(x, B, H, W, True), rowmajor=True, want_zq=False)[3].view(-1).cpu().numpy()
    x64, c64 = x.astype(np.float64), cb.astype(np.float64)
    cos = (x64 / np.linalg.norm(x64, axis=1, keepdims=True)) @ (c64 / np.linalg.norm(c64, axis=1, keepdims=True)).T
    top = np.sort(cos, axis=1)
    clear = (top[:, -1] - top[:, -2] >= 1e-4) if K > 1 else np.ones(N, bool)
    print(f"{(~clear).mean() * 100:.2f} % of the rows below the gap")
    if D > 1:
        assert (~clear).mean() <= 0.02
    assert np.array_equal(idx[clear], cos.argmax(1)[clear])


# ---- 4. the model ----------------------------------------------------------------------------------------------------------------

def _model(**kw):
    from vqvae_amd import conv
    from vqvae_amd.modules import VQVAE
    conv.set_conv_backend("hip")
    torch.manual_seed(0)
    m = VQVAE(32, 8, 1, 64, 16, 0.25, **kw).to(DEV)
    with torch.no_grad():
        m.vector_quantization.embedding.weight.copy_(0.3 * torch.randn(64, 16, generator=torch.Generator().manual_seed(9)))
    return m


def _x(B=4):
    return torch.randn(B, 3, 32, 32, generator=torch.Generator().manual_seed(1)).to(DEV)


def test_model_eval_forward_is_encoder_restatement_decoder():
    from vqvae_amd import conv
    m, x = _model(cosine_sim=True).eval(), _x()
    called = []
    m._forward_c = lambda *a, **k: called.append(1)         # the fused whole-path entry quantizes un-normalised z_e: never taken
    with torch.no_grad():
        loss, x_hat, ppl = m(x)
        z_e = conv.encoder_forward(m.encoder, x, pre_quant=m.pre_quantization_conv)           # row-major (B, 8, 8, 16)
        zn, En, c = R.quantize(_rows(z_e, True), m.vector_quantization.embedding.weight.cpu().numpy(), 0.25)
        assert np.abs(np.linalg.norm(c.z_q.astype(np.float64), axis=1) - 1.0).max() <= 2.0 ** -22
        # without a graph the decoder takes the restatement's code rows e^ = E^[idx] themselves (the value of z^ + (e^ - z^) without
        # its last rounding), as decode_indices does; the quantizer's own z_q output stays the straight-through form's bits
        _same_bits_nan_aside(_rows(m.vector_quantization.quantize(z_e, rowmajor=True)[1], True), c.z_q, "quantize()'s z_q")
        want = conv.decoder_forward(m.decoder, _layout(c.e[0], 4, 8, 8, False), rowmajor_in=False)
        idx = m.encode(x)
    assert not called
    assert np.array_equal(_bits(x_hat), _bits(want))
    np.testing.assert_allclose(float(loss), c.loss, rtol=1e-5)
    np.testing.assert_allclose(float(ppl), c.perplexity[0], rtol=1e-5)
    assert np.array_equal(idx.view(-1).cpu().numpy(), c.idx[0])                                # encode(x): the forward's indices
    m.train()
    _, _, ppl_t = m(x)                                                                         # the training forward: the same indices
    np.testing.assert_allclose(float(ppl_t), c.perplexity[0], rtol=1e-5)
    with torch.no_grad():
        assert torch.equal(m.encode(x), idx)


def test_model_decode_indices_of_encode_equals_the_forward():
    """decode_indices(encode(x)) equals the eval forward's x_hat bit for bit: both decode the rows e^ = E^[idx] of the normalised
    codebook through one helper.  The training forward decodes the straight-through form z^ + (e^ - z^), one rounding away from e^,
    and agrees to the plain model's wire-format tolerance."""
    m, x = _model(cosine_sim=True).eval(), _x()
    with torch.no_grad():
        _, x_hat, _ = m(x)
        idx = m.encode(x)
        dec = m.decode_indices(idx, 4, 8, 8)
        En = m.vector_quantization.normalized_codebook()
        from vqvae_amd import conv, functional as F
        want = conv.decoder_forward(m.decoder, F.vq_decode_indices(idx.view(-1), En, 4, 8, 8), rowmajor_in=False)
    assert np.array_equal(_bits(dec), _bits(want))                                             # vq_decode_indices(idx, E^) -> decoder
    diff = (dec - x_hat).abs()
    print(f"decode_indices(encode(x)) vs forward: max |diff| = {float(diff.max()):.3e}, "
          f"{int((_bits(dec) != _bits(x_hat)).sum())} of {dec.numel()} elements differ in their bits")
    with pytest.raises(IndexError):
        m.decode_indices(torch.full_like(idx, 64), 4, 8, 8)
    assert np.array_equal(_bits(dec), _bits(x_hat))
    m.train()
    _, x_hat_train, _ = m(x)                                                                   # decodes z^ + (e^ - z^)
    np.testing.assert_allclose(dec.cpu().numpy(), x_hat_train.detach().cpu().numpy(), atol=1e-6, rtol=1e-5)


@pytest.mark.parametrize("ema", [False, True])
def test_model_training_step_and_cache_rekey(ema):
    m, x = _model(cosine_sim=True, **({"ema_decay": 0.99} if ema else {})).train(), _x()
    vq = m.vector_quantization
    opt = torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=1e-3)
    with torch.no_grad():
        m.eval()
        idx0 = m.encode(x)
        E0 = vq.normalized_codebook()
        m.train()
        v_before = vq.embedding.weight._version
        assert torch.equal(m.encode(x), idx0) and vq.embedding.weight._version == v_before     # encode never updates an EMA codebook
    from vqvae_amd import training as T
    embedding_loss, x_hat, perplexity = m(x)
    stats = T.step_losses(embedding_loss, x_hat, perplexity, x, 0.06)
    stats[1].backward()
    opt.step()
    torch.cuda.synchronize()
    for n, p in m.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    if not ema:
        assert float(vq.embedding.weight.grad.abs().max()) > 0
    assert vq.embedding.weight._version > v_before
    m.eval()
    with torch.no_grad():
        E1 = vq.normalized_codebook()
        assert E1 is not E0 and not torch.equal(E1, E0)                                        # the caches re-key
        _same_bits_nan_aside(E1.cpu().numpy(), R.l2norm(vq.embedding.weight.cpu().numpy())[0], "E^ after the step")
        m(x)
        from vqvae_amd import conv
        z_e = conv.encoder_forward(m.encoder, x, pre_quant=m.pre_quantization_conv)
        zn, En, c = R.quantize(_rows(z_e, True), vq.embedding.weight.cpu().numpy(), 0.25)
        assert np.array_equal(m.encode(x).view(-1).cpu().numpy(), c.idx[0])


def test_model_init_codebook_and_the_default_model():
    m, x = _model(cosine_sim=True).eval(), _x(8)
    v = m.vector_quantization.embedding.weight._version
    m.init_codebook_(x, iters=4, generator=torch.Generator(device=DEV).manual_seed(2))
    assert m.vector_quantization.embedding.weight._version > v
    with torch.no_grad():
        idx = m.encode(x)
    assert idx.unique().numel() > 1
    # with the option off the model is the one built without the keyword
    a, b = _model().eval(), _model(cosine_sim=False).eval()
    with torch.no_grad():
        for p, q in zip(a(x), b(x)):
            assert np.array_equal(_bits(p), _bits(q))
        assert torch.equal(a.encode(x), b.encode(x))
    a.train(), b.train()
    for p, q in zip(a(x), b(x)):
        assert np.array_equal(_bits(p), _bits(q))


# ---- 5. capture ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rowmajor", [True, False])
def test_forward_and_backward_capture_into_a_graph(rowmajor):
    """a linear chain on one stream: l2norm_rows, then l2norm_rows_backward, captured and replayed on new inputs"""
    from vqvae_amd import functional as F
    B, D, H, W, K = 5, 64, 8, 8, 512
    x, cb, g, y, d, gx = _case(B, D, H, W, K, 1.0)
    xs, gs = torch.zeros_like(_layout(x, B, H, W, rowmajor)), torch.zeros_like(_layout(g, B, H, W, rowmajor))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        F.l2norm_rows_backward(*F.l2norm_rows(xs, rowmajor=rowmajor), gs, rowmajor=rowmajor)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y_g, d_g = F.l2norm_rows(xs, rowmajor=rowmajor)
        gx_g = F.l2norm_rows_backward(y_g, d_g, gs, rowmajor=rowmajor)
    xs.copy_(_layout(x, B, H, W, rowmajor))
    gs.copy_(_layout(g, B, H, W, rowmajor))
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        _same_bits_nan_aside(_rows(y_g, rowmajor), y, "replayed y")
        _same_bits_nan_aside(d_g.cpu().numpy(), d, "replayed denom")
        _same_bits_nan_aside(_rows(gx_g, rowmajor), gx, "replayed grad_x")
