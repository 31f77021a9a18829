"""Every capped-grid kernel that had no test past its launch cap (tests/grid_caps.py: the table, the shapes and the allocator used
here), through the front end its small-shape tests call, at the smallest shape whose unit count exceeds cap * 256 with a last lap
that ends inside a workgroup.

Each test compares every output element with a plain restatement of the operation in fp64 (or, where the operation is exact in
fp32 -- a mask, a gather, a copy, one addition -- bit for bit with torch's own op), evaluated on the device a block at a time where
the tensors are large.  The bound is the one the entry's small-shape test uses, imported from that test's module; no tolerance is
new.  Inputs hold no zeros, the front end's buffers start as NaNs between guards (grid_caps.guarded), and the guards must come back
untouched: a lap that is skipped shows as NaNs, a lap that runs past the end as a broken guard.  The sums get one more case each, a
single value 10^6 times the others in the second lap's range."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import grid_caps as G
from tests import pixelcnn_envelope as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BETA = 0.25
STEP = 1 << 21                                   # rows (or elements) per block of a restatement evaluated on the device


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    bad = got.reshape(-1).view(torch.int32) != want.reshape(-1).view(torch.int32)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements differ, the first at {int(bad.nonzero()[0])}"


def _blocks(n, step=STEP):
    return [slice(a, min(n, a + step)) for a in range(0, n, step)]


# ---------------------------------------------------------------------------------------------------------------- train.hip
@pytest.mark.parametrize("case", list(G.VQB))
def test_vq_backward_grad_z(case):
    """vqb_gradz_kernel past 65536 workgroups in its three forms: grad_z = grad_zq + g 2 / (N D) (z - e_idx) in fp64"""
    from tests.test_training_gpu import GRAD_Z_TOL
    from vqvae_amd import training as T
    B, D, H, W, K, rowmajor, displaced = G.VQB[case]
    N, gen = B * H * W, _gen(1)
    shape = (B, H, W, D) if rowmajor else (B, D, H, W)
    z = G.nan_filled(shape, DEV, 1 if displaced else 0).normal_(generator=gen)
    cb = torch.randn((K, D), device=DEV, generator=gen)
    idx = torch.randint(0, K, (N, 1), device=DEV, generator=gen)
    gzq = torch.randn(shape, device=DEV, generator=gen)
    g = 0.7
    with G.guarded() as guard:
        gz, none = T.vq_backward(z, cb, idx, gzq, torch.tensor(g, device=DEV), BETA, rowmajor=rowmajor, need_codebook=False)
    guard.check(gz)
    assert none is None and gz.shape == z.shape and (gz.data_ptr() % 16 == 0) and (z.data_ptr() % 16 == (4 if displaced else 0))
    c, cb64, ib = g * 2.0 / (float(N) * float(D)), cb.double(), idx.view(B, H, W)
    for s in _blocks(B, STEP // (H * W)):
        e = cb64[ib[s]]                                                   # (b, H, W, D)
        want = gzq[s].double() + c * (z[s].double() - (e if rowmajor else e.permute(0, 3, 1, 2)))
        torch.testing.assert_close(gz[s].double(), want, **GRAD_Z_TOL)


@pytest.mark.parametrize("pattern", G.SUM_PATTERNS)
def test_vq_backward_codebook_gradient(pattern):
    """segsum_keys_kernel past 4096 workgroups through the codebook gradient: grad_E_k = g 2 beta / (N D) (n_k e_k - sum of the
    code's rows) in fp64.  spike: rows and codes of size 1e-3 and one row of 1e3 in the second lap's range"""
    from tests.test_training_gpu import grad_codebook_tol
    from vqvae_amd import training as T
    B, D, H, W, K = G.SEGSUM_VQ
    N, gen = B * H * W, _gen(2)
    small = 1e-3 if pattern == "spike" else 1.0
    z = torch.randn((B, H, W, D), device=DEV, generator=gen) * small
    cb = torch.randn((K, D), device=DEV, generator=gen) * small
    idx = torch.randint(0, K, (N, 1), device=DEV, generator=gen)
    if pattern == "spike":
        z.view(N, D)[4096 * 256 + 100] = 1e3
    g = 0.7
    with G.guarded() as guard:
        none, ge = T.vq_backward(z, cb, idx, None, torch.tensor(g, device=DEV), BETA, rowmajor=True, need_z=False)
    guard.check(ge)
    count = torch.bincount(idx.view(-1), minlength=K).double()
    zsum = torch.zeros((K, D), dtype=torch.float64, device=DEV).index_add_(0, idx.view(-1), z.view(N, D).double())
    want = g * 2.0 * BETA / (float(N) * float(D)) * (count[:, None] * cb.double() - zsum)
    assert none is None and float(want.abs().max()) > 0
    torch.testing.assert_close(ge.double(), want, **grad_codebook_tol(want))


def _recon_case(n, pattern, seed):
    gen = _gen(seed)
    small = 1.0 if pattern == "random" else 1e-3
    x = torch.randn((1, n), device=DEV, generator=gen) * small
    x_hat = torch.randn((1, n), device=DEV, generator=gen) * small
    if pattern == "spike":
        x_hat[0, 4 * (1024 * 256 + 50) + 1] = 1e3                          # a 4-vector of the second lap
    if pattern == "tail_spike":
        x_hat[0, n - 1] = 1e3                                             # the n % 4 tail behind the 4-wide laps
    return x, x_hat


@pytest.mark.parametrize("pattern", G.RECON_PATTERNS)
def test_step_losses_forward(pattern):
    """recon_partial_kernel past its 1024 workgroups, with an n % 4 tail: mean((x_hat - x)^2) / var in fp64"""
    from tests.test_training_gpu import RECON_TOL
    from vqvae_amd import training as T
    n = G.RECON_FORWARD
    x, x_hat = _recon_case(n, pattern, 3)
    el, pp, var = torch.tensor(0.0123, device=DEV), torch.tensor(37.5, device=DEV), 0.0632
    with G.guarded() as guard:
        stats = T.step_losses(el, x_hat, pp, x, var)
    guard.check(stats)
    recon = ((x_hat.double() - x.double()) ** 2).mean() / var
    got = stats.detach().double()
    torch.testing.assert_close(got[0], recon, **RECON_TOL)
    torch.testing.assert_close(got[1], recon + el.double(), **RECON_TOL)
    assert float(stats[2]) == 37.5


def test_step_losses_backward():
    """recon_backward_kernel past 65536 workgroups (and the forward's sum over 16 laps): d loss / d x_hat = 2 (x_hat - x) / (n var)"""
    from tests.test_training_gpu import RECON_GRAD_TOL, RECON_TOL
    from vqvae_amd import training as T
    n = G.RECON_BACKWARD
    x, x_hat = _recon_case(n, "random", 4)
    x_hat.requires_grad_(True)
    el, pp, var = torch.tensor(0.0123, device=DEV, requires_grad=True), torch.tensor(37.5, device=DEV), 0.0632
    with G.guarded() as guard:
        stats = T.step_losses(el, x_hat, pp, x, var)
        stats[1].backward()
    guard.check(stats)
    assert any(words == n for _, words in guard.buffers)              # (the gradient's buffer: autograd may hand on a copy of it)
    recon = ((x_hat.detach().double() - x.double()) ** 2).mean() / var
    torch.testing.assert_close(stats.detach().double()[0], recon, **RECON_TOL)
    assert float(el.grad) == 1.0
    for s in _blocks(n, 1 << 22):
        want = 2.0 * (x_hat.detach()[0, s].double() - x[0, s].double()) / (n * var)
        torch.testing.assert_close(x_hat.grad[0, s].double(), want, **RECON_GRAD_TOL)


# ------------------------------------------------------------------------------------------------------------- backward.hip
def test_relu_backward():
    """relu_backward_kernel past 65536 workgroups of 4-vectors, with an n % 4 tail: the mask, bit for bit"""
    from vqvae_amd import autograd_conv as A
    n, gen = G.RELU_BACKWARD, _gen(5)
    g = torch.randn((n,), device=DEV, generator=gen)
    y = torch.randn((n,), device=DEV, generator=gen)
    with G.guarded() as guard:
        got = A.relu_backward(g, y)
    guard.check(got)
    for s in _blocks(n, 1 << 24):
        _same_bits(got[s], torch.where(y[s] > 0, g[s], torch.zeros((), device=DEV)), f"elements from {s.start}")


# ------------------------------------------------------------------------------------------------------- vq_orthogonal.hip
def test_orthogonal_backward():
    """orth_backward_kernel past 2048 workgroups, from saved sums of the test's own (the forward is not part of this lap): the
    restatement's bits"""
    from tests import vq_orthogonal_ref as R
    from tests.test_vq_orthogonal_gpu import _check
    from vqvae_amd import functional as F
    K, D = G.ORTH_BACKWARD
    rng = np.random.default_rng(6)
    saved = rng.standard_normal((K, D))
    sel = (rng.random(K) < 0.9).astype(np.int32)
    M, gl = int(sel.sum()), np.float32(0.7)
    with G.guarded() as guard:
        got = F.vq_orthogonal_backward(torch.from_numpy(saved).to(DEV), torch.from_numpy(sel).to(DEV),
                                       torch.tensor(M, dtype=torch.int32, device=DEV), torch.tensor(float(gl), device=DEV))
    guard.check(got)
    _check(got, R.backward(saved, sel, M, gl), "grad_rows")


# ---------------------------------------------------------------------------------------------------------- vq_rotation.hip
def _rotation_restated(z, q, g, gs):
    """tests/vq_rotation_ref.py's grad_z, operation for operation, on (n, D) device tensors: fp64 +, *, / and sqrt are one correctly
    rounded IEEE operation each in torch's elementwise kernels as in numpy, and nothing here is fused.  The numpy form takes a
    minute on the 67 M elements of the 4-wide case; test_rotation_gradient holds this copy to the original's bits on its first rows."""
    from tests.vq_rotation_ref import MIN_NS2
    z64, q64, g64 = z.double(), q.double(), g.double()
    n, D = z.shape
    ee, qq, eq, eg, qg = (torch.zeros(n, dtype=torch.float64, device=z.device) for _ in range(5))
    for c in range(D):
        ee = ee + z64[:, c] * z64[:, c]
        qq = qq + q64[:, c] * q64[:, c]
        eq = eq + z64[:, c] * q64[:, c]
        eg = eg + z64[:, c] * g64[:, c]
        qg = qg + q64[:, c] * g64[:, c]
    ne, nq = torch.sqrt(ee), torch.sqrt(qq)
    p = ne * nq
    ns2 = 2.0 + 2.0 * (eq / p)
    rotate = (ee > 0) & (qq > 0) & torch.isfinite(ee) & torch.isfinite(qq) & (ns2 >= MIN_NS2)
    a = (eg / ne + qg / nq) / ns2
    ce = (2.0 * qg) / p - (2.0 * a) / ne
    cq = -((2.0 * a) / nq)
    lam = nq / ne
    rot = torch.empty_like(g)
    for c in range(D):
        rot[:, c] = (lam * ((g64[:, c] + ce * z64[:, c]) + cq * q64[:, c])).float()
    rot[~rotate] = g[~rotate]
    return rot + gs * (z - q), rotate


@pytest.mark.parametrize("case", list(G.ROT))
def test_rotation_gradient(case):
    """rot_gradz_body past 65536 workgroups of rows, 4-wide and element by element: the restatement's bits on every row"""
    from tests import vq_rotation_ref as R
    from tests.test_vq_rotation_gpu import _same_bits_nan_aside
    from vqvae_amd import training as T
    B, D, H, W, K, rowmajor = G.ROT[case]
    assert rowmajor or D == 1                                             # (NCHW with one channel: the rows are the map as it lies)
    N, gen = B * H * W, _gen(7)
    shape = (B, H, W, D) if rowmajor else (B, D, H, W)
    z = torch.randn(shape, device=DEV, generator=gen)
    cb = torch.randn((K, D), device=DEV, generator=gen)
    idx = torch.randint(0, K, (N,), device=DEV, generator=gen)
    gzq = torch.randn(shape, device=DEV, generator=gen)
    gl = np.float32(0.7)
    with G.guarded() as guard:
        gz, none = T.vq_backward(z, cb, idx, gzq, torch.tensor(float(gl), device=DEV), BETA, rowmajor=rowmajor, need_codebook=False,
                                 rotation=True)
    guard.check(gz)
    scale = np.float32(2.0 / (float(N) * float(D)))
    gs = float(np.float32(gl * scale))
    zr, gr, got = z.view(N, D), gzq.view(N, D), gz.view(N, D)
    n0 = 1 << 16
    first, _ = _rotation_restated(zr[:n0], cb[idx[:n0]], gr[:n0], gs)
    want0, _, rotate0 = R.grad_z(zr[:n0].cpu().numpy(), cb.cpu().numpy(), idx[:n0].cpu().numpy(), gr[:n0].cpu().numpy(), gl, scale)
    _same_bits_nan_aside(first.cpu().numpy(), want0, "the device copy of the restatement")
    assert rotate0.any() and (D > 1 or (~rotate0).any())                  # (D = 1: rows antipodal to their codes fall back)
    for s in _blocks(N):
        want, _ = _rotation_restated(zr[s], cb[idx[s]], gr[s], gs)
        assert bool(torch.isfinite(want).all())
        _same_bits(got[s], want, f"rows from {s.start}")


# -------------------------------------------------------------------------------------------------------------- vq_exact.hip
def test_onehot():
    """vq_onehot_kernel past 4096 workgroups: torch's scatter, bit for bit"""
    from vqvae_amd import functional as F
    N, K = G.ONEHOT
    idx = torch.randint(0, K, (N, 1), device=DEV, generator=_gen(8))
    with G.guarded() as guard:
        got = F.vq_onehot(idx, K)
    guard.check(got)
    _same_bits(got, torch.zeros((N, K), device=DEV).scatter_(1, idx, 1), "onehot")


def test_decode_indices():
    """vq_decode_indices_kernel past 4096 workgroups: the code rows as NCHW maps, bit for bit"""
    from vqvae_amd import functional as F
    B, D, H, W, K = G.DECODE_INDICES
    gen = _gen(9)
    cb = torch.randn((K, D), device=DEV, generator=gen)
    idx = torch.randint(0, K, (B * H * W,), device=DEV, generator=gen)
    with G.guarded() as guard:
        got = F.vq_decode_indices(idx, cb, B, H, W)
    guard.check(got)
    _same_bits(got, cb[idx.view(B, H, W)].permute(0, 3, 1, 2).contiguous(), "z_q")


# ----------------------------------------------------------------------------------------------------- model.hip, conv.hip
def _decoder_reference(m, idx, B, h4, w4, nl):
    from oracle import torch_port
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    cb = sd["vector_quantization.embedding.weight"]
    z_q = cb[idx.cpu().view(B, h4, w4)].permute(0, 3, 1, 2).contiguous()
    with torch.no_grad():
        return torch_port.decode(sd, z_q, nl).numpy()


def test_decode_gathers_rows_and_clears_maxima():
    """VQVAE.decode_indices on 4 x 4 latent maps (no gathering decoder kernel there): decode_gather_kernel past 65536 workgroups
    writes z_q into the workspace, and the per-image maxima the layers hand on are cleared by fill_words_kernel past its 1024
    workgroups.  The second lap of that clear is the last 61 images' z_q maxima and every image's maximum in front of the last
    layer.  A maximum that was not cleared keeps what the workspace held (here the NaN pattern, which no atomicMax of a finite
    float's bits replaces), and its consumer then forms its fp16 operand terms unscaled.  So the codes are of size 1e6: in front of
    the last layer every image then has values beyond fp16's 65504 (asserted on the reference's own activations), which an unscaled
    term turns into an infinity.  Every image against the reference's decoder on the gathered rows, at the whole path's bound for
    images of their own magnitude (tests/test_model_gpu.py, close_per_image)."""
    import torch.nn.functional as F
    from oracle import torch_port
    from tests.test_model_gpu import close_per_image
    from vqvae_amd import conv
    from vqvae_amd.modules import VQVAE
    conv.set_conv_backend("hip")
    h, rh, nl, K, D, B, h4, w4 = G.DECODE_MODEL
    torch.manual_seed(10)
    m = VQVAE(h, rh, nl, K, D, 0.25).eval()
    with torch.no_grad():
        m.vector_quantization.embedding.weight.copy_(torch.randn(K, D) * 1e6)
    idx = torch.randint(0, K, (B * h4 * w4,), generator=torch.Generator().manual_seed(10))
    ref = _decoder_reference(m, idx, B, h4, w4, nl)
    # the premise, on the first and last images: torch_port.decode's layers up to the last one's input
    sd, Dk = {k: v.detach().clone() for k, v in m.state_dict().items()}, torch_port.Dk
    some = torch.cat([idx.view(B, h4, w4)[:64], idx.view(B, h4, w4)[-64:]])
    with torch.no_grad():
        t = F.conv_transpose2d(sd["vector_quantization.embedding.weight"][some].permute(0, 3, 1, 2).contiguous(), sd[Dk + "0.weight"],
                               sd[Dk + "0.bias"], 1, 1)
        t = torch_port.residual_stack(t, sd[Dk + "1.stack.0.res_block.1.weight"], sd[Dk + "1.stack.0.res_block.3.weight"], nl)
        t = F.relu(F.conv_transpose2d(t, sd[Dk + "2.weight"], sd[Dk + "2.bias"], 2, 1))
    assert float(t.amax(dim=(1, 2, 3)).min()) > 2 * 65504.0
    md = m.to(DEV)
    with G.guarded() as guard:
        x_hat = md.decode_indices(idx.to(DEV), B, h4, w4)
    guard.check(x_hat)
    close_per_image(x_hat.cpu().numpy(), ref)


@pytest.mark.parametrize("where", list(G.ABSMAX_AT))
def test_image_maximum_in_the_last_lap(where):
    """act_absmax_kernel on one image of more than 64 * 16384 4-vectors: z_q's maximum, 1000 times every other value, sits in the
    last lap of the image's 64 parts, or in its very last 4-vector.  The decoder's first layer scales its fp16 operands by that
    maximum: missed, the large value overflows.  x_hat against the reference's decoder at the conv layers' bound
    (test_large_and_odd_shapes_stagewise_vs_oracle's for x_hat).  (The kernel's scalar tail cannot be reached: tests/grid_caps.py.)"""
    from tests.test_conv_gpu import close
    from vqvae_amd import conv
    from vqvae_amd.modules import VQVAE
    conv.set_conv_backend("hip")
    h, rh, nl, K, D, h4, w4 = G.ABSMAX_MODEL
    pixel, channel = G.ABSMAX_AT[where]
    n = h4 * w4 * D
    lap = 64 * 256 * 4
    assert n % 4 == 0 and n // lap * lap <= pixel * D + channel < n and (where != "last_vector" or pixel * D + channel == n - 1)
    torch.manual_seed(11)
    m = VQVAE(h, rh, nl, K, D, 0.25).eval()
    with torch.no_grad():
        cb = torch.randn(K, D)
        cb[K - 1] = 0.01
        cb[K - 1, channel] = 1000.0
        m.vector_quantization.embedding.weight.copy_(cb)
    idx = torch.randint(0, K - 1, (h4 * w4,), generator=torch.Generator().manual_seed(11))
    idx[pixel] = K - 1
    ref = _decoder_reference(m, idx, 1, h4, w4, nl)
    md = m.to(DEV)
    with G.guarded() as guard:
        x_hat = md.decode_indices(idx.to(DEV), 1, h4, w4)
    guard.check(x_hat)
    close(x_hat.cpu().numpy(), ref)


# -------------------------------------------------------------------------------------------------------------- pixelcnn.hip
def test_prior_gather_rows():
    """gather_rows_kernel past 65536 workgroups: torch's row gather, bit for bit"""
    from vqvae_amd import pixelcnn as P
    n, rows, C = G.PRIOR_GATHER
    gen = _gen(12)
    table = torch.randn((rows, C), device=DEV, generator=gen)
    idx = torch.randint(0, rows, (n,), device=DEV, generator=gen)
    with G.guarded() as guard:
        got = P._gather_rows(idx, table)
    guard.check(got)
    for s in _blocks(n, 1 << 22):
        _same_bits(got[s], table[idx[s]], f"rows from {s.start}")


def test_prior_im2col():
    """im2col_rows_kernel past 65536 workgroups: every tap's shifted copy (zero outside the map), bit for bit"""
    from vqvae_amd import pixelcnn as P
    B, H, W, C, taps = G.PRIOR_IM2COL
    tl = E.TAPS[taps]
    x = torch.randn((B, H, W, C), device=DEV, generator=_gen(13))
    with G.guarded() as guard:
        got = P._im2col(x, tl)
    guard.check(got)
    assert got.shape == (B, H, W, len(tl) * C)
    for t, (dy, dx) in enumerate(tl):
        _same_bits(got[..., t * C:(t + 1) * C], E.shift(x, dy, dx), f"tap {t}")


def test_prior_gate():
    """gated_activation_kernel past 65536 workgroups: tanh(a) sigmoid(g) of (a | g) = t1 + t2 + cond[b] in fp64, at the house
    tolerance of the prior's kernels (tests/pixelcnn_envelope.py)"""
    from vqvae_amd import pixelcnn as P
    B, HW, dim = G.PRIOR_GATE
    gen = _gen(14)
    t1 = torch.randn((B, 1, HW, 2 * dim), device=DEV, generator=gen)
    t2 = torch.randn((B, 1, HW, 2 * dim), device=DEV, generator=gen)
    cond = torch.randn((B, 2 * dim), device=DEV, generator=gen)
    with G.guarded() as guard:
        got = P._gate(t1, t2, cond, dim)
    guard.check(got)
    a, g = (t1.double() + t2.double() + cond.double()[:, None, None, :]).chunk(2, dim=-1)
    E.within(got, torch.tanh(a) * torch.sigmoid(g), "gate")


def test_prior_add():
    """add_kernel past 65536 workgroups of 4-vectors: one fp32 addition per element, bit for bit"""
    from vqvae_amd import pixelcnn as P
    n, gen = G.PRIOR_ADD, _gen(15)
    a = torch.randn((n,), device=DEV, generator=gen)
    b = torch.randn((n,), device=DEV, generator=gen)
    with G.guarded() as guard:
        got = P._add(a, b)
    guard.check(got)
    for s in _blocks(n, 1 << 24):
        _same_bits(got[s], a[s] + b[s], f"elements from {s.start}")


@pytest.mark.parametrize("pattern", G.SUM_PATTERNS)
def test_gather_rows_backward(pattern):
    """segsum_keys_kernel past 4096 workgroups through the embedding's backward: the rows' fp64 sums per index"""
    from vqvae_amd import pixelcnn as P
    n, rows, C = G.SEGSUM_GATHER
    gen = _gen(16)
    idx = torch.randint(0, rows, (n,), device=DEV, generator=gen)
    go = torch.randn((n, C), device=DEV, generator=gen) * (1e-3 if pattern == "spike" else 1.0)
    if pattern == "spike":
        go[4096 * 256 + 100] = 1e3
    with G.guarded() as guard:
        got = P.gather_rows_backward(idx, go, rows)
    guard.check(got)
    E.within(got, torch.zeros((rows, C), dtype=torch.float64, device=DEV).index_add_(0, idx, go.double()), "grad_table")


# -------------------------------------------------------------------------------------------------------------- conv_res.hip
def test_residual_layer_outside_the_fused_widths():
    """res_combine_kernel past 8192 workgroups: a residual layer of 4 channels (3 x 3 conv, 1 x 1 conv, then the skip in one more
    pass) on 32769 maps of 8 x 8, every element against the reference's layer at the conv layers' bound"""
    from oracle import torch_port
    from tests.test_conv_gpu import close
    from vqvae_amd import conv_hip
    from vqvae_amd.modules import ResidualStack
    C, Rh, B, H, W = G.RES_COMBINE
    torch.manual_seed(17)
    rs = ResidualStack(C, C, Rh, 1)
    x = torch.randn(B, C, H, W)
    w1, w2 = rs.stack[0].res_block[1].weight.detach(), rs.stack[0].res_block[3].weight.detach()
    ref = torch_port.residual_stack(x.clone(), w1, w2, 1).numpy()
    rsd = rs.to(DEV)
    t = conv_hip.nchw_to_rows(x.to(DEV))
    with G.guarded() as guard:
        y = conv_hip.res_layer(t, rsd.stack[0], 1 | 2)                    # relu_in | relu_out == a 1-layer stack
    guard.check(y)
    close(conv_hip.rows_to_nchw(y).cpu().numpy(), ref)


# ------------------------------------------------------------------------------------------- weight images: conv_ends.hip, conv.hip
def test_first_layer_weight_images():
    """conv_in_pack_kernel and conv_in_pack_bf3_kernel past their 16 workgroups (3 -> 96 channels: 4608 elements each): the first
    layer on images packed that way, through tests/test_conv_gpu.py's own check against torch's CPU op"""
    from tests import test_conv_gpu as TC
    with G.guarded() as guard:
        TC.test_conv_in_vs_torch_cpu(*G.CONV_IN_PACK)
    guard.check()


def test_last_layer_weight_images():
    """convt_out_pack_kernel and convt_out_pack_bf3_kernel past their 32 workgroups (160 -> 3 channels: 10240 elements)"""
    from tests import test_conv_gpu as TC
    torch.manual_seed(18)
    with G.guarded() as guard:
        TC.convt_out_case(*G.CONVT_OUT_PACK)
    guard.check()


def test_conv_weight_image():
    """conv_pack_images_kernel past 4096 workgroups (3 x 3, 352 -> 352 channels: 1 115 136 elements per image), read back by the
    three product schemes' kernels, through tests/test_conv_gpu.py's own check against torch's CPU op"""
    from tests import test_conv_gpu as TC
    kind, Cin, Cout, B, H, W = G.CONV_PACK
    case = (kind, lambda ci, co: nn.Conv2d(ci, co, 3, 1, 1), B, Cin, Cout, H, W)
    for exact in (0, 4, 8):
        with G.guarded() as guard:
            TC.test_conv_layer_vs_torch_cpu(case, False, False, exact)
        guard.check()


def test_taps_data_gradient_staging():
    """taps_transpose_kernel past 4096 workgroups: the data gradient of a 28-tap masked conv, 252 -> 504 channels (two slices of 14
    taps, 1 778 112 staged weights each), against fp64 shifted sums at the house tolerance"""
    from vqvae_amd import pixelcnn as P
    B, side, Cin, Cout, taps = G.TAPS_DGRAD
    tl = E.TAPS[taps]
    g = torch.Generator().manual_seed(19)
    w = torch.randn(Cout, Cin, 4, 7, generator=g) * 0.1
    gy = torch.randn(B, side, side, Cout, generator=g)
    wf, gd = w.reshape(Cout, Cin, len(tl)).double(), gy.double()
    ref = torch.zeros(B, side, side, Cin, dtype=torch.float64)
    for t, (dy, dx) in enumerate(tl):
        ref += E.shift(gd @ wf[:, :, t], -dy, -dx)
    with G.guarded() as guard:
        got = P.taps_dgrad(gy.to(DEV), nn.Module(), w.to(DEV), tl)
    guard.check(got)
    E.within(got, ref, "grad_x")


def test_taps_weight_gradient_split_reduce():
    """split_reduce_kernel past 4096 workgroups: the weight gradient of a 28-tap masked conv, 204 -> 188 channels (1 073 856
    elements), through tests/test_pixelcnn_envelope_gpu.py's own check against the fp64 shifted sums"""
    from tests.test_pixelcnn_envelope_gpu import _wgrad_check
    B, H, W, Cin, Cout, taps = G.TAPS_WGRAD
    g = torch.Generator().manual_seed(20)
    x = torch.randn(B, H, W, Cin, generator=g)
    gy = torch.randn(B, H, W, Cout, generator=g)
    with G.guarded() as guard:
        got, _ = _wgrad_check(gy, x, E.TAPS[taps], f"wgrad {Cin}->{Cout} {taps}")
    guard.check(got)


def test_sampler_weight_image():
    """pixelcnn_sample_pack_kernel past 4096 workgroups (dim = 252: layer 0's vertical stack is 504 x 21 x 252 = 2 667 168 weights):
    the cached sampler on that image, through tests/test_pixelcnn_envelope_gpu.py's own checks"""
    from tests.test_pixelcnn_envelope_gpu import _check_sampler, _sampler_inputs
    K, dim, nl, ncls, B, side, sigma = G.SAMPLE_PACK
    m = E.build(K, dim, nl, ncls, sigma).eval().to(DEV)
    label, u = _sampler_inputs(B, side, ncls)
    with G.guarded() as guard:
        idx, logits = m.generate_cached(label, (side, side), B, uniforms=u, return_logits=True)
    guard.check(idx, logits)
    assert idx.shape == (B, side, side) and logits.shape == (B, K, side, side)
    _check_sampler(m, idx, logits, label, u, nl, "dim = 252")


# ----------------------------------------------------------------------------------------------------------- vq_generic.hip
@pytest.mark.parametrize("vector_units", [False, True], ids=["mfma_fp32", "vector_units"])
def test_any_width_quantizers_lap_their_persistent_grids(vector_units):
    """vq_anyd_kernel (1094 tiles of 64 rows on at most 4 CUs' worth of workgroups) and vq_generic_kernel (8751 tiles of 8 rows on
    8 CUs' worth): 70003 rows of 3 channels, through tests/test_vq_generic_gpu.py's own check against the C oracle"""
    from tests import test_vq_generic_gpu as TG
    with G.guarded() as guard:
        TG.test_vq_generic_matches_oracle_fresh(*G.VQ_ANYD, vector_units)
    guard.check()
