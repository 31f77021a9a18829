"""The rotation-trick gradient on the GPU (vqvae_vq_backward_f32 with VQVAE_VQ_BWD_ROTATION through training.vq_backward, and the
modules' rotation_trick option) against the CPU restatement tests/vq_rotation_ref.py, whose arithmetic is the header of
vqvae_amd/csrc/vq_rotation.hip.

Tier 1: the restatement's bits in both layouts (a NaN compares as a NaN: its payload is not part of any contract).  Tier 2: fp64
torch autograd of the paper's forward, within 2^-24 |ref| + 2^-40 lam ||g|| per element.  Then reproducibility, the equivalences
with the unflagged entry, and the modules."""
import functools

import numpy as np
import pytest
import torch

from tests import vq_rotation_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BETA = 0.25

# (B, D, H, W, K): the smallest call; D = 1 (sign flips give antipodal rows); odd everything, no 16-byte path; N = 105, a partial
# tile and HW % 4 != 0; the flagship row, 320 rows cross a workgroup; D % 4 == 0 and no power of two; the widest
SHAPES = [(1, 1, 1, 1, 1), (3, 1, 7, 5, 4), (3, 3, 5, 3, 7), (3, 64, 7, 5, 64), (5, 64, 8, 8, 512), (2, 48, 8, 8, 96), (2, 256, 4, 4, 32)]
SCALES = [0.05, 1.0]


def _layout(rows, B, H, W, rowmajor):
    z = torch.from_numpy(np.ascontiguousarray(rows)).view(B, H, W, rows.shape[1])
    return (z if rowmajor else z.permute(0, 3, 1, 2)).contiguous().to(DEV)


def _rows(t, rowmajor):
    t = t.detach().cpu()
    t = t if rowmajor else t.permute(0, 2, 3, 1)
    return np.ascontiguousarray(t.contiguous().numpy().reshape(-1, t.shape[-1]))


def _same_bits_nan_aside(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN positions"
    diff = got.view(np.uint32)[~gn] != want.view(np.uint32)[~wn]
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} elements differ in their bits"


@functools.lru_cache(maxsize=None)
def _case(B, D, H, W, K, scale):
    """rows, codebook, g, the indices (the GPU forward's own, then the planted rows re-assigned by hand) and the restatement,
    computed once and left unchanged"""
    from vqvae_amd import functional as F
    N = B * H * W
    z, cb, g = R.draw(N, D, K, scale, 1000 * D + N + int(100 * scale))
    idx = F.vq_forward(_layout(z, B, H, W, True), torch.from_numpy(cb).to(DEV), BETA, rowmajor=True)[3].view(-1).cpu().numpy()
    cb, idx = R.plant_codes(z, cb, idx)
    gl = np.float32(0.7)
    want, rot, rotate = R.grad_z(z, cb, idx, g, gl, np.float32(2.0 / (float(N) * float(D))))
    for a in (z, cb, g, idx, want, rot, rotate):
        a.setflags(write=False)
    return z, cb, g, idx, gl, want, rot, rotate


def _run(z, cb, idx, g, gl, B, H, W, rowmajor, **kw):
    from vqvae_amd import training as T
    gz, ge = T.vq_backward(_layout(z, B, H, W, rowmajor), torch.from_numpy(np.ascontiguousarray(cb)).to(DEV),
                           torch.from_numpy(np.ascontiguousarray(idx)).to(DEV),
                           _layout(g, B, H, W, rowmajor) if g is not None else None,
                           torch.tensor(float(gl), device=DEV) if gl is not None else None, BETA, rowmajor=rowmajor, **kw)
    torch.cuda.synchronize()
    return gz, ge


# ---- 1. bits against the restatement ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("B,D,H,W,K", SHAPES)
def test_bits_against_the_restatement_in_both_layouts(B, D, H, W, K, scale):
    z, cb, g, idx, gl, want, rot, rotate = _case(B, D, H, W, K, scale)
    N = B * H * W
    if N >= 4:
        assert not rotate[:3].any() and rotate.sum() > 0        # the planted zero row, zero code and antipodal row fall back
        assert np.isnan(want[3]).all() and np.isfinite(np.delete(want, 3, axis=0)).all()      # the NaN of g stays in row 3
    if D == 1 and N >= 4:
        assert (~rotate[4:]).sum() > 0                          # antipodal rows by themselves
    for rowmajor in (True, False):
        gz, _ = _run(z, cb, idx, g, gl, B, H, W, rowmajor, need_codebook=False, rotation=True)
        _same_bits_nan_aside(_rows(gz, rowmajor), want, f"rowmajor={rowmajor}")


def test_tensors_offset_by_four_bytes_take_the_element_path_with_the_same_bits():
    from vqvae_amd import training as T
    B, D, H, W, K = 5, 64, 8, 8, 512
    z, cb, g, idx, gl, want, _, _ = _case(B, D, H, W, K, 1.0)

    def off(a):                                             # the same values in a tensor that starts 4 bytes past an aligned address
        buf = torch.empty(a.size + 1, dtype=torch.float32, device=DEV)
        v = buf[1:].view(a.shape)
        v.copy_(torch.from_numpy(np.ascontiguousarray(a)))
        assert v.data_ptr() % 16 == 4 and v.is_contiguous()
        return v

    zt, gt, ct = off(z.reshape(B, H, W, D)), off(g.reshape(B, H, W, D)), off(cb)
    gz, _ = T.vq_backward(zt, ct, torch.from_numpy(idx).to(DEV), gt, torch.tensor(float(gl), device=DEV), BETA, rowmajor=True,
                          need_codebook=False, rotation=True)
    torch.cuda.synchronize()
    _same_bits_nan_aside(_rows(gz, True), want, "offset tensors")


# ---- 2. the independent bound ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("B,D,H,W,K", SHAPES)
def test_within_the_bound_of_fp64_autograd(B, D, H, W, K, scale):
    z, cb, g, idx, gl, want, rot, rotate = _case(B, D, H, W, K, scale)
    # the rotation alone: no loss term (grad_loss = 0 leaves rot + 0 * (z - q) = rot wherever z - q is finite)
    gz, _ = _run(z, cb, idx, g, 0.0, B, H, W, True, need_codebook=False, rotation=True)
    got = _rows(gz, True).astype(np.float64)
    ok = rotate & np.isfinite(g).all(axis=1)
    if not ok.any():
        return
    with np.errstate(all="ignore"):
        ref, lam_g, _ = R.autograd_rot(z[ok], cb[idx[ok]], g[ok])
    err, bnd = np.abs(got[ok] - ref), R.bound(ref, lam_g)
    print(f"max err / bound = {(err / bnd).max():.4f} over {int(ok.sum())} rotated rows")
    assert (err <= bnd).all()


# ---- 3. reproducibility ----------------------------------------------------------------------------------------------------------

def test_same_bits_in_both_layouts_and_in_two_runs():
    B, D, H, W, K = 5, 64, 8, 8, 512
    z, cb, g, idx, gl, *_ = _case(B, D, H, W, K, 1.0)
    runs = [_rows(_run(z, cb, idx, g, gl, B, H, W, rm, need_codebook=False, rotation=True)[0], rm) for rm in (True, False, True, False)]
    for r in runs[1:]:
        _same_bits_nan_aside(r, runs[0], "layouts / runs")


# ---- 4. equivalences, bit for bit ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rowmajor", [True, False])
def test_equivalences_with_the_unflagged_entry(rowmajor):
    B, D, H, W, K = 3, 64, 7, 5, 64
    z, cb, g, idx, gl, want, rot, rotate = _case(B, D, H, W, K, 1.0)
    # flag + grad_zq = None == no flag
    a, _ = _run(z, cb, idx, None, gl, B, H, W, rowmajor, need_codebook=False, rotation=True)
    b, _ = _run(z, cb, idx, None, gl, B, H, W, rowmajor, need_codebook=False)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # grad_codebook with the flag == without it (and grad_z is the restatement's beside it)
    gz1, ge1 = _run(z, cb, idx, g, gl, B, H, W, rowmajor, rotation=True)
    _, ge0 = _run(z, cb, idx, g, gl, B, H, W, rowmajor)
    assert torch.equal(ge1.view(torch.int32), ge0.view(torch.int32))
    _same_bits_nan_aside(_rows(gz1, rowmajor), want, "grad_z beside the codebook gradient")
    # flag | COMMITMENT == the unflagged COMMITMENT call given grad_zq = the restatement's rot
    c, _ = _run(z, cb, idx, g, gl, B, H, W, rowmajor, need_codebook=False, commitment=True, rotation=True)
    d, _ = _run(z, cb, idx, rot, gl, B, H, W, rowmajor, need_codebook=False, commitment=True)
    _same_bits_nan_aside(_rows(c, rowmajor), _rows(d, rowmajor), "commitment")


# ---- 5. modules ------------------------------------------------------------------------------------------------------------------

def _quantizer_pair(cls, **kw):
    torch.manual_seed(3)
    off = cls(64, 16, BETA, **kw).to(DEV)
    on = cls(64, 16, BETA, rotation_trick=True, **kw).to(DEV)
    on.load_state_dict(off.state_dict())
    return off, on


@pytest.mark.parametrize("ema", [False, True])
def test_quantizer_modules_forward_bits_and_rotated_gradient(ema):
    from vqvae_amd.modules import VectorQuantizer, VectorQuantizerEMA
    off, on = _quantizer_pair(VectorQuantizerEMA if ema else VectorQuantizer)
    off.train(), on.train()
    g0 = torch.Generator().manual_seed(5)
    z0 = (0.02 * torch.randn(4, 16, 8, 8, generator=g0)).to(DEV)
    t = torch.randn(4, 16, 8, 8, generator=g0).to(DEV)
    cb = off.embedding.weight.detach().cpu().numpy().copy()
    outs = []
    for m in (off, on):
        z = z0.clone().requires_grad_(True)
        loss, z_q, ppl, _, idx = m(z)
        ((z_q * t).sum() + loss).backward()
        torch.cuda.synchronize()
        outs.append((loss.detach(), z_q.detach(), ppl.detach(), idx, z.grad, m.embedding.weight.grad))
    for a, b in zip(outs[0][:4], outs[1][:4]):
        assert torch.equal(a, b) and (a.dtype != torch.float32 or torch.equal(a.view(torch.int32), b.view(torch.int32)))
    N, D = 256, 16
    scale = np.float32((2.0 * BETA if ema else 2.0) / (float(N) * float(D)))
    want, _, rotate = R.grad_z(_rows(z0, False), cb, outs[1][3].view(-1).cpu().numpy(), _rows(t, False), None, scale)
    assert rotate.all()
    _same_bits_nan_aside(_rows(outs[1][4], False), want, "z.grad with the option on")
    assert not torch.equal(outs[0][4], outs[1][4])
    if ema:
        assert outs[0][5] is None and outs[1][5] is None
        assert torch.equal(off.embedding.weight, on.embedding.weight)                 # the codebook still updates, the same way
        assert not np.array_equal(on.embedding.weight.detach().cpu().numpy(), cb)
        assert torch.equal(off.ema_cluster_size, on.ema_cluster_size) and torch.equal(off.ema_w, on.ema_w)
    else:
        assert torch.equal(outs[0][5].view(torch.int32), outs[1][5].view(torch.int32))
        assert float(outs[1][5].abs().max()) > 0


def test_six_argument_autograd_call_is_todays():
    from vqvae_amd import functional as F, training as T
    z, cb, g, idx, gl, *_ = _case(3, 64, 7, 5, 64, 1.0)
    zt = _layout(z, 3, 7, 5, True).requires_grad_(True)
    w = torch.from_numpy(cb).to(DEV)
    loss, z_q, *_ = T.VQStraightThrough.apply(zt, w, BETA, True, F.vq_workspace(64, 64, DEV), False)
    gt = _layout(np.nan_to_num(g), 3, 7, 5, True)
    (z_q * gt).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(zt.grad, gt)                         # d z_q / d z = I


def test_one_training_step_of_the_model():
    from vqvae_amd import conv, training as T
    from vqvae_amd.modules import VQVAE
    conv.set_conv_backend("hip")
    torch.manual_seed(0)
    off = VQVAE(32, 8, 1, 64, 16, 0.25).to(DEV).train()
    on = VQVAE(32, 8, 1, 64, 16, 0.25, rotation_trick=True).to(DEV).train()
    on.load_state_dict(off.state_dict())
    x = torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(1)).to(DEV)
    res = []
    for m in (off, on):
        embedding_loss, x_hat, perplexity = m(x)
        stats = T.step_losses(embedding_loss, x_hat, perplexity, x, 0.06)
        stats[1].backward()
        torch.cuda.synchronize()
        res.append((embedding_loss.detach(), x_hat.detach(), perplexity.detach(), {n: p.grad for n, p in m.named_parameters()}))
    for a, b in zip(res[0][:3], res[1][:3]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    g0, g1 = res[0][3], res[1][3]
    assert all(v is not None and bool(torch.isfinite(v).all()) for v in g1.values())
    enc = [n for n in g1 if n.startswith(("encoder.", "pre_quantization_conv."))]
    dec = [n for n in g1 if n.startswith("decoder.")]
    assert enc and dec
    assert all(not torch.equal(g0[n], g1[n]) for n in enc)
    assert all(torch.equal(g0[n].view(torch.int32), g1[n].view(torch.int32)) for n in dec)
    n = "vector_quantization.embedding.weight"
    assert torch.equal(g0[n].view(torch.int32), g1[n].view(torch.int32))
