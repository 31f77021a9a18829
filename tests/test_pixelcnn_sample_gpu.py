"""GatedPixelCNN.generate_cached (csrc/pixelcnn_sample.hip) on the GPU: teacher-forced logits against the reference's forward and
the HIP forward, the documented draw, reproducibility and independence of images, the distribution, warm state, errors, and
sample_images."""
import numpy as np
import pytest
import torch

from oracle import pixelcnn_port
from tests import pixelcnn_sample_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ATOL, RTOL = 2e-4, 1e-4                       # tests/test_pixelcnn.py's tolerance for the forward

# (K, dim, n_layers, n_classes, B, side)
CASES = {"k512_dim64_l15_8x8": (512, 64, 15, 10, 4, 8), "k64_dim32_l3_6x6": (64, 32, 3, 5, 3, 6),
         "k256_dim64_l15_28x28": (256, 64, 15, 10, 2, 28), "k64_dim32_l2_64x64": (64, 32, 2, 4, 1, 64)}


def _build(K, dim, nl, ncls, seed=0):
    from vqvae_amd.pixelcnn import GatedPixelCNN
    torch.manual_seed(seed)
    m = GatedPixelCNN(K, dim, nl, ncls).eval()
    with torch.no_grad():
        for n_, p in m.named_parameters():
            if n_.endswith("bias"):
                p.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(len(n_) + seed)) * 0.05)
    return m.to(DEV)


def _inputs(B, side, ncls, seed=3):
    g = torch.Generator().manual_seed(seed)
    label = torch.randint(0, ncls, (B,), generator=g)
    u = torch.rand((B, side, side), generator=g)
    return label.to(DEV), u.to(DEV)


def _check_parity(m, idx, logits, label, nl):
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        ref = pixelcnn_port.forward(sd, idx.cpu(), label.cpu(), nl).numpy()
    got = logits.cpu().numpy()
    np.testing.assert_allclose(got, ref, atol=ATOL, rtol=RTOL)
    hip = m(idx, label).cpu().numpy()
    np.testing.assert_allclose(got, hip, atol=ATOL, rtol=RTOL)


@pytest.mark.parametrize("name", list(CASES))
def test_teacher_forced_parity_and_draw(name):
    K, dim, nl, ncls, B, side = CASES[name]
    m = _build(K, dim, nl, ncls)
    label, u = _inputs(B, side, ncls)
    idx, logits = m.generate_cached(label, (side, side), B, uniforms=u, return_logits=True)
    assert idx.shape == (B, side, side) and idx.dtype == torch.int64
    assert logits.shape == (B, K, side, side)
    assert int(idx.min()) >= 0 and int(idx.max()) < K
    _check_parity(m, idx, logits, label, nl)
    want, near = R.inverse_cdf(logits.cpu().numpy(), u.cpu().numpy())
    got = idx.cpu().numpy()
    # K boundaries, each with a window of 2e-5 of the total: about K * 2e-5 of the draws (1 % at K = 512) are exempt
    assert near.sum() <= max(4, near.size // 30), f"{near.sum()} of {near.size} draws near a CDF boundary"
    assert np.array_equal(got[~near], want[~near])


def test_reproducible_and_images_independent():
    K, dim, nl, ncls, B, side = CASES["k512_dim64_l15_8x8"]
    m = _build(K, dim, nl, ncls)
    B = 6
    label, u = _inputs(B, side, ncls, seed=11)
    i1, l1 = m.generate_cached(label, (side, side), B, uniforms=u, return_logits=True)
    i2, l2 = m.generate_cached(label, (side, side), B, uniforms=u, return_logits=True)
    assert torch.equal(i1, i2)
    assert torch.equal(l1.view(torch.int32), l2.view(torch.int32))
    sub = torch.tensor([4, 1], device=DEV)
    i3, l3 = m.generate_cached(label[sub], (side, side), 2, uniforms=u[sub].contiguous(), return_logits=True)
    assert torch.equal(i3, i1[sub])
    assert torch.equal(l3.view(torch.int32), l1[sub].view(torch.int32))


def test_distribution_is_softmax_of_the_head_bias():
    from scipy.stats import chi2
    K, B, side = 8, 64, 8
    m = _build(K, 16, 3, 2)
    bias = torch.tensor([0.5, -1.0, 0.0, 1.2, -0.3, 0.8, -2.0, 0.1])
    with torch.no_grad():
        for n_, p in m.named_parameters():
            p.zero_()
        m.output_conv[2].bias.copy_(bias.to(DEV))
    gen = torch.Generator(device=DEV).manual_seed(1234)
    idx = m.generate_cached(torch.zeros(B, dtype=torch.int64, device=DEV), (side, side), B, generator=gen)
    counts = np.bincount(idx.cpu().numpy().ravel(), minlength=K)
    expected = torch.softmax(bias.double(), 0).numpy() * idx.numel()
    stat = float(((counts - expected) ** 2 / expected).sum())
    assert stat < chi2.ppf(0.999, K - 1), (stat, counts, expected)


def test_warm_state_adam_step_and_load_state_dict():
    from vqvae_amd.pixelcnn import cross_entropy
    K, dim, nl, ncls, B, side = CASES["k64_dim32_l3_6x6"]
    m = _build(K, dim, nl, ncls)
    label, u = _inputs(B, side, ncls, seed=21)
    i0, l0 = m.generate_cached(label, (side, side), B, uniforms=u, return_logits=True)
    # an Adam step on the HIP training path
    opt = torch.optim.Adam(m.parameters(), lr=1e-2)
    m.train()
    x = torch.randint(0, K, (B, side, side), generator=torch.Generator().manual_seed(2)).to(DEV)
    loss = cross_entropy(m(x, label), x)
    opt.zero_grad()
    loss.backward()
    opt.step()
    m.eval()
    i1, l1 = m.generate_cached(label, (side, side), B, uniforms=u, return_logits=True)
    assert not torch.equal(l1, l0), "the step changed nothing the sampler sees: a stale image"
    _check_parity(m, i1, l1, label, nl)
    # load_state_dict of another model
    other = _build(K, dim, nl, ncls, seed=7)
    m.load_state_dict(other.state_dict())
    i2, l2 = m.generate_cached(label, (side, side), B, uniforms=u, return_logits=True)
    io, lo = other.generate_cached(label, (side, side), B, uniforms=u, return_logits=True)
    assert torch.equal(i2, io) and torch.equal(l2.view(torch.int32), lo.view(torch.int32))
    _check_parity(m, i2, l2, label, nl)


def test_mask_a_junk_has_no_effect_and_is_zeroed():
    K, dim, nl, ncls, B, side = CASES["k64_dim32_l3_6x6"]
    label, u = _inputs(B, side, ncls, seed=31)
    clean = _build(K, dim, nl, ncls)
    i0, l0 = clean.generate_cached(label, (side, side), B, uniforms=u, return_logits=True)
    for warm in (True, False):
        m = clean if warm else _build(K, dim, nl, ncls)
        vs, hs = m.layers[0].vert_stack.weight, m.layers[0].horiz_stack.weight
        vs.data[:, :, -1] = 3.0                              # `.data`: no version bump (weights_init's path)
        hs.data[:, :, :, -1] = -3.0
        i1, l1 = m.generate_cached(label, (side, side), B, uniforms=u, return_logits=True)
        assert torch.equal(i1, i0) and torch.equal(l1.view(torch.int32), l0.view(torch.int32)), warm
        assert float(vs.detach()[:, :, -1].abs().max()) == 0.0 and float(hs.detach()[:, :, :, -1].abs().max()) == 0.0


def test_errors():
    from vqvae_amd._lib import VqvaeHipError
    from vqvae_amd.pixelcnn import GatedPixelCNN
    m = _build(16, 8, 2, 3)
    lab = torch.zeros(2, dtype=torch.int64, device=DEV)
    with pytest.raises(VqvaeHipError):
        m.generate_cached(lab.cpu(), (4, 4), 2)
    with pytest.raises(VqvaeHipError):
        GatedPixelCNN(16, 8, 2, 3).generate_cached(lab, (4, 4), 2)          # module on the CPU
    with pytest.raises(VqvaeHipError):
        m.generate_cached(lab, (4, 6), 2)
    with pytest.raises(VqvaeHipError):
        GatedPixelCNN(16, 6, 2, 3).to(DEV).generate_cached(lab, (4, 4), 2)   # dim % 4
    with torch.no_grad():
        m.output_conv[2].bias[5] = float("nan")
    with pytest.raises(VqvaeHipError, match="non-finite"):
        m.generate_cached(lab, (4, 4), 2)


def test_sample_images_decodes_its_own_indices():
    from vqvae_amd.modules import VQVAE
    from vqvae_amd.pixelcnn import sample_images
    torch.manual_seed(0)
    vq = VQVAE(128, 32, 2, 512, 64, 0.25).eval().to(DEV)
    prior = _build(512, 64, 3, 10)
    label, u = _inputs(4, 8, 10, seed=41)
    idx, x_hat = sample_images(prior, vq, label, (8, 8), 4, uniforms=u)
    assert idx.shape == (4, 8, 8) and x_hat.shape == (4, 3, 32, 32)
    with torch.no_grad():
        ref = vq.decode_indices(idx, 4, 8, 8)
    assert torch.equal(x_hat.view(torch.int32), ref.view(torch.int32))
    assert torch.equal(idx, prior.generate_cached(label, (8, 8), 4, uniforms=u))
