"""GatedPixelCNN.generate_cached's sampling controls on the GPU (csrc/pixelcnn_sample.hip, pixelcnn_sample_kernel<true>):
temperature, top-k and top-p against the fp64 statement of their rules, exact ties and truncation on logits that are known
exactly, given codes (teacher forcing, prefixes, scattered positions), reproducibility, complete_images and the errors."""
import numpy as np
import pytest
import torch

from oracle import pixelcnn_port
from tests import pixelcnn_sample_filter_ref as F

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ATOL, RTOL = 2e-4, 1e-4                       # tests/test_pixelcnn.py's tolerance for the forward

# (K, dim, n_layers, n_classes, B, side): where the draw's thread mapping (512 threads, ceil(K / 512) consecutive codes each) can break
CASES = {"k64": (64, 32, 3, 5, 3, 6),          # fewer codes than threads
         "k512": (512, 64, 15, 10, 4, 8),      # one code per thread; the real model
         "k1000": (1000, 16, 2, 3, 2, 5),      # two codes per thread, a ragged last thread
         "k8192": (8192, 8, 1, 2, 2, 4)}       # the envelope's K, 16 codes per thread
OPTIONS = {"T0.7": dict(temperature=0.7), "k5": dict(top_k=5), "kK-1": dict(top_k=-1), "p0.9": dict(top_p=0.9),
           "T1.3_k40_p0.8": dict(temperature=1.3, top_k=40, top_p=0.8)}


def _options(name, K):
    o = dict(OPTIONS[name])
    if "top_k" in o:
        o["top_k"] = K - 1 if o["top_k"] < 0 else min(o["top_k"], K - 1)
    return o


def _window(K):
    """The share of positions that filtered_draw may exempt is at most 4 K window: K boundaries of width 2 window for the CDF and
    again for the nucleus.  1e-5 gives 2 % at K = 512 and 4 % at K = 1000; at K = 8192 it would give 33 %, so there 1e-6: 3.3 %."""
    return 1e-6 if K > 1000 else 1e-5


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


def _check_draw(idx, logits, u, opts, K, what, free=None):
    """indices equal filtered_draw wherever it does not call the position near a boundary (and, with `free`, where it was drawn)"""
    want, near = F.filtered_draw(logits.cpu().numpy(), u.cpu().numpy(), window=_window(K), **opts)
    got = idx.cpu().numpy()
    cap = max(4, near.size // 15)
    print(f"\n[{what}] {int(near.sum())} of {near.size} draws near a boundary (cap {cap})")
    assert near.sum() <= cap, f"{near.sum()} of {near.size} draws near a boundary"      # a condition on the inputs, not a tolerance
    ok = ~near if free is None else (~near & free)
    assert np.array_equal(got[ok], want[ok]), (what, np.argwhere(ok & (got != want))[:8])


def _bits(t):
    return t.view(torch.int32)


def test_plain_path_unchanged():
    K, dim, nl, ncls, B, side = CASES["k512"]
    m = _build(K, dim, nl, ncls)
    label, u = _inputs(B, side, ncls)
    i0, l0 = m.generate_cached(label, (side, side), B, uniforms=u, return_logits=True)
    for kw in (dict(temperature=1.0, top_k=None, top_p=None, given=None), dict(top_k=K), dict(top_p=1.0), dict(top_k=0),
               dict(top_k=K + 7, top_p=1.0, temperature=1)):
        i1, l1 = m.generate_cached(label, (side, side), B, uniforms=u, return_logits=True, **kw)
        assert torch.equal(i1, i0) and torch.equal(_bits(l1), _bits(l0)), kw
    # the filtered kernel with nothing to filter (every position free) draws the same bits: its e_k are the plain ones
    free = torch.full((B, side, side), -1, dtype=torch.int64, device=DEV)
    i2, l2 = m.generate_cached(label, (side, side), B, uniforms=u, return_logits=True, given=free)
    assert torch.equal(i2, i0) and torch.equal(_bits(l2), _bits(l0))


@pytest.mark.parametrize("opt", list(OPTIONS))
@pytest.mark.parametrize("case", list(CASES))
def test_filtered_draws_follow_the_rule(case, opt):
    K, dim, nl, ncls, B, side = CASES[case]
    opts = _options(opt, K)
    m = _build(K, dim, nl, ncls)
    label, u = _inputs(B, side, ncls)
    idx, logits = m.generate_cached(label, (side, side), B, uniforms=u, return_logits=True, **opts)
    assert idx.shape == (B, side, side) and idx.dtype == torch.int64 and logits.shape == (B, K, side, side)
    assert int(idx.min()) >= 0 and int(idx.max()) < K
    _check_parity(m, idx, logits, label, nl)
    _check_draw(idx, logits, u, opts, K, f"{case} {opt}")


def _bias_model(bias):
    """every parameter zero but the last bias: the logits are the bias, exactly, at every position"""
    m = _build(len(bias), 16, 3, 2)
    with torch.no_grad():
        for p in m.parameters():
            p.zero_()
        m.output_conv[2].bias.copy_(torch.as_tensor(bias, dtype=torch.float32).to(DEV))
    return m


def _bias_counts(bias, **kw):
    B, side = 64, 8
    m = _bias_model(bias)
    gen = torch.Generator(device=DEV).manual_seed(1234)
    idx = m.generate_cached(torch.zeros(B, dtype=torch.int64, device=DEV), (side, side), B, generator=gen, **kw)
    return np.bincount(idx.cpu().numpy().ravel(), minlength=len(bias))


def _chi_square(counts, probs):
    from scipy.stats import chi2
    probs = np.asarray(probs, dtype=np.float64)
    sup = probs > 0
    assert counts[~sup].sum() == 0, counts
    assert (counts[sup] > 0).all(), counts
    expected = probs[sup] / probs[sup].sum() * counts.sum()
    stat = float(((counts[sup] - expected) ** 2 / expected).sum())
    assert stat < chi2.ppf(0.999, sup.sum() - 1), (stat, counts, expected)


def test_exact_ties_and_truncation():
    tied = [1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    # top_k = 2 of three tied maxima: the two lower indices, each with half of the draws
    _chi_square(_bias_counts(tied, top_k=2), [0.5, 0.5, 0, 0, 0, 0, 0, 0])
    # top_k = 4: the three maxima and the first of the tied zeros, at e : e : e : 1
    e = np.e
    _chi_square(_bias_counts(tied, top_k=4), [e, e, e, 1.0, 0, 0, 0, 0])
    # the masses ranked before the codes are 0, 0.5, 0.75, 0.875 of S: top_p = 0.6 keeps {0, 1} at 2/3, 1/3
    p = [0.5, 0.25, 0.125, 0.125]
    nucleus = list(np.log(np.array(p))) + [-20.0] * 4
    _chi_square(_bias_counts(nucleus, top_p=0.6), [0.5, 0.25, 0, 0, 0, 0, 0, 0])
    _chi_square(_bias_counts(nucleus, top_p=0.76), [0.5, 0.25, 0.125, 0, 0, 0, 0, 0])     # of the tied 0.125s the lower index
    # the same probabilities in another index order: ranked by logit, drawn by index
    perm = list(np.log(np.array([0.125, 0.5, 0.125, 0.25]))) + [-20.0] * 4
    _chi_square(_bias_counts(perm, top_p=0.76), [0.125, 0.5, 0, 0.25, 0, 0, 0, 0])
    # temperature on exact logits: log p / 0.5 squares the probabilities
    _chi_square(_bias_counts(nucleus, temperature=0.5, top_k=4), [0.25, 0.0625, 0.015625, 0.015625, 0, 0, 0, 0])


def test_greedy_whatever_the_uniforms():
    B, side = 4, 8
    u = torch.rand((B, side, side), generator=torch.Generator().manual_seed(5))
    u[0, 0, :4] = torch.tensor([0.0, 0.99999994, 0.5, 1e-30])
    lab = torch.zeros(B, dtype=torch.int64, device=DEV)
    idx = _bias_model([1.0, 1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]).generate_cached(lab, (side, side), B, uniforms=u.to(DEV), top_k=1)
    assert int(idx.abs().max()) == 0                                   # the tied maxima: the lowest index
    bias = [0.5, -1.0, 0.0, 1.2, -0.3, 1.25, -2.0, 0.1]
    idx = _bias_model(bias).generate_cached(lab, (side, side), B, uniforms=u.to(DEV), top_k=1)
    assert torch.equal(idx, torch.full_like(idx, 5))


def test_temperature_limit_is_greedy():
    """T = 1e-3 against top_k = 1.  Where the top two logits differ by more than 1e-2, every other code has at most exp(-10) of the
    maximum's mass: with K = 64 less than 0.3 % of the total lies before or after the argmax in the CDF, so a uniform in
    [0.01, 0.99] draws the argmax.  Both runs read the same logits up to an image's first position that does not qualify, so up to
    there the maps must agree; at least 90 % of the positions must qualify (a condition on the model, stated here).
    The condition decides the head's scale: with the Xavier head the 64 logits have a standard deviation of 0.19 and the top two are
    within 1e-2 of each other at one position in six (18 of 108 on the reference's forward).  The gap grows with the logits'
    spread, so the last conv's weight is multiplied by 8 (standard deviation 1.5, about one position in fifty)."""
    K, dim, nl, ncls, B, side = CASES["k64"]
    m = _build(K, dim, nl, ncls)
    with torch.no_grad():
        m.output_conv[2].weight.mul_(8.0)
    label, u = _inputs(B, side, ncls)
    u = 0.01 + 0.98 * u
    ig, lg = m.generate_cached(label, (side, side), B, uniforms=u, return_logits=True, top_k=1)
    it, lt = m.generate_cached(label, (side, side), B, uniforms=u, return_logits=True, temperature=1e-3)
    top2 = lt.permute(0, 2, 3, 1).topk(2, -1).values
    clear = ((top2[..., 0] - top2[..., 1]) > 1e-2).reshape(B, -1).cpu()
    assert torch.equal(it.reshape(B, -1).cpu()[clear], lt.argmax(1).reshape(B, -1).cpu()[clear])
    prefix = clear.long().cumprod(1).bool()                             # before the image's first unclear position
    print(f"\n[temperature limit] {int(clear.sum())} of {clear.numel()} positions clear, {int(prefix.sum())} in the common prefixes")
    assert clear.sum() >= 0.9 * clear.numel(), f"only {int(clear.sum())} of {clear.numel()} positions qualify"
    assert torch.equal(it.reshape(B, -1).cpu()[prefix], ig.reshape(B, -1).cpu()[prefix])
    assert torch.equal(_bits(lt).permute(0, 2, 3, 1).reshape(B, side * side, K).cpu()[prefix],
                       _bits(lg).permute(0, 2, 3, 1).reshape(B, side * side, K).cpu()[prefix])


@pytest.mark.parametrize("case", ["k64", "k512"])
def test_given_full_teacher_forcing(case):
    K, dim, nl, ncls, B, side = CASES[case]
    m = _build(K, dim, nl, ncls)
    label, u = _inputs(B, side, ncls)
    g = torch.Generator().manual_seed(17)
    given = torch.randint(0, K, (B, side, side), generator=g).to(DEV)
    out, logits = m.generate_cached(label, (side, side), B, uniforms=u, return_logits=True, given=given)
    assert torch.equal(out, given)
    _check_parity(m, given, logits, label, nl)
    u2 = torch.rand((B, side, side), generator=g).to(DEV)
    out2, logits2 = m.generate_cached(label, (side, side), B, uniforms=u2, return_logits=True, given=given, top_k=3, temperature=2.0)
    assert torch.equal(out2, given) and torch.equal(_bits(logits2), _bits(logits))
    assert torch.equal(m.generate_cached(label, (side, side), B, uniforms=u2, given=given), given)


@pytest.mark.parametrize("case", ["k64", "k512"])
def test_given_prefix_continues_the_free_draw(case):
    K, dim, nl, ncls, B, side = CASES[case]
    m = _build(K, dim, nl, ncls)
    label, u = _inputs(B, side, ncls)
    i0, l0 = m.generate_cached(label, (side, side), B, uniforms=u, return_logits=True)
    given = i0.clone()
    given[:, side // 2:] = -1
    i1, l1 = m.generate_cached(label, (side, side), B, uniforms=u, return_logits=True, given=given)
    assert torch.equal(i1, i0) and torch.equal(_bits(l1), _bits(l0))
    assert torch.equal(m.generate_cached(label, (side, side), B, uniforms=u, given=given), i0)       # the head skipped where given
    # and with filters: the prefix of a filtered draw continues to the same filtered draw
    opts = dict(temperature=0.8, top_k=20, top_p=0.9)
    j0, k0 = m.generate_cached(label, (side, side), B, uniforms=u, return_logits=True, **opts)
    given = j0.clone()
    given[:, side // 2:] = -1
    j1, k1 = m.generate_cached(label, (side, side), B, uniforms=u, return_logits=True, given=given, **opts)
    assert torch.equal(j1, j0) and torch.equal(_bits(k1), _bits(k0))
    assert torch.equal(m.generate_cached(label, (side, side), B, uniforms=u, given=given, **opts), j0)


@pytest.mark.parametrize("case", ["k64", "k512", "k1000"])
def test_given_scattered(case):
    K, dim, nl, ncls, B, side = CASES[case]
    m = _build(K, dim, nl, ncls)
    label, u = _inputs(B, side, ncls)
    i0 = m.generate_cached(label, (side, side), B, uniforms=u, top_k=5)
    g = torch.Generator().manual_seed(23)
    mask = (torch.rand((B, side, side), generator=g) < 0.5).to(DEV)
    other = (i0 + 1 + torch.randint(0, K - 1, (B, side, side), generator=g).to(DEV)) % K       # never the code that was drawn
    assert not bool((other == i0).any())
    given = torch.where(mask, other, torch.full_like(other, -1))
    out, logits = m.generate_cached(label, (side, side), B, uniforms=u, return_logits=True, given=given, top_k=5)
    assert torch.equal(out[mask], given[mask])
    assert int(out.min()) >= 0 and int(out.max()) < K
    _check_parity(m, out, logits, label, nl)
    _check_draw(out, logits, u, dict(top_k=5), K, f"{case} scattered", free=(~mask).cpu().numpy())
    assert torch.equal(m.generate_cached(label, (side, side), B, uniforms=u, given=given, top_k=5), out)


def test_given_code_out_of_range():
    K, dim, nl, ncls, B, side = CASES["k64"]
    m = _build(K, dim, nl, ncls)
    label, u = _inputs(B, side, ncls)
    given = torch.full((B, side, side), -1, dtype=torch.int64, device=DEV)
    given[1, 2, 3] = K
    with pytest.raises(IndexError):
        m.generate_cached(label, (side, side), B, uniforms=u, given=given)
    given[1, 2, 3] = K - 1
    assert int(m.generate_cached(label, (side, side), B, uniforms=u, given=given)[1, 2, 3]) == K - 1


def test_given_images_independent():
    K, dim, nl, ncls, _, side = CASES["k512"]
    m = _build(K, dim, nl, ncls)
    B = 6
    label, u = _inputs(B, side, ncls, seed=11)
    g = torch.Generator().manual_seed(29)
    given = torch.randint(0, K, (B, side, side), generator=g).to(DEV)
    given[:, 3:] = -1
    given[2] = -1                                                       # one image all free, one all given
    given[5] = torch.randint(0, K, (side, side), generator=g).to(DEV)
    i1, l1 = m.generate_cached(label, (side, side), B, uniforms=u, return_logits=True, given=given, top_p=0.9)
    sub = torch.tensor([4, 1], device=DEV)
    i3, l3 = m.generate_cached(label[sub], (side, side), 2, uniforms=u[sub].contiguous(), return_logits=True,
                               given=given[sub].contiguous(), top_p=0.9)
    assert torch.equal(i3, i1[sub]) and torch.equal(_bits(l3), _bits(l1[sub]))
    sub = torch.tensor([5, 2, 0], device=DEV)
    i4 = m.generate_cached(label[sub], (side, side), 3, uniforms=u[sub].contiguous(), given=given[sub].contiguous(), top_p=0.9)
    assert torch.equal(i4, i1[sub])


def test_batch_above_the_cu_count():
    """A batch with more images than the GPU has CUs runs the filtered kernel's two-workgroups-per-CU form (held to 128 registers):
    the same bits as the same images in batches of 37, which run the other form; the rule on 8 of the images."""
    K, dim, nl, ncls, _, side = CASES["k64"]
    B = torch.cuda.get_device_properties(DEV).multi_processor_count + 44
    m = _build(K, dim, nl, ncls)
    label, u = _inputs(B, side, ncls, seed=13)
    opts = dict(temperature=0.8, top_k=20, top_p=0.9)
    given = torch.randint(0, K, (B, side, side), generator=torch.Generator().manual_seed(31)).to(DEV)
    given[:, 2:] = -1
    given[::3] = -1
    idx, logits = m.generate_cached(label, (side, side), B, uniforms=u, return_logits=True, given=given, **opts)
    for b0 in range(0, B, 37):
        s = slice(b0, min(b0 + 37, B))
        i2, l2 = m.generate_cached(label[s].contiguous(), (side, side), s.stop - s.start, uniforms=u[s].contiguous(),
                                   return_logits=True, given=given[s].contiguous(), **opts)
        assert torch.equal(i2, idx[s]) and torch.equal(_bits(l2), _bits(logits[s])), b0
    pick = torch.tensor([0, 1, 2, 3, B - 4, B - 3, B - 2, B - 1], device=DEV)
    _check_parity(m, idx[pick], logits[pick], label[pick], nl)
    _check_draw(idx[pick], logits[pick], u[pick], opts, K, "B above the CU count", free=(given[pick] < 0).cpu().numpy())
    assert torch.equal(idx[given >= 0], given[given >= 0])


def test_reproducible():
    K, dim, nl, ncls, B, side = CASES["k512"]
    m = _build(K, dim, nl, ncls)
    label, u = _inputs(B, side, ncls, seed=11)
    opts = dict(temperature=0.8, top_k=50, top_p=0.9)
    i1, l1 = m.generate_cached(label, (side, side), B, uniforms=u, return_logits=True, **opts)
    i2, l2 = m.generate_cached(label, (side, side), B, uniforms=u, return_logits=True, **opts)
    assert torch.equal(i1, i2) and torch.equal(_bits(l1), _bits(l2))
    assert torch.equal(m.generate_cached(label, (side, side), B, uniforms=u, **opts), i1)


def test_complete_images():
    from vqvae_amd.modules import VQVAE
    from vqvae_amd.pixelcnn import complete_images
    torch.manual_seed(0)
    vq = VQVAE(128, 32, 2, 512, 64, 0.25).eval().to(DEV)
    prior = _build(512, 64, 3, 10)
    label, u = _inputs(4, 8, 10, seed=41)
    x = torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(43)).to(DEV)
    idx, x_hat = complete_images(prior, vq, x, label, 4, uniforms=u, top_p=0.95)
    assert idx.shape == (4, 8, 8) and idx.dtype == torch.int64 and x_hat.shape == (4, 3, 32, 32)
    with torch.no_grad():
        enc = vq.encode(x).reshape(4, 8, 8)
        ref = vq.decode_indices(idx, 4, 8, 8)
    assert torch.equal(idx[:, :4], enc[:, :4])
    assert torch.equal(_bits(x_hat), _bits(ref))
    given = enc.clone()
    given[:, 4:] = -1
    assert torch.equal(idx, prior.generate_cached(label, (8, 8), 4, uniforms=u, given=given, top_p=0.95))
    assert not torch.equal(idx[:, 4:], enc[:, 4:])                      # the lower half is sampled, not copied


def test_errors():
    m = _build(16, 8, 2, 3)
    lab = torch.zeros(2, dtype=torch.int64, device=DEV)
    free = torch.full((2, 4, 4), -1, dtype=torch.int64, device=DEV)
    assert m.generate_cached(lab, (4, 4), 2, given=free).shape == (2, 4, 4)
    for bad in (free.cpu(), free[:, :3].contiguous(), free[:1], free.to(torch.int32), free.float(), [[-1] * 4] * 4):
        with pytest.raises(ValueError):
            m.generate_cached(lab, (4, 4), 2, given=bad)
    for kw in (dict(temperature=0), dict(temperature=float("inf")), dict(top_k=-1), dict(top_p=0), dict(top_p=1.0001)):
        with pytest.raises(ValueError):
            m.generate_cached(lab, (4, 4), 2, **kw)
