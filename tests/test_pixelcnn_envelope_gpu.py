"""The GatedPixelCNN prior at the corners of its documented envelope and at the batches it is measured at, against references:
whole-model forward + backward against the fp64 restatement (tests/pixelcnn_train_ref.py) and the reference's forward
(oracle/pixelcnn_port.py); single kernels at the sizes a B = 1024 step gives them against their defining fp64 sums; the cached
sampler against the reference's forward and the documented draw.  Case tables, planner queries and mirrors, and the ReLU-decision rule:
tests/pixelcnn_envelope.py (tests/test_pixelcnn_envelope_cpu.py asserts which kernel form each case reaches).

Tolerances are the project's own, none is new: gradients, tap sums and conv outputs atol 1e-5 max|ref| + rtol 1e-4 over the whole
tensor (tests/test_training_gpu.py), loss rtol 1e-5, logits atol 2e-4 + rtol 1e-4 (tests/test_pixelcnn.py), cross-entropy loss
rtol 1e-6 + atol 1e-6, the draw's exemption of tests/test_pixelcnn_sample_gpu.py."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import pixelcnn_port
from tests import pixelcnn_envelope as E
from tests import pixelcnn_sample_ref as S
from tests import pixelcnn_train_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ATOL, RTOL = 2e-4, 1e-4                       # tests/test_pixelcnn.py's tolerance for the forward


def _cus():
    return torch.cuda.get_device_properties(DEV).multi_processor_count


def _port_logits(m, x, label, nl):
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        return pixelcnn_port.forward(sd, x.cpu(), label.cpu(), nl)


def _step(m, x, label):
    from vqvae_amd import pixelcnn
    logits = m(x, label)
    logits.retain_grad()
    loss = pixelcnn.cross_entropy(logits, x)
    m.zero_grad(set_to_none=True)
    loss.backward()
    torch.cuda.synchronize()
    return logits.detach(), loss.detach(), logits.grad.detach(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}


# ------------------------------------------------------------------------------------------------------------ A. whole model
@pytest.mark.parametrize("case", list(E.MODEL_CASES))
def test_model_forward_backward_vs_restatement(case):
    """Loss, grad_logits and every parameter gradient (whole tensors) against the fp64 restatement under the device's own ReLU
    decisions (tests/pixelcnn_envelope.py); eval logits against the reference's forward; training logits = eval logits and a
    second backward = the first, bit for bit; non-zero gradients on the mask-'A' taps, exactly zero rows for absent codes.

    Measured on an MI355X (worst |err| / tolerance over all parameter gradients; ReLU decisions that differ from fp64's): see the
    table in DESIGN.md, section 5."""
    K, dim, nl, ncls, B, side = E.MODEL_CASES[case]
    # the wide-form condition with this device's CU count: the batch cases must reach what they are named for here too
    if B >= 505:
        assert E.conv_is_wide(B, side, dim, E.HIDDEN, _cus()) and E.conv_is_wide(B, side, E.HIDDEN, K, _cus()), _cus()
    if B >= 1024 and case != "k512_d64_l15_c10_b1024_s8":
        assert E.conv_is_wide(B, side, dim, 2 * dim, _cus()), _cus()
    m = E.build(K, dim, nl, ncls).to(DEV)
    x, label = E.model_inputs(K, ncls, B, side)
    xd, ld = x.to(DEV), label.to(DEV)
    le = m.eval()(xd, ld)
    t, lh = E.device_hidden(m, xd, ld)
    assert torch.equal(lh, le), "the test's copy of the eval forward has drifted from GatedPixelCNN._forward_eval"
    np.testing.assert_allclose(le.cpu().numpy(), _port_logits(m, x, label, nl).numpy(), atol=ATOL, rtol=RTOL)
    lt, loss, gl, grads = _step(m.train(), xd, ld)
    assert torch.equal(lt, le), "training-mode logits are not the eval logits"
    _, loss2, gl2, grads2 = _step(m, xd, ld)
    assert torch.equal(loss, loss2) and torch.equal(gl, gl2)
    for k in grads:
        assert torch.equal(grads[k], grads2[k]), f"{k}: a second backward gives other bits"
    t_nchw = t.permute(0, 3, 1, 2).cpu()
    del t, lh, lt, gl2, grads2
    state = {k: p.detach().cpu() for k, p in m.named_parameters()}
    keep = {}
    rl, rgl, rgrads = R.loss_and_grads(state, x, label, nl, head_mask=(t_nchw > 0), keep=keep)
    n_diff, r_hidden = E.check_hidden(t_nchw, keep["pre"])
    np.testing.assert_allclose(float(loss), float(rl), rtol=1e-5)
    ratios = {"grad_logits": E.err_ratio(gl, rgl)}
    assert set(rgrads) == set(grads)
    for k in rgrads:
        ratios[k] = E.err_ratio(grads[k], rgrads[k])
    worst = max(ratios, key=ratios.get)
    print(f"\n[envelope A] {case}: ReLU decisions differing {n_diff} of {t_nchw.numel()}, hidden {r_hidden:.3g}, "
          f"worst |err|/tol {ratios[worst]:.3g} ({worst}), grad_logits {ratios['grad_logits']:.3g}")
    bad = {k: round(v, 3) for k, v in ratios.items() if not v <= 1.0}
    assert not bad, f"max |err| / tolerance above 1: {bad}"
    assert float(grads["layers.0.vert_stack.weight"][:, :, -1].abs().max()) > 0
    assert float(grads["layers.0.horiz_stack.weight"][:, :, :, -1].abs().max()) > 0
    absent = np.setdiff1d(np.arange(K), x.numpy().ravel())
    assert np.all(grads["embedding.weight"].cpu().numpy()[absent] == 0)


def test_training_with_k_not_a_multiple_of_4_is_refused():
    """K = 10: the eval forward is the reference's; a training step raises (the head's data gradient needs Cin % 4 == 0), leaves no
    gradient behind, and the next eval forward is still right"""
    from vqvae_amd import pixelcnn
    from vqvae_amd._lib import VqvaeHipError
    K, dim, nl, ncls, B, side = 10, 32, 2, 3, 4, 8
    m = E.build(K, dim, nl, ncls).to(DEV)
    x, label = E.model_inputs(K, ncls, B, side)
    xd, ld = x.to(DEV), label.to(DEV)
    ref = _port_logits(m, x, label, nl).numpy()
    np.testing.assert_allclose(m.eval()(xd, ld).cpu().numpy(), ref, atol=ATOL, rtol=RTOL)
    m.train()
    m.zero_grad(set_to_none=True)
    with pytest.raises(VqvaeHipError):
        pixelcnn.cross_entropy(m(xd, ld), xd).backward()
    torch.cuda.synchronize()
    assert all(p.grad is None for p in m.parameters())
    np.testing.assert_allclose(m.eval()(xd, ld).cpu().numpy(), ref, atol=ATOL, rtol=RTOL)


# ----------------------------------------------------------------------------------------------------------- B. single kernels
def _taps_weight(Cout, Cin, taps, g):
    kh = len({t[0] for t in taps})
    return torch.randn(Cout, Cin, kh, len(taps) // kh, generator=g) * 0.1


@pytest.mark.parametrize("B,side,Cin,Cout,taps", E.TAPS_FORWARD_CASES, ids=lambda v: str(v))
def test_taps_forward_and_data_gradient_wide_form(B, side, Cin, Cout, taps):
    """conv_hip.conv_taps at batches that run the eight-wave form of conv_tile8_bf3_kernel in tap-list mode (ceil(B / 8) *
    ntile / 4 >= CUs; B = 2041 the first such batch, 2041 and 2049 leave one image in the last workgroup; 28 taps: two chained
    slices), and pixelcnn.taps_dgrad with an addend (the same kernels over the negated taps; wide where the forward's Cin gives
    a multiple of four tiles: the 128 -> 256 case) against fp64 shifted sums"""
    from vqvae_amd import conv_hip, pixelcnn
    tl = E.TAPS[taps]
    assert E.conv_is_wide(B, side, Cin, Cout, _cus())
    g = torch.Generator().manual_seed(B + len(tl))
    x = torch.randn(B, side, side, Cin, generator=g)
    w = _taps_weight(Cout, Cin, tl, g)
    bias = torch.randn(Cout, generator=g)
    gy = torch.randn(B, side, side, Cout, generator=g)
    addend = torch.randn(B, side, side, Cin, generator=g)
    wf = w.reshape(Cout, Cin, len(tl)).double()
    xd64, gd64 = x.double(), gy.double()
    ref_y = bias.double().expand(B, side, side, Cout).clone()
    ref_x = addend.double().clone()
    for t, (dy, dx) in enumerate(tl):
        ref_y += E.shift(xd64, dy, dx) @ wf[:, :, t].T
        ref_x += E.shift(gd64 @ wf[:, :, t], -dy, -dx)
    del xd64, gd64
    hold = nn.Module()
    xd, wd, bd = x.to(DEV), w.to(DEV), bias.to(DEV)
    got = conv_hip.conv_taps(xd, hold, wd, bd, tl)
    r_y = E.within(got, ref_y, "y")
    assert torch.equal(got, conv_hip.conv_taps(xd, hold, wd, bd, tl))
    gyd, ad = gy.to(DEV), addend.to(DEV)
    got_x = pixelcnn.taps_dgrad(gyd, hold, wd, tl, addend=ad)
    r_x = E.within(got_x, ref_x, "grad_x")
    assert torch.equal(got_x, pixelcnn.taps_dgrad(gyd, hold, wd, tl, addend=ad))
    print(f"\n[envelope B] taps forward B={B} {Cin}->{Cout} {taps}: y {r_y:.3g}, grad_x {r_x:.3g}")


@pytest.mark.parametrize("B,Cin,Cout", E.CONV1X1_CASES, ids=lambda v: str(v))
def test_head_1x1_wide_form(B, Cin, Cout):
    """the prior's 512-wide 1 x 1 layers on 8 x 8 maps in the eight-wave form (from B = 505): bias + output ReLU, and the mask
    epilogue y = mask > 0 ? conv : 0 of the data-gradient launches"""
    from vqvae_amd import conv_hip
    assert E.conv_is_wide(B, 8, Cin, Cout, _cus())
    g = torch.Generator().manual_seed(B + Cin)
    x = torch.randn(B, 8, 8, Cin, generator=g)
    w = torch.randn(Cout, Cin, 1, 1, generator=g) * (Cin ** -0.5)
    bias = torch.randn(Cout, generator=g) * 0.5
    mask = torch.randn(B, 8, 8, Cout, generator=g)
    pre = x.double() @ w[:, :, 0, 0].double().T + bias.double()
    hold = nn.Module()
    xd, wd, bd, md = x.to(DEV), w.to(DEV), bias.to(DEV), mask.to(DEV)
    amax = float(pre.abs().max())
    got = conv_hip.conv(conv_hip.CONV_1x1, xd, hold, wd, bd, Cin, Cout, conv_hip.RELU_OUT)
    r1 = E.within(got, torch.relu(pre), "relu(conv)", absmax=amax)
    assert torch.equal(got, conv_hip.conv(conv_hip.CONV_1x1, xd, hold, wd, bd, Cin, Cout, conv_hip.RELU_OUT))
    got = conv_hip.conv(conv_hip.CONV_1x1, xd, hold, wd, bd, Cin, Cout, 0)
    r2 = E.within(got, pre, "conv")
    got = conv_hip.conv(conv_hip.CONV_1x1, xd, hold, wd, bd, Cin, Cout, 0, mask=md)
    r3 = E.within(got, pre * (mask > 0), "masked conv", absmax=amax)
    assert torch.equal(got, conv_hip.conv(conv_hip.CONV_1x1, xd, hold, wd, bd, Cin, Cout, 0, mask=md))
    assert bool((got[md <= 0] == 0).all())
    print(f"\n[envelope B] 1x1 B={B} {Cin}->{Cout}: relu {r1:.3g}, plain {r2:.3g}, masked {r3:.3g}")


def _wgrad_check(gy, x, tl, what):
    from vqvae_amd import pixelcnn
    gd, xd = gy.double(), x.double()
    ref = torch.stack([torch.einsum("bhwo,bhwi->oi", gd, E.shift(xd, dy, dx)) for dy, dx in tl], dim=-1)
    gyd, xdev = gy.to(DEV), x.to(DEV)
    got = pixelcnn.taps_wgrad(gyd, xdev, tl)
    assert torch.equal(got, pixelcnn.taps_wgrad(gyd, xdev, tl)), "a second call gives other bits"
    r = E.within(got, ref, what)
    print(f"\n[envelope B] {what}: {r:.3g}")
    return got, ref


@pytest.mark.parametrize("B,H,W,Cin,Cout,taps,ips,ns", E.WGRAD_MAP_CASES, ids=lambda v: str(v))
def test_taps_weight_gradient_map_kernel_many_images_per_split(B, H, W, Cin, Cout, taps, ips, ns):
    """taps_wgrad_map_kernel with `ips` images per split (8 / 8 / 32 at B = 1024, the bench batch; B = 1000: a shorter last split;
    96 -> 192: one and a half 64-wide tiles; B = 257 on 7 x 5: 129 splits, the last of one image) against the fp64 shifted sum"""
    tl = E.TAPS[taps]
    g = torch.Generator().manual_seed(B + len(tl) + Cin)
    x = torch.randn(B, H, W, Cin, generator=g)
    gy = torch.randn(B, H, W, Cout, generator=g)
    _wgrad_check(gy, x, tl, f"wgrad map B={B} {H}x{W} {Cin}->{Cout} {taps} ({ips} images x {ns} splits)")


@pytest.mark.parametrize("pattern", E.WGRAD_PATTERNS)
def test_taps_weight_gradient_map_kernel_image_magnitudes(pattern):
    """per-image magnitudes inside the splits (one image 10^6 larger, all-zero images in the middle of a split, magnitudes falling
    over a split): the kernel's products and sums are plain fp32 without scales, so the tolerance is the same"""
    B, H, W, Cin, Cout, taps = E.WGRAD_PATTERN_CASE
    tl = E.TAPS[taps]
    ips = E.taps_wgrad_plan(B, H, W, Cin, Cout, tl).per_split
    g = torch.Generator().manual_seed(E.WGRAD_PATTERNS.index(pattern))
    fa, fb = E.image_factors(pattern, B, ips)
    x = torch.randn(B, H, W, Cin, generator=g) * fb[:, None, None, None]
    gy = torch.randn(B, H, W, Cout, generator=g) * fa[:, None, None, None]
    _wgrad_check(gy, x, tl, f"wgrad map {pattern}")


@pytest.mark.parametrize("B,H,W,Cin,Cout,taps,nblk,ns", E.WGRAD_BLK_CASES, ids=lambda v: str(v))
def test_taps_weight_gradient_per_tap_kernel(B, H, W, Cin, Cout, taps, nblk, ns):
    """taps_wgrad_blk_kernel: 784 pixel blocks under the 64-split clamp; ragged channels (20 -> 40) with a partly filled last block
    in 3 splits; a 1 x 1 map where every tap but (0, 0) lies outside (exact zeros)"""
    tl = E.TAPS[taps]
    g = torch.Generator().manual_seed(B + H)
    x = torch.randn(B, H, W, Cin, generator=g)
    gy = torch.randn(B, H, W, Cout, generator=g)
    got, ref = _wgrad_check(gy, x, tl, f"wgrad per-tap B={B} {H}x{W} {Cin}->{Cout} {taps}")
    if H == 1 and W == 1:
        outside = [i for i, t in enumerate(tl) if t != (0, 0)]
        assert len(outside) == len(tl) - 1 and bool((got[:, :, outside] == 0).all())
        assert float(got[:, :, tl.index((0, 0))].abs().max()) > 0


@pytest.mark.parametrize("one_code", [False, True], ids=["uniform", "one_code"])
@pytest.mark.parametrize("n,rows,C", E.GATHER_CASES, ids=lambda v: str(v))
def test_gather_backward_at_step_sizes(n, rows, C, one_code):
    """vqvae_gather_rows_backward_f32 at the 65 536 rows of a B = 1024 step (uniform codes: 128 rows per code; one code: one
    segment of 65 536 rows in chunks) and at the class embedding's sizes (1024 images, 1 or 10 classes)"""
    from vqvae_amd import pixelcnn
    g = torch.Generator().manual_seed(n + rows + C)
    idx = torch.randint(0, rows, (n,), generator=g)
    if one_code:
        idx[:] = rows // 2
    go = torch.randn(n, C, generator=g)
    ref = torch.zeros(rows, C, dtype=torch.float64).index_add_(0, idx, go.double())
    got = pixelcnn.gather_rows_backward(idx.to(DEV), go.to(DEV), rows)
    E.within(got, ref, "grad_table")
    untouched = np.setdiff1d(np.arange(rows), idx.numpy())
    assert np.all(got.cpu().numpy()[untouched] == 0)
    assert torch.equal(got, pixelcnn.gather_rows_backward(idx.to(DEV), go.to(DEV), rows))


@pytest.mark.parametrize("P,C", E.BIAS_CASES, ids=lambda v: str(v))
def test_bias_gradient_at_step_sizes(P, C):
    """vqvae_bias_grad_wide_f32: 65 536 rows (the 512-block clamp, 128 rows per block) at widths that divide 256, do not, and
    exceed it; 8192 channels"""
    from vqvae_amd import pixelcnn
    g = torch.Generator().manual_seed(P + C)
    gy = torch.randn(P, C, generator=g) + 0.25
    got = pixelcnn.bias_grad(gy.to(DEV))
    E.within(got, gy.double().sum(0), "grad_b")
    assert torch.equal(got, pixelcnn.bias_grad(gy.to(DEV)))


@pytest.mark.parametrize("B,HW,dim", E.GATE_CASES, ids=lambda v: str(v))
def test_gate_backward_at_step_sizes(B, HW, dim):
    """vqvae_gated_activation_backward_f32 with the class term and accumulation into grad_cond, against autograd in fp64"""
    from vqvae_amd import pixelcnn
    g = torch.Generator().manual_seed(B + HW + dim)
    t1 = torch.randn(B, HW, 1, 2 * dim, generator=g) * 2
    cond = torch.randn(B, 2 * dim, generator=g)
    go = torch.randn(B, HW, 1, dim, generator=g)
    t = t1.double().requires_grad_(True)
    c = cond.double().requires_grad_(True)
    a, gg = (t + c[:, None, None, :]).chunk(2, dim=-1)
    (torch.tanh(a) * torch.sigmoid(gg) * go.double()).sum().backward()

    def run():
        gc = torch.full((B, 2 * dim), 0.5).to(DEV)
        return pixelcnn.gate_backward(t1.to(DEV), cond.to(DEV), go.to(DEV), dim, gc, accumulate=True), gc
    got, gc = run()
    E.within(got, t.grad, "grad_pre")
    E.within(gc, c.grad + 0.5, "grad_cond")
    got2, gc2 = run()
    assert torch.equal(got, got2) and torch.equal(gc, gc2)


@pytest.mark.parametrize("scale", [1.0, 80.0])
@pytest.mark.parametrize("B,K,side", E.CE_CASES, ids=lambda v: str(v))
def test_cross_entropy_at_step_sizes(B, K, side, scale):
    """vqvae_cross_entropy_f32 / _backward_f32: 65 536 rows (the fixed-order mean over many rows), K = 10 (54 idle lanes),
    K = 1000 (a ragged last pass), K = 8192"""
    from vqvae_amd import pixelcnn
    g = torch.Generator().manual_seed(int(scale) + K)
    logits = torch.randn(B, K, side, side, generator=g) * scale
    x = torch.randint(0, K, (B, side, side), generator=g)
    ld = logits.double().requires_grad_(True)
    ref = nn.functional.cross_entropy(ld.permute(0, 2, 3, 1).reshape(-1, K), x.view(-1))
    (ref * 1.5).backward()

    def run():
        lg = logits.to(DEV).requires_grad_(True)
        loss = pixelcnn.cross_entropy(lg, x.to(DEV))
        (loss * 1.5).backward()
        return loss.detach(), lg.grad
    loss, grad = run()
    np.testing.assert_allclose(float(loss), float(ref), rtol=1e-6, atol=1e-6)
    E.within(grad, ld.grad, "grad_logits")
    loss2, grad2 = run()
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)


# ------------------------------------------------------------------------------------------------------------ C. cached sampler
def _sampler_inputs(B, side, ncls, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, ncls, (B,), generator=g).to(DEV), torch.rand((B, side, side), generator=g).to(DEV)


def _check_sampler(m, idx, logits, label, u, nl, what):
    """test_pixelcnn_sample_gpu.py::test_teacher_forced_parity_and_draw's checks on given images"""
    K = logits.shape[1]
    assert int(idx.min()) >= 0 and int(idx.max()) < K
    got = logits.cpu().numpy()
    np.testing.assert_allclose(got, _port_logits(m, idx, label, nl).numpy(), atol=ATOL, rtol=RTOL)
    np.testing.assert_allclose(got, m(idx, label).cpu().numpy(), atol=ATOL, rtol=RTOL)
    want, near = S.inverse_cdf(got, u.cpu().numpy())
    print(f"\n[envelope C] {what}: {int(near.sum())} of {near.size} draws near a CDF boundary (cap {max(4, near.size // 30)})")
    assert near.sum() <= max(4, near.size // 30), f"{near.sum()} of {near.size} draws near a CDF boundary"
    assert np.array_equal(idx.cpu().numpy()[~near], want[~near])


@pytest.mark.parametrize("case", list(E.SAMPLE_CASES))
def test_sampler_corners(case):
    """K = 2 / 3 (idle threads in the draw), K = 513 and 8192 (ragged / 16 logits per thread), dim = 4 and 256 (every thread of the
    per-channel copies), one layer (no Hs carry), sides 1, 16 and 128"""
    K, dim, nl, ncls, B, side, sigma = E.SAMPLE_CASES[case]
    m = E.build(K, dim, nl, ncls, sigma).eval().to(DEV)
    label, u = _sampler_inputs(B, side, ncls)
    idx, logits = m.generate_cached(label, (side, side), B, uniforms=u, return_logits=True)
    assert idx.shape == (B, side, side) and idx.dtype == torch.int64 and logits.shape == (B, K, side, side)
    _check_sampler(m, idx, logits, label, u, nl, case)


def test_sampler_clamps_labels_outside_the_classes():
    K, dim, nl, ncls, B, side, sigma = E.SAMPLE_CASES["k16_d20_l3_c4_b2_s16"]
    m = E.build(K, dim, nl, ncls, sigma).eval().to(DEV)
    _, u = _sampler_inputs(B, side, ncls)
    bad = torch.tensor([-3, ncls + 5], device=DEV)
    i1, l1 = m.generate_cached(bad, (side, side), B, uniforms=u, return_logits=True)
    i2, l2 = m.generate_cached(bad.clamp(0, ncls - 1), (side, side), B, uniforms=u, return_logits=True)
    assert torch.equal(i1, i2) and torch.equal(l1.view(torch.int32), l2.view(torch.int32))


def test_sampler_bench_batch():
    """GatedPixelCNN(512, 64, 15, 10) at B = 1024: 32 images (first, last, a stride coprime to 1024) against the reference, and all
    1024 bit for bit against the same images sampled in batches of one and of 37 (the per-image workspace offsets)"""
    K, dim, nl, ncls, B, side, sigma = E.SAMPLE_BATCH_CASE
    m = E.build(K, dim, nl, ncls, sigma).eval().to(DEV)
    label, u = _sampler_inputs(B, side, ncls)
    idx, logits = m.generate_cached(label, (side, side), B, uniforms=u, return_logits=True)
    pick = torch.tensor(sorted({0, B - 1} | {(37 * i) % B for i in range(1, 31)}), device=DEV)
    assert pick.numel() == 32
    _check_sampler(m, idx[pick], logits[pick], label[pick], u[pick], nl, "B=1024, 32 images")
    for step in (37, 1):
        for b0 in range(0, B, step):
            n = min(step, B - b0)
            i2, l2 = m.generate_cached(label[b0:b0 + n].contiguous(), (side, side), n, uniforms=u[b0:b0 + n].contiguous(),
                                       return_logits=True)
            assert torch.equal(i2, idx[b0:b0 + n]), (step, b0)
            assert torch.equal(l2.view(torch.int32), logits[b0:b0 + n].view(torch.int32)), (step, b0)
