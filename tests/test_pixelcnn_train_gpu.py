"""GatedPixelCNN training on the HIP path (pixelcnn/gated_pixelcnn.py:78-111): the reference's train() body on the mirror module,
parameter gradients against the reference's recorded autograd (tests/golden/pixelcnn_train_cases.npz, tools/gen_golden_pixelcnn_train.py:
tensors of more than 1024 elements are recorded at 1024 seeded positions plus the mask-'A' taps and absent-code rows, with the whole
tensor's maximum for the atol; every element of every gradient is checked against the fp64 restatement at default sizes below),
the new kernels against fp64 CPU definitions, and bitwise reproducibility.

Tolerances.  Gradients: the house tolerance of tests/test_training_gpu.py, atol 1e-5 max|g| + rtol 1e-4 per tensor.  The HIP forward
forms its conv products from exact three-term bf16 splits (fp32-grade, tests/test_pixelcnn.py), the weight gradients are exact fp32
MFMA products and every reduction runs in fp32 / fp64 -- the differences to the reference's CPU autograd are reordered fp32 sums.
The 3-step loss trajectory: rtol 1e-5 (a mean over B H W rows of fp32 logits).  Parameters after 3 Adam steps: Adam moves an element
by about lr per step whatever its gradient's size, so an element whose gradient is at the level of the reordering differences may move
the other way: the bound is atol 1e-5 + rtol 1e-4 for all but 0.1 % of the recorded elements, and 6 lr for every one."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import pixelcnn_train_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
DEV = torch.device("cuda:0")
LR = 3e-4


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "pixelcnn_train_cases.npz"))


def _build(name, dims=None):
    from vqvae_amd.pixelcnn import GatedPixelCNN
    K, dim, nl, ncls = dims or R.CASES[name][:4]
    torch.manual_seed(0)
    m = GatedPixelCNN(K, dim, nl, ncls)
    R.perturb_biases(m)
    return m.to(DEV).train()


def _within(got, ref, what, absmax=None):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    lim = R.tolerance(ref, absmax)
    ratio = float((np.abs(got - ref) / lim).max())
    assert ratio <= 1.0, f"{what}: max |err| / tolerance = {ratio:.3g}"


def _vs_golden(golden, path, got):
    """got (the full tensor) at the golden's stored positions, against the stored values (tests/pixelcnn_train_ref.py::store)"""
    g, ref, amax = R.at_stored(golden, path, got)
    _within(g, ref, path, amax)
    assert abs(float(np.abs(got).max()) - amax) <= 1.1e-4 * amax, f"{path}: max |g|"         # the whole tensor's maximum


def _step_grads(m, x, label):
    K = m.output_conv[2].weight.shape[0]
    logits = m(x, label)
    logits.retain_grad()
    loss = nn.CrossEntropyLoss()(logits.permute(0, 2, 3, 1).contiguous().view(-1, K), x.view(-1))
    m.zero_grad()
    loss.backward()
    torch.cuda.synchronize()
    return loss.detach(), logits.grad.detach(), {k: p.grad.detach().clone() for k, p in m.named_parameters()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(R.CASES))
def test_reference_train_body_runs_on_the_mirror(name, golden):
    """gated_pixelcnn.py:78-99 as written (criterion, zero_grad, backward, Adam step) on the mirror: the 3-step loss trajectory of the
    reference, and for the small case its parameters afterwards."""
    K = R.CASES[name][0]
    model = _build(name)
    criterion = nn.CrossEntropyLoss().cuda()
    opt = torch.optim.Adam(model.parameters(), lr=LR)
    train_loss = []
    for x, label in R.train_batches(name):
        x = x.cuda()
        label = label.cuda()
        logits = model(x, label)
        logits = logits.permute(0, 2, 3, 1).contiguous()
        loss = criterion(
            logits.view(-1, K),
            x.view(-1)
        )
        opt.zero_grad()
        loss.backward()
        opt.step()
        train_loss.append(loss.item())
    np.testing.assert_allclose(train_loss, golden[f"{name}/traj_loss"], rtol=1e-5)
    if name == "k64_dim32_l3":
        for k, p in model.named_parameters():
            got, ref, _ = R.at_stored(golden, f"{name}/final/{k}", p.detach().cpu().numpy())
            err = np.abs(got - ref)
            assert err.max() <= 6 * LR, k
            assert np.mean(err > 1e-5 + 1e-4 * np.abs(ref)) <= 1e-3, k


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(R.CASES))
def test_parameter_gradients_vs_reference(name, golden):
    model = _build(name)
    x, label = R.inputs(name)
    loss, gl, grads = _step_grads(model, x.to(DEV), label.to(DEV))
    np.testing.assert_allclose(float(loss), float(golden[f"{name}/loss"]), rtol=1e-5)
    _vs_golden(golden, f"{name}/grad_logits", gl.cpu().numpy())
    for k in R.stored_names(golden, f"{name}/grad/"):
        _vs_golden(golden, f"{name}/grad/{k}", grads[k].cpu().numpy())
    # mask 'A': the zeroed taps still get the reference's nonzero gradient
    assert float(grads["layers.0.vert_stack.weight"][:, :, -1].abs().max()) > 0
    assert float(grads["layers.0.horiz_stack.weight"][:, :, :, -1].abs().max()) > 0
    # absent codes: exactly zero rows
    absent = np.setdiff1d(np.arange(R.CASES[name][0]), x.numpy().ravel())
    assert np.all(grads["embedding.weight"].cpu().numpy()[absent] == 0)


@pytest.mark.gpu
def test_training_logits_are_the_eval_logits():
    """same kernels, same sums: training-mode logits equal eval-mode logits bit for bit; eval / no_grad outputs need no grad"""
    model = _build("k512_dim64_l15")
    x, label = R.inputs("k512_dim64_l15")
    x, label = x.to(DEV), label.to(DEV)
    lt = model.train()(x, label)
    assert lt.requires_grad
    le = model.eval()(x, label)
    assert not le.requires_grad
    with torch.no_grad():
        ln = model.train()(x, label)
    assert not ln.requires_grad
    assert torch.equal(lt.detach(), le) and torch.equal(le, ln)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [4, 1024])
def test_gradients_are_bit_reproducible(B):
    """no floating-point atomics: two backward passes give the same bits (B = 1024 at 8 x 8: multi-split reductions)"""
    model = _build(None, (512, 64, 15, 10))
    g = torch.Generator().manual_seed(B)
    x = torch.randint(0, 512, (B, 8, 8), generator=g).to(DEV)
    label = torch.randint(0, 10, (B,), generator=g).to(DEV)
    _, _, g1 = _step_grads(model, x, label)
    _, _, g2 = _step_grads(model, x, label)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


def _shift(xd, dy, dx):
    B, H, W, Cc = xd.shape
    sh = torch.zeros_like(xd)
    ys, ye = max(0, -dy), min(H, H - dy)
    xs, xe = max(0, -dx), min(W, W - dx)
    if ys < ye and xs < xe:
        sh[:, ys:ye, xs:xe] = xd[:, ys + dy:ye + dy, xs + dx:xe + dx]
    return sh


TAP_CASES = [
    (5, 8, 8, 64, 128, [(ky - 1, kx - 1) for ky in range(2) for kx in range(3)]),
    (5, 8, 8, 64, 128, [(0, kx - 1) for kx in range(2)]),
    (3, 8, 8, 32, 64, [(0, kx - 3) for kx in range(4)]),
    (2, 6, 6, 32, 64, [(ky - 1, kx - 1) for ky in range(2) for kx in range(3)]),
    (2, 5, 7, 16, 24, [(-2, 3), (0, 0), (1, -1)]),
    (3, 8, 8, 64, 128, [(ky - 3, kx - 3) for ky in range(4) for kx in range(7)]),
    (2, 6, 6, 32, 64, [(ky - 3, kx - 3) for ky in range(4) for kx in range(7)]),
    (2, 16, 12, 32, 64, [(ky - 1, kx - 1) for ky in range(2) for kx in range(3)]),     # beyond 8 x 8: the per-tap kernel
]


@pytest.mark.gpu
@pytest.mark.parametrize("B,H,W,Cin,Cout,taps", TAP_CASES)
def test_taps_weight_and_data_gradient_vs_shifted_sum(B, H, W, Cin, Cout, taps):
    """vqvae_conv_taps_wgrad_f32: grad_w[co][ci][t] = sum gy[.., co] x[shifted by tap t, ci], and the tap data gradient
    grad_x = sum_t shift_{-t}(gy) W_t, both against fp64 CPU sums: atol 1e-5 max + rtol 1e-4"""
    from vqvae_amd import pixelcnn
    g = torch.Generator().manual_seed(len(taps) * 10 + Cin + H)
    n = len(taps)
    x = torch.randn(B, H, W, Cin, generator=g)
    gy = torch.randn(B, H, W, Cout, generator=g)
    w = torch.randn(Cout, Cin, 1, n, generator=g) * 0.1
    addend = torch.randn(B, H, W, Cin, generator=g)
    xd, gd = x.double(), gy.double()
    ref_w = torch.stack([torch.einsum("bhwo,bhwi->oi", gd, _shift(xd, dy, dx)) for dy, dx in taps], dim=-1)
    ref_x = addend.double().clone()
    for t, (dy, dx) in enumerate(taps):
        ref_x += _shift(gd @ w[:, :, 0, t].double(), -dy, -dx)
    got_w = pixelcnn.taps_wgrad(gy.to(DEV), x.to(DEV), taps).cpu()
    _within(got_w.numpy(), ref_w.numpy(), "grad_w")
    got_w2 = pixelcnn.taps_wgrad(gy.to(DEV), x.to(DEV), taps).cpu()
    assert torch.equal(got_w, got_w2)
    hold = nn.Module()
    got_x = pixelcnn.taps_dgrad(gy.to(DEV), hold, w.to(DEV), taps, addend=addend.to(DEV)).cpu()
    _within(got_x.numpy(), ref_x.numpy(), "grad_x")


@pytest.mark.gpu
@pytest.mark.parametrize("with_cond", [True, False])
def test_gate_backward_vs_autograd(with_cond):
    from vqvae_amd import pixelcnn
    g = torch.Generator().manual_seed(5)
    B, H, W, dim = 3, 6, 6, 96
    t1 = torch.randn(B, H, W, 2 * dim, generator=g) * 2
    cond = torch.randn(B, 2 * dim, generator=g) if with_cond else None
    go = torch.randn(B, H, W, dim, generator=g)
    t = t1.double().requires_grad_(True)
    c = cond.double().requires_grad_(True) if with_cond else None
    pre = t + c[:, None, None, :] if with_cond else t
    a, gg = pre.chunk(2, dim=-1)
    (torch.tanh(a) * torch.sigmoid(gg) * go.double()).sum().backward()
    gc = torch.full((B, 2 * dim), 0.5).to(DEV) if with_cond else None
    got = pixelcnn.gate_backward(t1.to(DEV), cond.to(DEV) if with_cond else None, go.to(DEV), dim, gc, accumulate=True)
    _within(got.cpu().numpy(), t.grad.numpy(), "grad_pre")
    if with_cond:
        _within(gc.cpu().numpy(), (c.grad + 0.5).numpy(), "grad_cond")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["random", "repeated", "one_code", "out_of_range", "wide"])
def test_gather_backward_vs_autograd(case):
    """segmented sums of nn.Embedding's backward: repeated indices, all rows to one code, absent codes (exact zero rows) and
    out-of-range indices (clamped into the table as the forward clamps them)"""
    from vqvae_amd import pixelcnn
    g = torch.Generator().manual_seed(11)
    rows, Cc, n = 512, (300 if case == "wide" else 64), 5000
    idx = torch.randint(0, 64, (n,), generator=g)
    if case == "one_code":
        idx[:] = 7
    if case == "out_of_range":
        idx[::7] = -3
        idx[1::7] = rows + 5
    go = torch.randn(n, Cc, generator=g)
    ref = torch.zeros(rows, Cc, dtype=torch.float64).index_add_(0, idx.clamp(0, rows - 1), go.double())
    got = pixelcnn.gather_rows_backward(idx.to(DEV), go.to(DEV), rows).cpu()
    _within(got.numpy(), ref.numpy(), "grad_table")
    untouched = np.setdiff1d(np.arange(rows), idx.clamp(0, rows - 1).numpy())
    assert np.all(got.numpy()[untouched] == 0)
    assert torch.equal(got, pixelcnn.gather_rows_backward(idx.to(DEV), go.to(DEV), rows).cpu())


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1.0, 80.0])
def test_cross_entropy_vs_autograd(scale):
    """vqvae_cross_entropy_f32 / _backward_f32 through pixelcnn.cross_entropy, including large-magnitude logits"""
    from vqvae_amd import pixelcnn
    g = torch.Generator().manual_seed(int(scale))
    B, K, H, W = 4, 512, 8, 8
    logits = torch.randn(B, K, H, W, generator=g) * scale
    x = torch.randint(0, K, (B, H, W), generator=g)
    ld = logits.double().requires_grad_(True)
    ref = nn.functional.cross_entropy(ld.permute(0, 2, 3, 1).reshape(-1, K), x.view(-1))
    (ref * 1.5).backward()
    lg = logits.to(DEV).requires_grad_(True)
    loss = pixelcnn.cross_entropy(lg, x.to(DEV))
    (loss * 1.5).backward()
    np.testing.assert_allclose(float(loss.detach()), float(ref), rtol=1e-6, atol=1e-6)
    _within(lg.grad.cpu().numpy(), ld.grad.numpy(), "grad_logits")


@pytest.mark.gpu
def test_wide_bias_gradient():
    from vqvae_amd import pixelcnn
    g = torch.Generator().manual_seed(2)
    gy = torch.randn(1000, 8, 8, 512, generator=g)
    _within(pixelcnn.bias_grad(gy.to(DEV)).cpu().numpy(), gy.double().sum((0, 1, 2)).numpy(), "grad_b")


@pytest.mark.gpu
def test_default_dims_b64_vs_restatement():
    """GatedPixelCNN(512, 64, 15, 10) at B = 64 on 8 x 8 maps -- beyond the goldens -- against the fp64 CPU restatement"""
    model = _build(None, (512, 64, 15, 10))
    g = torch.Generator().manual_seed(64)
    x = torch.randint(0, 512, (64, 8, 8), generator=g)
    label = torch.randint(0, 10, (64,), generator=g)
    loss, gl, grads = _step_grads(model, x.to(DEV), label.to(DEV))
    state = {k: p.detach().cpu() for k, p in model.named_parameters()}
    rl, rgl, rgrads = R.loss_and_grads(state, x, label, 15)
    np.testing.assert_allclose(float(loss), float(rl), rtol=1e-5)
    _within(gl.cpu().numpy(), rgl.numpy(), "grad_logits")
    for k in rgrads:
        _within(grads[k].cpu().numpy(), rgrads[k].numpy(), k)


@pytest.mark.gpu
def test_gated_layer_nchw_boundary_is_differentiable():
    """GatedMaskedConv2d.forward (models.py:64-84) under autograd: input and parameter gradients against torch autograd in fp64"""
    from vqvae_amd.pixelcnn import GatedMaskedConv2d
    torch.manual_seed(3)
    layer = GatedMaskedConv2d('B', 32, 3, True, 4)
    R.perturb_biases(layer)
    layer = layer.to(DEV).train()
    g = torch.Generator().manual_seed(4)
    x_v = torch.randn(2, 32, 8, 8, generator=g)
    x_h = torch.randn(2, 32, 8, 8, generator=g)
    h = torch.tensor([1, 3])
    wv, wh = torch.randn(2, 32, 8, 8, generator=g), torch.randn(2, 32, 8, 8, generator=g)
    xv, xh = x_v.to(DEV).requires_grad_(True), x_h.to(DEV).requires_grad_(True)
    ov, oh = layer(xv, xh, h.to(DEV))
    ((ov * wv.to(DEV)).sum() + (oh * wh.to(DEV)).sum()).backward()
    p = {k: v.detach().cpu().double().requires_grad_(True) for k, v in layer.named_parameters()}
    rv, rh = x_v.double().requires_grad_(True), x_h.double().requires_grad_(True)
    F = torch.nn.functional
    hh = F.embedding(h, p["class_cond_embedding.weight"])[:, :, None, None]
    h_vert = F.conv2d(rv, p["vert_stack.weight"], p["vert_stack.bias"], 1, (1, 1))[:, :, :8, :]
    gate = R._gate
    out_v = gate(h_vert + hh)
    h_horiz = F.conv2d(rh, p["horiz_stack.weight"], p["horiz_stack.bias"], 1, (0, 1))[:, :, :, :8]
    out = gate(F.conv2d(h_vert, p["vert_to_horiz.weight"], p["vert_to_horiz.bias"]) + h_horiz + hh)
    out_h = F.conv2d(out, p["horiz_resid.weight"], p["horiz_resid.bias"]) + rh
    ((out_v * wv.double()).sum() + (out_h * wh.double()).sum()).backward()
    _within(xv.grad.cpu().numpy(), rv.grad.numpy(), "x_v")
    _within(xh.grad.cpu().numpy(), rh.grad.numpy(), "x_h")
    for k, q in layer.named_parameters():
        _within(q.grad.cpu().numpy(), p[k].grad.numpy(), k)


@pytest.mark.gpu
def test_captured_training_step_replays_eager_gradients():
    """forward, loss and backward make no host synchronisation: the step captures into a graph whose replay gives the eager bits"""
    from vqvae_amd import pixelcnn
    model = _build("k512_dim64_l15")
    x, label = R.inputs("k512_dim64_l15")
    x, label = x.to(DEV), label.to(DEV)
    params = list(model.parameters())
    stream = torch.cuda.Stream(device=DEV)
    stream.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(stream):
        for _ in range(2):
            grads_eager = torch.autograd.grad(pixelcnn.cross_entropy(model(x, label), x), params)
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        grads = torch.autograd.grad(pixelcnn.cross_entropy(model(x, label), x), params)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(grads, grads_eager):
        assert torch.equal(a, b)
