"""Calls on WARM state (-m gpu): every other test file builds a model or a workspace, makes one call and compares it.  The product
runs the other way -- every call after the first trusts what earlier calls left behind: the quantizer workspace's prepared codebook
images (VectorQuantizer._workspace, shared by VectorQuantizer.forward, VQVAE._forward_c, encode and the training path), the whole-path
activation workspace (one per stream, grown to the largest batch seen, laid out differently by the fused, halo-tile and generic
paths), the packed weights and their scheme hint (VQVAE._c_weights), the host-side record of a step in parts, and LazyOneHot.

Each test runs a SEQUENCE of calls on one model or workspace and checks every step two ways:
  (a) against fresh state, bit for bit: the same call on a new model loaded from the current state_dict(), or on a new workspace
      (the kernels are deterministic: any difference is a state bug);
  (b) against the oracle where the size allows: oracle/vqvae_oracle.c for the quantizer (tests/test_fuzz_gpu.py's assertions),
      oracle/torch_port.py for the model (tests/test_model_gpu.py's tolerances).
Every reused buffer is filled with 0xFF bytes before its first use (NaN as fp32, -1 as an index), so a stale or unwritten read fails
on every run whatever memory the caching allocator hands back.  The activation workspace is scratch for each call
(include/vqvae_hip.h) and is filled again between complete calls -- never between the begin and the end of a step in parts; the
quantizer workspace only together with invalidate()."""
import itertools

import numpy as np
import pytest
import torch

from tests import cases, hetero

pytestmark = pytest.mark.gpu

DEFAULT_DIMS = (128, 32, 2, 512, 64, 0.25)


def dev():
    return torch.device("cuda:0")


def _same(a, b, what):
    """bit-for-bit equality of two tensors (NaN payloads included)"""
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {tuple(a.shape)} {a.dtype} vs {tuple(b.shape)} {b.dtype}"
    a, b = a.detach().contiguous().reshape(-1), b.detach().contiguous().reshape(-1)
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    assert torch.equal(a, b), f"{what}: not bit-identical"


def _same_all(got, want, names, what):
    for g, w, n in zip(got, want, names):
        _same(g, w, f"{what}: {n}")


# ---------------------------------------------------------------------------------------------------------------- quantizer
def _vq_check_oracle(out, ref, rowmajor, what):
    """tests/test_fuzz_gpu.py's assertions: indices, z_q bits with the NaN pattern, histogram exact; loss / perplexity"""
    loss, z_q, ppl, idx, hist = out
    if rowmajor:
        z_q = z_q.permute(0, 3, 1, 2)
    assert np.array_equal(idx.cpu().numpy(), ref["idx"]), f"{what}: indices"
    got, want = z_q.contiguous().cpu().numpy(), ref["z_q"]
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: z_q NaN pattern"
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32)), f"{what}: z_q bits"
    assert np.array_equal(hist.cpu().numpy(), ref["hist"]), f"{what}: histogram"
    np.testing.assert_allclose(loss.item(), ref["loss"], rtol=2e-6, err_msg=f"{what}: loss")
    np.testing.assert_allclose(ppl.item(), ref["perplexity"], rtol=1e-5, err_msg=f"{what}: perplexity")


VQ_OUT = ("loss", "z_q", "perplexity", "idx", "hist")

FORMS = {"default": {}, "exact_sweep": dict(exact_sweep=True), "bf16_filter": dict(bf16_filter=True),
         "form8": dict(form=8), "form16": dict(form=16)}


def _filled_ws(K, D, byte=255):
    from vqvae_amd import functional as Fh
    return Fh.vq_workspace(K, D, dev()).fill_(byte)


def _vq_inputs(K, D, B, H, W, seed):
    """rows near codes (a trained codebook's distances: close calls) plus a few far rows; the codebook has a duplicated code"""
    g = torch.Generator().manual_seed(seed)
    cb = torch.randn(K, D, generator=g)
    if K > 3:
        cb[K // 2] = cb[1]
    n = B * H * W
    z = cb[torch.randint(0, K, (n,), generator=g)] + 0.1 * torch.randn(n, D, generator=g)
    z[::7] = 2.0 * torch.randn(z[::7].shape, generator=g)
    return z.view(B, H, W, D).permute(0, 3, 1, 2).contiguous(), cb.contiguous()


def _layout(z, rowmajor):
    zd = z.to(dev())
    return zd.permute(0, 2, 3, 1).contiguous() if rowmajor else zd


VQ_SHAPES = [(D, K) for D in (7, 48, 200) for K in (33, 300, 1100)] + \
            [(D, K) for D in (32, 64, 128, 256) for K in (100, 512, 2000)]


@pytest.mark.parametrize("D,K", VQ_SHAPES)
def test_prepared_codebook_image_across_launch_forms(D, K):
    """A call without `prepared` on a filled workspace, then a call WITH `prepared` in another launch form on the same workspace:
    every ordered pair of the forms the shape accepts, NCHW and row-major alternating over the pairs.  Each call equals the same
    form on a fresh workspace bit for bit and the C oracle.  (Widths outside {32, 64, 128, 256}: the vector-units form used to write
    only ||e||^2, and the matrix-core kernel behind it read an image nobody had written.)  Filled with 0xFF bytes and again with
    zero bytes: 0xFF sets the generic kernel's non-finite-codebook flag, whose slow path reads only ||e||^2 and the codebook, so an
    unwritten image shows only where the flag reads zero."""
    from oracle import c_oracle
    from vqvae_amd import functional as Fh
    from vqvae_amd._lib import VqvaeHipError
    z, cb = _vq_inputs(K, D, 3, 8, 8, 100 * D + K)
    ref = c_oracle.vq_forward(z.numpy(), cb.numpy(), 0.25)
    cbd = cb.to(dev())
    fresh = {}
    for rowmajor in (False, True):
        zd = _layout(z, rowmajor)
        for name, kw in FORMS.items():
            try:
                out = Fh.vq_forward(zd, cbd, 0.25, rowmajor=rowmajor, workspace=_filled_ws(K, D), **kw)
            except VqvaeHipError:
                continue                                                   # a form this shape does not take
            _vq_check_oracle(out, ref, rowmajor, f"D={D} K={K} {name} rowmajor={rowmajor} (fresh workspace)")
            fresh[(name, rowmajor)] = out
    for (i, (a, b)), byte in itertools.product(enumerate(itertools.permutations(FORMS, 2)), (0xFF, 0x00)):
        rowmajor = i % 2 == 1
        if (a, rowmajor) not in fresh or (b, rowmajor) not in fresh:
            continue
        zd = _layout(z, rowmajor)
        ws = _filled_ws(K, D, byte)
        first = Fh.vq_forward(zd, cbd, 0.25, rowmajor=rowmajor, workspace=ws, prepared=False, **FORMS[a])
        second = Fh.vq_forward(zd, cbd, 0.25, rowmajor=rowmajor, workspace=ws, prepared=True, **FORMS[b])
        what = f"D={D} K={K} rowmajor={rowmajor} fill {byte:#04x}: {a} then {b} (prepared)"
        _same_all(first, fresh[(a, rowmajor)], VQ_OUT, what + " [first]")
        _vq_check_oracle(second, ref, rowmajor, what)
        _same_all(second, fresh[(b, rowmajor)], VQ_OUT, what)


@pytest.mark.parametrize("f1,f2", [("default", "default"), ("default", "bf16_filter"), ("bf16_filter", "default"),
                                   ("bf16_filter", "bf16_filter")])
@pytest.mark.parametrize("D,K", [(7, 40), (48, 300), (200, 1100), (64, 512), (64, 1500), (128, 256)])
def test_codebook_swap_on_a_used_workspace(D, K, f1, f2):
    """Codebook A with an Inf entry (its non-finite flag sends the call down the slow path) and a finite B on ONE workspace, the
    launch forms alternating f1, f2, f1, ... over the calls (X* = prepared):
        A, B, B*                      (the slow path's flag left behind by A)
        B, A, A*, B, B*               (the reverse: B's image and clear flag left behind when A comes)
    Every call on B matches the oracle on B and a fresh workspace bit for bit; every call on A matches a fresh workspace."""
    from oracle import c_oracle
    from vqvae_amd import functional as Fh
    z, cb_b = _vq_inputs(K, D, 2, 8, 8, 7 * D + K)
    cb_a = cb_b.clone()
    cb_a[K // 3, D // 2] = float("inf")
    cb_a[0] += 0.5
    ref_b = c_oracle.vq_forward(z.numpy(), cb_b.numpy(), 0.25)
    for rowmajor in (False, True):
        zd = _layout(z, rowmajor)
        cbs = {"A": cb_a.to(dev()), "B": cb_b.to(dev())}
        fresh = {(c, f): Fh.vq_forward(zd, cbs[c], 0.25, rowmajor=rowmajor, workspace=_filled_ws(K, D), **FORMS[f])
                 for c in "AB" for f in {f1, f2}}
        for f in {f1, f2}:
            _vq_check_oracle(fresh[("B", f)], ref_b, rowmajor, f"D={D} K={K} {f} rowmajor={rowmajor}: B on a fresh workspace")
        for seq in (["A", "B", "B*"], ["B", "A", "A*", "B", "B*"]):
            ws = _filled_ws(K, D)
            for j, step in enumerate(seq):
                c, f = step[0], (f1, f2)[j % 2]
                out = Fh.vq_forward(zd, cbs[c], 0.25, rowmajor=rowmajor, workspace=ws, prepared=step.endswith("*"), **FORMS[f])
                what = f"D={D} K={K} rowmajor={rowmajor} sequence {'-'.join(seq)} step {j} ({step}, {f})"
                _same_all(out, fresh[(c, f)], VQ_OUT, what)
                if c == "B":
                    _vq_check_oracle(out, ref_b, rowmajor, what)


# ---------------------------------------------------------------------------------------------------------------- model helpers
def _model(dims=DEFAULT_DIMS, seed=0, sd=None):
    from vqvae_amd import conv
    from vqvae_amd.modules import VQVAE
    conv.set_conv_backend("hip")
    torch.manual_seed(seed)
    m = VQVAE(*dims).eval()
    if sd is not None:
        m.load_state_dict({k: v.detach().cpu() for k, v in sd.items()}, strict=True)
    return m.to(dev())


def _fresh(m, dims):
    """a new model from m's current state_dict (and beta): nothing cached"""
    c = _model(dims, sd=m.state_dict())
    c.vector_quantization.beta = m.vector_quantization.beta
    return c


def _fill_vq(m):
    """the quantizer workspace of the current stream, created if need be, invalidated and filled with 0xFF"""
    vq = m.vector_quantization if hasattr(m, "vector_quantization") else m
    ws = vq._workspace()[0]
    vq.invalidate()
    ws.fill_(255)


def _fill_act(m, x):
    """the activation workspace of the current stream, grown to x's shape if need be, filled with 0xFF"""
    from vqvae_amd import _lib
    B, _, H, W = x.shape
    cw, _keep = m._c_weights()
    ws, _st = m._c_workspace(_lib.load(), cw, B, H, W, x.device)
    ws.fill_(255)


def _prime(m, x):
    _fill_vq(m)
    _fill_act(m, x)


FWD_OUT = ("loss", "x_hat", "perplexity", "idx")


def _fwd(m, x, **kw):
    with torch.no_grad():
        return m._forward_c(x, want_idx=True, **kw)


def _fresh_fwd(m, dims, x, **kw):
    c = _fresh(m, dims)
    _prime(c, x)
    return _fwd(c, x, **kw)


def _port_check(m, dims, x, out, what):
    """(b): the model's output against oracle/torch_port.py -- indices exact except flips explained by the z_e tolerance
    (hetero.explain_flips), x_hat atol 1e-5 + rtol 1e-4 on every image without a flip, loss / perplexity rtol 1e-5 without flips"""
    from oracle import torch_port
    h, rh, nl, K, D, beta = dims
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    B, _, H, W = x.shape
    loss, x_hat, ppl, idx = out
    with torch.no_grad():
        r_loss, r_xhat, r_ppl, r_ze, _r_zq, r_idx = torch_port.forward(sd, x.cpu().clone(), m.vector_quantization.beta, nl, full=True)
    got, want = idx.cpu().numpy().reshape(-1), r_idx.numpy().reshape(-1)
    zr = r_ze.permute(0, 2, 3, 1).reshape(-1, D).double().numpy()
    cmax = r_ze.abs().amax(dim=(0, 2, 3)).double().numpy()
    flips, worst = hetero.explain_flips(got, want, zr, sd["vector_quantization.embedding.weight"].double().numpy(), cmax)
    assert worst <= 1.0, f"{what}: an index flip is not explained by the z_e tolerance: gap = {worst:.3g} x the bound"
    assert len(flips) <= max(1, int(1e-3 * got.size)), f"{what}: {len(flips)} flips in {got.size} rows"
    clean = np.setdiff1d(np.arange(B), np.unique(flips // ((H // 4) * (W // 4))))
    np.testing.assert_allclose(x_hat.cpu().numpy()[clean], r_xhat.numpy()[clean], atol=1e-5, rtol=1e-4, err_msg=f"{what}: x_hat")
    if len(flips) == 0:
        np.testing.assert_allclose(loss.item(), r_loss.item(), rtol=1e-5, err_msg=f"{what}: loss")
        np.testing.assert_allclose(ppl.item(), r_ppl.item(), rtol=1e-5, err_msg=f"{what}: perplexity")
    return r_loss.item()


# ---------------------------------------------------------------------------------------------------------------- module level
@pytest.mark.parametrize("order", ["whole_path_first", "module_first"])
@pytest.mark.parametrize("D,vq_flags", [(64, 0), (48, 0), (48, 0x8)])
def test_whole_path_and_module_share_the_prepared_codebook(D, vq_flags, order):
    """VQVAE._forward_c (on the default shapes the fused path prepares through vq_prepare_impl) and m.vector_quantization(z) on ONE
    stream, i.e. one quantizer slot: the second call runs on the first one's image (prepared).  Both orders; D = 48 also with the
    vector-units quantizer form (VQVAE_VQ_BF16_FILTER) in the whole path."""
    from oracle import c_oracle
    dims = (128, 32, 2, 512, D, 0.25)
    m = _model(dims, seed=D)
    g = torch.Generator().manual_seed(D + vq_flags)
    x = torch.randn(4, 3, 32, 32, generator=g).to(dev())
    cb = m.vector_quantization.embedding.weight.detach().cpu()
    sel = torch.randint(0, 512, (2 * 64,), generator=g)
    z = (cb[sel] + 0.3 * cb.abs().mean() * torch.randn(2 * 64, D, generator=g)).view(2, 8, 8, D).permute(0, 3, 1, 2).contiguous()
    ref = c_oracle.vq_forward(z.numpy(), cb.numpy(), 0.25)
    zd = z.to(dev())
    want_fwd = _fresh_fwd(m, dims, x, vq_flags=vq_flags)
    c = _fresh(m, dims)
    _fill_vq(c)
    with torch.no_grad():
        want_vq = c.vector_quantization(zd)
    _prime(m, x)
    with torch.no_grad():
        if order == "whole_path_first":
            got_fwd = _fwd(m, x, vq_flags=vq_flags)
            got_vq = m.vector_quantization(zd)
        else:
            got_vq = m.vector_quantization(zd)
            got_fwd = _fwd(m, x, vq_flags=vq_flags)
    what = f"D={D} vq_flags={vq_flags:#x} {order}"
    _same_all(got_fwd, want_fwd, FWD_OUT, what + " forward")
    _same_all([got_vq[i] for i in (0, 1, 2, 4)], [want_vq[i] for i in (0, 1, 2, 4)], ("loss", "z_q", "perplexity", "idx"), what + " quantizer")
    hist = torch.bincount(got_vq[4].view(-1), minlength=512).to(torch.int32)
    _vq_check_oracle((got_vq[0], got_vq[1], got_vq[2], got_vq[4], hist), ref, False, what + " quantizer")


# ---------------------------------------------------------------------------------------------------------------- one model, many calls
def test_shape_changes_on_one_stream():
    """One model, one stream, one activation workspace grown to the largest batch: the fused step in parts on side streams (B = 4096),
    the single fused call (B = 37), halo tiles (64x64), the generic path (24x24), and B = 4096 again -- each equal to a fresh model bit
    for bit, the small ones also against torch_port."""
    dims = DEFAULT_DIMS
    m = _model(dims)
    g = torch.Generator().manual_seed(77)
    steps = [(4096, 32, 32, 4), (37, 32, 32, None), (3, 64, 64, None), (5, 24, 24, None), (4096, 32, 32, 4)]
    xs = {}
    for B, H, W, parts in steps:
        if (B, H, W) not in xs:
            xs[(B, H, W)] = torch.randn(B, 3, H, W, generator=g).to(dev())
    _fill_vq(m)
    for i, (B, H, W, parts) in enumerate(steps):
        x = xs[(B, H, W)]
        _fill_act(m, x)
        got = _fwd(m, x, parts=parts)
        want = _fresh_fwd(m, dims, x, parts=parts)
        what = f"step {i}: B={B} {H}x{W} parts={parts}"
        _same_all(got, want, FWD_OUT, what)
        if B < 64:
            _port_check(m, dims, x, got, what)


def test_entry_points_share_one_workspace():
    """forward -> encode -> decode_indices(encode's indices) -> forward on one model and stream: the second forward equals the first
    bit for bit, encode's indices equal the forward's, decode(encode(x)) equals a fresh model's decode bit for bit and the forward's
    x_hat within tests/test_model_gpu.py's tolerance."""
    dims = DEFAULT_DIMS
    m = _model(dims, seed=3)
    x = torch.randn(37, 3, 32, 32, generator=torch.Generator().manual_seed(3)).to(dev())
    _prime(m, x)
    with torch.no_grad():
        first = m._forward_c(x, want_idx=True)
        plain = m(x)
        idx = m.encode(x)
        dec = m.decode_indices(idx, 37, 8, 8)
        last = m._forward_c(x, want_idx=True)
    _same_all(last, first, FWD_OUT, "forward after encode / decode_indices")
    _same_all(plain, first[:3], FWD_OUT, "VQVAE.forward")
    _same(idx, first[3], "encode vs forward indices")
    c = _fresh(m, dims)
    _prime(c, x)
    with torch.no_grad():
        _same(c.encode(x), idx, "encode vs a fresh model")
        _same(c.decode_indices(first[3].clone(), 37, 8, 8), dec, "decode_indices vs a fresh model")
    np.testing.assert_allclose(dec.cpu().numpy(), first[1].cpu().numpy(), atol=1e-6, rtol=1e-5)
    _same_all(first, _fresh_fwd(m, dims, x), FWD_OUT, "forward vs a fresh model")
    _port_check(m, dims, x, first, "forward")


def test_parameter_updates_between_calls():
    """One in-place Adam step (the forward under autograd on the HIP kernels fills the backward holders), a second step whose gradients
    must equal a fresh model's, a write through .data plus invalidate_caches(), and load_state_dict of a trained checkpoint -- after each,
    the eval forward equals a fresh model from the current state_dict bit for bit, and torch_port; the scheme hint equals a fresh one's."""
    dims = DEFAULT_DIMS
    m = _model(dims, seed=5)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(37, 3, 32, 32, generator=g).to(dev())
    xt = torch.randn(32, 3, 32, 32, generator=g).to(dev())
    _prime(m, x)
    _fwd(m, x)                                                                       # warm every cache
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)

    def train_step(model):
        model.zero_grad(set_to_none=True)
        loss, x_hat, _ppl = model(xt)
        (loss + torch.mean((x_hat - xt) ** 2)).backward()

    train_step(m)
    opt.step()
    _prime(m, x)
    got = _fwd(m, x)
    _same_all(got, _fresh_fwd(m, dims, x), FWD_OUT, "after an Adam step")
    _port_check(m, dims, x, got, "after an Adam step")

    c = _fresh(m, dims)
    train_step(m)
    train_step(c)
    for (n, p), (_, q) in zip(m.named_parameters(), c.named_parameters()):
        _same(p.grad, q.grad, f"second step's gradient of {n} vs a fresh model")

    with torch.no_grad():
        w = m.encoder.conv_stack[2].weight
        w.data.copy_(w.data * 1.5 + 0.01)                                            # does not bump _version
    m.invalidate_caches()
    _prime(m, x)
    got = _fwd(m, x)
    _same_all(got, _fresh_fwd(m, dims, x), FWD_OUT, "after .data.copy_ + invalidate_caches()")
    _port_check(m, dims, x, got, "after .data.copy_ + invalidate_caches()")

    m.load_state_dict(cases.trained_state("trained_main_defaults"))
    _prime(m, x)
    got = _fwd(m, x)
    c = _fresh(m, dims)
    assert m.scheme_hint() == c.scheme_hint(), "scheme hint after load_state_dict"
    _same_all(got, _fresh_fwd(m, dims, x), FWD_OUT, "after load_state_dict")
    _port_check(m, dims, x, got, "after load_state_dict")


def test_beta_change_reaches_the_whole_path():
    """`m.vector_quantization.beta = 0.5` between two forwards (models/quantizer.py:63-64 reads the attribute on every call): the loss
    is a fresh beta = 0.5 model's and torch_port's, x_hat and perplexity are bit-identical to the run before the change."""
    dims = DEFAULT_DIMS
    m = _model(dims, seed=9)
    x = torch.randn(37, 3, 32, 32, generator=torch.Generator().manual_seed(9)).to(dev())
    _prime(m, x)
    before = _fwd(m, x)
    m.vector_quantization.beta = 0.5
    _fill_act(m, x)
    after = _fwd(m, x)
    _same(after[1], before[1], "x_hat after the beta change")
    _same(after[2], before[2], "perplexity after the beta change")
    _same(after[3], before[3], "indices after the beta change")
    fresh = _fresh_fwd(m, dims, x)
    _same_all(after, fresh, FWD_OUT, "beta = 0.5 vs a fresh beta = 0.5 model")
    assert after[0].item() != before[0].item(), "the loss did not change with beta"
    _port_check(m, dims, x, after, "beta = 0.5")
    with torch.no_grad():
        plain = m(x)
    _same_all(plain, after[:3], FWD_OUT, "VQVAE.forward with beta = 0.5")


def test_two_streams_alternate():
    """Forwards alternating between the default stream and a side stream, each stream with its own workspace and quantizer slot,
    without a synchronisation in between: each result equals a single-stream run on a fresh model bit for bit."""
    dims = DEFAULT_DIMS
    m = _model(dims, seed=11)
    g = torch.Generator().manual_seed(11)
    xs = [torch.randn(B, 3, 32, 32, generator=g).to(dev()) for B in (37, 256)]
    want = [_fresh_fwd(m, dims, x) for x in xs]
    side = torch.cuda.Stream(device=dev())
    main = torch.cuda.current_stream(dev())
    for st in (main, side):
        with torch.cuda.stream(st):
            _prime(m, xs[1])
    side.wait_stream(main)
    got = []
    for i in range(6):
        st = side if i % 2 else main
        with torch.cuda.stream(st):
            got.append((i % 3 % 2, _fwd(m, xs[i % 3 % 2])))
    main.wait_stream(side)
    torch.cuda.synchronize()
    for i, (k, out) in enumerate(got):
        _same_all(out, want[k], FWD_OUT, f"call {i} on the {'side' if i % 2 else 'default'} stream, input {k}")


def test_parts_protocol_abort_and_replaced_begin():
    """begin -> abort -> begin -> parts -> end, and a begin without an end replaced by a new begin -> parts -> end, on one workspace:
    loss, perplexity, x_hat and the indices equal the single call of a fresh model bit for bit; a following _forward_c in parts too."""
    from vqvae_amd import _lib
    from vqvae_amd import functional as Fh
    dims = DEFAULT_DIMS
    m = _model(dims, seed=13)
    B = 256
    x = torch.randn(B, 3, 32, 32, generator=torch.Generator().manual_seed(13)).to(dev())
    want = _fresh_fwd(m, dims, x, parts=1)
    L = _lib.load()
    with torch.no_grad():
        cw, _keep = m._c_weights()
    st = torch.cuda.current_stream(dev()).cuda_stream
    prep = Fh.VQ_CODEBOOK_PREPARED
    for seq in ("abort", "replace"):
        _prime(m, x)
        ws = m._c_workspace(L, cw, B, 32, 32, dev())[0]
        vws = m.vector_quantization._workspace()[0]
        x_hat = torch.empty_like(x)
        scal = torch.empty(2, device=dev())
        idx = torch.empty((B * 64, 1), dtype=torch.int64, device=dev())

        def begin(flags):
            _lib.check(L.vqvae_forward_begin_f32(cw, B, 32, 32, flags, ws.data_ptr(), ws.numel(), vws.data_ptr(), vws.numel(), st))

        def part(b0, bc, flags):
            _lib.check(L.vqvae_forward_part_f32(cw, x.data_ptr(), B, b0, bc, 32, 32, flags, x_hat.data_ptr(), idx.data_ptr(),
                                                ws.data_ptr(), ws.numel(), vws.data_ptr(), vws.numel(), st))

        begin(0)
        if seq == "abort":
            assert L.vqvae_forward_abort_f32(ws.data_ptr()) == 0
        else:
            part(0, 128, 0)                                 # a begun step left without its end
        begin(prep)
        part(128, 128, prep)
        part(0, 128, prep)
        _lib.check(L.vqvae_forward_end_f32(cw, B, 32, 32, scal.data_ptr(), scal.data_ptr() + 4, ws.data_ptr(), ws.numel(), st))
        _same_all((scal[0], x_hat, scal[1], idx), want, FWD_OUT, f"parts after '{seq}'")
    _fill_act(m, x)
    m.vector_quantization.invalidate()
    _same_all(_fwd(m, x, parts=4), want, FWD_OUT, "_forward_c in parts after the protocol sequences")


# ---------------------------------------------------------------------------------------------------------------- config 2
def test_config2_torch_convs_on_a_warm_model(capsys):
    """BASELINE config 2 (torch's convs on the device, the HIP quantizer: set_conv_backend("torch")) on a model whose HIP caches are
    warm, against torch_port at B = 1024 and B = 5: z_e per channel (hetero.per_channel_check), indices exact except flips explained by
    the z_e tolerance, x_hat atol 1e-5 + rtol 1e-4 on every image without a flip, loss / perplexity rtol 1e-5.  Back on "hip" the
    output is bit-identical to the output before the switch."""
    from oracle import torch_port
    from vqvae_amd import conv
    dims = DEFAULT_DIMS
    h, rh, nl, K, D, beta = dims
    m = _model(dims, seed=17)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    cb64 = sd["vector_quantization.embedding.weight"].double().numpy()
    g = torch.Generator().manual_seed(17)
    xs = [torch.randn(B, 3, 32, 32, generator=g) for B in (1024, 5)]
    _prime(m, xs[0].to(dev()))
    before = [_fwd(m, x.to(dev())) for x in xs]
    try:
        conv.set_conv_backend("torch")
        for x in xs:
            B = x.shape[0]
            xd = x.to(dev())
            with torch.no_grad():
                loss, x_hat, ppl = m(xd)
                idx = m.encode(xd)
                z_e = conv.encoder_forward(m.encoder, xd, m.pre_quantization_conv)
                r_ze = torch.cat([torch_port.encode(sd, x[i:i + 256].clone(), nl) for i in range(0, B, 256)])
                outs = [torch_port.quantize(r_ze[i:i + 256], sd["vector_quantization.embedding.weight"], beta) for i in range(0, B, 256)]
                r_zq = torch.cat([o[1] for o in outs])
                r_idx = torch.cat([o[4] for o in outs])
                r_xhat = torch.cat([torch_port.decode(sd, r_zq[i:i + 256].clone(), nl) for i in range(0, B, 256)])
            torch.cuda.synchronize()
            w_ze = hetero.per_channel_check(z_e.permute(0, 3, 1, 2).cpu().numpy(), r_ze.numpy(), f"config 2 B={B}: z_e", per_image=False)
            got, want = idx.cpu().numpy().reshape(-1), r_idx.numpy().reshape(-1)
            zr = r_ze.permute(0, 2, 3, 1).reshape(-1, D).double().numpy()
            cmax = r_ze.abs().amax(dim=(0, 2, 3)).double().numpy()
            flips, worst = hetero.explain_flips(got, want, zr, cb64, cmax)
            assert worst <= 1.0, f"config 2 B={B}: an index flip is not explained by the z_e tolerance: gap = {worst:.3g} x the bound"
            assert len(flips) <= max(1, int(1e-4 * got.size)), f"config 2 B={B}: {len(flips)} flips in {got.size} rows"
            clean = np.setdiff1d(np.arange(B), np.unique(flips // 64))
            err_xh = float(np.abs(x_hat.cpu().numpy()[clean] - r_xhat.numpy()[clean]).max())
            np.testing.assert_allclose(x_hat.cpu().numpy()[clean], r_xhat.numpy()[clean], atol=1e-5, rtol=1e-4, err_msg=f"config 2 B={B}: x_hat")
            # the reference's scalars of the whole batch: loss = mean of equal-sized slab losses, perplexity from its histogram
            p = np.bincount(want, minlength=K).astype(np.float64) / want.size
            np.testing.assert_allclose(ppl.item(), float(np.exp(-(p * np.log(p + 1e-10)).sum())), rtol=1e-5 if len(flips) == 0 else 1e-4,
                                       err_msg=f"config 2 B={B}: perplexity")
            if len(flips) == 0:
                r_loss = float(np.mean([o[0].item() for o in outs])) if B % 256 == 0 else outs[0][0].item()
                np.testing.assert_allclose(loss.item(), r_loss, rtol=1e-5, err_msg=f"config 2 B={B}: loss")
            with capsys.disabled():
                print(f"\n   config 2 (torch convs) B={B}: z_e worst {w_ze:.2e} of its channel maximum, max |x_hat - reference| "
                      f"{err_xh:.2e}, {len(flips)} index flips / {got.size} rows (worst {worst:.2f} x the bound)")
    finally:
        conv.set_conv_backend("hip")
    _fill_act(m, xs[0].to(dev()))
    for x, b in zip(xs, before):
        _same_all(_fwd(m, x.to(dev())), b, FWD_OUT, f"back on hip, B={x.shape[0]}")


# ---------------------------------------------------------------------------------------------------------------- LazyOneHot
def test_lazy_onehot_does_not_alias_the_returned_indices():
    """VectorQuantizer.forward's fourth output is materialised on first use; an in-place edit of the fifth (idx) before that must not
    change it -- the reference returns two independent tensors (models/quantizer.py:55-57, 76)."""
    from vqvae_amd.modules import VectorQuantizer
    torch.manual_seed(21)
    vq = VectorQuantizer(64, 32, 0.25).to(dev())
    z = torch.randn(2, 32, 8, 8, device=dev()) / 64
    with torch.no_grad():
        out = vq(z)
    expected = torch.nn.functional.one_hot(out[4].clone().view(-1), 64).float()
    assert int(out[4].max()) > 0
    out[4].zero_()
    assert torch.equal(out[3].materialize(), expected)
