"""The orthogonal regularization loss on the GPU: functional.vq_orthogonal_forward / vq_orthogonal_backward
(vqvae_vq_orthogonal_*_f32), training.OrthogonalLoss and the modules' keywords against the CPU restatement
tests/vq_orthogonal_ref.py, whose arithmetic is the header of vqvae_amd/csrc/vq_orthogonal.hip.  Every operation of the contract is a
correctly rounded IEEE operation in a fixed order, so loss, count, selected, saved (fp64) and grad_rows are compared bit for bit, on
every element (NaNs by position): in every way the entry is called, in two runs, with every buffer offset by 4 bytes (the fp64 ones by
8) and in a graph replay."""
import numpy as np
import pytest
import torch

from tests import vq_orthogonal_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
IDS = lambda s: "x".join(map(str, s))


def _dev(a, offset=0):
    """a numpy array (or None) on the device; offset: that many elements into a larger buffer"""
    if a is None:
        return None
    t = torch.from_numpy(np.array(a, order="C"))               # (a copy: the cases' arrays are read-only)
    if not offset:
        return t.to(DEV)
    buf = torch.empty(t.numel() + offset, dtype=t.dtype, device=DEV)
    v = buf[offset:].view(t.shape)
    v.copy_(t)
    return v


def _check(got, want, what):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    want = np.asarray(want)
    assert got.dtype == want.dtype and got.size == want.size, what
    assert R.same_bits(got.reshape(want.shape), want), f"{what}: bits differ"


def _check_all(outs, want, what):
    loss, M, sel, V, g = want
    _check(outs[0], loss, f"{what}: loss")
    _check(outs[1], np.int32(M), f"{what}: count")
    _check(outs[2], sel, f"{what}: selected")
    _check(outs[3], V, f"{what}: saved")
    _check(outs[4], g, f"{what}: grad_rows")


def _inputs(a, offset=0):
    gl = None if a["grad_loss"] is None else _dev(np.array([a["grad_loss"]], np.float32), offset).reshape(())
    return _dev(a["rows"], offset), _dev(a["hist"], offset), _dev(a["uniforms"], offset), a["max_codes"], gl


def _chain(rows, hist, u, max_codes, gl, ws=None):
    from vqvae_amd import functional as F
    loss, count, sel, saved = F.vq_orthogonal_forward(rows, hist, max_codes=max_codes, uniforms=u, want_saved=True, workspace=ws)
    return loss, count, sel, saved, F.vq_orthogonal_backward(saved, sel, count, gl)


def _raw_chain(a):
    """the C entries themselves on buffers of the test's own, every one 4 bytes (fp64: 8 bytes) past a 16-byte boundary"""
    from vqvae_amd import _lib
    L = _lib.load()
    rows, hist, u, max_codes, gl = _inputs(a, 1)
    K, D = rows.shape
    assert rows.data_ptr() % 16 == 4
    out = lambda n, dt, fill: torch.full((n + 1,), fill, dtype=dt, device=DEV)[1:]
    loss, count, sel = out(1, torch.float32, 7.0), out(1, torch.int32, 7), out(K, torch.int32, 7)
    saved, ws, grad = out(K * D, torch.float64, 7.0), out(K, torch.float64, 7.0), out(K * D, torch.float32, 7.0)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: None if t is None else t.data_ptr()
    assert L.vqvae_vq_orthogonal_forward_f32(p(rows), p(hist), p(u), max_codes or 0, K, D, 0, p(loss), p(count), p(sel), p(saved),
                                             p(ws), K * 8, st) == 0
    assert L.vqvae_vq_orthogonal_backward_f32(p(saved), p(sel), p(count), p(gl), K, D, p(grad), st) == 0
    torch.cuda.synchronize()
    return loss, count, sel, saved.view(K, D), grad.view(K, D)


@pytest.mark.parametrize("shape", R.GPU_SHAPES, ids=IDS)
def test_bits_of_every_call_in_two_runs_and_off_alignment(shape):
    from vqvae_amd import functional as F
    ws = F.vq_orthogonal_workspace(*shape, DEV)
    for name, (a, want) in R.expected(shape).items():
        t = _inputs(a)
        for run in range(2):
            outs = _chain(*t, ws=ws if run else None)
            torch.cuda.synchronize()
            assert outs[0].shape == () and outs[1].shape == () and outs[3].shape == shape and outs[4].shape == shape
            _check_all(outs, want, f"{name} run {run}")
        _check_all(_raw_chain(a), want, f"{name} offset")
        # without `saved` the loss, the count and the selection are the same
        loss, count, sel, none = F.vq_orthogonal_forward(t[0], t[1], max_codes=t[3], uniforms=t[2])
        assert none is None
        _check_all((loss, count, sel, outs[3], outs[4]), want, f"{name} without saved")


@pytest.mark.parametrize("shape", R.GPU_SHAPES, ids=IDS)
def test_bits_in_a_graph_replay(shape):
    """forward and backward are one chain of launches on one stream: captured, and replayed on new inputs with other values left in
    the outputs between the replays"""
    from vqvae_amd import functional as F
    ws = F.vq_orthogonal_workspace(*shape, DEV)
    for name, (a, want) in R.expected(shape).items():
        real = _inputs(a)
        static = [None if t is None or not isinstance(t, torch.Tensor) else torch.zeros_like(t) for t in real]
        static[3] = real[3]
        if static[1] is not None:
            static[1].fill_(1)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            _chain(*static, ws=ws)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = _chain(*static, ws=ws)
        for st, r in zip(static, real):
            if isinstance(st, torch.Tensor):
                st.copy_(r)
        for i in range(2):
            graph.replay()
            torch.cuda.synchronize()
            _check_all(outs, want, f"{name} replay {i}")
            for o in outs:
                o.fill_(7)
            ws.fill_(7)


def test_argument_errors_come_back_without_a_launch():
    from vqvae_amd import _lib, functional as F
    L = _lib.load()
    a, want = R.expected((5, 3))["hist"]
    rows, hist, u, _, gl = _inputs(a)
    st = torch.cuda.current_stream().cuda_stream
    loss, count = torch.full((), 7.0, device=DEV), torch.full((), 7, dtype=torch.int32, device=DEV)
    sel, saved = torch.full((5,), 7, dtype=torch.int32, device=DEV), torch.full((5, 3), 7.0, dtype=torch.float64, device=DEV)
    grad, ws = torch.full((5, 3), 7.0, device=DEV), torch.full((5,), 7.0, dtype=torch.float64, device=DEV)
    p = lambda t: t.data_ptr()
    fw = lambda K=5, D=3, flags=0, sel_=sel, ws_=p(ws), n=40: L.vqvae_vq_orthogonal_forward_f32(
        p(rows), p(hist), None, 0, K, D, flags, p(loss), p(count), p(sel_), p(saved), ws_, n, st)
    assert fw(K=16385) == -3 and fw(D=257) == -3 and fw(K=0) == -2 and fw(D=0) == -2 and fw(flags=1) == -3
    assert fw(sel_=hist) == -3 and fw(ws_=None) == -4 and fw(n=32) == -4
    assert L.vqvae_vq_orthogonal_backward_f32(p(saved), p(sel), p(count), None, 16385, 3, p(grad), st) == -3
    assert L.vqvae_vq_orthogonal_backward_f32(p(saved), p(sel), p(count), None, 5, 257, p(grad), st) == -3
    assert L.vqvae_vq_orthogonal_backward_f32(p(saved), p(sel), p(count), None, 5, 3, None, st) == -1
    with pytest.raises(_lib.VqvaeHipError):
        F.vq_orthogonal_forward(torch.zeros(4, 257, device=DEV))
    with pytest.raises(_lib.VqvaeHipError):
        F.vq_orthogonal_forward(rows, workspace=torch.empty(8, dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError):
        F.vq_orthogonal_forward(rows, max_codes=2)
    with pytest.raises(TypeError):
        F.vq_orthogonal_forward(rows, hist.to(torch.int64))
    torch.cuda.synchronize()
    for t in (loss, count, sel, saved, grad, ws):
        assert bool((t == 7).all())                                                                # nothing was launched
    assert fw() == 0
    torch.cuda.synchronize()
    _check(loss, want[0], "loss")
    _check(sel, want[2], "selected")


def test_orthogonal_loss_under_autograd():
    from vqvae_amd import training as T
    a, want = R.expected((96, 33))["cap_below"]
    rows, hist, u, max_codes, _ = _inputs(a)
    x = rows.clone().requires_grad_(True)
    loss = T.OrthogonalLoss.apply(x, hist, max_codes, u, None)
    _check(loss, want[0], "loss")
    loss.backward()
    _check(x.grad, want[4], "grad_rows")
    a, want = R.expected((96, 33))["hist"]
    rows, hist, _, _, gl = _inputs(a)
    x = rows.clone().requires_grad_(True)
    (T.OrthogonalLoss.apply(x, hist, None, None, None) * gl).backward()
    _check(x.grad, want[4], "grad_rows with an upstream scalar")


# ---- the modules ------------------------------------------------------------------------------------------------------------------

DIMS = (32, 8, 1, 64, 16, 0.25)
CONFIGS = [dict(), dict(cosine_sim=True), dict(codebook_dim=4), dict(cosine_sim=True, codebook_dim=4), dict(rotation_trick=True)]
ORTH = [dict(orthogonal_reg_weight=0.5), dict(orthogonal_reg_weight=10.0, orthogonal_reg_active_codes_only=True),
        dict(orthogonal_reg_weight=2.0, orthogonal_reg_active_codes_only=True, orthogonal_reg_max_codes=5)]


def _pair(cfg, orth):
    """the model with the option and the same model (same parameters) without"""
    from vqvae_amd.modules import VQVAE
    torch.manual_seed(11)
    m = VQVAE(*DIMS, **cfg, **orth).to(DEV).train()
    m0 = VQVAE(*DIMS, **cfg).to(DEV).train()
    m0.load_state_dict(m.state_dict())
    with torch.no_grad():                                     # codes of very different lengths and directions
        w = torch.randn(64, m.vector_quantization.e_dim, device=DEV) * torch.rand(64, 1, device=DEV)
        m.vector_quantization.embedding.weight.copy_(w)
        m0.vector_quantization.embedding.weight.copy_(w)
    return m, m0


@pytest.mark.parametrize("orth", ORTH, ids=["all", "active", "active_capped"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "+".join(c) or "plain")
def test_the_quantizer_adds_the_term_and_its_gradient(cfg, orth):
    """quantize on given rows against the chain written by hand from the functional calls: the loss is base + weight * term and
    embedding.weight.grad is what the hand-written backward gives, bit for bit"""
    from vqvae_amd import functional as F, training as T
    m, _ = _pair(cfg, orth)
    vq = m.vector_quantization
    weight = orth["orthogonal_reg_weight"]
    cos, E = vq.cosine_sim, vq.embedding.weight
    g = torch.Generator(device=DEV)
    vq.generator = g
    g.manual_seed(5)
    z = torch.randn(2, 4, 4, 16, device=DEV)
    assert vq.last_orthogonal_loss is None
    loss = vq.quantize(z, rowmajor=True)[0]
    loss.backward()
    torch.cuda.synchronize()
    # by hand
    g.manual_seed(5)
    with torch.no_grad():
        y = F.linear_rows(z, vq.project_in.weight, vq.project_in.bias, rowmajor=True) if "codebook_dim" in cfg else z
        unit, denom = F.l2norm_rows(E.detach())
        rows = F.l2norm_rows(y, rowmajor=True)[0] if cos else y
        codes = unit if cos else E.detach()
        base, _, _, idx, hist = F.vq_forward(rows, codes, 0.25, rowmajor=True)
        u = torch.rand(64, device=DEV, generator=g) if "orthogonal_reg_max_codes" in orth else None
        term, count, sel, saved = F.vq_orthogonal_forward(unit, hist if orth.get("orthogonal_reg_active_codes_only") else None,
                                                          max_codes=orth.get("orthogonal_reg_max_codes"), uniforms=u, want_saved=True)
        want_loss = base + weight * term
        one = torch.ones((), device=DEV)
        g_codes = T.vq_backward(rows, codes, idx, torch.zeros_like(rows), one, 0.25, rowmajor=True, need_z=False)[1]
        g_unit = F.vq_orthogonal_backward(saved, sel, count, one * weight)
        if cos:                                               # one normalised codebook: both gradients meet in front of its backward
            want_grad = F.l2norm_rows_backward(unit, denom, g_codes + g_unit)
        else:
            want_grad = g_codes + F.l2norm_rows_backward(unit, denom, g_unit)
    assert 1 <= int(count) <= 64 and ("orthogonal_reg_max_codes" not in orth or int(count) == 5)
    assert float(term) > 0 and bool(torch.isfinite(want_grad).all()) and bool(g_unit.any())
    _check(vq.last_orthogonal_loss, term.cpu().numpy(), "last_orthogonal_loss")
    _check(loss, want_loss.cpu().numpy(), "loss")
    _check(E.grad, want_grad.cpu().numpy(), "embedding.weight.grad")


@pytest.mark.parametrize("cfg", CONFIGS[:4], ids=lambda c: "+".join(c) or "plain")
def test_the_model_trains_with_the_term_and_is_unchanged_without_a_graph(cfg):
    from vqvae_amd import functional as F
    m, m0 = _pair(cfg, dict(orthogonal_reg_weight=0.5))
    vq = m.vector_quantization
    x = torch.randn(2, 3, 32, 32, device=DEV)
    el, xh, pp = m(x)
    el0, xh0, pp0 = m0(x)
    with torch.no_grad():
        term = F.vq_orthogonal_forward(F.l2norm_rows(vq.embedding.weight.detach())[0])[0]
    _check(vq.last_orthogonal_loss, term.cpu().numpy(), "last_orthogonal_loss")
    _check(el, (el0 + 0.5 * term).detach().cpu().numpy(), "training loss")
    _check(xh, xh0.detach().cpu().numpy(), "x_hat")
    _check(pp, pp0.detach().cpu().numpy(), "perplexity")
    (el + xh.square().mean()).backward()
    assert vq.embedding.weight.grad is not None and bool(torch.isfinite(vq.embedding.weight.grad).all())
    m.zero_grad(set_to_none=True)
    # no graph, eval mode, a frozen codebook: the term is not built and every output has the bits of the model without the option
    vq.last_orthogonal_loss = None
    with torch.no_grad():
        for a, b in zip(m(x), m0(x)):
            _check(a, b.cpu().numpy(), "train mode under no_grad")
    m.eval(), m0.eval()
    for a, b in zip(m(x), m0(x)):
        _check(a, b.detach().cpu().numpy(), "eval mode with grad enabled")
    with torch.no_grad():
        for a, b in zip(m(x), m0(x)):
            _check(a, b.cpu().numpy(), "eval mode")
        ia, ib = m.encode(x), m0.encode(x)
        _check(ia, ib.cpu().numpy(), "encode")
        _check(m.decode_indices(ia, 2, 8, 8), m0.decode_indices(ib, 2, 8, 8).cpu().numpy(), "decode_indices")
    m.train(), m0.train()
    vq.embedding.weight.requires_grad_(False), m0.vector_quantization.embedding.weight.requires_grad_(False)
    _check(m(x)[0], m0(x)[0].detach().cpu().numpy(), "a frozen codebook")
    assert vq.last_orthogonal_loss is None


def test_no_random_number_is_drawn_without_a_cap():
    m, _ = _pair(dict(), dict(orthogonal_reg_weight=1.0, orthogonal_reg_active_codes_only=True))
    z = torch.randn(2, 4, 4, 16, device=DEV)
    torch.manual_seed(3)
    m.vector_quantization.quantize(z, rowmajor=True)
    after = torch.rand(4, device=DEV)
    torch.manual_seed(3)
    assert torch.equal(after, torch.rand(4, device=DEV))
    m, _ = _pair(dict(), dict(orthogonal_reg_weight=1.0, orthogonal_reg_max_codes=8))
    torch.manual_seed(3)
    m.vector_quantization.quantize(z, rowmajor=True)                # the default CUDA generator: one draw of K values
    after = torch.rand(4, device=DEV)
    torch.manual_seed(3)
    torch.rand(64, device=DEV)
    assert torch.equal(after, torch.rand(4, device=DEV))
