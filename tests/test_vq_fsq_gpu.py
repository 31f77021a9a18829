"""Finite scalar quantization on the GPU: functional.fsq_forward / fsq_decode_indices, training.fsq_backward (vqvae_fsq_*_f32), the
FiniteScalarQuantizer module and VQVAE(fsq_levels=...) against the CPU restatement tests/vq_fsq_ref.py, whose arithmetic is the header
of vqvae_amd/csrc/vq_fsq.hip.

The device's fp64 tanh is not guaranteed correctly rounded, so indices are compared on rows whose every b lies more than 1e-9 from a
half-integer (a tanh a few ulps off moves b by about 1e-15); the seeded inputs leave out no row (tests/test_vq_fsq_cpu.py checks that).
z_q and the decode depend on the indices only, through correctly rounded operations: bit-equal.  grad_z and the parameter gradients
carry tanh's error and get the bounds written next to them."""
import functools

import numpy as np
import pytest
import torch

from tests import vq_fsq_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _dev(a, offset=False):
    """a numpy array on the device; offset: one float into a larger buffer, so that no 16-byte access path takes it"""
    t = torch.from_numpy(np.array(a, order="C"))               # (a copy: the cases' arrays are read-only)
    if not offset:
        return t.to(DEV)
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _layout(rows, B, H, W, rowmajor, offset=False):
    z = np.ascontiguousarray(rows).reshape(B, H, W, rows.shape[1])
    return _dev(z if rowmajor else z.transpose(0, 3, 1, 2), offset)


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
def _case(B, D, H, W, levels):
    """inputs and the restatement (forward, backward, plain parameter sums), computed once and left unchanged"""
    z, g, w_in, b_in, w_out, b_out = R.gpu_case_inputs(B, D, H, W, levels)
    f = R.forward(z, w_in, b_in, w_out, b_out, levels)
    r = R.backward(z, g, w_in, b_in, w_out, levels)
    pg, mags = R.param_grads(r)
    for a in (z, g, w_in, b_in, w_out, b_out, f.idx, f.z_q, f.hist, r.grad_z):
        a.setflags(write=False)
    return (z, g, w_in, b_in, w_out, b_out), f, r, pg, mags


def _run(case, B, H, W, levels, rowmajor, offset=False):
    """forward, decode of the forward's indices, and backward on the device -> dict of numpy arrays in row order"""
    from vqvae_amd import functional as F, training as T
    z, g, w_in, b_in, w_out, b_out = case
    zt, gt = _layout(z, B, H, W, rowmajor, offset), _layout(g, B, H, W, rowmajor, offset)
    p = [_dev(a, offset) for a in (w_in, b_in, w_out, b_out)]
    z_q, ppl, idx, hist = F.fsq_forward(zt, *p, levels, rowmajor=rowmajor)
    idx_only = F.fsq_forward(zt, *p, levels, rowmajor=rowmajor, want_zq=False, want_hist=False)
    assert idx_only[0] is None and idx_only[1] is None and idx_only[3] is None
    dec = F.fsq_decode_indices(idx, p[2], p[3], levels, B, H, W, rowmajor=rowmajor)
    gz, gp = T.fsq_backward(zt, gt, p[0], p[1], p[2], levels, rowmajor=rowmajor)
    gz_alone, none = T.fsq_backward(zt, gt, p[0], p[1], p[2], levels, rowmajor=rowmajor, need_params=False)
    assert none is None
    torch.cuda.synchronize()
    assert idx.shape == (B * H * W, 1) and z_q.shape == zt.shape and dec.shape == zt.shape and gz.shape == zt.shape
    return dict(z_q=_rows(z_q, rowmajor), ppl=float(ppl), idx=idx.view(-1).cpu().numpy(), idx_only=idx_only[2].view(-1).cpu().numpy(),
                hist=hist.cpu().numpy(), dec=_rows(dec, rowmajor), grad_z=_rows(gz, rowmajor), gz_alone=_rows(gz_alone, rowmajor),
                w_in=gp[0].cpu().numpy(), b_in=gp[1].cpu().numpy(), w_out=gp[2].cpu().numpy(), b_out=gp[3].cpu().numpy())


FLOATS = ("z_q", "dec", "grad_z", "gz_alone", "w_in", "b_in", "w_out", "b_out")


def _same_run(a, b, what):
    assert np.array_equal(a["idx"], b["idx"]) and np.array_equal(a["hist"], b["hist"]) and a["ppl"] == b["ppl"], what
    for n in FLOATS:
        _same_bits_nan_aside(a[n], b[n], f"{what}: {n}")


@pytest.mark.parametrize("B,D,H,W,levels", R.GPU_CASES)
def test_against_the_restatement_in_both_layouts_and_on_both_paths(B, D, H, W, levels):
    case, f, r, pg, mags = _case(B, D, H, W, levels)
    N = B * H * W
    clear = R.clear_rows(f, 1e-9)
    assert clear.all()                                         # (at most 1 % may be left out; these inputs leave out none)
    runs = {(rm, off): _run(case, B, H, W, levels, rm, off) for rm in (True, False) for off in (False, True)}
    again = _run(case, B, H, W, levels, True)
    got = runs[(True, False)]
    # reproducibility: every output bit-equal between the layouts, between the aligned and the offset path, and between two runs
    _same_run(got, again, "second run")
    for key, other in runs.items():
        _same_run(got, other, f"rowmajor={key[0]} offset={key[1]}")
    # the index, on the compared rows (all of them), and what follows from it bit for bit
    assert np.array_equal(got["idx"][clear], f.idx[clear]) and np.array_equal(got["idx_only"], got["idx"])
    assert ((got["idx"] >= 0) & (got["idx"] < f.k.K)).all()
    _same_bits_nan_aside(got["z_q"][clear], f.z_q[clear], "z_q")
    _same_bits_nan_aside(got["dec"], got["z_q"], "decode vs the forward's z_q")
    assert np.array_equal(got["hist"], f.hist) and got["hist"].sum() == N
    np.testing.assert_allclose(got["ppl"], float(f.perplexity), rtol=1e-6)
    # grad_z: one fp32 rounding plus a 4-ulp fp64 allowance on tanh through 1 - t^2 (vq_fsq_ref.grad_z_bound has the derivation)
    err, bound = np.abs(got["grad_z"].astype(np.float64) - r.grad_z.astype(np.float64)), R.grad_z_bound(r, case[2])
    print(f"grad_z: max err / bound = {(err / bound).max():.4f}")
    assert (err <= bound).all()
    _same_bits_nan_aside(got["gz_alone"], got["grad_z"], "grad_z without the parameter gradients")
    # parameter gradients: one fp32 rounding plus the fp64 accumulation error over at most 2^12 rows.  Every one of the N - 1
    # additions rounds a partial sum no larger than sum |term| by at most 2^-53 of it: N 2^-53 <= 2^-41 for N <= 2^12, the same
    # again for the plain sums they are compared with, and tanh's few ulps on the terms that carry t (c^ does not): 2^-40.
    assert N <= 2 ** 12
    for n in ("w_out", "b_out", "w_in", "b_in"):
        ref = pg[n].astype(np.float64)
        err, bound = np.abs(got[n].astype(np.float64) - ref), 2.0 ** -23 * np.abs(ref) + 2.0 ** -40 * mags[n] + 2.0 ** -149
        print(f"grad_{n}: max err / bound = {(err / bound).max():.4f}")
        assert (err <= bound).all(), n


def test_saturation_and_special_rows():
    """rows of +-1e4 saturate to the outermost levels, a zero row quantizes b_in; a NaN or an Inf makes its own row of z_q NaN with idx
    in [0, K) and touches no other row; out-of-range indices decode to NaN rows"""
    from vqvae_amd import functional as F, training as T
    B, D, H, W, levels = 2, 64, 4, 4, (8, 5, 5, 5)
    z, g, w_in, b_in, w_out, b_out = [a.copy() for a in R.draw(B * H * W, D, levels, 5)]
    z[1], z[2], z[3] = 1e4, -1e4, 0.0
    z[4, D // 2] = np.nan
    z[5], z[6, 0] = np.inf, -np.inf
    g[7, D - 1] = np.nan
    f = R.forward(z, w_in, b_in, w_out, b_out, levels)
    r = R.backward(z, g, w_in, b_in, w_out, levels)
    bad = [4, 5, 6]
    assert np.isnan(f.z_q[bad]).all() and np.isfinite(np.delete(f.z_q, bad, axis=0)).all()
    clear = R.clear_rows(f, 1e-9)
    assert clear[[0, 1, 2, 3]].all() and clear.sum() >= 32 - 4
    sat = R.codes(np.full((1, 4), 1e4, np.float32), f.k)[0][0]
    assert np.array_equal(sat, np.array([(l - 1 - l // 2) / (l // 2) for l in levels], np.float32))
    for rowmajor in (True, False):
        p = [_dev(a) for a in (w_in, b_in, w_out, b_out)]
        zt, gt = _layout(z, B, H, W, rowmajor), _layout(g, B, H, W, rowmajor)
        z_q, ppl, idx, hist = F.fsq_forward(zt, *p, levels, rowmajor=rowmajor)
        gz, gp = T.fsq_backward(zt, gt, p[0], p[1], p[2], levels, rowmajor=rowmajor)
        idx_n = idx.view(-1).cpu().numpy()
        assert ((idx_n >= 0) & (idx_n < f.k.K)).all() and int(hist.sum()) == B * H * W
        assert np.array_equal(idx_n[clear], f.idx[clear]) and np.array_equal(idx_n[bad], f.idx[bad])
        _same_bits_nan_aside(_rows(z_q, rowmajor), f.z_q, "z_q")                 # NaN rows in their places, every other row's bits
        gz_n = _rows(gz, rowmajor)
        assert np.array_equal(np.isnan(gz_n), np.isnan(r.grad_z)) and np.isnan(gz_n[7]).all() and np.isfinite(gz_n[[0, 1, 2, 3]]).all()
        ok = ~np.isnan(r.grad_z)
        assert (np.abs(gz_n.astype(np.float64) - r.grad_z)[ok] <= R.grad_z_bound(r, w_in)[ok]).all()
        assert all(bool(torch.isnan(t).any()) for t in gp)                       # the sums over rows do meet the NaN rows
        # decode: the forward's z_q on every row, NaN rows for indices out of range, an IndexError where the caller asks for the check
        dec = F.fsq_decode_indices(idx, p[2], p[3], levels, B, H, W, rowmajor=rowmajor)
        d_n = _rows(dec, rowmajor)
        keep = np.delete(np.arange(B * H * W), bad)
        _same_bits_nan_aside(d_n[keep], f.z_q[keep], "decode")
        assert np.isfinite(d_n[bad]).all()                                       # (the index of a NaN row is an ordinary index)
        wild = idx.clone()
        wild[0], wild[9], wild[31] = -1, f.k.K, 1 << 40
        with pytest.raises(IndexError):
            F.fsq_decode_indices(wild, p[2], p[3], levels, B, H, W, rowmajor=rowmajor)
        w_n = _rows(F.fsq_decode_indices(wild, p[2], p[3], levels, B, H, W, rowmajor=rowmajor, validate=False), rowmajor)
        assert np.isnan(w_n[[0, 9, 31]]).all()
        _same_bits_nan_aside(np.delete(w_n, [0, 9, 31], axis=0), np.delete(d_n, [0, 9, 31], axis=0), "decode beside the bad indices")


# ---- the module and the model ----------------------------------------------------------------------------------------------------

LV = (8, 5, 5, 5)


def _model(levels=LV, K=1000, **kw):
    from vqvae_amd import conv
    from vqvae_amd.modules import VQVAE
    conv.set_conv_backend("hip")
    torch.manual_seed(0)
    m = VQVAE(32, 8, 1, K, 16, 0.25, fsq_levels=levels, **kw).to(DEV)
    with torch.no_grad():                                       # a projection wide enough that many codes are in use: y of unit scale
        z_e = conv.encoder_forward(m.encoder, _x(), pre_quant=m.pre_quantization_conv)
        w = m.vector_quantization.project_in.weight
        w.copy_(torch.randn(w.shape, generator=torch.Generator().manual_seed(7)).to(DEV) * (1.5 / (4.0 * float(z_e.std()))))
    return m


def _x(B=4):
    return torch.randn(B, 3, 32, 32, generator=torch.Generator().manual_seed(1)).to(DEV)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def test_module_against_the_restatement():
    from vqvae_amd.modules import FiniteScalarQuantizer, LazyOneHot
    B, D, H, W, levels = 4, 64, 8, 8, LV
    case, f, r, pg, mags = _case(B, D, H, W, levels)
    q = FiniteScalarQuantizer(levels, D).to(DEV)
    with torch.no_grad():
        for p, a in zip(q._params(), case[2:]):
            p.copy_(_dev(a))
    with torch.no_grad():
        loss, z_q, ppl, onehot, idx = q(_layout(case[0], B, H, W, False))
        assert isinstance(onehot, LazyOneHot) and onehot.shape == (256, 1000) and float(loss) == 0.0 and loss.dim() == 0
        _same_bits_nan_aside(_rows(z_q, False), f.z_q, "module z_q")
        assert np.array_equal(idx.view(-1).cpu().numpy(), f.idx)
        assert torch.equal(onehot.argmax(1), idx.view(-1))
        assert torch.equal(q.codes().cpu(), torch.from_numpy(R.all_codes(levels)))
        _same_bits_nan_aside(q.codebook().cpu().numpy(), R.decode(np.arange(1000), case[4], case[5], levels), "codebook()")
    z = _layout(case[0], B, H, W, True).requires_grad_(True)
    loss, z_q, ppl, idx, hist = q.quantize(z, rowmajor=True)
    assert z_q.requires_grad and not idx.requires_grad and not hist.requires_grad and not ppl.requires_grad and not loss.requires_grad
    z_q.backward(_layout(case[1], B, H, W, True))
    assert (np.abs(_rows(z.grad, True).astype(np.float64) - r.grad_z) <= R.grad_z_bound(r, case[2])).all()
    for n, p in zip(("w_in", "b_in", "w_out", "b_out"), q._params()):
        ref = pg[n].astype(np.float64)
        assert (np.abs(p.grad.cpu().numpy() - ref) <= 2.0 ** -23 * np.abs(ref) + 2.0 ** -40 * mags[n] + 2.0 ** -149).all(), n
    from vqvae_amd._lib import VqvaeHipError
    with pytest.raises(VqvaeHipError):
        q(torch.zeros(1, D, 2, 2))                              # CPU tensors raise


def test_model_decode_indices_of_encode_equals_the_forward():
    m, x = _model().eval(), _x()
    with torch.no_grad():
        loss, x_hat, ppl = m(x)
        idx = m.encode(x)
        dec = m.decode_indices(idx, 4, 8, 8)
    assert loss.dim() == 0 and float(loss) == 0.0 and x_hat.shape == x.shape and float(ppl) > 1.0
    assert idx.shape == (256, 1) and int(idx.min()) >= 0 and int(idx.max()) < 1000 and idx.unique().numel() > 8
    assert np.array_equal(_bits(dec), _bits(x_hat))
    with pytest.raises(IndexError):
        m.decode_indices(torch.full_like(idx, 1000), 4, 8, 8)
    m.train()
    _, x_hat_train, ppl_train = m(x)                            # the training forward: the same indices, the kernel's own z_q
    assert float(ppl_train) == float(ppl)
    np.testing.assert_allclose(x_hat_train.detach().cpu().numpy(), x_hat.cpu().numpy(), atol=1e-6, rtol=1e-5)
    from vqvae_amd._lib import VqvaeHipError
    with pytest.raises(VqvaeHipError):
        m.init_codebook_(x)


def test_model_training_step_matches_the_torch_composition():
    """the same model, its quantizer replaced by fp64 torch ops under autograd (y rounded to fp32 as the contract rounds it, so the
    indices are the kernels'): the quantizer's parameter gradients within one fp32 rounding plus 2^-40 sum |term| of the CPU
    restatement and of the composition, the other parameters within the training tests' tolerance"""
    from vqvae_amd import training as T
    m, x = _model().train(), _x()
    vq = m.vector_quantization
    seen = {}
    hip_quantize = vq.quantize

    def spy(z, *, rowmajor=False, want_zq=True):
        out = hip_quantize(z, rowmajor=rowmajor, want_zq=want_zq)
        seen["z"] = z.detach().clone()
        out[1].register_hook(lambda gr: seen.__setitem__("g", gr.detach().clone()))
        return out

    def composed(z, *, rowmajor=False, want_zq=True):
        w_in, b_in, w_out, b_out = [p.double() for p in vq._params()]
        z_q = R.torch_composition(z.double(), w_in, b_in, w_out, b_out, LV, round_y=True).float()
        return torch.zeros((), device=z.device), z_q, seen["ppl"], seen["idx"], None

    def step(quantize):
        vq.quantize = quantize
        m.zero_grad(set_to_none=True)
        el, xh, pp = m(x)
        T.step_losses(el, xh, pp, x, 0.06)[1].backward()
        torch.cuda.synchronize()
        return xh.detach().clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}

    xh_hip, g_hip = step(spy)
    with torch.no_grad():
        seen["ppl"], seen["idx"] = hip_quantize(seen["z"], rowmajor=True)[2:4]
    xh_ref, g_ref = step(composed)
    del vq.quantize
    assert np.array_equal(_bits(xh_hip), _bits(xh_ref))         # z_q is bit-equal, so the decoder's input is
    r = R.backward(_rows(seen["z"], True), _rows(seen["g"], True), *[p.detach().cpu().numpy() for p in vq._params()[:3]], LV)
    pg, mags = R.param_grads(r)
    names = {"w_in": "vector_quantization.project_in.weight", "b_in": "vector_quantization.project_in.bias",
             "w_out": "vector_quantization.project_out.weight", "b_out": "vector_quantization.project_out.bias"}
    for n, full in names.items():
        got = g_hip[full].cpu().numpy().astype(np.float64)
        for what, ref in (("restatement", pg[n].astype(np.float64)), ("composition", g_ref[full].cpu().numpy().astype(np.float64))):
            assert (np.abs(got - ref) <= 2.0 ** -23 * np.abs(ref) + 2.0 ** -40 * mags[n] + 2.0 ** -149).all(), (n, what)
        assert float(np.abs(got).max()) > 0
    for full, ref in g_ref.items():
        if full not in names.values():
            scale = float(ref.abs().max())
            np.testing.assert_allclose(g_hip[full].cpu().numpy(), ref.cpu().numpy(), rtol=2e-4, atol=2e-5 * scale, err_msg=full)


def test_model_adam_steps_state_dict_and_default_model():
    from vqvae_amd import training as T
    m, x = _model().train(), _x(8)
    vq = m.vector_quantization
    before = [p.detach().clone() for p in vq._params()]
    opt = torch.optim.Adam(m.parameters(), lr=2e-3)
    losses = []
    for _ in range(6):
        opt.zero_grad(set_to_none=True)
        el, xh, pp = m(x)
        stats = T.step_losses(el, xh, pp, x, 0.06)
        stats[1].backward()
        opt.step()
        losses.append(float(stats[0]))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    for b, p in zip(before, vq._params()):
        assert not torch.equal(b, p.detach())
    # state_dict round trip: the four projection tensors and nothing else for the quantizer; the same outputs after loading
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    assert [k for k in sd if k.startswith("vector_quantization.")] == [
        "vector_quantization.project_in.weight", "vector_quantization.project_in.bias",
        "vector_quantization.project_out.weight", "vector_quantization.project_out.bias"]
    m2 = _model().eval()
    m2.load_state_dict(sd)
    m.eval()
    with torch.no_grad():
        a, b = m(x), m2(x)
        for p, q in zip(a, b):
            assert np.array_equal(_bits(p), _bits(q))
        assert torch.equal(m.encode(x), m2.encode(x))


def test_model_forward_captures_into_a_graph():
    m = _model().eval()
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
                assert np.array_equal(_bits(p), _bits(q))


@pytest.mark.parametrize("rowmajor", [True, False])
def test_forward_decode_and_backward_capture_into_a_graph(rowmajor):
    """a linear chain on one stream: forward (its histogram cleared by the chain itself), decode, backward; captured and replayed on
    new inputs, with other values left in the outputs between the replays"""
    from vqvae_amd import functional as F, training as T
    B, D, H, W, levels = 4, 64, 8, 8, LV
    case, f, r, pg, mags = _case(B, D, H, W, levels)
    want = _run(case, B, H, W, levels, rowmajor)
    zs, gs = torch.zeros_like(_layout(case[0], B, H, W, rowmajor)), torch.zeros_like(_layout(case[1], B, H, W, rowmajor))
    p = [_dev(a) for a in case[2:]]

    def chain():
        z_q, ppl, idx, hist = F.fsq_forward(zs, *p, levels, rowmajor=rowmajor)
        dec = F.fsq_decode_indices(idx, p[2], p[3], levels, B, H, W, rowmajor=rowmajor)
        gz, gp = T.fsq_backward(zs, gs, p[0], p[1], p[2], levels, rowmajor=rowmajor)
        return z_q, ppl, idx, hist, dec, gz, gp

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        chain()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        z_q, ppl, idx, hist, dec, gz, gp = chain()
    zs.copy_(_layout(case[0], B, H, W, rowmajor))
    gs.copy_(_layout(case[1], B, H, W, rowmajor))
    for i in range(2):
        graph.replay()
        torch.cuda.synchronize()
        got = dict(z_q=_rows(z_q, rowmajor), ppl=float(ppl), idx=idx.view(-1).cpu().numpy(), hist=hist.cpu().numpy(), dec=_rows(dec, rowmajor),
                   grad_z=_rows(gz, rowmajor), gz_alone=_rows(gz, rowmajor), w_in=gp[0].cpu().numpy(), b_in=gp[1].cpu().numpy(),
                   w_out=gp[2].cpu().numpy(), b_out=gp[3].cpu().numpy())
        _same_run(got, want, f"replay {i}")
        hist.fill_(1000)
        ppl.fill_(-1.0)
        z_q.fill_(7.0)


def test_sample_and_complete_images_with_a_small_prior():
    from vqvae_amd.pixelcnn import GatedPixelCNN, complete_images, sample_images
    m = _model((4, 4, 4), 64).eval()
    torch.manual_seed(3)
    prior = GatedPixelCNN(64, 16, 3, 10).eval().to(DEV)
    gen = torch.Generator().manual_seed(4)
    label = torch.randint(0, 10, (4,), generator=gen).to(DEV)
    u = torch.rand((4, 8, 8), generator=gen).to(DEV)
    idx, x_hat = sample_images(prior, m, label, (8, 8), 4, uniforms=u)
    assert idx.shape == (4, 8, 8) and x_hat.shape == (4, 3, 32, 32) and int(idx.min()) >= 0 and int(idx.max()) < 64
    with torch.no_grad():
        assert np.array_equal(_bits(x_hat), _bits(m.decode_indices(idx, 4, 8, 8)))
    x = _x()
    idx2, x_hat2 = complete_images(prior, m, x, label, 4, uniforms=u)
    with torch.no_grad():
        enc = m.encode(x).reshape(4, 8, 8)
        assert torch.equal(idx2[:, :4], enc[:, :4])
        assert np.array_equal(_bits(x_hat2), _bits(m.decode_indices(idx2, 4, 8, 8)))
    assert bool(torch.isfinite(x_hat).all()) and bool(torch.isfinite(x_hat2).all())
