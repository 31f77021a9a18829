"""The composed quantizer recipe on the GPU: the one-stage quantizer modules with every accepted combination of cosine_sim,
codebook_dim, rotation_trick, the orthogonal term, the code-entropy term and the EMA codebook, and the whole model behind three of
them, against tests/vq_recipe_ref.py -- an fp64 torch autograd composition that shares nothing with vqvae_amd.

THE TOLERANCE, per tensor: e_hip = max |hip - ref64| / max |ref64|, e_32 the same for the reference run in fp32 on the CPU, and
e_hip <= 4 max(e_32, 2^-22) (vq_recipe_ref.bound).  The HIP chain works in fp64 inside each kernel and rounds to fp32 at the kernels'
boundaries, so it should be no worse than a chain that rounds after every operation; the factor 4 covers another summation order
(e_32 is a single sample), the floor of four fp32 ulps of the tensor's maximum a tensor the fp32 composition happens to get exactly.
tests/test_vq_recipe_cpu.py shows that every wiring error it seeds into the reference lies at least 10 bounds outside (the mildest
1.4e3), and that no row of any case is within 1e-4 of a tie.  Indices and histograms are compared exactly.

With VQ_RECIPE_PARITY_OUT set to a file name every comparison appends `case tensor e_hip e_32 ratio` to it (profiles/vq_recipe_parity.txt
is such a file).
"""
import functools
import os

import numpy as np
import pytest
import torch

from tests import vq_ema_ref as EM
from tests import vq_recipe_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MIN_GAP = 1e-4
RESTART = ("cosine_sim", "codebook_dim", "ema")                    # the combination that also runs restart_threshold
RESTART_THRESHOLD = 0.015                                          # N_k = 0.01 count after the first update: codes with one row or none
SINGLE_ROOT = [("rotation_trick",), ("cosine_sim", "codebook_dim", "rotation_trick", "orthogonal", "entropy"),
               ("cosine_sim", "codebook_dim", "rotation_trick", "entropy", "ema")]


def _record(case, name, e_hip, e_32):
    ratio = e_hip / max(e_32, R.FLOOR)
    line = f"{case:78s} {name:26s} e_hip {e_hip:9.3e}  e_32 {e_32:9.3e}  e_hip / max(e_32, 2^-22) {ratio:7.3f}"
    print(line)
    out = os.environ.get("VQ_RECIPE_PARITY_OUT")
    if out:
        with open(out, "a") as fh:
            fh.write(line + "\n")


def _compare(case, got, r64, r32):
    """every tensor of r64 under the bound; all are measured (and recorded) before the first failure is raised"""
    bad = []
    for name, ref in r64.items():
        t = got[name]
        assert t.shape == ref.shape, (case, name, t.shape, ref.shape)
        assert torch.isfinite(t).all(), (case, name)
        e_hip, e_32 = R.rel_err(t, ref), R.rel_err(r32[name], ref)
        _record(case, name, e_hip, e_32)
        if not e_hip <= R.bound(e_32):
            bad.append((name, e_hip, e_32))
    assert not bad, (case, bad)


def _device_uniforms(n):
    """the first torch.rand(n) of a second device generator with the module's seed: the values the module will draw"""
    return torch.rand(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(R.UNIFORM_SEED)).cpu()


def _module(c, params, restart=False):
    """the combination's quantizer from vqvae_amd.modules with the case's parameters, in training mode, its generator seeded"""
    from vqvae_amd import modules as M
    o = R.combo_options(c)
    gen = torch.Generator(device=DEV).manual_seed(R.UNIFORM_SEED)
    kw = dict(rotation_trick=o["rotation_trick"], cosine_sim=o["cosine_sim"], generator=gen)
    if o["entropy_weight"] > 0:
        kw.update(entropy_weight=o["entropy_weight"], entropy_diversity_gamma=o["entropy_gamma"],
                  entropy_inv_temperature=o["entropy_inv_temperature"])
    if o["orth_weight"] > 0:
        kw.update(orthogonal_reg_weight=o["orth_weight"], orthogonal_reg_active_codes_only=o["orth_active_only"],
                  orthogonal_reg_max_codes=o["orth_max_codes"])
    if o["ema"]:
        kw.update(decay=R.EMA_DECAY, eps=R.EMA_EPS, restart_threshold=RESTART_THRESHOLD if restart else None)
    dims = (R.K, R.D, R.CDIM) if o["codebook_dim"] else (R.K, R.D)
    cls = {(False, False): M.VectorQuantizer, (False, True): M.VectorQuantizerEMA, (True, False): M.FactorizedVectorQuantizer,
           (True, True): M.FactorizedVectorQuantizerEMA}[(o["codebook_dim"] is not None, o["ema"])]
    q = cls(*dims, R.BETA, **kw).to(DEV).train()
    own = dict(q.named_parameters())
    assert sorted(own) == sorted(params)
    with torch.no_grad():
        for k, v in params.items():
            own[k].copy_(v)
        if o["ema"]:
            q.ema_w.copy_(params["embedding.weight"])
            q.ema_cluster_size.zero_()
    return q


def _to_layout(rows, rowmajor):
    t = rows.reshape(R.B, R.H, R.W, rows.shape[1])
    return (t if rowmajor else t.permute(0, 3, 1, 2)).contiguous().to(DEV)


def _to_rows(t, rowmajor):
    t = t.detach().cpu()
    t = t if rowmajor else t.permute(0, 2, 3, 1)
    return t.reshape(-1, t.shape[-1])


def _step(q, z, g, rowmajor, root="both"):
    """one forward and backward of the module -> (dict of the tensors _compare reads, idx (N,), hist (K,)); the gradients of the
    module's parameters are left in .grad"""
    for p in q.parameters():
        p.grad = None
    zt = _to_layout(z, rowmajor).requires_grad_(True)
    loss, z_q, perplexity, idx, hist = q.quantize(zt, rowmajor=rowmajor)
    gt = _to_layout(g, rowmajor)
    {"both": lambda: loss + (z_q * gt).sum(), "loss": lambda: loss, "z_q": lambda: (z_q * gt).sum()}[root]().backward()
    torch.cuda.synchronize()
    got = {"total": loss.detach().cpu(), "z_q": _to_rows(z_q, rowmajor), "perplexity": perplexity.detach().cpu(),
           "grad z": _to_rows(zt.grad, rowmajor)}
    if q.orthogonal_reg_weight > 0:
        got["orth"] = q.last_orthogonal_loss.cpu()
    if q.entropy_weight > 0:
        got["ent"] = q.last_entropy_losses.cpu()
    return got, idx.cpu().reshape(-1), hist.cpu()


def _param_grads(q, got, r64, ema, root="both"):
    """the parameters' gradients into `got`.  No gradient at all is accepted only where the reference's is identically zero: an EMA
    codebook (never a gradient), and the parameters behind an output the root does not use."""
    for k, p in q.named_parameters():
        name = "grad " + k
        if p.grad is None:
            assert not r64[name].any(), name
            assert (ema and k == "embedding.weight") or root != "both", name
            got[name] = torch.zeros_like(r64[name], dtype=torch.float32)
        else:
            got[name] = p.grad.cpu()
    if ema:
        assert q.embedding.weight.grad is None and not q.embedding.weight.requires_grad


def _check_indices(case, f64, idx, hist):
    gap = R.relative_gap(f64.d)
    assert int((gap < MIN_GAP).sum()) == 0, (case, float(gap.min()))               # no row is left out
    assert torch.equal(idx, f64.idx), (case, int((idx != f64.idx).sum()))
    assert torch.equal(hist.long(), f64.hist), case


def _check_ema_state(case, q, before, f64, f32, uniforms=None, threshold=None):
    """ema_cluster_size, ema_w and embedding.weight after the forward against vq_ema_ref.ema_update from the reference's y^ and
    indices; e_32: the same update from the fp32 reference's y^"""
    ups = [EM.ema_update(f.rows, f.idx, before["ema_cluster_size"], before["ema_w"], R.EMA_DECAY, R.EMA_EPS, threshold, uniforms)
           for f in (f64, f32)]
    if threshold is not None:
        assert 0 < int(ups[0]["dead"].sum()) < R.K and torch.equal(ups[0]["dead"], ups[1]["dead"])
    got = {"ema_cluster_size": q.ema_cluster_size.cpu(), "ema_w": q.ema_w.cpu(), "embedding.weight (EMA)": q.embedding.weight.detach().cpu()}
    r64, r32 = ({"ema_cluster_size": u["N"], "ema_w": u["m"], "embedding.weight (EMA)": u["e"]} for u in ups)
    _compare(case, got, r64, r32)


@functools.lru_cache(maxsize=None)
def _reference(c, root="both"):
    """the case with its fp64 and fp32 reference runs, computed once and left unchanged.  The cap's uniforms are the module's own
    first draw: a second device generator with its seed."""
    z, g, p, o = R.case(c)
    u = _device_uniforms(R.K) if o["orth_max_codes"] is not None else None
    f64, r64 = R.run(z, p, o, g, u, root=root)
    f32, r32 = R.run(z, p, o, g, u, dtype=torch.float32, root=root)
    return (z, g, p, o), f64, r64, f32, r32


@pytest.mark.parametrize("rowmajor", [True, False], ids=["rowmajor", "nchw"])
@pytest.mark.parametrize("c", R.combinations(), ids=R.combo_id)
def test_every_accepted_combination_against_the_reference(c, rowmajor):
    """indices and histogram exactly; loss, both option terms, perplexity, z_q and every gradient from (loss + sum(z_q g)).backward()
    under the bound; with EMA no codebook gradient and the state after the forward"""
    case = f"{R.combo_id(c)} [{'rowmajor' if rowmajor else 'nchw'}]"
    (z, g, p, o), f64, r64, f32, r32 = _reference(c)
    q = _module(c, p)
    before = {k: v.detach().cpu().clone() for k, v in q.state_dict().items()}
    got, idx, hist = _step(q, z, g, rowmajor)
    _check_indices(case, f64, idx, hist)
    _param_grads(q, got, r64, o["ema"])
    _compare(case, got, r64, r32)
    if o["ema"]:
        _check_ema_state(case, q, before, f64, f32)
    else:
        assert torch.equal(q.embedding.weight.detach().cpu(), before["embedding.weight"])


@pytest.mark.parametrize("root", ["loss", "z_q"])
@pytest.mark.parametrize("c", SINGLE_ROOT, ids=R.combo_id)
def test_backward_from_one_output_alone(c, root):
    """the backward from the loss alone (VQStraightThrough.backward's g_zq is None) and from z_q alone (g_loss is None)"""
    case = f"{R.combo_id(c)} [root {root}]"
    (z, g, p, o), f64, r64, f32, r32 = _reference(c, root)
    q = _module(c, p)
    got, idx, hist = _step(q, z, g, True, root)
    _check_indices(case, f64, idx, hist)
    _param_grads(q, got, r64, o["ema"], root)
    assert r64["grad z"].any()
    _compare(case, got, r64, r32)


@pytest.mark.parametrize("rowmajor", [True, False], ids=["rowmajor", "nchw"])
def test_ema_restart_rows_come_from_the_normalised_projected_rows(rowmajor):
    """restart_threshold with seeded uniforms: the dead codes take rows of y^, the rows the update runs from"""
    case = f"{R.combo_id(RESTART)} restart [{'rowmajor' if rowmajor else 'nchw'}]"
    (z, g, p, o), f64, r64, f32, r32 = _reference(RESTART)
    q = _module(RESTART, p, restart=True)
    before = {k: v.detach().cpu().clone() for k, v in q.state_dict().items()}
    got, idx, hist = _step(q, z, g, rowmajor)
    _check_indices(case, f64, idx, hist)
    _param_grads(q, got, r64, True)
    _compare(case, got, r64, r32)
    _check_ema_state(case, q, before, f64, f32, _device_uniforms(R.K), RESTART_THRESHOLD)


@pytest.mark.parametrize("c", R.WARM_SETS, ids=R.combo_id)
def test_a_second_step_on_warm_state(c):
    """one step, every parameter changed in place under no_grad, the reference re-synced from the module's fp32 values, and a second
    step on other rows under the same bound: a stale normalised codebook, a stale prepared image or a reused workspace shows here"""
    (z, g, p, o), f64, r64, f32, r32 = _reference(c)
    q = _module(c, p)
    got, idx, hist = _step(q, z, g, True)
    _check_indices(R.combo_id(c) + " [step 1]", f64, idx, hist)
    with torch.no_grad():
        for prm in q.parameters():
            if prm.grad is not None:
                prm.add_(-R.WARM_LR * prm.grad)
    now = {k: v.detach().cpu().clone() for k, v in q.named_parameters()}
    assert all(not torch.equal(now[k], p[k]) for k in p)                      # every parameter moved (an EMA codebook by its update)
    before = {k: v.detach().cpu().clone() for k, v in q.state_dict().items()}
    z2, g2, _, _ = R.warm_case(c)
    case = R.combo_id(c) + " [step 2]"
    f64, r64 = R.run(z2, now, o, g2)
    f32, r32 = R.run(z2, now, o, g2, dtype=torch.float32)
    got, idx, hist = _step(q, z2, g2, True)
    _check_indices(case, f64, idx, hist)
    _param_grads(q, got, r64, o["ema"])
    _compare(case, got, r64, r32)
    if o["ema"]:
        _check_ema_state(case, q, before, f64, f32)


@pytest.mark.parametrize("name", list(R.MODEL_SETS))
def test_whole_model_backward_behind_the_recipe(name):
    """VQVAE with an option quantizer: the loss and every parameter gradient of the encoder, the quantizer and the decoder against the
    reference's encoder and decoder (oracle/torch_port.py) around the recipe reference, all fp64, with
    tests/test_training_gpu.py's tolerances -- the conv path's two-term fp16 products dominate here, so the project's own numbers
    apply -- after the near-tie condition on the reference's z_e and equal indices"""
    from tests.test_training_gpu import _close_grad
    from vqvae_amd import conv
    from vqvae_amd.modules import VQVAE
    conv.set_conv_backend("hip")
    c = R.MODEL_SETS[name]
    o = R.combo_options(c)
    h, rh, nres, K, D = R.MODEL_DIMS
    torch.manual_seed(11)
    m = VQVAE(h, rh, nres, K, D, R.BETA, **R.model_kwargs(c)).train()
    x = torch.randn(R.MODEL_B, 3, R.MODEL_HW, R.MODEL_HW)
    sd = {k: v.detach().double().clone().requires_grad_(True) for k, v in m.state_dict().items() if v.dtype.is_floating_point}
    u = _device_uniforms(K) if o["orth_max_codes"] is not None else None
    f, x_hat, loss_ref = R.model_forward(sd, x.double(), nres, o, u)
    gap = R.relative_gap(f.d.detach())
    assert int((gap < MIN_GAP).sum()) == 0, float(gap.min())
    loss_ref.backward()

    md = m.to(DEV)
    vq = md.vector_quantization
    vq.generator = torch.Generator(device=DEV).manual_seed(R.UNIFORM_SEED)
    seen, inner = [], vq.quantize
    vq.quantize = lambda *a, **k: (seen.append(inner(*a, **k)), seen[-1])[1]
    xd = x.to(DEV)
    embedding_loss, x_hat_d, perplexity = md(xd)
    loss = torch.mean((x_hat_d - xd) ** 2) / 0.06 + embedding_loss
    loss.backward()
    torch.cuda.synchronize()
    (out,) = seen
    assert torch.equal(out[3].cpu().reshape(-1), f.idx) and torch.equal(out[4].cpu().long(), f.hist)
    np.testing.assert_allclose(loss.item(), loss_ref.item(), rtol=1e-5)
    np.testing.assert_allclose(perplexity.item(), f.perplexity.item(), rtol=1e-5)
    worst = {}
    for k, p in md.named_parameters():
        ref = sd[k].grad
        if o["ema"] and k == "vector_quantization.embedding.weight":
            assert ref is None and p.grad is None
            continue
        assert ref is not None and p.grad is not None and bool(ref.any()), k
        _close_grad(p.grad, ref.float(), k)
        if ref.dim() == 4:                                   # per filter slice as well, as test_full_model_backward_on_hip_matches_cpu_reference
            err = (p.grad.cpu().double() - ref).abs()
            m0, m1 = ref.abs().amax(dim=(1, 2, 3), keepdim=True), ref.abs().amax(dim=(0, 2, 3), keepdim=True)
            worst[k] = float((err / (2e-4 * ref.abs() + 2e-5 * torch.maximum(m0, m1) + 1e-30)).max())
    print("\n   weight gradients, worst error / per-slice limit:", {k.split(".weight")[0][-28:]: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst
