"""The composed quantizer recipe without a GPU: the independent reference (tests/vq_recipe_ref.py) against the restatements the
suite already pins, the near-tie condition of every case the GPU tests run, and the proof that the GPU tests' tolerance tells a wrong
graph from rounding.

The tolerance of tests/test_vq_recipe_gpu.py, per tensor: e = max |got - ref64| / max |ref64|, e_32 the same for the reference run in
fp32 on the CPU, and e_hip <= 4 max(e_32, 2^-22) (vq_recipe_ref.bound).  Everything that forms it is computed here, on the CPU.

Measured at the cases of this file (N = 105, D = 16, d = 8, K = 32, seed 0): the smallest relative gap between a row's best and
second-best squared distance is 1.4e-3 over the four search configurations; the fp32 composition picks the fp64 indices in all 48
combinations and its own error is at most 7.3e-6 (grad embedding.weight with the entropy term).  The mildest mutation is the swapped
beta, 1.4e3 bounds away on grad embedding.weight; 'orth_renormalised' moves nothing (5e-12 bounds) and cannot: see the reference's
docstring and test_renormalising_the_unit_codebook_is_an_identity.
"""
import functools

import numpy as np
import pytest
import torch

from tests import vq_recipe_ref as R

MIN_GAP = 1e-4
GRADED = lambda k: k == "total" or k.startswith("grad ")        # the tensors a mutation is graded on: the loss and the gradients


def _uniforms():
    return torch.rand(R.K, generator=torch.Generator().manual_seed(R.UNIFORM_SEED))


@functools.lru_cache(maxsize=None)
def _runs(c):
    """the case of a combination with its fp64 and fp32 runs and the per-tensor bound: computed once, left unchanged"""
    z, g, p, o = R.case(c)
    f64, r64 = R.run(z, p, o, g, _uniforms())
    f32, r32 = R.run(z, p, o, g, _uniforms(), dtype=torch.float32)
    bound = {k: R.bound(R.rel_err(r32[k], r64[k])) for k in r64}
    return (z, g, p, o), f64, r64, f32, bound


def _np(t):
    return t.detach().numpy()


# ---- the reference against the restatements, each within its own bound ------------------------------------------------------------------

def test_rotation_alone_is_the_rotation_restatement():
    from tests import vq_rotation_ref as RR
    (z, g, p, o), f, _, _, _ = _runs(("rotation_trick",))
    _, r = R.run(z, p, o, g, root="z_q")
    q = p["embedding.weight"][f.idx]
    want, lam_gnorm, value_err = RR.autograd_rot(_np(z), _np(q), _np(g))
    assert value_err.max() < 1e-14                                                       # the output has the value of q
    assert np.abs(_np(r["grad z"]) - want).max() <= 1e-13 * np.abs(want).max()
    got32, rotated = RR.rot(_np(z), _np(q), _np(g))
    assert rotated.all() and (np.abs(got32 - _np(r["grad z"])) <= RR.bound(_np(r["grad z"]), lam_gnorm)).all()
    assert not np.array_equal(want, _np(g).astype(np.float64))                           # and it is not the straight-through gradient


def test_cosine_alone_is_the_cosine_restatement():
    from tests import vq_cosine_ref as CR
    (z, g, p, o), f, r, _, _ = _runs(("cosine_sim",))
    zn, En, chain = CR.quantize(_np(z), _np(p["embedding.weight"]), R.BETA)
    assert (np.abs(zn - _np(f.rows)) <= CR.forward_bound(_np(f.rows))).all()
    assert (np.abs(En - _np(f.codes)) <= CR.forward_bound(_np(f.codes))).all()
    assert np.array_equal(np.asarray(chain.idx[0]).reshape(-1), _np(f.idx))
    # (the chain's loss is of fp32 unit rows: 2^-22 relative covers their rounding in a mean of squared differences)
    assert abs(float(chain.loss) - float(r["total"])) <= 2.0 ** -22 * float(r["total"])
    assert abs(float(chain.perplexity[0]) - float(r["perplexity"])) <= 1e-12 * float(r["perplexity"])
    # straight-through: d z_q / d z^ = I, so the gradient of sum(z_q g) is the normalisation's backward of g
    _, rz = R.run(z, p, o, g, root="z_q")
    y, denom = CR.l2norm(_np(z))
    got = CR.l2norm_backward(y, denom, _np(g))
    assert (np.abs(got - _np(rz["grad z"])) <= CR.backward_bound(_np(z), _np(g))[:, None]).all()
    _, want = CR.torch_normalize(_np(z), _np(g))
    assert np.abs(_np(rz["grad z"]) - want).max() <= 1e-13 * np.abs(want).max()


def test_codebook_dim_alone_is_the_linear_restatement():
    from tests import vq_linear_ref as LR
    (z, g, p, o), f, _, _, _ = _runs(("codebook_dim",))
    w_in, b_in, w_out = (_np(p[k]) for k in ("project_in.weight", "project_in.bias", "project_out.weight"))
    y = LR.forward(_np(z), w_in, b_in)
    assert (np.abs(y - _np(f.rows)) <= 2.0 ** -24 * np.abs(_np(f.rows)) + 2.0 ** -149).all()
    # from z_q alone: grad project_out = the sums over the rows of g and the codes, grad z = W_in^T W_out^T g (straight-through)
    _, r = R.run(z, p, o, g, root="z_q")
    q = _np(f.codes[f.idx])
    (gw, gb), (mw, mb) = LR.param_grads(q, _np(g))
    assert (np.abs(gw - _np(r["grad project_out.weight"])) <= 2.0 ** -45 * mw).all()
    assert (np.abs(gb - _np(r["grad project_out.bias"])) <= 2.0 ** -45 * mb).all()
    g_low = LR.grad_x(_np(g), w_out)                                                      # fp32: one rounding per element
    g_z = LR.grad_x(g_low, w_in)
    want = _np(r["grad z"])
    scale = np.abs(_np(g)).astype(np.float64) @ np.abs(w_out) @ np.abs(w_in)                  # the magnitude the two roundings are relative to
    assert (np.abs(g_z - want) <= 2.0 ** -23 * scale).all()
    (gw, gb), (mw, mb) = LR.param_grads(_np(z), g_low)
    assert (np.abs(gw - _np(r["grad project_in.weight"])) <= 2.0 ** -24 * (np.abs(_np(g)).astype(np.float64) @ np.abs(w_out)).T @ np.abs(_np(z))).all()
    assert (np.abs(gb - _np(r["grad project_in.bias"])) <= 2.0 ** -24 * (np.abs(_np(g)).astype(np.float64) @ np.abs(w_out)).sum(0)).all()


def test_the_orthogonal_term_is_the_orthogonal_restatement():
    """on the restatement's own operands -- the fp32 unit rows -- with this case's histogram and uniforms, under the bounds
    tests/test_vq_orthogonal_cpu.py derives for fp64 autograd of the same formula"""
    from tests import vq_cosine_ref as CR, vq_orthogonal_ref as OR
    (z, g, p, o), f, r, _, _ = _runs(("orthogonal",))
    u = _uniforms()
    rows, _ = CR.l2norm(_np(p["embedding.weight"]))
    K, D = rows.shape
    loss, M, sel, V = OR.forward(rows, _np(f.hist).astype(np.int32), _np(u), o["orth_max_codes"])
    chosen = R.select_codes(K, f.hist, True, o["orth_max_codes"], u)
    assert M == 20 < int((f.hist > 0).sum()) < K and np.array_equal(np.flatnonzero(sel), chosen)     # the histogram and the cap both select
    n = torch.from_numpy(rows.astype(np.float64)).requires_grad_(True)
    ref = R.orthogonal_term(n, chosen)
    ref.backward()
    ref = ref.detach()
    s2 = float(ref) + 1.0 / M
    assert abs(float(loss) - float(ref)) <= 2.0 ** -24 * abs(float(ref)) + 2.0 ** -53 * (4 * D * np.sqrt(s2) + 2 * (K + 322) * s2 + 4 * max(s2, 1.0))
    grad = OR.backward(V, sel, M, None)
    mag = (4.0 / (M * M)) * np.abs(rows.astype(np.float64))[sel != 0].sum(0)[None, :]
    assert (np.abs(grad - _np(n.grad)) <= 2.0 ** -24 * np.abs(_np(n.grad)) + (2 * D + 2 * K + 8) * 2.0 ** -53 * mag + 2.0 ** -149).all()
    # and the single-option run's term is this formula on the fp64 unit rows: the fp32 rounding of the rows moves G by 2^-22 at most
    assert abs(float(r["orth"]) - float(ref)) <= 4 * 2.0 ** -22 * s2


def test_the_entropy_term_is_the_entropy_restatement():
    from tests import vq_entropy_ref as ER
    (z, g, p, o), f, r, _, _ = _runs(("entropy",))
    s, gamma, w = o["entropy_inv_temperature"], o["entropy_gamma"], o["entropy_weight"]
    zn, En = _np(z), _np(p["embedding.weight"])
    ef = ER.forward(zn, En, s, gamma)
    fb = ER.fwd_bounds(ef, zn.shape[0], En.shape[0], zn.shape[1], s, gamma)
    for got, want, b in zip(_np(r["ent"]), (ef.term, ef.P, ef.H), (fb["term"], fb["P"], fb["H"])):
        assert abs(got - want) <= ER.SIDES * b
    assert float(ef.P) > 0.1 and (ef.p > 0.1 / En.shape[0]).sum(1).min() >= 2             # several codes carry mass: the term has a gradient
    # the term's own gradients: the run with the option minus the run without it, both from the loss alone
    _, on = R.run(z, p, o, root="loss")
    _, off = R.run(z, p, R.combo_options(()), root="loss")
    eb = ER.backward(zn, En, ef.avg, ef.rowstat, w, s, gamma)
    b_gz, b_gE = ER.bwd_bounds(eb, ef, zn, En, w, s, gamma)
    for name, want, b in (("grad z", eb.grad_z64, b_gz), ("grad embedding.weight", eb.grad_E64, b_gE)):
        got = _np(on[name] - off[name])
        assert np.abs(want).max() > 1e-4
        assert (np.abs(got - want) <= ER.SIDES * b + 2.0 ** -50 * np.abs(_np(off[name]))).all(), name


def test_ema_alone_is_the_commitment_gradient():
    from tests import vq_ema_ref as EM
    (z, g, p, o), f, r, _, _ = _runs(("ema",))
    e = p["embedding.weight"][f.idx]
    want = EM.commitment_grad(z, e, g, 1.0, R.BETA)
    assert float((r["grad z"] - want).abs().max()) <= 1e-14 * float(want.abs().max())
    assert not r["grad embedding.weight"].any()
    assert abs(float(r["total"]) - R.BETA * float(((e.double() - z.double()) ** 2).mean())) <= 1e-15


# ---- the cases of the GPU tests ---------------------------------------------------------------------------------------------------------

def test_there_are_48_combinations():
    cs = R.combinations()
    assert len(cs) == len(set(cs)) == 48 and not any("orthogonal" in c and "ema" in c for c in cs)


@pytest.mark.parametrize("c", R.combinations(), ids=R.combo_id)
def test_no_row_is_near_a_tie_and_fp32_picks_the_same_codes(c):
    """every row: (second-best - best) / second-best >= 1e-4 in the fp64 reference.  No row is left out: the cap is zero."""
    _, f64, _, f32, _ = _runs(c)
    gap = R.relative_gap(f64.d)
    left_out = int((gap < MIN_GAP).sum())
    assert left_out == 0, f"{left_out} rows within {MIN_GAP} of a tie, smallest gap {float(gap.min()):.3g}"
    assert torch.equal(f64.idx, f32.idx)
    used = int((f64.hist > 0).sum())
    assert R.ORTH["orth_max_codes"] < used < R.K                    # a few codes are unused, and more are used than the cap keeps


def test_the_model_cases_are_away_from_ties():
    """the three whole-model cases: the same condition on the reference's z_e (the model is drawn on the CPU: no GPU is needed)"""
    for name, c in R.MODEL_SETS.items():
        f = _model_reference(name)[0]
        gap = R.relative_gap(f.d)
        assert int((gap < MIN_GAP).sum()) == 0, (name, float(gap.min()))


@pytest.mark.parametrize("c", R.WARM_SETS, ids=R.combo_id)
def test_the_warm_second_steps_are_away_from_ties(c):
    """the second step of the warm-state tests, at the parameters the reference arrives at after its own first step"""
    z, g, p, o = R.warm_case(c)
    f64, _ = R.run(z, p, o, g)
    f32, r32 = R.run(z, p, o, g, dtype=torch.float32)
    gap = R.relative_gap(f64.d)
    assert int((gap < MIN_GAP).sum()) == 0, float(gap.min())
    assert torch.equal(f64.idx, f32.idx)
    # (after the step a code lies so far from every row that its softmax weight underflows in fp32: 0 log 0 = 0, not a NaN)
    assert all(bool(torch.isfinite(t).all()) for t in r32.values())
    assert not torch.equal(p["embedding.weight"], R.case(c)[2]["embedding.weight"])           # the codebook did move


def _model_reference(name, uniforms=None):
    """-> (namespace, x_hat, loss, sd of fp64 leaves, x fp32) of a whole-model case at its freshly drawn state"""
    from vqvae_amd.modules import VQVAE
    c = R.MODEL_SETS[name]
    h, rh, nres, K, D = R.MODEL_DIMS
    torch.manual_seed(11)
    m = VQVAE(h, rh, nres, K, D, R.BETA, **R.model_kwargs(c))
    x = torch.randn(R.MODEL_B, 3, R.MODEL_HW, R.MODEL_HW)
    sd = {k: v.detach().double().clone().requires_grad_(True) for k, v in m.state_dict().items() if v.dtype.is_floating_point}
    u = uniforms if uniforms is not None else torch.rand(K, generator=torch.Generator().manual_seed(R.UNIFORM_SEED))
    return R.model_forward(sd, x.double(), nres, R.combo_options(c), u) + (sd, x)


# ---- the tolerance discriminates --------------------------------------------------------------------------------------------------------

DISCRIMINATED = [m for m in R.MUTATIONS if m != "orth_renormalised"]


@pytest.mark.parametrize("mutation", DISCRIMINATED)
def test_every_mutation_lies_ten_bounds_outside(mutation):
    """in every combination whose graph the mutation touches, the loss or a gradient moves by at least 10 times its bound"""
    touched = 0
    for c in R.combinations():
        (z, g, p, o), _, r64, _, bound = _runs(c)
        if not R.MUTATIONS[mutation](o):
            continue
        touched += 1
        _, rm = R.run(z, p, o, g, _uniforms(), mutation=mutation)
        moved = {k: R.rel_err(rm[k], r64[k]) / bound[k] for k in r64 if GRADED(k)}
        assert max(moved.values()) >= 10.0, (mutation, R.combo_id(c), moved)
    assert touched >= 8


def test_renormalising_the_unit_codebook_is_an_identity():
    """'orth_renormalised' is the one listed slip that is no error: normalising unit rows again changes neither the value nor -- the
    tangent projection being idempotent -- any gradient.  Stated as an equality, so that nobody reads a later difference as rounding."""
    for c in R.combinations():
        (z, g, p, o), _, r64, _, bound = _runs(c)
        if not R.MUTATIONS["orth_renormalised"](o):
            continue
        _, rm = R.run(z, p, o, g, _uniforms(), mutation="orth_renormalised")
        for k in r64:
            assert R.rel_err(rm[k], r64[k]) <= 1e-12, (R.combo_id(c), k)


def test_the_bound_is_formed_as_stated():
    assert R.bound(0.0) == 4 * 2.0 ** -22 and R.bound(1e-5) == 4e-5 and R.FACTOR == 4.0
    assert R.rel_err(torch.zeros(3), torch.zeros(3)) == 0.0 and R.rel_err(torch.ones(3), torch.zeros(3)) == float("inf")
    # the fp32 composition's own error stays small: the bound is a rounding bound in every combination
    bounds = [v for c in R.combinations() for v in _runs(c)[4].values()]
    assert all(np.isfinite(v) for v in bounds) and max(bounds) <= 4 * 1e-5
