"""fp64 numpy restatement of the optimizer step of vqvae_amd/csrc/optim.hip (Adam / AMSGrad / AdamW with an optional global-norm
clip), the input family the optimizer tests draw from, and the rounding-count bounds they assert.  Imports nothing from oracle/ or
from the package.

    g' = g * clip_coef                     (clipping on)
    g' = g' + wd * p                       (coupled)          |  p = p * (1 - lr * wd)   (decoupled)
    m' = m + (1 - b1) * (g' - m)
    v' = b2 * v + (1 - b2) * g' * g'
    vmax' = max(vmax, v')                  (amsgrad)
    denom = sqrt(vmax' or v') / sqrt(1 - b2^t) + eps
    p' = p - lr / (1 - b1^t) * m' / denom
"""
import numpy as np

EPS23, EPS21 = 2.0 ** -23, 2.0 ** -21


def grad_norm(grads):
    """fp64 global L2 norm of a list of arrays"""
    return float(np.sqrt(sum(float(np.sum(np.asarray(g, dtype=np.float64) ** 2)) for g in grads)))


def clip_coef(total_norm, max_norm):
    """torch.nn.utils.clip_grad_norm_'s coefficient"""
    return min(1.0, max_norm / (total_norm + 1e-6))


def step(p, g, m, v, vmax, t, *, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, decoupled=False, amsgrad=False, clip=None):
    """one step in fp64; t is the step count AFTER this step (1 for the first).  -> dict(p, m, v, vmax, g1): the new values and the
    gradient g' that entered the moments (vmax is returned unchanged without amsgrad)"""
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    vmax = None if vmax is None else np.asarray(vmax, dtype=np.float64)
    g1 = g * clip if clip is not None else g
    if wd != 0:
        if decoupled:
            p = p * (1.0 - lr * wd)
        else:
            g1 = g1 + wd * p
    m1 = m + (1.0 - b1) * (g1 - m)
    v1 = b2 * v + (1.0 - b2) * g1 * g1
    if amsgrad:
        vmax = np.maximum(vmax, v1)
        d = vmax
    else:
        d = v1
    with np.errstate(invalid="ignore", divide="ignore"):
        denom = np.sqrt(d) / np.sqrt(1.0 - b2 ** t) + eps
        p1 = p - lr / (1.0 - b1 ** t) * m1 / denom
    return {"p": p1, "m": m1, "v": v1, "vmax": vmax, "g1": g1}


def check_step(got, ref, p0, m0, amsgrad, where="", enforce=True):
    """the single-step bounds.  got: dict of fp32 arrays p, m, v (, vmax) after the step; ref: step()'s result on the same fp32 inputs
    p0, m0, ...; u = |p'_ref - p0|.
        |dp| <= 2^-23 |p'| + 2^-21 u       |dm| <= 2^-23 max(|m|, |g'|)       |dv| <= 2^-21 v'       vmax as v
    (two to three roundings for m', four for v', about eight along u).  Prints the largest ratio to each bound, then asserts
    (enforce=False: prints only -- for torch's own fp32 step under coupled weight decay, see tests/test_optim_cpu.py)."""
    p0 = np.asarray(p0, dtype=np.float64)
    m0 = np.asarray(m0, dtype=np.float64)
    u = np.abs(ref["p"] - p0)
    items = [("p", np.abs(got["p"].astype(np.float64) - ref["p"]), EPS23 * np.abs(ref["p"]) + EPS21 * u),
             ("m", np.abs(got["m"].astype(np.float64) - ref["m"]), EPS23 * np.maximum(np.abs(m0), np.abs(ref["g1"]))),
             ("v", np.abs(got["v"].astype(np.float64) - ref["v"]), EPS21 * ref["v"])]
    if amsgrad:
        items.append(("vmax", np.abs(got["vmax"].astype(np.float64) - ref["vmax"]), EPS21 * ref["vmax"]))
    worst = {}
    for name, err, bound in items:
        fin = np.isfinite(ref[name])
        err, bound = err[fin], bound[fin]
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
        worst[name] = float(ratio.max()) if ratio.size else 0.0
    print(f"adam single-step error / bound {where}: " + "  ".join(f"{k} {r:.3f}" for k, r in worst.items()))
    for k, r in worst.items():
        assert not enforce or r <= 1.0, f"{where}: {k} exceeds its single-step bound by a factor {r:.3f}"
    return worst


def family_params(n, seed):
    """parameters 0.1 N(0, 1), fp32"""
    return (0.1 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def family_grads(n, steps, seed):
    """the recorded gradients of a trajectory, fp32 (steps, n): per step a scale 10^U(-6, 2) times N(0, 1); on every seventh step
    every second element is zero; non-zero |g| is kept at 1e-12 or above (nothing in the family lands in fp32 subnormals, where an
    fp64 restatement and any fp32 implementation legitimately part ways)"""
    rng = np.random.default_rng(seed)
    out = np.empty((steps, n), dtype=np.float32)
    for s in range(steps):
        g = (10.0 ** rng.uniform(-6, 2)) * rng.standard_normal(n)
        g = np.where(np.abs(g) < 1e-12, np.where(g < 0, -1e-12, 1e-12), g)
        if s % 7 == 6:
            g[1::2] = 0.0
        out[s] = g.astype(np.float32)
    return out


def preset_state(n, seed, amsgrad):
    """a plausible state after many steps (fp32): m ~ 1e-2 N(0,1), v = m^2-ish positive, vmax >= v"""
    rng = np.random.default_rng(seed)
    m = (1e-2 * rng.standard_normal(n)).astype(np.float32)
    v = (1e-4 * rng.uniform(0.1, 2.0, n)).astype(np.float32)
    vmax = (v * rng.uniform(1.0, 3.0, n).astype(np.float32)).astype(np.float32) if amsgrad else None
    return m, v, vmax


def trajectory(p0, grads, **kw):
    """the fp64 trajectory over the recorded gradients from zero state -> final fp64 p"""
    n = p0.shape[0]
    p, m, v = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    vmax = np.zeros(n) if kw.get("amsgrad") else None
    for t, g in enumerate(grads, 1):
        r = step(p, g, m, v, vmax, t, **kw)
        p, m, v, vmax = r["p"], r["m"], r["v"], r["vmax"]
    return p


def torch_cpu_trajectory(p0, grads, *, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, decoupled=False, amsgrad=False):
    """torch.optim.Adam(foreach=False) on the CPU in fp32 over the same recorded gradients -> final fp32 p (numpy)"""
    import torch
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, amsgrad=amsgrad, foreach=False,
                           decoupled_weight_decay=decoupled)
    for g in grads:
        p.grad = torch.from_numpy(g.copy())
        opt.step()
    return p.detach().numpy().copy()


def trajectory_bound(p_ref64, p_torch32):
    """what the HIP trajectory's max error against fp64 may be: four times torch's own fp32 error, plus one ulp of max |p|"""
    torch_err = float(np.abs(p_torch32.astype(np.float64) - p_ref64).max())
    pmax = float(np.abs(p_ref64).max())
    return 4.0 * torch_err + float(np.spacing(np.float32(pmax))), torch_err, pmax
