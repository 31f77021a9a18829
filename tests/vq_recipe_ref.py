"""The composed one-stage quantizer -- cosine_sim, codebook_dim, rotation_trick, the orthogonal term, the code-entropy term and the EMA
codebook together -- as one plain torch composition written from the papers' formulas.  dtype-generic: the tests run it on the CPU in
fp64 (the reference) and in fp32 (the rounding a chain that rounds after every operation carries).  Nothing of vqvae_amd and none of
the other tests/*_ref.py restatements is used: every gradient is torch autograd's of the forward below.  (The EMA buffer update is a
state update outside the gradient graph: the tests take it from tests/vq_ema_ref.py.)

With rows z (N, D), parameters E = embedding.weight (K, d), W_in (d, D), b_in, W_out (D, d), b_out:

    y      = z W_in^T + b_in with codebook_dim, else z                                        (ViT-VQGAN, arXiv 2110.04627, 3.2)
    y^, E^ = y / clamp(||y||, 1e-12), E / clamp(||E||, 1e-12) with cosine_sim, else y, E      (the same section)
    idx    = argmin_k ||y^ - E^_k||^2;  q = E^[idx]
    loss   = mean((q.detach() - y^)^2) + beta mean((q - y^.detach())^2)                        (arXiv 1711.00937, eq. 3)
             with EMA: beta mean((q.detach() - y^)^2), and E takes no gradient anywhere        (the same paper, appendix A.1)
    value  = y^ + (q - y^).detach(), or with rotation_trick lam (y^ - 2 r (r^T y^) + 2 q^ (e^^T y^)), e^ = y^ / ||y^||, q^ = q / ||q||,
             r = (e^ + q^) / ||e^ + q^||, lam = ||q|| / ||y^||, all four detached: it has the value of q   (arXiv 2410.06424, eq. 5)
    z_q    = value W_out^T + b_out with codebook_dim, else value
    orth   = ||E^_s E^_s^T||_F^2 / M^2 - 1 / M over the M selected codes s                     (arXiv 2112.00384, 3.2)
             E^ is the search's own node with cosine_sim (the codebook is normalised once), l2norm(E) otherwise; selected are all
             codes, or with active_codes_only those of this forward's histogram > 0; under max_codes the first max_codes of them in
             the order (u_k, k) of the uniforms u
    p      = softmax_k(-s ||y^_n - E^_k||^2) over the (N, K) array;  P = mean_n H(p_n);  H = H(mean_n p_n)
    ent    = P - gamma H, on the operands the search ran on; with EMA the codebook enters it detached     (MaskGIT's tokenizer, LlamaGen)
    total  = loss + orth_weight orth + entropy_weight ent;  perplexity = exp(-sum_k m_k log(m_k + 1e-10)), m = histogram / N

`mutation=` applies ONE wiring error, for the tests that show the tolerance tells a wrong graph from rounding (MUTATIONS).  Two
of the names need a word:
  * 'search_raw' searches the un-normalised rows AND codes.  Un-normalising the rows alone cannot change an index: against unit codes
    ||y - E^_k||^2 = ||y||^2 + 1 - 2 y . E^_k has the argmin of the cosine.
  * 'orth_renormalised' normalises the already normalised codebook once more in front of the orthogonal term.  It is kept because it is
    the likeliest slip of all, and it is NOT an error: the normalisation's Jacobian at a unit row is the tangent projection
    I - e^ e^^T, the first normalisation's is (I - e^ e^^T) / ||E||, and a projection applied twice is itself.  The CPU test states
    this as an equality; the wiring error next to it that does move the gradient is 'orth_raw' (the term on E as stored).
"""
from types import SimpleNamespace

import torch

EPS = 1e-12
PARAMS = ("embedding.weight", "project_in.weight", "project_in.bias", "project_out.weight", "project_out.bias")

# name -> the options a combination must have for the mutation to touch its graph
MUTATIONS = {
    "beta_swapped": lambda o: not o["ema"],                                     # beta on the other term
    "rotation_dropped": lambda o: o["rotation_trick"],                         # straight-through where the rotation should act
    "orth_norm_detached": lambda o: o["orth_weight"] > 0,                      # the term's normalisation passes no gradient to ||E||
    "orth_renormalised": lambda o: o["orth_weight"] > 0 and o["cosine_sim"],   # (an identity: see above)
    "orth_raw": lambda o: o["orth_weight"] > 0 and not o["cosine_sim"],        # the term on the codebook as stored
    "entropy_raw": lambda o: o["entropy_weight"] > 0 and o["cosine_sim"],      # the entropy term on the un-normalised operands
    "gamma_sign": lambda o: o["entropy_weight"] > 0,                           # P + gamma H
    "entropy_ema_attached": lambda o: o["entropy_weight"] > 0 and o["ema"],    # the entropy term's codebook not detached under EMA
    "loss_after_project_out": lambda o: o["codebook_dim"] is not None,         # the loss in the wide space
    "search_raw": lambda o: o["cosine_sim"],                                   # the search on the un-normalised rows and codes
}


def options(cosine_sim=False, codebook_dim=None, rotation_trick=False, ema=False, beta=0.25, orth_weight=0.0, orth_active_only=False,
            orth_max_codes=None, entropy_weight=0.0, entropy_gamma=1.0, entropy_inv_temperature=100.0):
    return dict(cosine_sim=bool(cosine_sim), codebook_dim=codebook_dim, rotation_trick=bool(rotation_trick), ema=bool(ema),
                beta=float(beta), orth_weight=float(orth_weight), orth_active_only=bool(orth_active_only), orth_max_codes=orth_max_codes,
                entropy_weight=float(entropy_weight), entropy_gamma=float(entropy_gamma),
                entropy_inv_temperature=float(entropy_inv_temperature))


def l2norm(x):
    return x / x.norm(dim=1, keepdim=True).clamp(min=EPS)


def sq_dist(a, b):
    """(N, K): ||a_n - b_k||^2 with the differences in the open"""
    return ((a[:, None, :] - b[None, :, :]) ** 2).sum(2)


def select_codes(K, hist, active_only, max_codes, uniforms):
    """the selected codes, ascending: every code, or those with hist > 0; under a cap the first max_codes by (u_k, k)"""
    cand = [k for k in range(K) if not active_only or int(hist[k]) > 0]
    if max_codes is not None and len(cand) > max_codes:
        cand = sorted(k for _, k in sorted((float(uniforms[k]), k) for k in cand)[:max_codes])
    return cand


def orthogonal_term(unit, sel):
    if not sel:
        return unit.sum() * 0.0
    s = unit[torch.tensor(sel)]
    M = float(len(sel))
    return ((s @ s.t()) ** 2).sum() / (M * M) - 1.0 / M


def entropy_term(rows, codes, s, gamma):
    """-> (P - gamma H, P, H) of softmax_k(-s d_nk)"""
    logp = torch.log_softmax(-s * sq_dist(rows, codes), dim=1)
    p = logp.exp()
    P = -(p * logp).sum(1).mean()
    avg = p.mean(0)
    # 0 log 0 = 0, with no gradient: in fp32 a code far from every row has p = 0 in every row (exp underflows below -103), and the
    # derivative log avg + 1 of a term that no row feeds must not meet that 0 as an infinity
    live = avg > 0
    H = -torch.where(live, avg * torch.log(torch.where(live, avg, torch.ones_like(avg))), torch.zeros_like(avg)).sum()
    return P - gamma * H, P, H


def rotate(y, q):
    """the rotation trick's output: the value of q, the gradient lam R^T g for y"""
    with torch.no_grad():
        ny, nq = y.norm(dim=1, keepdim=True), q.norm(dim=1, keepdim=True)
        eh, qh = y / ny, q / nq
        r = eh + qh
        r = r / r.norm(dim=1, keepdim=True)
        lam = nq / ny
    return lam * (y - 2.0 * r * (r * y).sum(1, keepdim=True) + 2.0 * qh * (eh * y).sum(1, keepdim=True))


def forward(z, params, opts, uniforms=None, mutation=None):
    """z (N, D) rows and params (name -> tensor) of one dtype, leaves of the caller's graph; opts: options(); uniforms (K,): the cap's
    draws.  -> namespace: total, loss, z_q (N, D), idx (N,), hist (K,), perplexity, orth and ent (term, P, H) (None where the option
    is off), rows and codes (the search's operands), d (N, K)."""
    if mutation is not None and mutation not in MUTATIONS:
        raise ValueError(f"unknown mutation {mutation!r}")
    o = opts
    E = params["embedding.weight"]
    K = E.shape[0]
    if o["ema"]:
        E = E.detach()
    factorized = o["codebook_dim"] is not None
    y = z @ params["project_in.weight"].t() + params["project_in.bias"] if factorized else z
    rows, codes = (l2norm(y), l2norm(E)) if o["cosine_sim"] else (y, E)
    d = sq_dist(y, E) if mutation == "search_raw" else sq_dist(rows, codes)
    idx = d.detach().argmin(1)
    hist = torch.bincount(idx, minlength=K)
    q = codes[idx]

    commit, book = ((q.detach() - rows) ** 2).mean(), ((q - rows.detach()) ** 2).mean()
    value = rows + (q - rows).detach()
    if o["rotation_trick"] and mutation != "rotation_dropped":
        value = rotate(rows, q)
    z_q = value @ params["project_out.weight"].t() + params["project_out.bias"] if factorized else value
    if mutation == "loss_after_project_out":
        wide = q @ params["project_out.weight"].t() + params["project_out.bias"]
        commit, book = ((wide.detach() - z) ** 2).mean(), ((wide - z.detach()) ** 2).mean()
    if o["ema"]:
        loss = o["beta"] * commit
    elif mutation == "beta_swapped":
        loss = o["beta"] * commit + book
    else:
        loss = commit + o["beta"] * book
    total = loss

    orth = None
    if o["orth_weight"] > 0.0:
        unit = codes if o["cosine_sim"] else l2norm(E)
        if mutation == "orth_norm_detached":
            unit = E / E.detach().norm(dim=1, keepdim=True).clamp(min=EPS)
        elif mutation == "orth_renormalised":
            unit = l2norm(codes)
        elif mutation == "orth_raw":
            unit = E
        orth = orthogonal_term(unit, select_codes(K, hist, o["orth_active_only"], o["orth_max_codes"], uniforms))
        total = total + o["orth_weight"] * orth

    ent = None
    if o["entropy_weight"] > 0.0:
        a, b = (y, E) if mutation == "entropy_raw" else (rows, codes)
        if mutation == "entropy_ema_attached":
            b = l2norm(params["embedding.weight"]) if o["cosine_sim"] else params["embedding.weight"]
        gamma = -o["entropy_gamma"] if mutation == "gamma_sign" else o["entropy_gamma"]
        ent = entropy_term(a, b, o["entropy_inv_temperature"], gamma)
        total = total + o["entropy_weight"] * ent[0]

    m = hist.to(z.dtype) / z.shape[0]
    perplexity = torch.exp(-(m * torch.log(m + 1e-10)).sum())
    return SimpleNamespace(total=total, loss=loss, z_q=z_q, idx=idx, hist=hist, perplexity=perplexity, orth=orth, ent=ent, rows=rows,
                           codes=codes, d=d)


def run(z, params, opts, g=None, uniforms=None, mutation=None, dtype=torch.float64, root="both"):
    """forward and backward at `dtype` on the CPU from fp32 (or any) values: the root is total + sum(z_q g) ('both'), total alone
    ('loss') or sum(z_q g) alone ('z_q').  -> (namespace of forward(), detached; dict name -> tensor): 'total', 'z_q', 'perplexity',
    'orth', 'ent' (3,) and 'grad z', 'grad <parameter>' of every parameter the combination has -- zeros where no gradient arrives."""
    zt = z.detach().to("cpu", dtype).clone().requires_grad_(True)
    pt = {k: v.detach().to("cpu", dtype).clone().requires_grad_(True) for k, v in params.items()}
    f = forward(zt, pt, opts, uniforms, mutation)
    out = {"total": f.total.detach(), "z_q": f.z_q.detach(), "perplexity": f.perplexity.detach()}
    if f.orth is not None:
        out["orth"] = f.orth.detach()
    if f.ent is not None:
        out["ent"] = torch.stack([t.detach() for t in f.ent])
    if root != "none":
        top = {"both": lambda: f.total + (f.z_q * g.to("cpu", dtype)).sum(), "loss": lambda: f.total,
               "z_q": lambda: (f.z_q * g.to("cpu", dtype)).sum()}[root]()
        leaves = [zt] + list(pt.values())
        grads = torch.autograd.grad(top, leaves, allow_unused=True)
        for name, leaf, gr in zip(["z"] + list(pt), leaves, grads):
            out["grad " + name] = torch.zeros_like(leaf) if gr is None else gr
    f.rows, f.codes, f.d = f.rows.detach(), f.codes.detach(), f.d.detach()
    return f, out


def relative_gap(d):
    """(N,): (second-best - best) / second-best of every row's squared distances"""
    two = torch.topk(d, 2, dim=1, largest=False).values
    return (two[:, 1] - two[:, 0]) / two[:, 1]


def rel_err(got, ref):
    """max |got - ref| / max |ref| (inf where a zero tensor moved, 0 where it did not)"""
    diff, scale = float((got.double() - ref.double()).abs().max()), float(ref.double().abs().max())
    if diff == 0.0:
        return 0.0
    return diff / scale if scale > 0.0 else float("inf")


FLOOR = 2.0 ** -22            # four fp32 ulps of the tensor's maximum
FACTOR = 4.0


def bound(e_32):
    """the tolerance rule: FACTOR * max(the fp32 composition's own error, FLOOR)"""
    return FACTOR * max(e_32, FLOOR)


# ---- the cases of the tests: every accepted combination at one small shape -------------------------------------------------------------

B, H, W, D, K, CDIM = 3, 5, 7, 16, 32, 8
N = B * H * W
BETA = 0.25
ORTH = dict(orth_weight=0.5, orth_active_only=True, orth_max_codes=20)
ENT = dict(entropy_weight=0.3, entropy_gamma=1.0, entropy_inv_temperature=50.0)
FLAGS = ("cosine_sim", "codebook_dim", "rotation_trick", "orthogonal", "entropy", "ema")


def combinations():
    """the 48 accepted subsets of FLAGS (the orthogonal term trains the codebook by its gradient: not with EMA), as tuples of names"""
    out = []
    for bits in range(1 << len(FLAGS)):
        c = tuple(n for i, n in enumerate(FLAGS) if bits >> i & 1)
        if not ("orthogonal" in c and "ema" in c):
            out.append(c)
    return out


def combo_id(c):
    return "+".join(c) if c else "plain"


def combo_options(c):
    return options(cosine_sim="cosine_sim" in c, codebook_dim=CDIM if "codebook_dim" in c else None, rotation_trick="rotation_trick" in c,
                   ema="ema" in c, beta=BETA, **(ORTH if "orthogonal" in c else {}), **(ENT if "entropy" in c else {}))


def draw(n=N, dim=D, k=K, cdim=None, seed=0):
    """-> z (n, dim) rows, g (n, dim) the upstream gradient of z_q, params, all fp32: rows and projected rows of scale 0.1 and a
    codebook drawn at that scale, so that several codes carry mass in the softmax at inv_temperature = 50 and a few codes stay unused"""
    gen = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=gen)
    z, g = 0.1 * rn(n, dim), rn(n, dim)
    d = dim if cdim is None else cdim
    params = {"embedding.weight": 0.1 * rn(k, d)}
    if cdim is not None:
        params.update({"project_in.weight": rn(cdim, dim) / dim ** 0.5, "project_in.bias": 0.02 * rn(cdim),
                       "project_out.weight": rn(dim, cdim) / cdim ** 0.5, "project_out.bias": 0.02 * rn(dim)})
    return z, g, params


SEED = 0
UNIFORM_SEED = 77             # of the cap's draws: the CPU tests draw on the CPU, the GPU tests on the device, each side twice


def case(c, seed=SEED):
    """(z, g, params, opts) of a combination: the draws depend on codebook_dim alone"""
    o = combo_options(c)
    return draw(cdim=o["codebook_dim"], seed=seed) + (o,)



WARM_SETS = [("cosine_sim", "codebook_dim", "entropy"), ("cosine_sim", "codebook_dim", "entropy", "ema")]
WARM_LR, EMA_DECAY, EMA_EPS = 0.1, 0.99, 1e-5


def warm_case(c):
    """the second step's (z, g) -- another draw of the same shape -- and, for the CPU tests, the parameters the reference itself
    arrives at after one step: p - WARM_LR grad p in fp64, rounded to fp32; with EMA the codebook of the first update instead.  (The
    GPU tests take the second step's parameters from the module: these differ from them by rounding.)"""
    from tests import vq_ema_ref
    z, g, params, o = case(c)
    f, r = run(z, params, o, g)
    new = {k: (v.double() - WARM_LR * r["grad " + k]).float() for k, v in params.items()}
    if o["ema"]:
        E = params["embedding.weight"]
        new["embedding.weight"] = vq_ema_ref.ema_update(f.rows, f.idx, torch.zeros(E.shape[0]), E, EMA_DECAY, EMA_EPS)["e"].float()
    z2, g2, _ = draw(cdim=o["codebook_dim"], seed=SEED + 1)
    return z2, g2, new, o


# ---- the whole model: the reference's encoder and decoder (oracle/torch_port.py) around the composition -------------------------------

MODEL_DIMS, MODEL_HW, MODEL_B = (64, 16, 1, 64, 32), 16, 6          # 4x4 latent maps: 96 rows, D = 32, K = 64
MODEL_SETS = {
    "cosine+codebook_dim+entropy+orthogonal": ("cosine_sim", "codebook_dim", "orthogonal", "entropy"),
    "cosine+codebook_dim+entropy+orthogonal+rotation": ("cosine_sim", "codebook_dim", "rotation_trick", "orthogonal", "entropy"),
    "ema+cosine+codebook_dim+entropy+rotation": ("cosine_sim", "codebook_dim", "rotation_trick", "entropy", "ema"),
}


def model_kwargs(c):
    """the VQVAE constructor's keywords of a combination"""
    kw = dict(cosine_sim="cosine_sim" in c, rotation_trick="rotation_trick" in c)
    if "codebook_dim" in c:
        kw["codebook_dim"] = CDIM
    if "ema" in c:
        kw["ema_decay"] = 0.99
    if "orthogonal" in c:
        kw.update(orthogonal_reg_weight=ORTH["orth_weight"], orthogonal_reg_active_codes_only=ORTH["orth_active_only"],
                  orthogonal_reg_max_codes=ORTH["orth_max_codes"])
    if "entropy" in c:
        kw.update(entropy_weight=ENT["entropy_weight"], entropy_diversity_gamma=ENT["entropy_gamma"],
                  entropy_inv_temperature=ENT["entropy_inv_temperature"])
    return kw


def model_forward(sd, x, n_res, opts, uniforms=None):
    """sd: a state dict of leaves (name -> tensor of x's dtype).  -> (forward()'s namespace on the rows of z_e, x_hat, the training
    loss mean((x_hat - x)^2) / 0.06 + total)"""
    from oracle import torch_port
    z_e = torch_port.encode(sd, x.clone(), n_res)
    b, dim, h, w = z_e.shape
    pre = "vector_quantization."
    f = forward(z_e.permute(0, 2, 3, 1).reshape(-1, dim), {k: sd[pre + k] for k in PARAMS if pre + k in sd}, opts, uniforms)
    x_hat = torch_port.decode(sd, f.z_q.reshape(b, h, w, dim).permute(0, 3, 1, 2).contiguous(), n_res)
    return f, x_hat, ((x_hat - x) ** 2).mean() / 0.06 + f.total
