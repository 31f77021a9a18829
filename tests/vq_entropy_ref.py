"""CPU restatement of the code-entropy loss (the header of vqvae_amd/csrc/vq_entropy.hip is the contract): numpy, fp64 throughout,
the (N, K) arrays in the open -- this is the composition the kernels stream.  With s = inv_temperature, rows z_n, codes e_k:

    d_nk = (zz_n + ee_k) - 2 dot_nk;  l_nk = -s d_nk;  p_nk = softmax_k(l_nk) shifted by the row maximum
    H_n = -sum_k p_nk log p_nk (p = 0: 0);  P = mean_n H_n;  avg_k = mean_n p_nk;  H = -sum_k avg_k log avg_k (0 log 0 = 0)
    term = P - gamma H;  losses = float32(term, P, H);  rowstat = (lse_n, H_n)
    backward, g = grad_loss, L_k = log avg_k (0 where avg_k = 0), M_n = sum_j p_nj L_j, p_nk = exp(l_nk - lse_n):
    a_nk = (g / N) p_nk [-(log p_nk + H_n) + gamma (L_k - M_n)]
    grad_z_n = float32(-2 s sum_k a_nk (z_n - e_k));  grad_E_k = float32(2 s sum_n a_nk (z_n - e_k))

exp and log are not correctly rounded on the device and the sums are added in another order, so the comparison is by the bounds
below (derived in tests/test_vq_entropy_gpu.py's docstring), for which forward() and backward() return the magnitudes.
"""
from types import SimpleNamespace

import numpy as np

U = 2.0 ** -53
FN = 8.0                      # ulps allowed for one device exp / log together with the correctly rounded operations next to it
SIDES = 2.0                   # both sides of a comparison carry an error of the derived form


def draw(N, D, K, seed, regime, s=100.0):
    """-> z (N, D), E (K, D) fp32.  'saturated': rows sit near codes that lie far apart on the softmax's scale at inverse temperature s
    -- two codes about 12 apart in the logits, so that p is nearly one-hot and the next code still has a gradient; 'onehot': codes
    thousands apart in the logits at s = 100, so that every other probability underflows to 0, unused codes have avg = 0 and the
    gradients vanish; 'soft': everything so close on the scale of s = 100 that several codes carry mass."""
    rng = np.random.default_rng(seed)
    E = rng.standard_normal((K, D)).astype(np.float32)
    if regime == "onehot":
        z = (E[rng.integers(0, K, N)] + 0.05 * rng.standard_normal((N, D))).astype(np.float32)
    elif regime == "saturated":
        sigma = np.sqrt(6.0 / (s * D))
        E = (sigma * E).astype(np.float32)
        z = (E[rng.integers(0, K, N)] + 0.1 * sigma * rng.standard_normal((N, D))).astype(np.float32)
    else:
        E = (0.05 / np.sqrt(D) * E).astype(np.float32)
        z = (0.05 / np.sqrt(D) * rng.standard_normal((N, D))).astype(np.float32)
    return z, E


def _logits(z, E, s):
    z, E = z.astype(np.float64), E.astype(np.float64)
    zz, ee = (z * z).sum(1), (E * E).sum(1)
    d = (zz[:, None] + ee[None, :]) - 2.0 * (z @ E.T)
    return -s * d, zz, ee


def _xlogx(x):
    return np.where(x > 0.0, x * np.log(np.where(x > 0.0, x, 1.0)), 0.0)


def forward(z, E, s, gamma):
    l, zz, ee = _logits(z, E, s)
    m = l.max(1, keepdims=True)
    x = l - m
    ex = np.exp(x)
    S = ex.sum(1)
    lse = m[:, 0] + np.log(S)
    Hn = np.log(S) - np.where(ex > 0.0, ex * x, 0.0).sum(1) / S
    p = np.exp(l - lse[:, None])
    avg = p.mean(0)
    P, H = Hn.mean(), -_xlogx(avg).sum()
    term = P - gamma * H
    return SimpleNamespace(l=l, zz=zz, ee=ee, p=p, lse=lse, Hn=Hn, avg=avg, P=P, H=H, term=term,
                           losses=np.array([term, P, H], dtype=np.float32), rowstat=np.stack([lse, Hn], 1))


def backward(z, E, avg, rowstat, g, s, gamma, drop=None):
    """drop: None, or 'confidence' / 'diversity' (that bracket term of a_nk left out) or 'sign' (gamma's sign flipped): the broken
    variants the CPU test shows to lie outside the bounds"""
    l, _, _ = _logits(z, E, s)
    N = z.shape[0]
    lse, Hn = rowstat[:, 0], rowstat[:, 1]
    logp = l - lse[:, None]
    p = np.exp(logp)
    L = np.where(avg > 0.0, np.log(np.where(avg > 0.0, avg, 1.0)), 0.0)
    M = p @ L
    conf = -(logp + Hn[:, None])
    div = gamma * (L[None, :] - M[:, None])
    if drop == "confidence":
        conf = 0.0 * conf
    elif drop == "diversity":
        div = 0.0 * div
    elif drop == "sign":
        div = -div
    br = conf + div
    a = (g / N) * p * br
    z64, E64 = z.astype(np.float64), E.astype(np.float64)
    gz = -2.0 * s * (z64 * a.sum(1)[:, None] - a @ E64)
    gE = 2.0 * s * (a.T @ z64 - E64 * a.sum(0)[:, None])
    return SimpleNamespace(p=p, logp=logp, L=L, M=M, br=br, a=a, grad_z=gz.astype(np.float32), grad_E=gE.astype(np.float32),
                           grad_z64=gz, grad_E64=gE)


# ---- the bounds (one side; the comparisons use SIDES times them) ---------------------------------------------------------------------

def eps_logit(f, D, s):
    """per row: the logits' absolute error, (2 D + 8) u s (zz_n + ee_k + 2 sum_c |z_c e_kc|) <= (2 D + 8) u 2 s (zz_n + max ee)"""
    return (2 * D + 8) * U * 2.0 * s * (f.zz + f.ee.max())


def fwd_bounds(f, N, K, D, s, gamma):
    """-> dict of one-side bounds: lse (N), Hn (N), avg (K), P, H, term (the scalars before their fp32 rounding)"""
    LK = np.log(max(K, 2))
    el = eps_logit(f, D, s)
    eps = 3.0 * el + (FN + K + 12) * U                                          # S's relative error, with the logits' on top
    b_lse = eps + (FN + 2) * U * (np.abs(f.lse) + LK)
    b_hn = 4.0 * (1.0 + LK) * eps
    b_P = b_hn.mean() + (N + 16) * U * f.P
    rel_p = el + b_lse + (FN + 2) * U                                           # p = exp(l - lse)
    plogp = -_xlogx(f.p)
    b_avg = ((f.p * rel_p[:, None]).sum(0) + U * plogp.sum(0)) / N + (N + 2) * U * f.avg + 2.0 ** -1000
    logavg = np.abs(np.log(np.where(f.avg > 0.0, f.avg, 1.0)))
    b_H = ((logavg + 1.0) * b_avg).sum() + (K + FN + 8) * U * np.abs(_xlogx(f.avg)).sum()
    b_term = b_P + abs(gamma) * b_H + 4 * U * (abs(f.P) + abs(gamma * f.H))
    return dict(lse=b_lse, Hn=b_hn, avg=b_avg, P=b_P, H=b_H, term=b_term)


def f32_round(ref):
    """one rounding to fp32 of a value whose fp64 error may carry it across a rounding boundary, and the denormal floor"""
    return 2.0 ** -23 * np.abs(ref) + 2.0 ** -149


def bwd_bounds(r, f, z, E, g, s, gamma):
    """-> one-side bounds of grad_z (N, D) and grad_E (K, D) before their fp32 rounding.  f: the forward of the same inputs (zz, ee);
    avg and rowstat are inputs of the backward, the same on both sides."""
    N, D = z.shape
    K = E.shape[0]
    el = eps_logit(f, D, s)[:, None]
    absL = np.abs(r.L)[None, :]
    Hn = -_xlogx(r.p).sum(1)
    ML = (r.p * absL).sum(1)
    b_M = (el[:, 0] + (2 * FN + K + 8) * U) * ML + U * np.abs(r.L).max() * Hn
    d_p = r.p * (el + (FN + 1) * U) + U * r.p * np.abs(r.logp)
    d_br = el + 3 * U * np.abs(r.logp) + 2 * U * Hn[:, None] + abs(gamma) * ((FN + 2) * U * absL + b_M[:, None]
                                                                             + 2 * U * np.abs(r.M)[:, None]) + 2 * U * np.abs(r.br)
    b_a = (abs(g) / N) * (d_p * np.abs(r.br) + r.p * d_br) + 4 * U * np.abs(r.a)
    az, aE = np.abs(z.astype(np.float64)), np.abs(E.astype(np.float64))
    wz = b_a + (K + 4) * U * np.abs(r.a)
    wE = b_a + (N + 4) * U * np.abs(r.a)
    b_gz = 2.0 * s * (wz @ aE + az * wz.sum(1)[:, None]) * (1 + 4 * U)
    b_gE = 2.0 * s * (wE.T @ az + aE * wE.sum(0)[:, None]) * (1 + 4 * U)
    return b_gz, b_gE
