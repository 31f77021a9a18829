"""The rotation-trick z gradient restated on the CPU: the arithmetic of vqvae_amd/csrc/vq_rotation.hip's header, operation by
operation.  A loop over the channels, vectorised over the rows, everything np.float64 (numpy's +, *, / and sqrt on float64 are one
correctly rounded IEEE operation each, and nothing here is fused), then one cast to fp32: compared bitwise with the GPU.

`autograd_rot` is the independent reference: fp64 torch autograd of the paper's forward lam (e - 2 r (r^T e) + 2 q^ (e^^T e)) with
lam, r, e^, q^ detached (Fifty et al., arXiv 2410.06424).

Rows are (N, D) fp32 in the quantizer's row order (tests/rvq_ref.py's to_rows / to_nchw change layouts)."""
import numpy as np

F32 = np.float32
MIN_NS2 = 2.0 ** -20


def coefficients(z, q, g):
    """-> rotate (N,) bool, ce, cq, lam (N,) float64, from the five sums added in ascending channel order"""
    z, q, g = (np.asarray(a, F32).astype(np.float64) for a in (z, q, g))
    N, D = z.shape
    with np.errstate(all="ignore"):
        ee, qq, eq, eg, qg = (np.zeros(N) for _ in range(5))
        for c in range(D):
            ee = ee + z[:, c] * z[:, c]
            qq = qq + q[:, c] * q[:, c]
            eq = eq + z[:, c] * q[:, c]
            eg = eg + z[:, c] * g[:, c]
            qg = qg + q[:, c] * g[:, c]
        ne, nq = np.sqrt(ee), np.sqrt(qq)
        p = ne * nq
        ns2 = 2.0 + 2.0 * (eq / p)
        rotate = (ee > 0) & (qq > 0) & np.isfinite(ee) & np.isfinite(qq) & (ns2 >= MIN_NS2)
        a = (eg / ne + qg / nq) / ns2
        ce = (2.0 * qg) / p - (2.0 * a) / ne
        cq = -((2.0 * a) / nq)
        lam = nq / ne
    return rotate, ce, cq, lam


def rot(z, q, g):
    """rot (N, D) fp32: lam R^T g per row, g itself on the rows that are not rotated; and the rotate mask"""
    z32, q32, g32 = (np.asarray(a, F32) for a in (z, q, g))
    rotate, ce, cq, lam = coefficients(z32, q32, g32)
    z64, q64, g64 = z32.astype(np.float64), q32.astype(np.float64), g32.astype(np.float64)
    out = np.empty_like(g32)
    with np.errstate(all="ignore"):
        for c in range(z32.shape[1]):
            out[:, c] = (lam * ((g64[:, c] + ce * z64[:, c]) + cq * q64[:, c])).astype(F32)
    out[~rotate] = g32[~rotate]
    return out, rotate


def grad_z(z, codebook, idx, g, g_loss, scale):
    """the entry's grad_z with the flag: rot + gs * (z - q) in fp32, gs = fp32(g_loss) * fp32(scale) (g_loss None = 1)"""
    z32 = np.asarray(z, F32)
    q32 = np.asarray(codebook, F32)[np.asarray(idx)]
    r, rotate = rot(z32, q32, g)
    gs = F32((F32(1.0) if g_loss is None else F32(g_loss)) * F32(scale))
    with np.errstate(all="ignore"):
        out = (r + (gs * (z32 - q32).astype(F32)).astype(F32)).astype(F32)
    return out, r, rotate


def autograd_rot(z, q, g):
    """fp64 autograd of the paper's forward -> (d/de sum(z~_q * g) (N, D) float64, lam ||g|| (N,), max |z~_q - q| / ||q|| over rows)"""
    import torch
    e = torch.from_numpy(np.asarray(z, F32).astype(np.float64)).requires_grad_(True)
    qt = torch.from_numpy(np.asarray(q, F32).astype(np.float64))
    gt = torch.from_numpy(np.asarray(g, F32).astype(np.float64))
    with torch.no_grad():
        ne, nq = e.norm(dim=1, keepdim=True), qt.norm(dim=1, keepdim=True)
        eh, qh = e / ne, qt / nq
        s = eh + qh
        r = s / s.norm(dim=1, keepdim=True)
        lam = nq / ne
    zt = lam * (e - 2.0 * r * (r * e).sum(1, keepdim=True) + 2.0 * qh * (eh * e).sum(1, keepdim=True))
    (zt * gt).sum().backward()
    value_err = ((zt.detach() - qt).norm(dim=1) / nq[:, 0]).numpy()
    return e.grad.numpy(), (lam[:, 0] * gt.norm(dim=1)).numpy(), value_err


def bound(ref, lam_gnorm):
    """the issue's elementwise bound: 2^-24 |ref| (the one fp32 rounding) + 2^-40 lam ||g|| (about 10 D roundings of 2^-53 at D = 256,
    relative to the magnitude of the three terms)"""
    return 2.0 ** -24 * np.abs(ref) + 2.0 ** -40 * lam_gnorm[:, None]


def draw(N, D, K, scale, seed, plant=True):
    """z (N, D) at `scale`, a codebook of K rows drawn from z plus noise, g ~ N(0, 1); with N >= 4 and plant: row 0 of z zero, row 1
    assigned (by the caller, see `planted_idx`) to a zero code, row 2's code exactly -z, a NaN in row 3 of g."""
    rng = np.random.default_rng(seed)
    z = (scale * rng.standard_normal((N, D))).astype(F32)
    cb = (z[rng.integers(0, N, K)] + 0.3 * scale * rng.standard_normal((K, D))).astype(F32)
    g = rng.standard_normal((N, D)).astype(F32)
    if plant and N >= 4:
        z[0] = 0.0
        g[3, D // 2] = np.nan
    return z, cb, g


def plant_codes(z, cb, idx):
    """after the indices are known (N >= 4, K >= 2 free of the rows' own codes is not needed: the rows are re-assigned by hand):
    row 1 -> a zero code, row 2 -> a code that is exactly -z[2].  Uses the last two codes when K >= 3 (else what there is).
    -> (cb, idx) copies"""
    cb, idx = cb.copy(), np.asarray(idx).copy()
    N, K = z.shape[0], cb.shape[0]
    if N < 4:
        return cb, idx
    kz = K - 1
    cb[kz] = 0.0
    idx[1] = kz
    if K >= 2:
        ka = K - 2
        cb[ka] = -z[2]
        idx[2] = ka
    return cb, idx
