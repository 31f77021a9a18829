"""fp64 restatement, on the CPU, of the EMA codebook update (arXiv 1711.00937 Appendix A.1; include/vqvae_hip.h,
vqvae_vq_ema_update_f32) and of VectorQuantizerEMA's loss and z gradient.  Test infrastructure only."""
from __future__ import annotations

import torch


def restart_rows(uniforms: torch.Tensor, N: int) -> torch.Tensor:
    """r_k = min(floor(u_k N), N - 1), with u_k the fp32 uniform taken to fp64"""
    return torch.clamp(torch.floor(uniforms.double().cpu() * N).long(), 0, N - 1)


def ema_update(z: torch.Tensor, idx: torch.Tensor, cluster_size: torch.Tensor, ema_w: torch.Tensor, decay: float,
               eps: float = 1e-5, threshold: float | None = None, uniforms: torch.Tensor | None = None):
    """z: (N, D) rows; idx: (N,) codes; cluster_size (K,), ema_w (K, D) the state before the update.
    -> dict of fp64 tensors: N (updated counts), m (updated sums), e (new codebook), n, smoothed (N tilde), dead (bool mask)"""
    z = z.detach().double().cpu()
    idx = idx.detach().reshape(-1).long().cpu()
    K, D = ema_w.shape
    Nrows = z.shape[0]
    c = torch.bincount(idx, minlength=K).double()
    s = torch.zeros(K, D, dtype=torch.float64).index_add_(0, idx, z)
    Nk = decay * cluster_size.double().cpu() + (1.0 - decay) * c
    m = decay * ema_w.double().cpu() + (1.0 - decay) * s
    n = Nk.sum()
    smoothed = (Nk + eps) / (n + K * eps) * n
    e = m / smoothed[:, None]
    dead = torch.zeros(K, dtype=torch.bool)
    if threshold is not None:
        dead = Nk < threshold
        r = restart_rows(uniforms, Nrows)
        e[dead] = z[r[dead]]
    return {"N": Nk, "m": m, "e": e, "n": n, "smoothed": smoothed, "dead": dead}


def ema_update_loop(z, idx, cluster_size, ema_w, decay, eps=1e-5, threshold=None, uniforms=None):
    """the same update written as a plain per-row / per-code loop (checks the vectorised restatement)"""
    z = z.detach().double().cpu()
    idx = idx.detach().reshape(-1).long().cpu()
    K, D = ema_w.shape
    Nrows = z.shape[0]
    c = [0.0] * K
    s = [[0.0] * D for _ in range(K)]
    for i in range(Nrows):
        k = int(idx[i])
        c[k] += 1.0
        for d in range(D):
            s[k][d] += float(z[i, d])
    Nk = [decay * float(cluster_size[k]) + (1.0 - decay) * c[k] for k in range(K)]
    m = [[decay * float(ema_w[k, d]) + (1.0 - decay) * s[k][d] for d in range(D)] for k in range(K)]
    n = 0.0
    for k in range(K):
        n += Nk[k]
    e = []
    for k in range(K):
        if threshold is not None and Nk[k] < threshold:
            r = min(int(float(uniforms[k]) * Nrows // 1), Nrows - 1)
            e.append([float(z[r, d]) for d in range(D)])
        else:
            sm = (Nk[k] + eps) / (n + K * eps) * n
            e.append([m[k][d] / sm for d in range(D)])
    return {"N": torch.tensor(Nk, dtype=torch.float64), "m": torch.tensor(m, dtype=torch.float64),
            "e": torch.tensor(e, dtype=torch.float64), "n": torch.tensor(n, dtype=torch.float64)}


def commitment_grad(z, e_idx, g_zq, g_loss, beta):
    """dz = g_zq + g_loss 2 beta (z - e_idx) / (N D), z / e_idx / g_zq of one layout, fp64"""
    z = z.double()
    return g_zq.double() + float(g_loss) * 2.0 * beta * (z - e_idx.double()) / z.numel()


def rows_of(z: torch.Tensor, rowmajor: bool) -> torch.Tensor:
    """(B,H,W,D) or (B,D,H,W) -> (N, D) rows in the quantizer's row order"""
    return (z if rowmajor else z.permute(0, 2, 3, 1)).reshape(-1, z.shape[-1] if rowmajor else z.shape[1])
