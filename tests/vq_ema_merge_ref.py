"""fp64 restatement, on the CPU, of the split EMA codebook update (vqvae_amd/csrc/vq_ema_merge.hip states the contract): one
shard's sufficient statistics, and the update from the statistics of R shards added in shard order.  Uses nothing of vqvae_amd.
Test infrastructure only."""
from __future__ import annotations

import torch


def pick(u: torch.Tensor, n: int) -> torch.Tensor:
    """clamp(floor(double(u) n), 0, n - 1): the restart row of a shard of n rows, the shard of n shards"""
    return torch.clamp(torch.floor(u.detach().double().cpu() * n).long(), 0, n - 1)


def stats(z: torch.Tensor, idx: torch.Tensor, K: int, row_uniforms: torch.Tensor | None = None) -> torch.Tensor:
    """z: (N, D) rows of one shard; idx: (N,) codes.  -> (K, C) fp64: [count | per-code sums | restart candidates], C = D + 1
    without row_uniforms, 2 D + 1 with them (candidate k = row pick(u_k, N) of z)."""
    z = z.detach().double().cpu()
    idx = torch.clamp(idx.detach().reshape(-1).long().cpu(), 0, K - 1)
    N, D = z.shape
    assert N >= 1 and idx.numel() == N
    c = torch.bincount(idx, minlength=K).double()
    s = torch.zeros(K, D, dtype=torch.float64).index_add_(0, idx, z)
    cols = [c[:, None], s]
    if row_uniforms is not None:
        cols.append(z[pick(row_uniforms, N)])
    return torch.cat(cols, dim=1)


def merge(st: torch.Tensor, D: int):
    """st: (R, K, C) -> (c (K,), S (K, D)): counts added, sums added in shard order starting from shard 0's value itself"""
    c, S = st[0, :, 0].clone(), st[0, :, 1:D + 1].clone()
    for r in range(1, st.shape[0]):
        c = c + st[r, :, 0]
        S = S + st[r, :, 1:D + 1]
    return c, S


def apply(st, cluster_size: torch.Tensor, ema_w: torch.Tensor, decay: float, eps: float = 1e-5, threshold: float | None = None,
          shard_uniforms: torch.Tensor | None = None):
    """st: (R, K, C) fp64 or a list of (K, C); cluster_size (K,), ema_w (K, D): the state before the update.
    -> dict of fp64 tensors: N, m, e, n, dead (bool mask), shard (the shard j_k a restarted code takes its candidate from)"""
    if isinstance(st, (list, tuple)):
        st = torch.stack(list(st))
    st = st.detach().double().cpu()
    R, K, C = st.shape
    D = ema_w.shape[1]
    assert C in (D + 1, 2 * D + 1)
    c, S = merge(st, D)
    Nk = decay * cluster_size.detach().double().cpu() + (1.0 - decay) * c
    m = decay * ema_w.detach().double().cpu() + (1.0 - decay) * S
    n = Nk.sum()
    e = m / ((Nk + eps) / (n + K * eps) * n)[:, None]
    dead = torch.zeros(K, dtype=torch.bool)
    shard = torch.zeros(K, dtype=torch.long)
    if threshold is not None and threshold >= 0:
        assert C == 2 * D + 1 and shard_uniforms is not None
        dead = Nk < threshold
        shard = pick(shard_uniforms, R)
        cand = st[shard, torch.arange(K), D + 1:]
        e[dead] = cand[dead]
    return {"N": Nk, "m": m, "e": e, "n": n, "dead": dead, "shard": shard}


def cut(n: int, sizes):
    """[(lo, hi)] of consecutive shards of the given sizes, which must cover n items"""
    assert sum(sizes) == n
    out, lo = [], 0
    for s in sizes:
        out.append((lo, lo + s))
        lo += s
    return out
