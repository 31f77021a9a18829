"""Batch sharding across GPUs: one process per GPU, replicated weights, no
data-path collective.  x_hat / z_q / indices of a shard are exactly what the reference computes on
that shard.  `embedding_loss` and `perplexity` are batch-GLOBAL scalars in the reference
(models/quantizer.py:63-64,70-71); `merge_vq_stats` rebuilds the full-batch values from per-shard
(squared-error sum, histogram) with ONE all-reduce of K+1 numbers -- optional, off the hot path."""
from __future__ import annotations

import torch


def shard_bounds(n_items: int, world_size: int, rank: int):
    """Contiguous, balanced [lo, hi) slice of the batch for `rank` (first n%world ranks get one extra)."""
    q, r = divmod(n_items, world_size)
    lo = rank * q + min(rank, r)
    return lo, lo + q + (1 if rank < r else 0)


def vq_stats_from_outputs(loss: torch.Tensor, hist: torch.Tensor, n_rows: int, D: int, beta: float):
    """Per-shard sufficient statistics: sum((z_q-z)^2) recovered from loss = (1+beta)*mean, and counts."""
    sq = loss.double() / (1.0 + beta) * (n_rows * D)
    return torch.cat([sq.reshape(1), hist.double()])


def merge_vq_stats(stats: torch.Tensor, n_rows_total: int, D: int, beta: float, group=None):
    """All-reduce the (K+1)-vector and return (embedding_loss, perplexity) of the FULL batch,
    following models/quantizer.py:63-64 and :70-71."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        stats = stats.clone()
        dist.all_reduce(stats, op=dist.ReduceOp.SUM, group=group)
    sq, hist = stats[0], stats[1:]
    m = (sq / (n_rows_total * D)).float()
    loss = m + beta * m
    p = (hist / n_rows_total).float()
    perplexity = torch.exp(-torch.sum(p * torch.log(p + 1e-10)))
    return loss, perplexity


def _world(group):
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist.get_world_size(group)
    return 1


def _takes_device_tensors(group) -> bool:
    import torch.distributed as dist
    # (RCCL goes by the name nccl; gloo takes device tensors for some collectives only, all_gather not among them)
    try:
        return "cuda:nccl" in str(dist.get_backend_config(group)) or dist.get_backend(group) == "nccl"
    except Exception:       # an older torch without get_backend_config
        return dist.get_backend(group) == "nccl"


def all_gather_ema_stats(stats: torch.Tensor, group=None) -> torch.Tensor:
    """This rank's (A, K, C) pending EMA statistics (functional.vq_ema_stats records, in the order they were taken) -> the
    (W * A, K, C) records of all W ranks, rank-major: rank 0's A records first.  Every rank receives the same bytes, and the sum
    over shards happens afterwards, in functional.vq_ema_apply's fixed order: the collective's own order never reaches a bit.
    Without an initialised process group, or with one rank, the input is returned and no collective is issued.  A group whose
    backend cannot take device tensors (gloo with device statistics) is served through the host: the one host sync of the
    feature."""
    W = _world(group)
    if W <= 1:
        return stats
    import torch.distributed as dist
    stats = stats.contiguous()
    if stats.is_cuda and not _takes_device_tensors(group):
        host = stats.cpu()
        out = torch.empty((W,) + tuple(host.shape), dtype=host.dtype)
        dist.all_gather(list(out.unbind(0)), host, group=group)
        return out.reshape((W * host.shape[0],) + tuple(host.shape[1:])).to(stats.device)
    out = torch.empty((W,) + tuple(stats.shape), dtype=stats.dtype, device=stats.device)
    dist.all_gather(list(out.unbind(0)), stats, group=group)
    return out.reshape((W * stats.shape[0],) + tuple(stats.shape[1:]))


def broadcast_ema_uniforms(u: torch.Tensor, group=None) -> torch.Tensor:
    """Every rank gets rank 0's restart uniforms, in place (all ranks must restart the same codes on the same candidates).  No
    collective without an initialised group or with one rank; through the host where the backend cannot take device tensors."""
    if _world(group) <= 1:
        return u
    import torch.distributed as dist
    src = dist.get_global_rank(group, 0) if group is not None else 0
    if u.is_cuda and not _takes_device_tensors(group):
        host = u.cpu()
        dist.broadcast(host, src=src, group=group)
        u.copy_(host)
    else:
        dist.broadcast(u, src=src, group=group)
    return u
