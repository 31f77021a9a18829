"""Grouped (product) vector quantization restated on the CPU: the contract of vqvae_amd/csrc/vq_grouped.hip's header.

Per group the indices are the C oracle's (tests/rvq_ref.assign: the reference quantizer's argmin, bit for bit) on the group's slab;
the gather and z_q = z + (e - z) are numpy fp32, one IEEE operation each, so they are compared bitwise with the GPU.  Group losses
and perplexities are fp64 (tests/rvq_ref.stage_stats); `mean_loss` is the device's fp32 combination of fp32 group losses.  grad_z
is mirrored in the header's fp32 order (bitwise); the EMA update per group is tests/vq_ema_ref.ema_update on the slab.

Rows are (N, D) fp32 in the quantizer's row order; codebooks a list of G (K, d) fp32 arrays, d = D / G."""
from types import SimpleNamespace

import numpy as np

from tests import rvq_ref as R

F32 = np.float32


def slabs(rows, G):
    """-> (G, N, d): slab g holds the channels [g d, (g + 1) d) of every row, bit for bit"""
    rows = np.ascontiguousarray(rows, F32)
    N, D = rows.shape
    assert D % G == 0
    return np.ascontiguousarray(rows.reshape(N, G, D // G).transpose(1, 0, 2))


def slab_layout(sl, B, H, W, rowmajor):
    """(G, N, d) -> the layout of slabs_out: (G, B, H, W, d) when rowmajor, else (G, B, d, H, W)"""
    G, N, d = sl.shape
    s = sl.reshape(G, B, H, W, d)
    return np.ascontiguousarray(s if rowmajor else s.transpose(0, 1, 4, 2, 3))


def gather(books, idx, K):
    """(N, D): the groups' code rows side by side; an index outside [0, K) gives NaN in that group's segment, and only there"""
    parts = []
    for E, i in zip(books, idx):
        E = np.ascontiguousarray(E, F32)
        i = np.asarray(i, np.int64)
        ok = (i >= 0) & (i < K)
        e = E[np.where(ok, i, 0)].copy()
        e[~ok] = np.nan
        parts.append(e)
    return np.ascontiguousarray(np.concatenate(parts, axis=1), F32)


def mean_loss(loss_group):
    """((l_0 + l_1) + ...) / (float)G in fp32, group order, starting from l_0 itself, one division"""
    l = np.asarray(loss_group, F32)
    with np.errstate(all="ignore"):
        acc = l[0]
        for g in range(1, len(l)):
            acc = F32(acc + l[g])
        return F32(acc / F32(len(l)))


def forward(rows, books, beta, idx=None):
    """idx: use these (G, N) indices instead of assigning.
    -> idx (G, N), slabs (G, N, d), e (N, D), z_q (N, D), hist (G, K), loss_group, perplexity (G,) fp64, loss fp64"""
    rows = np.ascontiguousarray(rows, F32)
    G, K = len(books), books[0].shape[0]
    sl = slabs(rows, G)
    ids, hist, ls, pp = [], [], [], []
    with np.errstate(all="ignore"):
        for g in range(G):
            E = np.ascontiguousarray(books[g], F32)
            i = R.assign(sl[g], E) if idx is None else np.asarray(idx[g], np.int64)
            l, p, h = R.stage_stats(sl[g], E[i], i, K, beta)
            ids.append(i), hist.append(h), ls.append(l), pp.append(p)
        e = gather(books, ids, K)
        z_q = (rows + (e - rows).astype(F32)).astype(F32)
        loss = ls[0]
        for g in range(1, G):
            loss = loss + ls[g]
        loss = loss / G
    return SimpleNamespace(idx=np.stack(ids), slabs=sl, e=e, z_q=z_q, hist=np.stack(hist), loss_group=np.array(ls),
                           perplexity=np.array(pp), loss=loss)


def z_q_of(rows, books, idx):
    """z + (e - z) from given (G, N) indices, fp32"""
    rows = np.ascontiguousarray(rows, F32)
    with np.errstate(all="ignore"):
        e = gather(books, idx, books[0].shape[0])
        return (rows + (e - rows).astype(F32)).astype(F32)


def grad_z_mirror(rows, books, idx, grad_zq, g, beta=None):
    """grad_z in the header's order, fp32: g' = g / (float)G; gs = g' * fp32(2 / (N d)) (beta given: fp32(2 beta / (N d)), the
    commitment-only form); grad_zq + gs * (z - e)"""
    rows = np.ascontiguousarray(rows, F32)
    N, D = rows.shape
    G = len(books)
    d = D // G
    s = F32((2.0 if beta is None else 2.0 * float(F32(beta))) / (float(N) * float(d)))
    with np.errstate(all="ignore"):
        gs = F32(F32(F32(g) / F32(G)) * s)
        e = gather(books, idx, books[0].shape[0])
        out = (gs * (rows - e).astype(F32)).astype(F32)
        if grad_zq is not None:
            out = (np.asarray(grad_zq, F32) + out).astype(F32)
    return out


def codebook_grads(rows, books, idx, g, beta):
    """fp64: grad_E_g[k] = (g / G) 2 beta / (N d) sum_{i: idx_g,i = k} (e_k - slab_g,i)"""
    rows = np.ascontiguousarray(rows, F32)
    N, D = rows.shape
    G, K = len(books), books[0].shape[0]
    d = D // G
    sl = slabs(rows, G)
    out = []
    for gi in range(G):
        E = books[gi].astype(np.float64)
        acc = np.zeros((K, d))
        np.add.at(acc, idx[gi], E[idx[gi]] - sl[gi].astype(np.float64))
        out.append(float(g) / G * 2.0 * beta / (N * d) * acc)
    return out


def ema_step(rows, idx, cluster_size, ema_w, decay, eps=1e-5, threshold=None, uniforms=None):
    """one EMA update per group (tests/vq_ema_ref.ema_update on the slab).  cluster_size (G, K), ema_w (G, K, d) torch tensors: the
    state before; uniforms: (G, K) or None.  -> list of G dicts as ema_update returns them"""
    import torch

    from tests import vq_ema_ref as E
    G = ema_w.shape[0]
    sl = slabs(rows, G)
    return [E.ema_update(torch.from_numpy(sl[g]), torch.from_numpy(np.asarray(idx[g], np.int64)), cluster_size[g], ema_w[g], decay,
                         eps, threshold, None if uniforms is None else uniforms[g]) for g in range(G)]
