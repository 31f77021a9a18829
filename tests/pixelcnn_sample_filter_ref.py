"""fp64 restatement of the cached sampler's filtered draw (top-k, temperature, top-p)  --  TEST INFRASTRUCTURE ONLY.

The rules of vqvae_pixelcnn_sample_ex_f32 (include/vqvae_hip.h), written down independently of csrc/pixelcnn_sample.hip: a stable
sort for the ranking where the kernel bisects on integer keys, fp64 sums where it keeps fixed-order fp32 ones.  Nothing under
vqvae_amd/ imports it.
"""
from __future__ import annotations

import numpy as np


def filtered_draw(logits, u, temperature=1.0, top_k=0, top_p=1.0, window=1e-5):
    """logits (B, K, H, W): the fp32 logits each position was drawn from, as the kernel returns them; u (B, H, W) uniforms.
    -> (indices (B, H, W), near (B, H, W) bool).

    The top-k set is exact: code j stays iff #{i : l_i > l_j or (l_i == l_j and i < j)} < top_k, on the fp32 values.  Temperature,
    the nucleus and the CDF are fp64.  near marks the positions where fp32 rounding may decide otherwise: some ranked cumulative mass
    lies within window * S of top_p * S (the nucleus may end one code earlier or later), or u S' lies within window * S' of some
    C_k (as pixelcnn_sample_ref.inverse_cdf)."""
    l32 = np.moveaxis(np.asarray(logits, dtype=np.float32), 1, -1)
    K = l32.shape[-1]
    top_k = 0 if top_k is None else int(top_k)
    top_p = 1.0 if top_p is None else float(top_p)
    # rank by (l descending, index ascending): a stable sort of -l (-0.0 and 0.0 compare equal, so the index decides between them)
    order = np.argsort(-l32, axis=-1, kind="stable")
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.broadcast_to(np.arange(K), order.shape).copy(), axis=-1)
    keep = rank < top_k if 1 <= top_k < K else np.ones(l32.shape, dtype=bool)
    lg = l32.astype(np.float64)
    m = np.where(keep, lg, -np.inf).max(-1, keepdims=True)
    e = np.where(keep, np.exp((lg - m) / float(temperature)), 0.0)
    near = np.zeros(l32.shape[:-1], dtype=bool)
    if top_p < 1.0:
        s = e.sum(-1, keepdims=True)
        es = np.take_along_axis(e, order, axis=-1)
        before = np.cumsum(es, -1) - es                                       # the mass ranked strictly before each code
        stay_sorted = before < top_p * s
        stay_sorted[..., 0] = True                                            # the top-ranked code always stays
        kept_sorted = np.take_along_axis(keep, order, axis=-1)
        close = (np.abs(before - top_p * s) <= window * s) & kept_sorted
        near |= close[..., 1:].any(-1)
        stay = np.empty_like(stay_sorted)
        np.put_along_axis(stay, order, stay_sorted, axis=-1)
        e = np.where(stay, e, 0.0)
    c = np.cumsum(e, -1)
    s2 = c[..., -1:]
    t = np.asarray(u, dtype=np.float64)[..., None] * s2
    idx = (t >= c).sum(-1)
    last = K - 1 - np.argmax((e > 0)[..., ::-1], axis=-1)                     # the fallback: the last e_k > 0
    idx = np.minimum(idx, last)
    near |= (np.abs(c - t) <= window * s2).any(-1)
    return idx, near


def surviving(logits, temperature=1.0, top_k=0, top_p=1.0):
    """the codes the filters leave at one position, logits (K,) -> sorted list: what a fine grid of uniforms draws (every code
    whose CDF step is wider than 1 / 4096 of the total)"""
    n = 4096
    lg = np.broadcast_to(np.asarray(logits, dtype=np.float32)[None, :, None, None], (n, len(logits), 1, 1))
    us = (np.arange(n, dtype=np.float64) + 0.5) / n
    idx, _ = filtered_draw(lg, us[:, None, None], temperature, top_k, top_p)
    return sorted(set(int(i) for i in idx.ravel()))
