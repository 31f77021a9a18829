"""fp64 restatement of the cached sampler's recurrence in torch ops  --  TEST INFRASTRUCTURE ONLY.

What csrc/pixelcnn_sample.hip computes, written down independently of it: per row y the vertical stacks of every layer read only
rows above y (layer 0 the embedded input at rows y-3 .. y-1, the dy = 0 taps zeroed by make_causal; layer L >= 1 V_{L-1} at rows
y-1 and y), per position (y, x) the horizontal stacks read Hs_{L-1} at (y, x-1) and (y, x) (layer 0 the embedded input at
(y, x-3 .. x-1)).  Each step below slices out exactly those inputs, so agreement with oracle/pixelcnn_port.forward on every position
of a teacher-forced map checks the dependency analysis itself.  Nothing under vqvae_amd/ imports it.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F


def _gate(t, cond):
    a, g = (t + cond).chunk(2, dim=-1)
    return torch.tanh(a) * torch.sigmoid(g)


def recurrence_logits(sd, x, label, n_layers):
    """sd: GatedPixelCNN state_dict (not modified); x (B,H,W) int64 teacher-forced map; label (B,) -> logits (B, K, H, W) fp64
    where position (y, x) sees only what the sampler has when it draws (y, x)."""
    p = {k: v.detach().double().clone() for k, v in sd.items()}
    p["layers.0.vert_stack.weight"][:, :, -1] = 0
    p["layers.0.horiz_stack.weight"][:, :, :, -1] = 0
    B, H, W = x.shape
    emb = F.embedding(x, p["embedding.weight"])                               # (B,H,W,dim)
    dim = emb.shape[-1]
    V = [torch.zeros(B, H, W, dim, dtype=torch.float64) for _ in range(n_layers)]
    v2h = [torch.zeros(B, H, W, 2 * dim, dtype=torch.float64) for _ in range(n_layers)]
    cond = [F.embedding(label, p[f"layers.{i}.class_cond_embedding.weight"]) for i in range(n_layers)]
    for y in range(H):                                                        # per row: vertical stacks of every layer
        for i in range(n_layers):
            q = f"layers.{i}."
            wv = p[q + "vert_stack.weight"]                                   # (2dim, dim, kh, kw)
            k = wv.shape[-1]
            src = emb if i == 0 else V[i - 1]
            pad = F.pad(src, (0, 0, k // 2, k // 2))                          # zero columns on both sides
            hv = p[q + "vert_stack.bias"].expand(B, W, 2 * dim).clone()
            for ky in range(wv.shape[2]):
                yy = y + ky - wv.shape[2] + 1
                if yy < 0 or (i == 0 and yy == y):                           # padding; layer 0 never reads its own row
                    continue
                assert yy < y or (i > 0 and yy == y)
                for kx in range(k):
                    hv = hv + pad[:, yy, kx:kx + W, :] @ wv[:, :, ky, kx].T
            V[i][:, y] = _gate(hv, cond[i][:, None, :])
            v2h[i][:, y] = hv @ p[q + "vert_to_horiz.weight"][:, :, 0, 0].T + p[q + "vert_to_horiz.bias"]
    Hs = [torch.zeros(B, H, W, dim, dtype=torch.float64) for _ in range(n_layers)]
    K = p["output_conv.2.weight"].shape[0]
    out = torch.zeros(B, K, H, W, dtype=torch.float64)
    for y in range(H):                                                        # per position: horizontal stacks and the head
        for x_ in range(W):
            for i in range(n_layers):
                q = f"layers.{i}."
                wh = p[q + "horiz_stack.weight"]                              # (2dim, dim, 1, kw)
                kw = wh.shape[-1]
                hh = p[q + "horiz_stack.bias"].expand(B, 2 * dim).clone()
                for kx in range(kw):
                    xx = x_ + kx - kw + 1
                    if xx < 0 or (i == 0 and xx == x_):
                        continue
                    src = emb[:, y, xx] if i == 0 else Hs[i - 1][:, y, xx]
                    hh = hh + src @ wh[:, :, 0, kx].T
                o = _gate(v2h[i][:, y, x_] + hh, cond[i])
                r = o @ p[q + "horiz_resid.weight"][:, :, 0, 0].T + p[q + "horiz_resid.bias"]
                Hs[i][:, y, x_] = r + Hs[i - 1][:, y, x_] if i > 0 else r
            t = torch.relu(Hs[-1][:, y, x_] @ p["output_conv.0.weight"][:, :, 0, 0].T + p["output_conv.0.bias"])
            out[:, :, y, x_] = t @ p["output_conv.2.weight"][:, :, 0, 0].T + p["output_conv.2.bias"]
    return out


def inverse_cdf(logits, u, window=1e-5):
    """The documented draw in fp64 on given logits (B, K, H, W) and uniforms (B, H, W): the smallest k with u S < C_k.
    -> (indices (B,H,W), near (B,H,W) bool: u S within window * S of some C_k, where fp32 rounding may pick the neighbour)."""
    lg = np.moveaxis(np.asarray(logits, dtype=np.float64), 1, -1)
    e = np.exp(lg - lg.max(-1, keepdims=True))
    c = np.cumsum(e, -1)
    s = c[..., -1:]
    t = np.asarray(u, dtype=np.float64)[..., None] * s
    idx = (t >= c).sum(-1)
    idx = np.minimum(idx, lg.shape[-1] - 1)
    near = (np.abs(c - t) <= window * s).any(-1)
    return idx, near
