"""Residual vector quantization restated on the CPU: the operation order of vqvae_amd/csrc/vq_residual.hip's header.

Per stage the indices are the C oracle's (oracle.c_oracle.vq_indices_rows: the reference quantizer's argmin, bit for bit); the
gather, the subtraction r_{q+1} = r_q - e_q, the sum S = ((e_0 + e_1) + ...) and z_q = z + (S - z) are numpy fp32, one IEEE
operation each, so they are compared bitwise with the GPU.  Losses and perplexities are fp64.  grad_z exists twice: mirrored in
the header's fp32 order (bitwise), and in fp64 with the per-element rounding bound the issue states.  autograd_chain is the
composition torch differentiates: every stage oracle.torch_port.quantize_train, r_{q+1} = r_q - e_q.detach().

Rows are (N, D) fp32 in the quantizer's row order; codebooks a list of Q (K, D) fp32 arrays (shared: the same array Q times)."""
from types import SimpleNamespace

import numpy as np

F32 = np.float32


def to_rows(z_nchw):
    z = np.asarray(z_nchw)
    return np.ascontiguousarray(z.transpose(0, 2, 3, 1).reshape(-1, z.shape[1]))


def to_nchw(rows, B, H, W):
    return np.ascontiguousarray(np.asarray(rows).reshape(B, H, W, -1).transpose(0, 3, 1, 2))


def assign(rows, codebook):
    from oracle import c_oracle
    return c_oracle.vq_indices_rows(np.ascontiguousarray(rows, F32), np.ascontiguousarray(codebook, F32), threads=1)


def stage_stats(r, e, idx, K, beta):
    """the quantizer's loss and perplexity for one stage, in fp64 (models/quantizer.py:63-64, :70-71)"""
    with np.errstate(all="ignore"):
        d = e.astype(np.float64) - r.astype(np.float64)
        mse = (d * d).mean()
        hist = np.bincount(idx, minlength=K).astype(np.int32)
        p = hist.astype(np.float64) / len(idx)
        ppl = np.exp(-(p * np.log(p + 1e-10)).sum())
    return mse + beta * mse, ppl, hist


def chain(rows, books, beta, idx=None):
    """The forward.  idx: use these (Q, N) indices instead of assigning (decode, backward).
    -> idx (Q, N), r [r_0 .. r_Q], e [e_0 .. e_{Q-1}], S, z_q, hist (Q, K), loss_stage, perplexity (Q,) fp64, loss fp64"""
    rows = np.ascontiguousarray(rows, F32)
    Q, K = len(books), books[0].shape[0]
    r, e, ids, hist, ls, pp = [rows], [], [], [], [], []
    with np.errstate(all="ignore"):
        for q in range(Q):
            E = np.ascontiguousarray(books[q], F32)
            i = assign(r[q], E) if idx is None else np.asarray(idx[q], np.int64)
            eq = E[i]                                         # the row's bits
            l, p, h = stage_stats(r[q], eq, i, K, beta)
            ids.append(i), e.append(eq), hist.append(h), ls.append(l), pp.append(p)
            r.append((r[q] - eq).astype(F32))                 # one fp32 subtraction per element
        S = e[0]
        for q in range(1, Q):
            S = (S + e[q]).astype(F32)
        z_q = (rows + (S - rows).astype(F32)).astype(F32)
        loss = ls[0]
        for q in range(1, Q):
            loss = loss + ls[q]
    return SimpleNamespace(idx=np.stack(ids), r=r, e=e, S=S, z_q=z_q, hist=np.stack(hist), loss_stage=np.array(ls),
                           perplexity=np.array(pp), loss=loss)


def draw_books(rows, K, Q, shared, seed):
    """Stage q's codebook: K rows drawn (with replacement) from r_q of the chain so far, so the residuals really shrink and some
    rows equal a code exactly -- the next stage's row is then all zeros.  shared: E_0 for every stage."""
    g = np.random.default_rng(seed)
    rows = np.ascontiguousarray(rows, F32)
    books, r = [], rows
    with np.errstate(all="ignore"):
        for q in range(Q):
            ok = np.flatnonzero(np.isfinite(r).all(axis=1))    # (the special-value tests: codes are finite rows)
            E = books[0] if (shared and q) else r[ok[g.integers(0, len(ok), K)]].copy()
            books.append(E)
            r = (r - E[assign(r, E)]).astype(F32)
    return books


def grad_z_mirror(rows, books, idx, grad_zq, g):
    """grad_z in the header's order, fp32: gs = g * fp32(2 / (N D)); A = ((r_1 + r_2) + ...) + r_Q; grad_zq + gs * A"""
    c = chain(rows, books, 0.0, idx=idx)
    N, D = rows.shape
    gs = F32(F32(g) * F32(2.0 / (float(N) * float(D))))
    with np.errstate(all="ignore"):
        A = c.r[1]
        for q in range(2, len(books) + 1):
            A = (A + c.r[q]).astype(F32)
        out = (gs * A).astype(F32)
        if grad_zq is not None:
            out = (np.asarray(grad_zq, F32) + out).astype(F32)
    return out


def grad_z_bound(Q, abs_grad_zq, cz, abs_diffs):
    """grad_z's per-element bound against the fp64 value: 2 (Q + 2) 2^-24 (|grad_zq| + |c| sum_q |r_q - e_q|), c = g 2 / (N D); plain
    arithmetic on arrays of any kind (the GPU test of the 4-wide kernels evaluates it on device tensors)"""
    return 2.0 * (Q + 2) * 2.0 ** -24 * (abs_grad_zq + abs(cz) * abs_diffs)


def grads(rows, books, idx, grad_zq, g, beta, shared=False):
    """fp64 gradients of the closed forms, from the contract's fp32 residuals r_q and codes e_q:
         grad_z      = grad_zq + g 2/(N D) sum_q (r_q - e_q)
         grad_E_q[k] = g 2 beta/(N D) sum_{i: idx_q,i = k} (e_k - r_q,i)
    -> grad_z (N, D), its per-element bound 2 (Q + 2) 2^-24 (|grad_zq| + c sum_q |r_q - e_q|) with c = g 2 / (N D), the per-stage
    codebook gradients [Q x (K, D)], and what the caller's codebooks receive (those, or with shared their stage-order sum)."""
    c = chain(rows, books, 0.0, idx=idx)
    N, D = rows.shape
    Q, K = len(books), books[0].shape[0]
    cz = float(g) * 2.0 / (N * D)
    diffs = [c.r[q].astype(np.float64) - c.e[q].astype(np.float64) for q in range(Q)]
    gzq = np.zeros((N, D)) if grad_zq is None else np.asarray(grad_zq, np.float64)
    gz = gzq + cz * sum(diffs)
    bound = grad_z_bound(Q, np.abs(gzq), cz, sum(np.abs(d) for d in diffs))
    ge = []
    for q in range(Q):
        acc = np.zeros((K, D))
        np.add.at(acc, c.idx[q], -diffs[q])                   # e_k - r_q,i
        ge.append(float(g) * 2.0 * beta / (N * D) * acc)
    return gz, bound, ge, ([sum(ge[1:], ge[0])] if shared else ge)


def autograd_chain(z_nchw, books, beta):
    """torch autograd of the composition: every stage torch_port.quantize_train, r_{q+1} = r_q - e_q.detach().  z_nchw and the
    (distinct) codebook tensors must require grad; books lists one tensor per stage (shared: the same tensor Q times).
    -> loss, z_q (B,D,H,W), idx (Q, N)"""
    import torch
    from oracle import torch_port
    B, D, H, W = z_nchw.shape
    r, S, loss, ids = z_nchw, None, None, []
    for E in books:
        l, _, _, _, idx = torch_port.quantize_train(r, E, beta)
        e = E.detach()[idx.view(-1)].view(B, H, W, D).permute(0, 3, 1, 2)
        ids.append(idx.view(-1))
        r = r - e
        S = e if S is None else S + e
        loss = l if loss is None else loss + l
    z_q = z_nchw + (S - z_nchw).detach()
    return loss, z_q, torch.stack(ids)
