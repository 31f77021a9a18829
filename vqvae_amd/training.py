"""Training-step companions of the forward path.

  * `vq_backward`           the VectorQuantizer gradients on the GPU (vqvae_vq_backward_f32)
  * `VQStraightThrough`     autograd.Function pairing the fused HIP forward with that backward, so
                            `main.py:74-79` (loss.backward()) works with the HIP quantizer; the convs
                            must then run on the "torch" backend (their backward is torch's)
  * `vq_grouped_backward`,
    `GroupedStraightThrough` grouped (product) quantization's gradients (vqvae_vq_grouped_backward_f32) and its autograd pairing
  * `fsq_backward`,
    `FSQStraightThrough`    finite scalar quantization's gradients (vqvae_fsq_backward_f32) and its autograd pairing
  * `lfq_backward`,
    `LFQStraightThrough`    lookup-free quantization's gradients, its entropy loss included (vqvae_lfq_backward_f32), and its
                            autograd pairing
  * `LinearRows`            the per-row linear map y = W x + b (vqvae_linear_rows_forward_f32 / _backward_f32) under autograd: the
                            projections of the factorized quantizers
  * `step_losses`           `recon_loss`, `loss` and `perplexity` of main.py:75-76,81-83 in one fused
                            reduction, returned as ONE 3-element device tensor (one D2H copy per step)

No CPU path and no fallback: CPU tensors raise VqvaeHipError.
"""
from __future__ import annotations

import torch

from . import _lib
from . import functional as F_hip


def _bwd_args(z_e, idx, grad_zq, grad_loss, rowmajor):
    """what the three quantizer backwards share in front of their codebooks: -> ((B, D, H, W), and the dense forms of z_e, idx,
    grad_zq -- z_e's shape, or None -- and grad_loss -- a device scalar, or None)"""
    dims = _lib.map_dims("z_e", z_e, rowmajor)
    _lib.check_dev("idx", idx, torch.int64)
    z_e = _lib.dense(z_e, 4)                   # (the entries pick their kernels' width by these pointers)
    return dims, z_e, _lib.dense(idx, 8), _lib.same_shape("grad_zq", grad_zq, z_e), _lib.device_scalar("grad_loss", grad_loss)


def _bwd_launch(entry, what, dims, z_e, books, idx, grad_zq, grad_loss, beta, flags, need_z, need_books, **count):
    """... and behind them: the gradients' and the workspace's allocation and the launch of vqvae_<entry>_f32.  count: Q=stages or
    G=groups of an entry that takes a list of codebooks, nothing for the one-codebook entry.  -> (grad_z, codebook gradients)"""
    B, D, H, W = dims
    K, multi = books[0].shape[0], bool(count)
    dev = z_e.device
    with torch.cuda.device(dev):
        gz = torch.empty_like(z_e) if need_z else None
        ge = [torch.empty_like(c) for c in books] if need_books else None
        ws = _lib.workspace(f"vqvae_{entry}_workspace_bytes", what, "1 <= K <= 16384, 1 <= D <= 256, 1 <= N < 2^31, at most 16 stages or groups",
                            dict(N=B * H * W, K=K, D=D, **count), dev) if need_books else None
        _lib.check(getattr(_lib.load(), f"vqvae_{entry}_f32")(
            z_e.data_ptr(), _lib.ptr_array(books) if multi else books[0].data_ptr(), idx.data_ptr(), _lib.ptr(grad_zq),
            _lib.ptr(grad_loss), B, D, H, W, K, *count.values(), float(beta), flags, _lib.ptr(gz),
            _lib.ptr_array(ge) if multi else _lib.ptr(ge and ge[0]), *_lib.ws_args(ws), _lib.stream_ptr(z_e)))
    return gz, ge


def vq_backward(z_e, codebook, idx, grad_zq, grad_loss, beta, *, rowmajor=False, need_z=True, need_codebook=True,
                commitment=False, rotation=False):
    """Gradients of VectorQuantizer.forward (models/quantizer.py:63-67) w.r.t. z_e and the codebook.

    z_e / grad_zq: (B,D,H,W), or (B,H,W,D) when rowmajor.  grad_loss: 0-dim device tensor or None (=1).
    commitment=True: the z gradient of VectorQuantizerEMA's loss beta * mse instead (no codebook gradient).
    rotation=True: grad_zq reaches grad_z through the rotation trick (arXiv 2410.06424; csrc/vq_rotation.hip states the arithmetic
    and its fallback rows) instead of unchanged; needs need_z.  The codebook gradient is the same either way.
    Returns (grad_z or None, grad_codebook or None)."""
    if commitment and need_codebook:
        raise ValueError("the commitment-only gradient has no codebook term")
    if rotation and not need_z:
        raise ValueError("the rotation trick changes grad_z only: need_z must be set")
    dims, z_e, idx, grad_zq, grad_loss = _bwd_args(z_e, idx, grad_zq, grad_loss, rowmajor)
    _lib.check_dev("codebook", codebook)
    if codebook.dim() != 2 or codebook.shape[1] != dims[1] or idx.numel() != z_e.numel() // dims[1]:
        raise ValueError("shape mismatch between z_e, codebook and idx")
    flags = (F_hip.VQ_ROWMAJOR if rowmajor else 0) | (F_hip.VQ_BWD_COMMITMENT if commitment else 0) | \
        (F_hip.VQ_BWD_ROTATION if rotation else 0)
    gz, ge = _bwd_launch("vq_backward", "VQ backward", dims, z_e, [_lib.dense(codebook, 4)], idx, grad_zq, grad_loss, beta, flags,
                         need_z, need_codebook)
    return gz, ge and ge[0]


class VQStraightThrough(torch.autograd.Function):
    """(z_e, codebook) -> (loss, z_q, perplexity, idx, hist) with the reference's gradient structure
    [MEASURED in SURVEY.md 8b]: loss and z_q differentiable, perplexity / idx / hist not; d z_q / d z = I, or with rotation=True
    the rotation trick's lam R^T per row (vq_backward's rotation).  The forward is the same either way."""

    @staticmethod
    def forward(ctx, z_e, codebook, beta, rowmajor, workspace, prepared, rotation=False):
        z = _lib.dense(z_e.detach(), _lib.vq_align(codebook.shape[1]))
        w = _lib.dense(codebook.detach(), _lib.vq_align(codebook.shape[1]))
        loss, z_q, perplexity, idx, hist = F_hip.vq_forward(z, w, beta, rowmajor=rowmajor, workspace=workspace,
                                                            prepared=prepared)
        ctx.save_for_backward(z, w, idx)
        ctx.beta, ctx.rowmajor, ctx.rotation = beta, rowmajor, bool(rotation)
        ctx.mark_non_differentiable(perplexity, idx, hist)
        return loss, z_q, perplexity, idx, hist

    @staticmethod
    def backward(ctx, g_loss, g_zq, *_unused):
        z, w, idx = ctx.saved_tensors
        need_z, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if g_loss is None:
            g_loss = torch.zeros((), dtype=torch.float32, device=z.device)
        gz, gw = vq_backward(z, w, idx, g_zq, g_loss, ctx.beta, rowmajor=ctx.rowmajor, need_z=need_z,
                             need_codebook=need_w, rotation=ctx.rotation and need_z)
        return gz, gw, None, None, None, None, None


class VQEMAStraightThrough(torch.autograd.Function):
    """VectorQuantizerEMA's forward under autograd: (z_e, codebook) -> (beta * mse, z_q, perplexity, idx, hist).  Only z_e gets a
    gradient (dz = g_zq + g 2 beta (z - e_idx) / (N D)); the codebook is moved by the EMA update, which writes it in place right
    after this forward.  So the backward must not read the live weight: it keeps its own copy of the codebook it quantized with.
    rotation=True: g_zq goes through the rotation trick, as in VQStraightThrough."""

    @staticmethod
    def forward(ctx, z_e, codebook, beta, rowmajor, workspace, prepared, rotation=False):
        z = _lib.dense(z_e.detach(), _lib.vq_align(codebook.shape[1]))
        w = _lib.dense(codebook.detach(), _lib.vq_align(codebook.shape[1]))
        mse, z_q, perplexity, idx, hist = F_hip.vq_forward(z, w, 0.0, rowmajor=rowmajor, workspace=workspace, prepared=prepared)
        ctx.save_for_backward(z, w.clone(), idx)
        ctx.beta, ctx.rowmajor, ctx.rotation = beta, rowmajor, bool(rotation)
        ctx.mark_non_differentiable(perplexity, idx, hist)
        return mse * beta, z_q, perplexity, idx, hist

    @staticmethod
    def backward(ctx, g_loss, g_zq, *_unused):
        z, w, idx = ctx.saved_tensors
        gz = None
        if ctx.needs_input_grad[0]:
            if g_loss is None:
                g_loss = torch.zeros((), dtype=torch.float32, device=z.device)
            gz, _ = vq_backward(z, w, idx, g_zq, g_loss, ctx.beta, rowmajor=ctx.rowmajor, need_codebook=False, commitment=True,
                                rotation=ctx.rotation)
        return gz, None, None, None, None, None, None


class L2NormRows(torch.autograd.Function):
    """x -> x / max(||row||, eps), forward and backward on the HIP kernels (functional.l2norm_rows / l2norm_rows_backward;
    csrc/vq_cosine.hip): what the cosine-similarity codebook puts in front of the quantizer, for z_e and for the codebook.
    apply(x, rowmajor=False, eps=1e-12); x: a 4-D map in the quantizer's layouts or a 2-D (K, D) tensor."""

    @staticmethod
    def forward(ctx, x, rowmajor=False, eps=1e-12):
        y, denom = F_hip.l2norm_rows(x.detach(), rowmajor=rowmajor, eps=eps)
        ctx.save_for_backward(y, denom)
        ctx.rowmajor, ctx.eps = rowmajor, eps
        return y

    @staticmethod
    def backward(ctx, g):
        y, denom = ctx.saved_tensors
        return F_hip.l2norm_rows_backward(y, denom, g, rowmajor=ctx.rowmajor, eps=ctx.eps), None, None


class _StepLosses(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x_hat, x, embedding_loss, perplexity, inv_var):
        _lib.check_dev("x_hat", x_hat)
        _lib.check_dev("x", x)
        xh, xx = _lib.dense(x_hat.detach()), _lib.dense(x.detach())
        if xh.shape != xx.shape:
            raise ValueError("x_hat and x must have the same shape")
        dev = xh.device
        L = _lib.load()
        with torch.cuda.device(dev):
            out = torch.empty(3, dtype=torch.float32, device=dev)
            ws = torch.empty(L.vqvae_recon_loss_workspace_bytes(), dtype=torch.uint8, device=dev)
            el = _lib.dense(embedding_loss.detach().reshape(1), 4) if embedding_loss is not None else None
            pp = _lib.dense(perplexity.detach().reshape(1), 4) if perplexity is not None else None
            _lib.check(L.vqvae_recon_loss_f32(xh.data_ptr(), xx.data_ptr(), xh.numel(), float(inv_var), _lib.ptr(el), _lib.ptr(pp),
                                              out.data_ptr(), *_lib.ws_args(ws), _lib.stream_ptr(xh)))
        ctx.save_for_backward(xh, xx)
        ctx.inv_var = float(inv_var)
        return out

    @staticmethod
    def backward(ctx, g):
        xh, xx = ctx.saved_tensors
        gx = gel = None
        if ctx.needs_input_grad[0]:
            gsum = _lib.dense((g[0] + g[1]).reshape(1), 4)       # recon_loss feeds out[0] and out[1]
            gx = torch.empty_like(xh)
            with torch.cuda.device(xh.device):
                _lib.check(_lib.load().vqvae_recon_loss_backward_f32(xh.data_ptr(), xx.data_ptr(), xh.numel(),
                                                                     ctx.inv_var, gsum.data_ptr(), gx.data_ptr(),
                                                                     _lib.stream_ptr(xh)))
        if ctx.needs_input_grad[2]:
            gel = g[1].reshape(())
        return gx, None, gel, None, None


def step_losses(embedding_loss, x_hat, perplexity, x, x_train_var):
    """-> 3-element fp32 device tensor [recon_loss, loss, perplexity] (main.py:75-76, 81-83).

    `stats[1].backward()` is `loss.backward()` of main.py:78; `stats.tolist()` is the single D2H copy
    that replaces the three `.cpu()` calls of main.py:81-83."""
    return _StepLosses.apply(x_hat, x, embedding_loss, perplexity, 1.0 / float(x_train_var))


# ---- residual vector quantization (csrc/vq_residual.hip) -------------------------------------------------------------------------

def vq_residual_backward(z_e, codebooks, idx, grad_zq, grad_loss, beta, *, rowmajor=False, shared=False, need_z=True,
                         need_codebooks=True):
    """Gradients of functional.vq_residual_forward (vqvae_vq_residual_backward_f32): what autograd derives when every stage is the
    reference quantizer and r_{q+1} = r_q - e_q.detach().

    z_e / grad_zq: (B,D,H,W), or (B,H,W,D) when rowmajor.  idx: the forward's (Q, N) indices.  grad_loss: 0-dim device tensor or
    None (= 1).  -> (grad_z or None, list of codebook gradients -- one per codebook, one in all when shared -- or None)."""
    dims, z_e, idx, grad_zq, grad_loss = _bwd_args(z_e, idx, grad_zq, grad_loss, rowmajor)
    books, nb = F_hip._residual_books(codebooks, shared)
    N = z_e.numel() // dims[1]
    if books[0].shape[1] != dims[1] or idx.numel() % N or idx.numel() == 0:
        raise ValueError("shape mismatch between z_e, the codebooks and idx")
    Q = idx.numel() // N
    if nb is not None and nb != Q:
        raise ValueError(f"{Q} stages of indices for {nb} codebooks")
    if not (need_z or need_codebooks):
        return None, None
    flags = (F_hip.VQ_ROWMAJOR if rowmajor else 0) | (F_hip.VQ_RESIDUAL_SHARED if shared else 0)
    return _bwd_launch("vq_residual_backward", "residual VQ backward", dims, z_e, books, idx, grad_zq, grad_loss, beta, flags,
                       need_z, need_codebooks, Q=Q)


class RVQStraightThrough(torch.autograd.Function):
    """(z_e, E_0 .. ) -> (loss, z_q, perplexity (Q,), idx (Q, N), hist (Q, K), loss_stage (Q,)) of the residual quantizer: loss and
    z_q differentiable (d z_q / d z = I), the rest not.  apply(z_e, beta, rowmajor, shared, n_q, workspace, prepared, *codebooks)."""

    @staticmethod
    def forward(ctx, z_e, beta, rowmajor, shared, n_q, workspace, prepared, *codebooks):
        al = _lib.vq_align(codebooks[0].shape[1])
        z = _lib.dense(z_e.detach(), al)
        books = [_lib.dense(c.detach(), al) for c in codebooks]
        loss, z_q, perplexity, idx, hist, loss_stage = F_hip.vq_residual_forward(
            z, books, beta, rowmajor=rowmajor, shared=shared, n_q=n_q, workspace=workspace, prepared=prepared)
        ctx.save_for_backward(z, idx, *books)
        ctx.beta, ctx.rowmajor, ctx.shared = beta, rowmajor, shared
        ctx.mark_non_differentiable(perplexity, idx, hist, loss_stage)
        return loss, z_q, perplexity, idx, hist, loss_stage

    @staticmethod
    def backward(ctx, g_loss, g_zq, *_unused):
        z, idx, *books = ctx.saved_tensors
        need_z = ctx.needs_input_grad[0]
        need_w = any(ctx.needs_input_grad[7:])
        if g_loss is None:
            g_loss = torch.zeros((), dtype=torch.float32, device=z.device)
        gz, ge = vq_residual_backward(z, books, idx, g_zq, g_loss, ctx.beta, rowmajor=ctx.rowmajor, shared=ctx.shared,
                                      need_z=need_z, need_codebooks=need_w)
        if ge is None:
            ge = [None] * len(books)
        return (gz, None, None, None, None, None, None) + tuple(ge)


# ---- grouped (product) vector quantization (csrc/vq_grouped.hip) -----------------------------------------------------------------

def vq_grouped_backward(z_e, codebooks, idx, grad_zq, grad_loss, beta, *, rowmajor=False, need_z=True, need_codebooks=True,
                        commitment=False):
    """Gradients of functional.vq_grouped_forward (vqvae_vq_grouped_backward_f32): per group those of vq_backward on the group's
    channels with the upstream loss gradient grad_loss / G.

    z_e / grad_zq: (B,D,H,W), or (B,H,W,D) when rowmajor.  idx: the forward's (G, N) indices.  grad_loss: 0-dim device tensor or
    None (= 1).  commitment=True: the z gradient of the EMA form's loss, beta * the mean of the groups' mse (no codebook gradients).
    -> (grad_z or None, list of G codebook gradients or None)."""
    if commitment and need_codebooks:
        raise ValueError("the commitment-only gradient has no codebook term")
    dims, z_e, idx, grad_zq, grad_loss = _bwd_args(z_e, idx, grad_zq, grad_loss, rowmajor)
    books = _lib.books(codebooks, 1, 16, 4)
    G = len(books)
    if books[0].shape[1] * G != dims[1] or idx.numel() * dims[1] != G * z_e.numel():
        raise ValueError("shape mismatch between z_e, the codebooks and idx")
    if not (need_z or need_codebooks):
        return None, None
    flags = (F_hip.VQ_ROWMAJOR if rowmajor else 0) | (F_hip.VQ_BWD_COMMITMENT if commitment else 0)
    return _bwd_launch("vq_grouped_backward", "grouped VQ backward", dims, z_e, books, idx, grad_zq, grad_loss, beta, flags,
                       need_z, need_codebooks, G=G)


class GroupedStraightThrough(torch.autograd.Function):
    """(z_e, E_0 .. E_{G-1}) -> (loss, z_q, perplexity (G,), idx (G, N), hist (G, K), loss_group (G,), slabs or None) of the grouped
    quantizer: loss and z_q differentiable (d z_q / d z = I), the rest not.
    apply(z_e, beta, rowmajor, commitment, want_slabs, workspace, prepared, *codebooks).  commitment: the EMA form -- the forward runs
    with beta 0 and returns beta * the mean of the groups' mse, only z_e gets a gradient, and the backward keeps its own copies of
    the codebooks (the EMA update writes the live ones right after the forward)."""

    @staticmethod
    def forward(ctx, z_e, beta, rowmajor, commitment, want_slabs, workspace, prepared, *codebooks):
        z = _lib.dense(z_e.detach(), 4)
        books = [_lib.dense(c.detach(), 4) for c in codebooks]
        out = F_hip.vq_grouped_forward(z, books, 0.0 if commitment else beta, rowmajor=rowmajor, want_slabs=want_slabs,
                                       workspace=workspace, prepared=prepared)
        loss, z_q, perplexity, idx, hist, loss_group = out[:6]
        slabs = out[6] if want_slabs else None
        if commitment:
            loss, loss_group = loss * beta, loss_group * beta
            books = [c.clone() for c in books]
        ctx.save_for_backward(z, idx, *books)
        ctx.beta, ctx.rowmajor, ctx.commitment = beta, rowmajor, bool(commitment)
        # (one call: a second one would replace the first's list)
        ctx.mark_non_differentiable(perplexity, idx, hist, loss_group, *([slabs] if slabs is not None else []))
        return loss, z_q, perplexity, idx, hist, loss_group, slabs

    @staticmethod
    def backward(ctx, g_loss, g_zq, *_unused):
        z, idx, *books = ctx.saved_tensors
        need_z = ctx.needs_input_grad[0]
        need_w = any(ctx.needs_input_grad[7:]) and not ctx.commitment
        if g_loss is None:
            g_loss = torch.zeros((), dtype=torch.float32, device=z.device)
        gz, ge = vq_grouped_backward(z, books, idx, g_zq, g_loss, ctx.beta, rowmajor=ctx.rowmajor, need_z=need_z,
                                     need_codebooks=need_w, commitment=ctx.commitment)
        if ge is None:
            ge = [None] * len(books)
        return (gz, None, None, None, None, None, None) + tuple(ge)


# ---- finite scalar quantization (csrc/vq_fsq.hip) --------------------------------------------------------------------------------

def fsq_backward(z_e, grad_zq, w_in, b_in, w_out, levels, *, rowmajor=False, need_z=True, need_params=True):
    """Gradients of functional.fsq_forward's z_q (vqvae_fsq_backward_f32): rounding is straight-through, tanh and both projections
    are differentiated; t is recomputed from z_e.  z_e / grad_zq: (B,D,H,W), or (B,H,W,D) when rowmajor.
    -> (grad_z or None, (grad_w_in, grad_b_in, grad_w_out, grad_b_out) or None).  The parameter gradients are fp64 sums in a fixed
    order: the same bits in both layouts and in every run."""
    B, D, H, W = _lib.map_dims("z_e", z_e, rowmajor)
    _lib.check_dev("grad_zq", grad_zq)
    grad_zq = _lib.same_shape("grad_zq", grad_zq, z_e)
    if not (need_z or need_params):
        return None, None
    lv, c_lv, _ = F_hip._fsq_levels(levels)
    d = len(lv)
    w_in, b_in, w_out = F_hip._fsq_params(D, d, w_in=w_in, b_in=b_in, w_out=w_out)
    z_e = _lib.dense(z_e, 4)
    dev = z_e.device
    with torch.cuda.device(dev):
        gz = torch.empty_like(z_e) if need_z else None
        gp, p = _param_grads(w_in, b_in, w_out, need_params)
        ws = F_hip.fsq_backward_workspace(B * H * W, D, d, dev) if need_params else None
        _lib.check(_lib.load().vqvae_fsq_backward_f32(
            z_e.data_ptr(), grad_zq.data_ptr(), w_in.data_ptr(), b_in.data_ptr(), w_out.data_ptr(), c_lv, d, B, D, H, W,
            F_hip.VQ_ROWMAJOR if rowmajor else 0, _lib.ptr(gz), *p, *_lib.ws_args(ws), _lib.stream_ptr(z_e)))
    return gz, gp


def _param_grads(w_in, b_in, w_out, need_params):
    """-> (the four empty parameter gradients of a projected-code quantizer -- like w_in, b_in, w_out and b_out (D,) -- or None,
    their four pointers or Nones)"""
    if not need_params:
        return None, [None] * 4
    gp = (torch.empty_like(w_in), torch.empty_like(b_in), torch.empty_like(w_out), w_out.new_empty(w_out.shape[0]))
    return gp, [t.data_ptr() for t in gp]


class FSQStraightThrough(torch.autograd.Function):
    """(z_e, w_in, b_in, w_out, b_out) -> (z_q, perplexity, idx, hist) of finite scalar quantization: z_q differentiable with respect
    to z_e and the four parameters, the rest not.  apply(z_e, w_in, b_in, w_out, b_out, levels, rowmajor)."""

    @staticmethod
    def forward(ctx, z_e, w_in, b_in, w_out, b_out, levels, rowmajor):
        z = _lib.dense(z_e.detach(), 4)
        params = [_lib.dense(t.detach(), 4) for t in (w_in, b_in, w_out, b_out)]
        z_q, perplexity, idx, hist = F_hip.fsq_forward(z, *params, levels, rowmajor=rowmajor)
        ctx.save_for_backward(z, *params[:3])
        ctx.levels, ctx.rowmajor = tuple(levels), rowmajor
        ctx.mark_non_differentiable(perplexity, idx, hist)
        return z_q, perplexity, idx, hist

    @staticmethod
    def backward(ctx, g_zq, *_unused):
        z, w_in, b_in, w_out = ctx.saved_tensors
        need_z, need_p = ctx.needs_input_grad[0], any(ctx.needs_input_grad[1:5])
        gz, gp = fsq_backward(z, g_zq, w_in, b_in, w_out, ctx.levels, rowmajor=ctx.rowmajor, need_z=need_z, need_params=need_p)
        gp = gp if gp is not None else (None,) * 4
        return (gz,) + tuple(g if n else None for g, n in zip(gp, ctx.needs_input_grad[1:5])) + (None, None)


# ---- lookup-free quantization (csrc/vq_lfq.hip) ----------------------------------------------------------------------------------

def lfq_backward(z_e, grad_zq, grad_loss, avg, w_in, b_in, w_out, n_e, *, beta=0.25, entropy_weight=0.1, diversity_gamma=1.0,
                 inv_temperature=100.0, rowmajor=False, need_z=True, need_params=True, workspace=None):
    """Gradients of functional.lfq_forward's z_q and loss (vqvae_lfq_backward_f32): rounding is straight-through, the commitment and
    entropy terms are differentiated through the factorised softmax.  grad_zq (z_e's shape) may be None (zero); grad_loss is a device
    scalar or None (one); avg is the forward's (K,) fp64, or None when the loss has no gradient.
    -> (grad_z or None, (grad_w_in, grad_b_in, grad_w_out, grad_b_out) or None), in fixed-order fp64 sums."""
    B, D, H, W = _lib.map_dims("z_e", z_e, rowmajor)
    grad_zq = _lib.same_shape("grad_zq", grad_zq, z_e)
    if not (need_z or need_params):
        return None, None
    d = F_hip._lfq_bits(n_e)
    w_in, b_in, w_out = F_hip._fsq_params(D, d, w_in=w_in, b_in=b_in, w_out=w_out)
    if avg is not None:
        _lib.check_dev("avg", avg, torch.float64)
        if avg.numel() != n_e:
            raise ValueError("avg must hold n_e values")
        avg = _lib.dense(avg, 8)
    grad_loss = _lib.device_scalar("grad_loss", grad_loss)
    z_e = _lib.dense(z_e, 4)
    dev = z_e.device
    with torch.cuda.device(dev):
        gz = torch.empty_like(z_e) if need_z else None
        gp, p = _param_grads(w_in, b_in, w_out, need_params)
        ws = workspace if workspace is not None else F_hip.lfq_workspace(B * H * W, D, d, dev)
        _lib.check(_lib.load().vqvae_lfq_backward_f32(
            z_e.data_ptr(), _lib.ptr(grad_zq), _lib.ptr(grad_loss), _lib.ptr(avg), w_in.data_ptr(), b_in.data_ptr(), w_out.data_ptr(),
            d, B, D, H, W, F_hip.VQ_ROWMAJOR if rowmajor else 0, beta, entropy_weight, diversity_gamma, inv_temperature,
            _lib.ptr(gz), *p, *_lib.ws_args(ws), _lib.stream_ptr(z_e)))
    return gz, gp


class LFQStraightThrough(torch.autograd.Function):
    """(z_e, w_in, b_in, w_out, b_out) -> (z_q, loss, perplexity, idx, hist, losses, avg) of lookup-free quantization: z_q and loss
    (0-dim) differentiable with respect to z_e and the four parameters, the rest not.
    apply(z_e, w_in, b_in, w_out, b_out, n_e, (beta, entropy_weight, diversity_gamma, inv_temperature), rowmajor)."""

    @staticmethod
    def forward(ctx, z_e, w_in, b_in, w_out, b_out, n_e, weights, rowmajor):
        z = _lib.dense(z_e.detach(), 4)
        params = [_lib.dense(t.detach(), 4) for t in (w_in, b_in, w_out, b_out)]
        beta, we, gamma, inv_t = (float(v) for v in weights)
        z_q, perplexity, idx, hist, losses, avg = F_hip.lfq_forward(
            z, *params, n_e, beta=beta, entropy_weight=we, diversity_gamma=gamma, inv_temperature=inv_t, rowmajor=rowmajor)
        ctx.save_for_backward(z, *params[:3], avg)
        ctx.n_e, ctx.weights, ctx.rowmajor = n_e, (beta, we, gamma, inv_t), rowmajor
        loss = losses[0].clone()
        ctx.mark_non_differentiable(perplexity, idx, hist, losses, avg)
        return z_q, loss, perplexity, idx, hist, losses, avg

    @staticmethod
    def backward(ctx, g_zq, g_loss, *_unused):
        z, w_in, b_in, w_out, avg = ctx.saved_tensors
        need_z, need_p = ctx.needs_input_grad[0], any(ctx.needs_input_grad[1:5])
        beta, we, gamma, inv_t = ctx.weights
        if g_zq is None and g_loss is None:
            return (None,) * 8
        gl = g_loss.to(torch.float32).reshape(()) if g_loss is not None else None
        gz, gp = lfq_backward(z, g_zq, gl, avg if g_loss is not None else None, w_in, b_in, w_out, ctx.n_e, beta=beta, entropy_weight=we,
                              diversity_gamma=gamma, inv_temperature=inv_t, rowmajor=ctx.rowmajor, need_z=need_z, need_params=need_p)
        gp = gp if gp is not None else (None,) * 4
        return (gz,) + tuple(g if n else None for g, n in zip(gp, ctx.needs_input_grad[1:5])) + (None, None, None)


# ---- the per-row linear map: a factorized codebook's projections (csrc/vq_linear.hip) --------------------------------------------

class LinearRows(torch.autograd.Function):
    """x -> W x + b on every row, forward and backward on the HIP kernels (functional.linear_rows / linear_rows_backward): differentiable
    with respect to x, w and b, and the backward asks only for the gradients that needs_input_grad names.
    apply(x, w, b, rowmajor=False); x: a 4-D map in the quantizer's layouts or a 2-D (K, Cin) tensor."""

    @staticmethod
    def forward(ctx, x, w, b, rowmajor=False):
        x_, w_ = _lib.dense(x.detach(), 4), _lib.dense(w.detach(), 4)
        y = F_hip.linear_rows(x_, w_, b.detach(), rowmajor=rowmajor)
        ctx.save_for_backward(x_, w_)
        ctx.rowmajor = rowmajor
        return y

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        want = tuple(ctx.needs_input_grad[:3])
        if not any(want):
            return None, None, None, None
        return F_hip.linear_rows_backward(x, g, w, rowmajor=ctx.rowmajor, want=want) + (None,)


# ---- orthogonal regularization of a codebook (csrc/vq_orthogonal.hip) ------------------------------------------------------------

class OrthogonalLoss(torch.autograd.Function):
    """rows (K, D) -> the orthogonal regularization loss of the rows as they stand, forward and backward on the HIP kernels
    (functional.vq_orthogonal_forward / vq_orthogonal_backward): differentiable with respect to rows only.  The forward saves V, the
    fp64 sums its pass forms anyway; the backward is one elementwise kernel.
    apply(rows, hist, max_codes, uniforms, workspace): hist (K,) int32 or None, max_codes with uniforms (K,) or None each."""

    @staticmethod
    def forward(ctx, rows, hist, max_codes, uniforms, workspace):
        loss, count, selected, saved = F_hip.vq_orthogonal_forward(rows.detach(), hist, max_codes=max_codes, uniforms=uniforms,
                                                                   want_saved=True, workspace=workspace)
        ctx.save_for_backward(saved, selected, count)
        return loss

    @staticmethod
    def backward(ctx, g):
        saved, selected, count = ctx.saved_tensors
        return F_hip.vq_orthogonal_backward(saved, selected, count, _lib.dense(g, 4)), None, None, None, None


# ---- the code-entropy loss of a learned codebook (csrc/vq_entropy.hip) --------------------------------------------------------------

class CodeEntropyLoss(torch.autograd.Function):
    """(z, codebook) -> term = P - gamma * H of the rows' softmax over the codes, forward and backward on the HIP kernels
    (functional.vq_entropy_forward / vq_entropy_backward): differentiable in z and in the codebook, and only the gradients that
    needs_input_grad names are formed.  The forward saves avg (K) and the rows' log-sum-exp and entropy (N, 2), all fp64; the (N, K)
    softmax never exists.  apply(z, codebook, inv_temperature, gamma, rowmajor, workspace) -> term (0-dim).  last_losses: the device
    3-vector (term, P, H) of the latest forward in this process, for a caller that logs the two entropies."""

    last_losses = None

    @staticmethod
    def forward(ctx, z, codebook, inv_temperature, gamma, rowmajor, workspace):
        losses, avg, rowstat = F_hip.vq_entropy_forward(z.detach(), codebook.detach(), inv_temperature=inv_temperature, gamma=gamma,
                                                        rowmajor=rowmajor, want_saved=True, workspace=workspace)
        ctx.save_for_backward(z, codebook, avg, rowstat)
        ctx.opts = (float(inv_temperature), float(gamma), bool(rowmajor), workspace)
        CodeEntropyLoss.last_losses = losses
        return losses[0].clone()

    @staticmethod
    def backward(ctx, g):
        z, codebook, avg, rowstat = ctx.saved_tensors
        s, gamma, rowmajor, ws = ctx.opts
        want = (ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        if not any(want):
            return None, None, None, None, None, None
        gz, ge = F_hip.vq_entropy_backward(z.detach(), codebook.detach(), avg, rowstat, _lib.dense(g, 4), inv_temperature=s, gamma=gamma,
                                           rowmajor=rowmajor, want=want, workspace=ws)
        return gz, ge, None, None, None, None
