"""Host-side mirror of the reference's GatedPixelCNN prior (pixelcnn/models.py) on libvqvae_hip.so.

Same class names, constructor signatures, sub-module / parameter names (hence `state_dict` keys) and default
initialisation as the reference, so a PixelCNN checkpoint written by `pixelcnn/gated_pixelcnn.py` loads unchanged:

    GatedPixelCNN(input_dim=256, dim=64, n_layers=15, n_classes=10)
        .forward(x (B,H,W) int64, label (B,) int64) -> logits (B, input_dim, H, W)          (models.py:118-127)
        .generate(label, shape=(8, 8), batch_size=64) -> (B, *shape) int64                   (models.py:129-142)
        .generate_cached(label, shape, batch_size, *, uniforms, generator, return_logits,   the same draw, one cached kernel
                         temperature, top_k, top_p, given)

Activations are row-major (B,H,W,C); a masked convolution is a stride-1 convolution over its causal tap list
(round 4: vqvae_conv_taps_forward_f32 -- the conv path's kernels with an explicit tap list, no im2col pass; lists of more than
16 taps, i.e. the first layer's 4 x 7 vertical stack, run as a chain of launches over slices of the list); embeddings, the gated
activation (+ class-conditional term) and the residual add are small HIP kernels (csrc/pixelcnn.hip).  The
categorical sampling of `generate` uses torch's softmax + multinomial on the device, as the reference does.

Training (pixelcnn/gated_pixelcnn.py:78-111).  When the module is in training mode, grad is enabled and some parameter requires
grad, `GatedPixelCNN.forward` and `GatedMaskedConv2d.forward` build an autograd graph whose every layer runs forward AND backward on
libvqvae_hip.so (csrc/pixelcnn_backward.hip): one autograd.Function per gated layer, the embeddings, the 1x1 head convs and the
layout changes.  The forward is the same sequence of launches as the eval path, so the logits are the same bits.  Backward:
tap-list weight gradients (vqvae_conv_taps_wgrad_f32, over the FULL tap list -- the mask-'A' taps get the nonzero gradient the
reference's autograd gives them), tap-list data gradients through the forward's tap kernels with the taps negated and the weight
transposed per tap (vqvae_conv_taps_pack_dgrad_f32), the 1x1 layers through the conv path's CONVT_1x1 kernels and
vqvae_conv_wgrad_ex_f32, the gated activation's backward with the class-conditional per-image sums, and sort-based segmented sums
for both embeddings.  No floating-point atomics: two backward passes give the same bits.  `cross_entropy` is the HIP form of the
reference's criterion.  Every other case (eval mode, torch.no_grad(), generate, the hipGraph sampler) runs the forward-only path.
No CPU path, no fallback.

Sampling (csrc/pixelcnn_sample.hip).  `generate_cached` keeps each layer's state and computes only what the next pixel needs: per
row the vertical stacks of every layer, per position the horizontal stacks, the head and one draw -- one kernel, one workgroup per
image.  Its draw takes a temperature, top-k and top-p, and positions whose code is given are not drawn (a second instantiation of
the kernel; the plain draw keeps its own).  `sample_images` decodes its maps with VQVAE.decode_indices; `complete_images` keeps the
top latent rows of encoded images and samples the rest.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from . import _cache, _lib, conv_hip
from ._lib import VqvaeHipError, ptr, ws_args, stream_ptr as _sp
from .autograd_conv import CONVT_1x1, _holder, conv_wgrad, relu_backward
from .conv_hip import CONV_1x1, RELU_OUT


SAMPLE_NONFINITE, SAMPLE_GIVEN_RANGE = 1, 2          # VQVAE_SAMPLE_* status bits of the cached sampler (include/vqvae_hip.h)


def weights_init(m):
    """models.py:9-16 (the reference prints when a module has no .weight; the RNG stream is what matters)."""
    classname = m.__class__.__name__
    if classname.find('Conv') != -1:
        try:
            nn.init.xavier_uniform_(m.weight.data)
            m.bias.data.fill_(0)
        except AttributeError:
            pass


class GatedActivation(nn.Module):
    def forward(self, x):                                       # parameter-free; fused into the HIP kernels
        raise VqvaeHipError("GatedActivation is fused into GatedMaskedConv2d's HIP forward")


class _Holder:
    pass


def _gather_rows(idx, table):
    idx = _lib.dense(idx, 8).view(-1)
    n, Cc = idx.numel(), table.shape[1]
    out = torch.empty((n, Cc), dtype=torch.float32, device=table.device)
    _lib.check(_lib.load().vqvae_gather_rows_f32(idx.data_ptr(), _lib.dense(table.detach()).data_ptr(), n, Cc,
                                                 table.shape[0], out.data_ptr(), _sp(out)))
    return out


def _im2col(x_rows, taps):
    x_rows = _lib.dense(x_rows)
    B, H, W, Cc = x_rows.shape
    n = len(taps)
    dy = (C.c_int8 * n)(*[t[0] for t in taps])
    dx = (C.c_int8 * n)(*[t[1] for t in taps])
    out = torch.empty((B, H, W, n * Cc), dtype=torch.float32, device=x_rows.device)
    _lib.check(_lib.load().vqvae_im2col_rows_f32(x_rows.data_ptr(), B, H, W, Cc, n, C.cast(dy, C.c_void_p),
                                                 C.cast(dx, C.c_void_p), out.data_ptr(), _sp(out)))
    return out


def _gate(t1, t2, cond, dim):
    t1, t2, cond = _lib.dense(t1, 4), _lib.dense(t2, 4), _lib.dense(cond, 4)     # (element-wise kernels)
    B, H, W, _ = t1.shape
    out = torch.empty((B, H, W, dim), dtype=torch.float32, device=t1.device)
    _lib.check(_lib.load().vqvae_gated_activation_f32(t1.data_ptr(), ptr(t2), ptr(cond), B, H * W, dim, out.data_ptr(), _sp(out)))
    return out


def _add(a, b):
    a, b = _lib.dense(a), _lib.dense(b)
    out = torch.empty_like(a)
    _lib.check(_lib.load().vqvae_add_f32(a.data_ptr(), b.data_ptr(), a.numel(), out.data_ptr(), _sp(a)))
    return out


# ------------------------------------------------------------------------------------------------------------------ training

def _autograd_wanted(mod):
    """the autograd path runs in training mode, with grad enabled, when some parameter requires grad; everything else runs the
    forward-only path (eval, torch.no_grad(), generate, the hipGraph sampler)"""
    return mod.training and torch.is_grad_enabled() and any(p.requires_grad for p in mod.parameters())


def _ws(nbytes, dev):
    return torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=dev)


def _taps_arrays(taps, sign=1):
    k = len(taps)
    return (C.c_int8 * k)(*[sign * t[0] for t in taps]), (C.c_int8 * k)(*[sign * t[1] for t in taps])


def bias_grad(g):
    """per-channel sums over all pixels of a row-major gradient (vqvae_bias_grad_wide_f32: any width)"""
    g = _lib.dense(g, 4)
    Cc = g.shape[-1]
    L = _lib.load()
    n = L.vqvae_bias_grad_wide_workspace_bytes(Cc)
    ws = _ws(n, g.device)
    out = torch.empty(Cc, dtype=torch.float32, device=g.device)
    _lib.check(L.vqvae_bias_grad_wide_f32(g.data_ptr(), g.numel() // Cc, Cc, out.data_ptr(), ws.data_ptr(), n, _sp(g)))
    return out


def taps_wgrad(gy, x, taps):
    """(Cout, Cin, ntaps): grad_w[co][ci][t] = sum gy[b,y,x,co] x[b, y+dy_t, x+dx_t, ci]  (vqvae_conv_taps_wgrad_f32)"""
    gy, x = _lib.dense(gy), _lib.dense(x)
    B, H, W, Cin = x.shape
    Cout, n = gy.shape[3], len(taps)
    L = _lib.load()
    ws = _lib.workspace("vqvae_conv_taps_wgrad_workspace_bytes", "tap-list weight gradient", "1 to 32 taps, Cin and Cout multiples of 4",
                        dict(taps=n, Cin=Cin, Cout=Cout), x.device)
    gw = torch.empty((Cout, Cin, n), dtype=torch.float32, device=x.device)
    dy, dx = _taps_arrays(taps)
    _lib.check(L.vqvae_conv_taps_wgrad_f32(gy.data_ptr(), x.data_ptr(), B, H, W, Cin, Cout, n, C.cast(dy, C.c_void_p),
                                           C.cast(dx, C.c_void_p), gw.data_ptr(), *ws_args(ws), _sp(x)))
    return gw


def taps_dgrad(gy, mod, weight, taps, addend=None):
    """grad_x of conv_hip.conv_taps: the tap kernels over the negated taps with the per-tap transposed weight, packed per weight
    version on a holder of `mod` (vqvae_conv_taps_pack_dgrad_f32); lists longer than 16 taps run as the forward's slices, each
    launch adding to the previous one's result; `addend` rides in the first launch's epilogue."""
    gy = _lib.dense(gy)
    B, H, W, Cout = gy.shape
    Cin, n = weight.shape[1], len(taps)
    L = _lib.load()
    hold = _holder(mod, ("taps_dgrad", tuple(taps)))
    nsl = (n + 15) // 16
    per = (n + nsl - 1) // nsl
    y = _lib.dense(addend) if addend is not None else None
    for s0 in range(0, n, per):
        sl = taps[s0:s0 + per]
        k = len(sl)
        dy, dx = _taps_arrays(sl)
        ndy, ndx = _taps_arrays(sl, -1)

        def pack(w, buf, dy=dy, dx=dx, k=k, s0=s0):
            return L.vqvae_conv_taps_pack_dgrad_f32(w.data_ptr(), n, s0, k, C.cast(dy, C.c_void_p), C.cast(dx, C.c_void_p), Cin,
                                                    Cout, buf.data_ptr(), _sp(w))
        packed = conv_hip._packed(hold, ("taps_dgrad", s0), weight, lambda k=k: L.vqvae_conv_taps_pack_dgrad_bytes(k, Cin, Cout), pack)
        out = torch.empty((B, H, W, Cin), dtype=torch.float32, device=gy.device)
        _lib.check(L.vqvae_conv_taps_forward_ep_f32(gy.data_ptr(), packed.data_ptr(), None, B, H, W, Cout, Cin, k,
                                                    C.cast(ndy, C.c_void_p), C.cast(ndx, C.c_void_p), 0,
                                                    ptr(y), None, out.data_ptr(), _sp(gy)))
        y = out
    return y


def gate_backward(t1, cond, go, dim, gcond=None, accumulate=False):
    """grad of (a|g) -> tanh(a) sigmoid(g) at (a|g) = t1 + cond[b]; with gcond (B, 2 dim): [+]= the per-image sums over HW"""
    t1, cond = _lib.dense(t1, 4), _lib.dense(cond, 4)
    B, H, W, _ = t1.shape
    gpre = torch.empty((B, H, W, 2 * dim), dtype=torch.float32, device=t1.device)
    go = _lib.dense(go, 4)
    _lib.check(_lib.load().vqvae_gated_activation_backward_f32(
        t1.data_ptr(), None, ptr(cond), go.data_ptr(), B, H * W, dim, gpre.data_ptr(), ptr(gcond) if accumulate else None, ptr(gcond),
        _sp(go)))
    return gpre


def gather_rows_backward(idx, g, rows):
    """grad_table (rows, C) of out = table[idx]: fixed-order segmented sums (vqvae_gather_rows_backward_f32)"""
    idx, g = _lib.dense(idx, 8).view(-1), _lib.dense(g, 4)
    n, Cc = idx.numel(), g.shape[-1]
    L = _lib.load()
    ws = _lib.workspace("vqvae_gather_rows_backward_workspace_bytes", "embedding backward", "1 <= n < 2^31, C >= 1, 1 <= rows <= 2^24",
                        dict(n=n, C=Cc, rows=rows), g.device)
    out = torch.empty((rows, Cc), dtype=torch.float32, device=g.device)
    _lib.check(L.vqvae_gather_rows_backward_f32(idx.data_ptr(), g.data_ptr(), n, Cc, rows, out.data_ptr(), *ws_args(ws), _sp(g)))
    return out


class _GatherFn(torch.autograd.Function):
    """nn.Embedding: out[i] = table[idx[i]] (vqvae_gather_rows_f32), backward the segmented sum over idx."""

    @staticmethod
    def forward(ctx, idx, table):
        ctx.save_for_backward(idx)
        ctx.rows = table.shape[0]
        return _gather_rows(idx, table)

    @staticmethod
    def backward(ctx, g):
        idx, = ctx.saved_tensors
        return None, gather_rows_backward(idx, g, ctx.rows) if ctx.needs_input_grad[1] else None


class _RowsToNchwFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t):
        return conv_hip.rows_to_nchw(t.detach())

    @staticmethod
    def backward(ctx, g):
        return conv_hip.nchw_to_rows(g)


class _NchwToRowsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t):
        return conv_hip.nchw_to_rows(t.detach())

    @staticmethod
    def backward(ctx, g):
        return conv_hip.rows_to_nchw(g)


class _Conv1x1Fn(torch.autograd.Function):
    """One 1x1 conv of the output head (models.py:111-115) on row-major activations.  relu_out: the ReLU between the two convs,
    whose backward the next conv's data gradient applies in its epilogue (mask_input=True there)."""

    @staticmethod
    def forward(ctx, x, weight, bias, mod, relu_out, mask_input):
        x = _lib.dense(x.detach())
        Cout, Cin = weight.shape[0], weight.shape[1]
        y = conv_hip.conv(CONV_1x1, x, mod, weight.detach(), bias.detach(), Cin, Cout, RELU_OUT if relu_out else 0)
        ctx.save_for_backward(x, weight.detach())
        ctx.mod, ctx.mask_input = mod, mask_input
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gy = _lib.dense(gy)
        Cout, Cin = w.shape[0], w.shape[1]
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = conv_hip.conv(CONVT_1x1, gy, _holder(ctx.mod, ("dgrad", CONV_1x1)), w, None, Cout, Cin, 0,
                               mask=x if ctx.mask_input else None)
        if ctx.needs_input_grad[1]:
            gw = conv_wgrad(gy, x, 1, 1, 0)
        if ctx.needs_input_grad[2]:
            gb = bias_grad(gy)
        return gx, gw, gb, None, None, None


class _GatedLayerFn(torch.autograd.Function):
    """One GatedMaskedConv2d (models.py:64-84) after its class embedding's gather: (x_v, x_h, cond) -> (out_v, out_h), row-major.
    Backward, given g_out_v and g_out_h:
      horiz_resid    g_out = W_hr^T g_out_h;  its weight / bias gradients;  residual: g_out_h passes on to x_h
      gate 2         g_pre2 = gate'(v2h + cond) g_out;  g_cond = per-image sums of g_pre2
      gate 1         g_pre1 = gate'(h_vert + cond) g_out_v;  g_cond += its sums
      vert_to_horiz  g_h_vert = W_vh^T g_pre2 + g_pre1 (the epilogue's addend);  gradients from (g_pre2, h_vert)
      horiz_stack    g_x_h = taps^T g_pre2 (+ g_out_h);  gradients from (g_pre2, x_h)
      vert_stack     g_x_v = taps^T g_h_vert (+ g_x_h where both stacks read one tensor);  gradients from (g_h_vert, x_v)"""

    @staticmethod
    def forward(ctx, x_v, x_h, cond, layer, same, *params):
        x_v, x_h, cond = _lib.dense(x_v.detach()), _lib.dense(x_h.detach()), cond.detach()
        out_v, out_h, h_vert, v2h, out = layer._forward_parts(x_v, x_h, cond)
        ctx.save_for_backward(x_v, x_h, cond, h_vert, v2h, out)
        ctx.layer, ctx.same = layer, same
        ctx.set_materialize_grads(False)
        return out_v, out_h

    @staticmethod
    def backward(ctx, g_ov, g_oh):
        x_v, x_h, cond, h_vert, v2h, out = ctx.saved_tensors
        L, dim = ctx.layer, ctx.layer.dim
        vs, vh, hs, hr = L.vert_stack, L.vert_to_horiz, L.horiz_stack, L.horiz_resid
        if g_oh is None:
            g_oh = torch.zeros_like(out)
        g_oh = _lib.dense(g_oh)
        g_out = conv_hip.conv(CONVT_1x1, g_oh, _holder(L, ("dgrad", "horiz_resid")), hr.weight.detach(), None, dim, dim, 0)
        gw_hr, gb_hr = conv_wgrad(g_oh, out, 1, 1, 0), bias_grad(g_oh)
        B = x_v.shape[0]
        g_cond = torch.empty((B, 2 * dim), dtype=torch.float32, device=x_v.device)
        g_pre2 = gate_backward(v2h, cond, g_out, dim, g_cond)
        g_pre1 = gate_backward(h_vert, cond, g_ov, dim, g_cond, accumulate=True) if g_ov is not None else None
        g_h_vert = conv_hip.conv(CONVT_1x1, g_pre2, _holder(L, ("dgrad", "vert_to_horiz")), vh.weight.detach(), None, 2 * dim,
                                 2 * dim, 0, addend=g_pre1)
        gw_vh, gb_vh = conv_wgrad(g_pre2, h_vert, 1, 1, 0), bias_grad(g_pre2)
        g_x_h = taps_dgrad(g_pre2, L, hs.weight.detach(), L._htaps, addend=g_oh if L.residual else None)
        gw_hs, gb_hs = taps_wgrad(g_pre2, x_h, L._htaps).view_as(hs.weight), bias_grad(g_pre2)
        g_x_v = taps_dgrad(g_h_vert, L, vs.weight.detach(), L._vtaps, addend=g_x_h if ctx.same else None)
        gw_vs, gb_vs = taps_wgrad(g_h_vert, x_v, L._vtaps).view_as(vs.weight), bias_grad(g_h_vert)
        return (g_x_v, None if ctx.same else g_x_h, g_cond, None, None,
                gw_vs, gb_vs, gw_vh, gb_vh, gw_hs, gb_hs, gw_hr, gb_hr)


class _CrossEntropyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rows, targets):
        rows, targets = _lib.dense(rows.detach(), 4), _lib.dense(targets, 8).view(-1)
        N, K = rows.shape
        L = _lib.load()
        nb = L.vqvae_cross_entropy_workspace_bytes(N)
        ws = _ws(nb, rows.device)
        loss = torch.empty((), dtype=torch.float32, device=rows.device)
        _lib.check(L.vqvae_cross_entropy_f32(rows.data_ptr(), targets.data_ptr(), N, K, loss.data_ptr(), ws.data_ptr(), nb, _sp(rows)))
        ctx.save_for_backward(rows, targets)
        return loss

    @staticmethod
    def backward(ctx, g):
        rows, targets = ctx.saved_tensors
        N, K = rows.shape
        g = _lib.dense(g.detach().reshape(1), 4)
        gx = torch.empty_like(rows)
        _lib.check(_lib.load().vqvae_cross_entropy_backward_f32(rows.data_ptr(), targets.data_ptr(), N, K, g.data_ptr(), gx.data_ptr(),
                                                                _sp(rows)))
        return gx, None


def cross_entropy(logits, x):
    """nn.CrossEntropyLoss()(logits.permute(0, 2, 3, 1).contiguous().view(-1, K), x.view(-1)) of gated_pixelcnn.py:91-96 on the HIP
    kernels: logits (B, K, H, W) as GatedPixelCNN.forward returns them, x (B, H, W) int64 -> 0-dim loss, differentiable.
    Max-subtracted log-sum-exp per row, fixed-order mean; targets outside [0, K) give NaN."""
    if not logits.is_cuda or logits.dtype != torch.float32 or x.dtype != torch.int64:
        raise VqvaeHipError("cross_entropy needs CUDA(HIP) float32 logits and int64 targets: there is no CPU path")
    B, K, H, W = logits.shape
    if tuple(x.shape) != (B, H, W):
        raise ValueError(f"targets of shape {tuple(x.shape)} do not match logits {tuple(logits.shape)}")
    rows = _NchwToRowsFn.apply(logits.contiguous()).view(-1, K)
    return _CrossEntropyFn.apply(rows, x)


class GatedMaskedConv2d(nn.Module):
    """Mirrors pixelcnn/models.py:29-84."""

    def __init__(self, mask_type, dim, kernel, residual=True, n_classes=10):
        super().__init__()
        assert kernel % 2 == 1, "Kernel size must be odd"
        self.mask_type = mask_type
        self.residual = residual
        self.dim, self.kernel = dim, kernel
        self.class_cond_embedding = nn.Embedding(n_classes, 2 * dim)
        self.vert_stack = nn.Conv2d(dim, dim * 2, (kernel // 2 + 1, kernel), 1, (kernel // 2, kernel // 2))
        self.vert_to_horiz = nn.Conv2d(2 * dim, 2 * dim, 1)
        self.horiz_stack = nn.Conv2d(dim, dim * 2, (1, kernel // 2 + 1), 1, (0, kernel // 2))
        self.horiz_resid = nn.Conv2d(dim, dim, 1)
        self.gate = GatedActivation()
        k = kernel
        # tap lists in the (ky, kx) order of the weight tensors; the conv's crop (:70, :74) keeps rows / columns
        # y + ky - k//2 and x + kx - k//2
        self._vtaps = [(ky - k // 2, kx - k // 2) for ky in range(k // 2 + 1) for kx in range(k)]
        self._htaps = [(0, kx - k // 2) for kx in range(k // 2 + 1)]

    def make_causal(self):                                      # models.py:60-62 (in place, like the reference)
        # through the parameter under no_grad, NOT `.data`: a `.data` write leaves `_version` alone, and the packed-weight cache
        # (conv_hip._packed, keyed on (data_ptr, _version)) would keep an image packed from un-masked or re-initialised weights
        #  -- e.g. after the reference's own `weights_init`, which writes through `.data`
        # The write bumps the version on EVERY call, so the one mask-'A' layer re-packs per forward (two small pack launches, also
        # inside a stream capture) -- the price of never serving a stale image for the layer whose weights the forward itself edits.
        with torch.no_grad():
            self.vert_stack.weight[:, :, -1].zero_()
            self.horiz_stack.weight[:, :, :, -1].zero_()

    def _masked(self, x_rows, conv, taps, tag):
        """One masked conv (bias included): the conv kernels over the tap list."""
        # (mask 'A': make_causal's in-place zeroing bumps the version and re-packs, conv_hip._packed; its 4 x 7 vertical stack is two
        # slices of 14 taps, the second launch adding to the first)
        return conv_hip.conv_taps(x_rows, conv, conv.weight, conv.bias, taps)

    def forward_rows(self, x_v, x_h, label):
        """x_v, x_h row-major (B,H,W,dim); label (B,) int64 -> (out_v, out_h) row-major."""
        if self.mask_type == 'A':
            self.make_causal()
        cond = _gather_rows(label, self.class_cond_embedding.weight)                       # :68
        return self._forward_parts(x_v, x_h, cond)[:2]

    def _forward_parts(self, x_v, x_h, cond):
        """The layer after the class embedding's gather -> (out_v, out_h, h_vert, v2h, out): the outputs and what backward reads."""
        dim = self.dim
        h_vert = self._masked(x_v, self.vert_stack, self._vtaps, "vert")                   # :69-70
        out_v = _gate(h_vert, None, cond, dim)                                              # :71
        h_horiz = self._masked(x_h, self.horiz_stack, self._htaps, "horiz")                # :73-74
        # :75, :77  v2h + h_horiz in the 1x1 conv's epilogue (same sum, same order: (v2h + h_horiz) + cond in the gate)
        v2h = conv_hip.conv(CONV_1x1, h_vert, self.vert_to_horiz, self.vert_to_horiz.weight, self.vert_to_horiz.bias,
                            2 * dim, 2 * dim, 0, addend=h_horiz)
        out = _gate(v2h, None, cond, dim)
        # :78-79  the horizontal residual in the 1x1 conv's epilogue
        out_h = conv_hip.conv(CONV_1x1, out, self.horiz_resid, self.horiz_resid.weight, self.horiz_resid.bias, dim,
                              dim, 0, addend=x_h.contiguous() if self.residual else None)
        return out_v, out_h, h_vert, v2h, out

    def train_rows(self, x_v, x_h, label):
        """forward_rows under autograd: the same launches, with what backward needs kept (_GatedLayerFn)."""
        if self.mask_type == 'A':
            self.make_causal()                                   # before the weights are handed to the Function
        cond = _GatherFn.apply(label.contiguous().view(-1), self.class_cond_embedding.weight)
        same = x_v is x_h                                        # the first layer: both stacks read the embedded input
        ps = (self.vert_stack.weight, self.vert_stack.bias, self.vert_to_horiz.weight, self.vert_to_horiz.bias,
              self.horiz_stack.weight, self.horiz_stack.bias, self.horiz_resid.weight, self.horiz_resid.bias)
        return _GatedLayerFn.apply(x_v, x_h, cond, self, same, *ps)

    def forward(self, x_v, x_h, h):
        """NCHW boundary of the reference (models.py:64-84)."""
        if _autograd_wanted(self):
            ov, oh = self.train_rows(_NchwToRowsFn.apply(x_v), _NchwToRowsFn.apply(x_h), h)
            return _RowsToNchwFn.apply(ov), _RowsToNchwFn.apply(oh)
        ov, oh = self.forward_rows(conv_hip.nchw_to_rows(x_v), conv_hip.nchw_to_rows(x_h), h)
        return conv_hip.rows_to_nchw(ov), conv_hip.rows_to_nchw(oh)


class GatedPixelCNN(nn.Module):
    """Mirrors pixelcnn/models.py:87-142."""

    def __init__(self, input_dim=256, dim=64, n_layers=15, n_classes=10):
        super().__init__()
        self.dim = dim
        self.embedding = nn.Embedding(input_dim, dim)
        self.layers = nn.ModuleList()
        for i in range(n_layers):
            mask_type = 'A' if i == 0 else 'B'
            kernel = 7 if i == 0 else 3
            residual = False if i == 0 else True
            self.layers.append(GatedMaskedConv2d(mask_type, dim, kernel, residual, n_classes))
        self.output_conv = nn.Sequential(nn.Conv2d(dim, 512, 1), nn.ReLU(True), nn.Conv2d(512, input_dim, 1))
        self.apply(weights_init)

    def forward(self, x, label):
        if _autograd_wanted(self):
            return self._forward_train(x, label)
        with torch.no_grad():
            return self._forward_eval(x, label)

    def _check(self, x):
        if not x.is_cuda or x.dtype != torch.int64:
            raise VqvaeHipError("GatedPixelCNN.forward needs CUDA(HIP) int64 indices: there is no CPU path")
        if self.dim % 4:
            raise VqvaeHipError("dim must be a multiple of 4 for the HIP kernels")

    def _forward_train(self, x, label):
        """forward under autograd: the launches of _forward_eval, each layer an autograd.Function with a HIP backward."""
        self._check(x)
        B, H, W = x.shape
        t = _GatherFn.apply(x.contiguous().view(-1), self.embedding.weight).view(B, H, W, self.dim)
        x_v, x_h = t, t
        for layer in self.layers:
            x_v, x_h = layer.train_rows(x_v, x_h, label)
        c0, c2 = self.output_conv[0], self.output_conv[2]
        t = _Conv1x1Fn.apply(x_h, c0.weight, c0.bias, c0, True, False)
        t = _Conv1x1Fn.apply(t, c2.weight, c2.bias, c2, False, True)
        return _RowsToNchwFn.apply(t)

    def _forward_eval(self, x, label):
        self._check(x)
        B, H, W = x.shape
        t = _gather_rows(x, self.embedding.weight).view(B, H, W, self.dim)                  # :119-121
        x_v, x_h = t, t
        for layer in self.layers:
            x_v, x_h = layer.forward_rows(x_v, x_h, label)
        c0, c2 = self.output_conv[0], self.output_conv[2]
        t = conv_hip.conv(CONV_1x1, x_h, c0, c0.weight, c0.bias, self.dim, c0.weight.shape[0], RELU_OUT)
        t = conv_hip.conv(CONV_1x1, t, c2, c2.weight, c2.bias, c0.weight.shape[0], c2.weight.shape[0], 0)
        return conv_hip.rows_to_nchw(t)                                                     # (B, input_dim, H, W)

    @torch.no_grad()
    def generate(self, label, shape=(8, 8), batch_size=64, use_graph=False):
        """models.py:129-142: one full forward per position, categorical sample from the softmax.

        use_graph=True captures the forward once into a hipGraph and replays it for each of the H*W positions:
        a forward is ~110 small launches, so at sampling batch sizes the eager loop is launch-bound."""
        param = next(self.parameters())
        x = torch.zeros((batch_size, *shape), dtype=torch.int64, device=param.device)
        label = label.contiguous()
        if use_graph:
            _lib.profile_enable(False)
            stream = torch.cuda.Stream(device=param.device)
            stream.wait_stream(torch.cuda.current_stream(param.device))
            with torch.cuda.stream(stream):
                for _ in range(2):
                    self.forward(x, label)                       # warm-up: weight packing, allocator pools
            stream.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=stream):
                static_logits = self.forward(x, label)
        for i in range(shape[0]):
            for j in range(shape[1]):
                if use_graph:
                    graph.replay()
                    logits = static_logits
                else:
                    logits = self.forward(x, label)
                probs = torch.softmax(logits[:, :, i, j], -1)
                x[:, i, j].copy_(probs.multinomial(1).squeeze(-1))
        return x

    def _sampler_image(self):
        """The cached sampler's packed image (vqvae_pixelcnn_sample_pack_f32), kept in the module's side table and keyed on every
        parameter's (data_ptr, _version, device, shape).  make_causal runs first, as in the reference's generate; its in-place write
        bumps the mask-A weights' versions on every call, so the key is taken BEFORE it and stored with the versions AFTER it: a
        parameter changed between two calls (an optimizer step, load_state_dict, an in-place edit) misses, make_causal alone does
        not.  The masked taps are never packed, so a `.data` write to them cannot make the image stale."""
        params = list(self.parameters())

        def key():
            return tuple((p.data_ptr(), p._version, str(p.device), tuple(p.shape)) for p in params)

        before = key()
        self.layers[0].make_causal()
        side = _cache.side(self)
        hit = side.get("sampler_image")
        L = _lib.load()
        p0 = params[0]
        if hit is not None and hit[0] == before:
            img, mark = hit[1], hit[2]
            _cache.wait_ready(mark, p0.device)
        else:
            K, dim, n_layers = self.embedding.num_embeddings, self.dim, len(self.layers)
            n_classes = self.layers[0].class_cond_embedding.num_embeddings
            nb = L.vqvae_pixelcnn_sample_packed_bytes(K, dim, n_layers, n_classes)
            if nb == 0:
                raise VqvaeHipError(f"cached sampler: K={K}, dim={dim}, n_layers={n_layers} not supported")
            img = _ws(nb, p0.device)
            keep = [_lib.dense(p.detach(), 4) for p in params]             # alive until the pack launches are queued
            ptrs = (C.c_void_p * len(keep))(*[t.data_ptr() for t in keep])
            _lib.check(L.vqvae_pixelcnn_sample_pack_f32(ptrs, len(params), K, dim, n_layers, n_classes, img.data_ptr(), nb,
                                                        _sp(p0)))
            mark = _cache.mark_ready(p0.device)
        side["sampler_image"] = (key(), img, mark)
        return img

    @torch.no_grad()
    def generate_cached(self, label, shape=(8, 8), batch_size=64, *, uniforms=None, generator=None, return_logits=False,
                        temperature=1.0, top_k=None, top_p=None, given=None):
        """models.py:129-142 on the cached sampler (csrc/pixelcnn_sample.hip): one kernel that keeps every layer's state and computes
        only what each next pixel needs, instead of one full forward per position.

        label (batch_size,) int64 on the module's device; shape = (H, W) with H == W.  uniforms (batch_size, H, W) fp32 in [0, 1)
        drive the draws (drawn with torch.rand(generator=generator) when not given): position (y, x) takes the smallest code k
        whose running sum of exp(l - max l) exceeds u times the total.  Returns the (batch_size, H, W) int64 codes and, with
        return_logits, also the (batch_size, K, H, W) logits each position was drawn from.  Like generate, it leaves the mask-A
        taps zeroed.  Raises VqvaeHipError for CPU tensors, non-square or unsupported shapes and non-finite logits.

        Sampling controls (vqvae_pixelcnn_sample_ex_f32 states the exact rules), applied in this order: top_k keeps the top_k
        largest logits (ties go to the lower code; 1 is greedy decoding; None, 0 or >= K is off); temperature > 0 divides the
        logits; top_p in (0, 1] keeps the most probable codes up to a mass of top_p (None or 1 is off).  given, a (batch_size, H, W)
        int64 tensor on the device, fixes the code wherever it is >= 0 and leaves the negative positions to the draw; with
        return_logits the logits of given positions are returned too (teacher-forced logits).  ValueError for bad option values
        and shapes, IndexError for a given code >= K."""
        temperature = float(temperature)
        top_k = 0 if top_k is None else int(top_k)
        top_p = 1.0 if top_p is None else float(top_p)
        if not (0.0 < temperature < float("inf")):
            raise ValueError(f"temperature must be finite and > 0, got {temperature}")
        if top_k < 0:
            raise ValueError(f"top_k must be >= 0 or None, got {top_k}")
        if not (0.0 < top_p <= 1.0):
            raise ValueError(f"top_p must be in (0, 1], got {top_p}")
        p0 = self.embedding.weight
        if not p0.is_cuda or not torch.is_tensor(label) or not label.is_cuda:
            raise VqvaeHipError("generate_cached needs the module and label on a CUDA(HIP) device: there is no CPU path")
        H, W = (int(s) for s in shape)
        if H != W:
            raise VqvaeHipError(f"generate_cached samples square maps only, got {H} x {W}")
        B = int(batch_size)
        if given is not None:
            if not torch.is_tensor(given) or not given.is_cuda or given.dtype != torch.int64 or tuple(given.shape) != (B, H, W):
                raise ValueError(f"given must be a CUDA(HIP) int64 tensor of shape ({B}, {H}, {W})")
        dev = p0.device
        label = _lib.dense(label.to(device=dev, dtype=torch.int64), 8)
        if label.shape != (B,):
            raise ValueError(f"label must have shape ({B},), got {tuple(label.shape)}")
        if self.output_conv[0].weight.shape[0] != 512:
            raise VqvaeHipError("cached sampler: the output head must be 512 wide, as GatedPixelCNN builds it")
        K, dim, n_layers = self.embedding.num_embeddings, self.dim, len(self.layers)
        n_classes = self.layers[0].class_cond_embedding.num_embeddings
        L = _lib.load()
        nws = L.vqvae_pixelcnn_sample_workspace_bytes(B, H, W, dim, n_layers)
        if nws == 0 or L.vqvae_pixelcnn_sample_packed_bytes(K, dim, n_layers, n_classes) == 0:
            raise VqvaeHipError(f"cached sampler: B={B}, {H} x {W}, K={K}, dim={dim}, n_layers={n_layers} not supported")
        with torch.cuda.device(dev):
            img = self._sampler_image()
            if uniforms is None:
                uniforms = torch.rand((B, H, W), generator=generator, device=dev)
            elif not uniforms.is_cuda or uniforms.dtype != torch.float32 or tuple(uniforms.shape) != (B, H, W):
                raise VqvaeHipError(f"uniforms must be a CUDA(HIP) float32 tensor of shape ({B}, {H}, {W})")
            uniforms = _lib.dense(uniforms.to(dev), 4)
            out = torch.empty((B, H, W), dtype=torch.int64, device=dev)
            logits = torch.empty((B, K, H, W), dtype=torch.float32, device=dev) if return_logits else None
            status = torch.empty(B, dtype=torch.int32, device=dev)
            ws = _ws(nws, dev)
            if given is not None:
                given = _lib.dense(given.to(dev), 8)
            # (1, 0, 1, NULL) is vqvae_pixelcnn_sample_f32: the plain kernel
            _lib.check(L.vqvae_pixelcnn_sample_ex_f32(img.data_ptr(), img.numel(), label.data_ptr(), uniforms.data_ptr(), B, H, W, K,
                                                      dim, n_layers, n_classes, temperature, top_k, top_p,
                                                      ptr(given), out.data_ptr(), ptr(logits), status.data_ptr(),
                                                      ws.data_ptr(), nws, _sp(out)))
            bad = bad_given = 0
            if int((status != 0).sum()):
                st = status.cpu()
                bad = int(((st & SAMPLE_NONFINITE) != 0).sum())
                bad_given = int(((st & SAMPLE_GIVEN_RANGE) != 0).sum())
        if bad_given:
            raise IndexError(f"cached sampler: a given code >= {K} in {bad_given} of {B} images (status VQVAE_SAMPLE_GIVEN_RANGE)")
        if bad:
            raise VqvaeHipError(f"cached sampler: non-finite logits in {bad} of {B} images (status VQVAE_SAMPLE_NONFINITE)")
        return (out, logits) if return_logits else out


def sample_images(prior, vqvae, label, shape=(8, 8), batch_size=64, **kw):
    """The reference pipeline's last step: latent maps sampled from the prior (GatedPixelCNN.generate_cached, keyword arguments
    passed on) decoded by the VQ-VAE (VQVAE.decode_indices) -> (indices (B, H, W) int64, x_hat (B, C, 4 H, 4 W))."""
    idx = prior.generate_cached(label, shape, batch_size, **kw)
    H, W = idx.shape[1], idx.shape[2]
    return idx, vqvae.decode_indices(idx, batch_size, H, W)


@torch.no_grad()
def complete_images(prior, vqvae, x, label, keep_rows, **kw):
    """Completes partly known images: x (B, C, 4 H, 4 W) is encoded (VQVAE.encode), latent rows [0, keep_rows) are kept as given codes,
    the prior samples the remaining rows (GatedPixelCNN.generate_cached(given=...), keyword arguments passed on) and the VQ-VAE
    decodes the map (VQVAE.decode_indices) -> (indices (B, H, W) int64, x_hat (B, C, 4 H, 4 W))."""
    B = x.shape[0]
    enc = vqvae.encode(x)
    if enc.numel() % B:
        raise ValueError(f"{enc.numel()} codes do not divide into {B} maps")
    n = enc.numel() // B
    H = int(round(n ** 0.5))
    if H * H != n:
        raise ValueError(f"complete_images needs square latent maps, got {n} codes per image")
    keep_rows = int(keep_rows)
    if not 0 <= keep_rows <= H:
        raise ValueError(f"keep_rows must be in [0, {H}], got {keep_rows}")
    given = enc.reshape(B, H, H).to(torch.int64).clone()
    given[:, keep_rows:] = -1
    idx = prior.generate_cached(label, (H, H), B, given=given, **kw)
    return idx, vqvae.decode_indices(idx, B, H, H)
