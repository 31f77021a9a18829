"""torch-tensor front end of the C ABI: allocates outputs/workspaces with torch's
caching allocator, passes raw device pointers and the current HIP stream to
libvqvae_hip.so.  PyTorch is plumbing here (memory + streams); every kernel that
runs is ours.  No CPU path: CPU tensors are rejected.  The argument plumbing the
wrappers share (device and shape checks, map dimensions, workspaces, optional
pointers) is `_lib`'s "front-end helpers".
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._lib import check_dev, dense, map_dims, ptr, ptr_array, stream_ptr, written, ws_args

VQ_ROWMAJOR = 0x1
VQ_CODEBOOK_PREPARED = 0x2
VQ_EXACT_SWEEP = 0x4
VQ_BF16_FILTER = 0x8
VQ_UNFUSED = 0x40
VQ_UNITS64_8WAVES = 0x100
VQ_UNITS32_16WAVES = 0x200
# whole-path product scheme (vqvae_forward_f32 / vqvae_encoder_ex_f32 / vqvae_decoder_ex_f32)
FWD_CONV_BF16_SPLIT = 0x1000
FWD_CONV_EXACT_FP32 = 0x2000
FWD_DEBUG_ZE = 0x4000            # tests: the fused encoder+quantizer kernel also writes its z_e (include/vqvae_hip.h)
VQ_UNITS32_8WAVES = 0x400
VQ_BWD_COMMITMENT = 0x800        # vqvae_vq_backward_f32: grad_z of beta * mse only (VectorQuantizerEMA)
VQ_BWD_ROTATION = 0x20000        # vqvae_vq_backward_f32: grad_zq reaches grad_z through the rotation trick (csrc/vq_rotation.hip)


def _table(name, t, width=None):
    """(K, D) of a device fp32 table of two dimensions, D == width where one is given"""
    check_dev(name, t)
    if t.dim() != 2 or (width is not None and t.shape[1] != width):
        raise ValueError(f"{name} must be a 2-D (K, D{'' if width is None else f' = {width}'}) tensor, got {tuple(t.shape)}")
    return t.shape


def _indices(idx, n, what="B*H*W"):
    """the dense form of n indices (their device and dtype are the caller's first check)"""
    if idx.numel() != n:
        raise ValueError(f"idx must hold {what} = {n} indices")
    return dense(idx, 8)


def vq_workspace(K: int, D: int, device) -> torch.Tensor:
    return _lib.workspace("vqvae_vq_workspace_bytes", "VectorQuantizer", "D <= 256, K <= 16384", dict(N=0, K=K, D=D), device)


def vq_forward(z_e: torch.Tensor, codebook: torch.Tensor, beta: float, *, rowmajor: bool = False,
               workspace: torch.Tensor | None = None, prepared: bool = False, want_zq: bool = True,
               exact_sweep: bool = False, bf16_filter: bool = False, form: int = 0):
    """Fused VectorQuantizer forward (models/quantizer.py:29-76).

    z_e: (B,D,H,W) contiguous, or (B,H,W,D) contiguous when rowmajor.
    Returns (loss 0-dim, z_q like z_e or None, perplexity 0-dim, idx (N,1) int64, hist (K,) int32).
    exact_sweep=True forces the exhaustive fp32-MFMA kernel, bf16_filter=True round 1's two-sweep bf16 filter
    kernel, instead of the default (single-sweep fp16 screen with the stream tracker: D=64 rows, row-major or NCHW maps of
    32 k pixels); all three produce identical bits, the flags exist for testing and A/B timing.  form: 8 / 16 forces the
    stream-tracker kernel's launch form (64-row units on eight waves / 32-row units on sixteen waves per CU; 0 = by row count).
    """
    B, D, H, W = map_dims("z_e", z_e, rowmajor)
    check_dev("codebook", codebook)
    K, Dc = codebook.shape
    if Dc != D:
        # the reference silently mis-reshapes here (view(-1, e_dim), quantizer.py:46); be strict
        raise ValueError(f"channel dim {D} != embedding dim {Dc}")
    z_e = dense(z_e, _lib.vq_align(D))
    codebook = dense(codebook, _lib.vq_align(D))
    dev = z_e.device
    with torch.cuda.device(dev):
        if workspace is None:
            workspace = vq_workspace(K, D, dev)
            prepared = False
        z_q = torch.empty_like(z_e) if want_zq else None
        idx = torch.empty((B * H * W, 1), dtype=torch.int64, device=dev)
        hist = torch.empty((K,), dtype=torch.int32, device=dev)
        scal = torch.empty((2,), dtype=torch.float32, device=dev)
        flags = (VQ_ROWMAJOR if rowmajor else 0) | (VQ_CODEBOOK_PREPARED if prepared else 0) | \
            (VQ_EXACT_SWEEP if exact_sweep else 0) | (VQ_BF16_FILTER if bf16_filter else 0) | \
            (VQ_UNITS32_16WAVES if form == 16 else (VQ_UNITS64_8WAVES if form == 8 else 0))
        _lib.check(_lib.load().vqvae_vq_forward_f32(
            z_e.data_ptr(), codebook.data_ptr(), B, D, H, W, K, float(beta), flags, ptr(z_q), idx.data_ptr(), hist.data_ptr(),
            scal.data_ptr(), scal.data_ptr() + 4, *ws_args(workspace), stream_ptr(z_e)))
    return scal[0], z_q, scal[1], idx, hist


def vq_onehot(idx: torch.Tensor, K: int) -> torch.Tensor:
    """min_encodings (N,K) fp32 (models/quantizer.py:55-57)."""
    check_dev("idx", idx, torch.int64)
    idx = dense(idx, 8)
    N = idx.numel()
    out = torch.empty((N, K), dtype=torch.float32, device=idx.device)
    with torch.cuda.device(idx.device):
        _lib.check(_lib.load().vqvae_vq_onehot_f32(idx.data_ptr(), N, K, out.data_ptr(), stream_ptr(idx)))
    return out


def vq_decode_indices(idx: torch.Tensor, codebook: torch.Tensor, B: int, H: int, W: int, *, validate: bool = True) -> torch.Tensor:
    """indices -> z_q (B,D,H,W) (visualization.ipynb:358-365).  validate=False: no range check (for indices that come from the
    quantizer; the kernel never reads outside the codebook, a bad index shows as NaN rows)."""
    check_dev("idx", idx, torch.int64)
    check_dev("codebook", codebook)
    codebook = dense(codebook, 4)
    K, D = codebook.shape
    idx = _indices(idx, B * H * W)
    if validate:
        _lib.check_index_range(idx, K, "decode_indices")
    out = _lib.like_map(idx, D, False, (B, H, W))
    with torch.cuda.device(idx.device):
        _lib.check(_lib.load().vqvae_vq_decode_indices_f32(idx.data_ptr(), codebook.data_ptr(), B, D, H, W, K,
                                                           out.data_ptr(), stream_ptr(idx)))
    return out


def vq_ema_workspace(N: int, K: int, D: int, device) -> torch.Tensor:
    return _lib.workspace("vqvae_vq_ema_workspace_bytes", "EMA codebook update", "K <= 16384, D <= 256, N < 2^31",
                          dict(N=N, K=K, D=D), device)


def _ema_state(ema_cluster_size, ema_w, codebook, what, K=None, D=None):
    """-> (K, D) of the EMA state an update writes: three device fp32 tensors of matching shapes, and of the K or D given"""
    for name, t in (("ema_cluster_size", ema_cluster_size), ("ema_w", ema_w), ("codebook", codebook)):
        check_dev(name, t)
    if codebook.dim() != 2 or (K or codebook.shape[0], D or codebook.shape[1]) != codebook.shape or ema_w.shape != codebook.shape \
            or ema_cluster_size.shape != codebook.shape[:1]:
        raise ValueError(f"shape mismatch between {what}, ema_cluster_size, ema_w and codebook")
    return codebook.shape


def vq_ema_update(z_e: torch.Tensor, idx: torch.Tensor, ema_cluster_size: torch.Tensor, ema_w: torch.Tensor,
                  codebook: torch.Tensor, decay: float, eps: float = 1e-5, *, threshold: float | None = None,
                  uniforms: torch.Tensor | None = None, rowmajor: bool = False, workspace: torch.Tensor | None = None):
    """One EMA codebook update (arXiv 1711.00937 Appendix A.1; vqvae_vq_ema_update_f32) from the rows z_e and the indices the
    forward assigned them.  Writes ema_cluster_size (K,), ema_w (K, D) and codebook (K, D) in place through their data pointers
    (no autograd version bump: the caller owns that; a strided one is computed in a dense temporary and copied back
    with copy_).  threshold / uniforms: restart codes whose averaged count is below
    threshold on the rows floor(u_k N) of z_e; both or neither.  z_e: (B,D,H,W), or (B,H,W,D) when rowmajor."""
    B, D, H, W = map_dims("z_e", z_e, rowmajor)
    check_dev("idx", idx, torch.int64)
    K, _ = _ema_state(ema_cluster_size, ema_w, codebook, "z_e, idx", D=D)
    idx = _indices(idx, B * H * W)
    if (threshold is None) != (uniforms is None):
        raise ValueError("restart needs both threshold and uniforms")
    uniforms = _lib.k_values("uniforms", uniforms, K)
    z_e = dense(z_e, 4)
    dev = z_e.device
    with torch.cuda.device(dev), written(ema_cluster_size, 4) as cs, written(ema_w, 4) as ew, written(codebook, 4) as cb:
        if workspace is None:
            workspace = vq_ema_workspace(B * H * W, K, D, dev)
        _lib.check(_lib.load().vqvae_vq_ema_update_f32(
            z_e.data_ptr(), idx.data_ptr(), B, D, H, W, K, float(decay), float(eps),
            float(threshold) if threshold is not None else -1.0, ptr(uniforms), VQ_ROWMAJOR if rowmajor else 0,
            cs.data_ptr(), ew.data_ptr(), cb.data_ptr(), *ws_args(workspace), stream_ptr(z_e)))
    return codebook


def vq_ema_stats_workspace(N: int, K: int, D: int, device) -> torch.Tensor:
    return _lib.workspace("vqvae_vq_ema_stats_workspace_bytes", "EMA statistics", "K <= 16384, D <= 256, 1 <= N < 2^31",
                          dict(N=N, K=K, D=D), device)


def vq_ema_stats(z_e: torch.Tensor, idx: torch.Tensor, K: int, *, row_uniforms: torch.Tensor | None = None,
                 rowmajor: bool = False, workspace: torch.Tensor | None = None, out: torch.Tensor | None = None) -> torch.Tensor:
    """One shard's sufficient statistics of the EMA codebook update (vqvae_vq_ema_stats_f32; csrc/vq_ema_merge.hip states the
    record): -> stats (K, C) float64 with the counts in column 0, the fp64 per-code sums of the rows in columns 1 .. D and, with
    row_uniforms (K fp32 in [0, 1)), the shard's restart candidates in columns D + 1 .. 2 D.  C = D + 1 or 2 D + 1.
    z_e: (B,D,H,W), or (B,H,W,D) when rowmajor; idx: the forward's indices.  out: a contiguous (K, C) float64 tensor to write."""
    B, D, H, W = map_dims("z_e", z_e, rowmajor)
    check_dev("idx", idx, torch.int64)
    K = int(K)
    idx = _indices(idx, B * H * W, "one index per row of z_e: B*H*W")
    row_uniforms = _lib.k_values("row_uniforms", row_uniforms, K)
    C = D + 1 if row_uniforms is None else 2 * D + 1
    dev = z_e.device
    if out is not None:
        check_dev("out", out, torch.float64)
        if out.shape != (K, C):
            raise ValueError(f"out must be a ({K}, {C}) tensor")
    z_e = dense(z_e, 4)
    with torch.cuda.device(dev):
        if workspace is None:
            workspace = vq_ema_stats_workspace(B * H * W, K, D, dev)
        if out is None:
            out = torch.empty((K, C), dtype=torch.float64, device=dev)
        with written(out, 8) as o:
            _lib.check(_lib.load().vqvae_vq_ema_stats_f32(
                z_e.data_ptr(), idx.data_ptr(), B, D, H, W, K, ptr(row_uniforms), VQ_ROWMAJOR if rowmajor else 0, o.data_ptr(),
                *ws_args(workspace), stream_ptr(z_e)))
    return out


def vq_ema_apply_workspace(R: int, K: int, D: int, device) -> torch.Tensor:
    return _lib.workspace("vqvae_vq_ema_apply_workspace_bytes", "EMA apply", "1 <= R <= 1024, K <= 16384, D <= 256",
                          dict(R=R, K=K, D=D), device)


def vq_ema_apply(stats, ema_cluster_size: torch.Tensor, ema_w: torch.Tensor, codebook: torch.Tensor, decay: float,
                 eps: float = 1e-5, *, threshold: float | None = None, shard_uniforms: torch.Tensor | None = None,
                 workspace: torch.Tensor | None = None):
    """One EMA codebook update from the statistics of R shards (vqvae_vq_ema_apply_f32): counts and sums are added in shard order
    in fp64, then vq_ema_update's arithmetic.  stats: (R, K, C) float64, or a list of R (K, C) tensors (stacked here).  Writes
    ema_cluster_size (K,), ema_w (K, D) and codebook (K, D) in place through their data pointers (no autograd version bump).
    threshold / shard_uniforms (K fp32 in [0, 1)): a code whose averaged count is below threshold takes the candidate of shard
    floor(v_k R) -- the records must carry candidates (C = 2 D + 1); both or neither."""
    if isinstance(stats, (list, tuple)):
        for s in stats:
            check_dev("stats", s, torch.float64)
        if not stats or any(s.dim() != 2 or s.shape != stats[0].shape for s in stats):
            raise ValueError("stats must be a (R, K, C) tensor or a non-empty list of (K, C) tensors of one shape")
        stats = torch.stack(list(stats))
    check_dev("stats", stats, torch.float64)
    if stats.dim() != 3:
        raise ValueError("stats must be (R, K, C)")
    R, K, C = stats.shape
    _, D = _ema_state(ema_cluster_size, ema_w, codebook, "stats", K=K)
    if C not in (D + 1, 2 * D + 1):
        raise ValueError("shape mismatch between stats, ema_cluster_size, ema_w and codebook")
    if (threshold is None) != (shard_uniforms is None):
        raise ValueError("restart needs both threshold and shard_uniforms")
    shard_uniforms = _lib.k_values("shard_uniforms", shard_uniforms, K)
    if shard_uniforms is not None and C != 2 * D + 1:
        raise ValueError("restart needs statistics taken with row_uniforms (C = 2 D + 1)")
    stats = dense(stats, 8)
    dev = stats.device
    with torch.cuda.device(dev), written(ema_cluster_size, 4) as cs, written(ema_w, 4) as ew, written(codebook, 4) as cb:
        if workspace is None:
            workspace = vq_ema_apply_workspace(R, K, D, dev)
        _lib.check(_lib.load().vqvae_vq_ema_apply_f32(
            stats.data_ptr(), R, K, D, C, float(decay), float(eps), float(threshold) if threshold is not None else -1.0,
            ptr(shard_uniforms), cs.data_ptr(), ew.data_ptr(), cb.data_ptr(), *ws_args(workspace), stream_ptr(stats)))
    return codebook


def vq_kmeans_workspace(N: int, K: int, D: int, device) -> torch.Tensor:
    """one workspace for vq_kmeans_seed and vq_kmeans_update at these sizes"""
    return _lib.workspace("vqvae_vq_kmeans_workspace_bytes", "k-means initialisation",
                          "1 <= K <= 16384, 1 <= D <= 256, 1 <= N < 2^31", dict(N=N, K=K, D=D), device)


def vq_kmeans_seed(z_e: torch.Tensor, K: int, uniforms: torch.Tensor, *, rowmajor: bool = False,
                   workspace: torch.Tensor | None = None):
    """k-means++ seeding (vqvae_vq_kmeans_seed_f32) of a K-code codebook on the rows of z_e, driven by K fp32 uniforms in [0, 1):
    -> (codebook (K, D) whose code k is row rows[k] of z_e bit for bit, rows (K,) int64).  z_e: (B,D,H,W), or (B,H,W,D) when
    rowmajor.  The numeric contract is the header of csrc/vq_kmeans.hip."""
    B, D, H, W = map_dims("z_e", z_e, rowmajor)
    check_dev("uniforms", uniforms)
    uniforms = _lib.k_values("uniforms", uniforms, K)
    z_e = dense(z_e, 4)
    dev = z_e.device
    with torch.cuda.device(dev):
        if workspace is None:
            workspace = vq_kmeans_workspace(B * H * W, K, D, dev)
        codebook = torch.empty((K, D), dtype=torch.float32, device=dev)
        rows = torch.empty((K,), dtype=torch.int64, device=dev)
        _lib.check(_lib.load().vqvae_vq_kmeans_seed_f32(
            z_e.data_ptr(), B, D, H, W, K, uniforms.data_ptr(), VQ_ROWMAJOR if rowmajor else 0, codebook.data_ptr(),
            rows.data_ptr(), *ws_args(workspace), stream_ptr(z_e)))
    return codebook, rows


def vq_kmeans_update(z_e: torch.Tensor, idx: torch.Tensor, codebook: torch.Tensor, *, uniforms: torch.Tensor | None = None,
                     rowmajor: bool = False, workspace: torch.Tensor | None = None) -> torch.Tensor:
    """One Lloyd mean update (vqvae_vq_kmeans_update_f32) from the rows z_e and the indices the quantizer assigned them: every code
    with rows becomes their mean, written into codebook (K, D) in place through its data pointer (no autograd version bump: the
    caller owns that); a code without rows keeps its bits, or with uniforms (K fp32 in [0, 1)) takes row floor(u_k N) of z_e.
    -> counts (K,) int32.  z_e: (B,D,H,W), or (B,H,W,D) when rowmajor."""
    B, D, H, W = map_dims("z_e", z_e, rowmajor)
    check_dev("idx", idx, torch.int64)
    K = _table("codebook", codebook, D)[0]
    idx = _indices(idx, B * H * W)
    uniforms = _lib.k_values("uniforms", uniforms, K)
    z_e = dense(z_e, 4)
    dev = z_e.device
    with torch.cuda.device(dev), written(codebook, 4) as cb:
        if workspace is None:
            workspace = vq_kmeans_workspace(B * H * W, K, D, dev)
        counts = torch.empty((K,), dtype=torch.int32, device=dev)
        _lib.check(_lib.load().vqvae_vq_kmeans_update_f32(
            z_e.data_ptr(), idx.data_ptr(), B, D, H, W, K, ptr(uniforms), VQ_ROWMAJOR if rowmajor else 0, cb.data_ptr(),
            counts.data_ptr(), *ws_args(workspace), stream_ptr(z_e)))
    return counts


def vq_kmeans(z_e: torch.Tensor, K: int, iters: int = 10, *, generator: torch.Generator | None = None, reseed_empty: bool = True,
              rowmajor: bool = False, trace: list | None = None):
    """k-means on the rows of z_e: k-means++ seeding, then `iters` rounds of assignment by the quantizer (vq_forward, indices only)
    and the mean update.  -> (codebook (K, D), counts (K,) int32 of the last assignment; of no assignment, all zero, when iters = 0).
    Uniforms come from torch.rand on the device (`generator`, or the default CUDA generator): K for the seeding and, with
    reseed_empty, K per round for codes that lost every row.  Nothing synchronises with the host.  trace: a list that receives,
    per round, (the codebook the round assigned against, its indices) -- for tests."""
    B, D, H, W = map_dims("z_e", z_e, rowmajor)
    if iters < 0:
        raise ValueError("iters must be >= 0")
    z_e = dense(z_e, _lib.vq_align(D))            # (the rows go to the quantizer every round)
    dev = z_e.device
    with torch.cuda.device(dev):
        ws = vq_kmeans_workspace(B * H * W, K, D, dev)
        codebook, _ = vq_kmeans_seed(z_e, K, torch.rand(K, device=dev, generator=generator), rowmajor=rowmajor, workspace=ws)
        counts = torch.zeros((K,), dtype=torch.int32, device=dev)
        vws = vq_workspace(K, D, dev) if iters else None
        for _ in range(iters):
            _, _, _, idx, _ = vq_forward(z_e, codebook, 0.0, rowmajor=rowmajor, workspace=vws, prepared=False, want_zq=False)
            if trace is not None:
                trace.append((codebook.clone(), idx))
            u = torch.rand(K, device=dev, generator=generator) if reseed_empty else None
            counts = vq_kmeans_update(z_e, idx, codebook, uniforms=u, rowmajor=rowmajor, workspace=ws)
    return codebook, counts


# ---- l2-normalised rows: the cosine-similarity codebook (csrc/vq_cosine.hip) -----------------------------------------------------

def l2norm_rows(x: torch.Tensor, *, rowmajor: bool = False, eps: float = 1e-12):
    """Every row divided by its l2 norm (vqvae_l2norm_forward_f32; torch.nn.functional.normalize along the channels):
    -> (y like x, denom (N,) fp32 = max(||row||, eps)).  x: (B,D,H,W), (B,H,W,D) when rowmajor, or a 2-D (K, D) tensor -- a codebook,
    rows as they stand.  The numeric contract is the header of csrc/vq_cosine.hip."""
    B, D, H, W, rm = map_dims("x", x, rowmajor, allow_2d=True)
    x = dense(x, 4)
    dev = x.device
    with torch.cuda.device(dev):
        y = torch.empty_like(x)
        denom = torch.empty((B * H * W,), dtype=torch.float32, device=dev)
        _lib.check(_lib.load().vqvae_l2norm_forward_f32(x.data_ptr(), B, D, H, W, float(eps), VQ_ROWMAJOR if rm else 0,
                                                        y.data_ptr(), denom.data_ptr(), stream_ptr(x)))
    return y, denom


def l2norm_rows_backward(y: torch.Tensor, denom: torch.Tensor, grad_y: torch.Tensor, *, rowmajor: bool = False,
                         eps: float = 1e-12) -> torch.Tensor:
    """grad_x of l2norm_rows from its outputs (y, denom) and grad_y (vqvae_l2norm_backward_f32): (g - y (y . g)) / denom per row, and
    g / eps on rows where the clamp was active.  eps must be the forward's."""
    B, D, H, W, rm = map_dims("y", y, rowmajor, allow_2d=True)
    check_dev("denom", denom)
    grad_y = _lib.same_shape("grad_y", grad_y, y)
    if denom.numel() != B * H * W:
        raise ValueError("denom must hold one value per row of y")
    y, denom = dense(y, 4), dense(denom, 4)
    with torch.cuda.device(y.device):
        grad_x = torch.empty_like(y)
        _lib.check(_lib.load().vqvae_l2norm_backward_f32(y.data_ptr(), denom.data_ptr(), grad_y.data_ptr(), B, D, H, W, float(eps),
                                                         VQ_ROWMAJOR if rm else 0, grad_x.data_ptr(), stream_ptr(y)))
    return grad_x


# ---- residual vector quantization (csrc/vq_residual.hip) -------------------------------------------------------------------------
VQ_RESIDUAL_SHARED = 0x10000


def _residual_books(codebooks, shared, align=4):
    """-> (contiguous (K, D) codebooks, one per distinct codebook; stage count, None when only the caller knows it)"""
    books = _lib.books(codebooks, 1, None, align)
    n = len(books)                                # shared: one codebook and n_q, or the same codebook listed once per stage
    return (books[:1] if shared else books), (None if shared and n == 1 else n)


def vq_residual_workspace(N: int, K: int, D: int, Q: int, device, *, shared: bool = False) -> torch.Tensor:
    """workspace of vq_residual_forward: one prepared codebook image per distinct codebook and one residual map"""
    return _lib.workspace("vqvae_vq_residual_workspace_bytes", "residual quantizer", "1 <= Q <= 16, K <= 16384, D <= 256, N < 2^31",
                          dict(N=N, K=K, D=D, Q=Q, shared=1 if shared else 0), device)


def vq_residual_forward(z_e: torch.Tensor, codebooks, beta: float, *, rowmajor: bool = False, shared: bool = False,
                        n_q: int | None = None, want_zq: bool = True, want_residual: bool = False,
                        workspace: torch.Tensor | None = None, prepared: bool = False):
    """Residual quantization (vqvae_vq_residual_forward_f32): stage q quantizes, with the reference quantizer, what stage q - 1
    left over.  codebooks: a sequence of Q (K, D) tensors; with shared=True every stage uses the first (pass it Q times, or once
    with n_q=Q).
    z_e: (B,D,H,W), or (B,H,W,D) when rowmajor.
    -> (loss 0-dim, z_q like z_e or None, perplexity (Q,), idx (Q, N) int64, hist (Q, K) int32, loss_stage (Q,)), and with
    want_residual a seventh value, r_Q like z_e.  prepared: `workspace` holds every stage's codebook image from a previous call
    with the same codebooks.  The numeric contract is the header of csrc/vq_residual.hip."""
    B, D, H, W = map_dims("z_e", z_e, rowmajor)
    books, Q = _residual_books(codebooks, shared, _lib.vq_align(D))     # (the stages' quantizer)
    if Q is None:
        Q = 1 if n_q is None else int(n_q)
    elif n_q is not None and n_q != Q:
        raise ValueError("n_q differs from the number of codebooks")
    K, Dc = books[0].shape
    if Dc != D:
        raise ValueError(f"channel dim {D} != embedding dim {Dc}")
    z_e = dense(z_e, _lib.vq_align(D))
    dev = z_e.device
    N = B * H * W
    with torch.cuda.device(dev):
        if workspace is None:
            workspace = vq_residual_workspace(N, K, D, Q, dev, shared=shared)
            prepared = False
        z_q = torch.empty_like(z_e) if want_zq else None
        res = torch.empty_like(z_e) if want_residual else None
        idx = torch.empty((Q, N), dtype=torch.int64, device=dev)
        hist = torch.empty((Q, K), dtype=torch.int32, device=dev)
        scal = torch.empty((2 * Q + 1,), dtype=torch.float32, device=dev)
        flags = (VQ_ROWMAJOR if rowmajor else 0) | (VQ_CODEBOOK_PREPARED if prepared else 0) | (VQ_RESIDUAL_SHARED if shared else 0)
        _lib.check(_lib.load().vqvae_vq_residual_forward_f32(
            z_e.data_ptr(), ptr_array(books), B, D, H, W, K, Q, float(beta), flags, ptr(z_q), idx.data_ptr(), hist.data_ptr(),
            scal.data_ptr(), scal.data_ptr() + 4 * Q, scal.data_ptr() + 8 * Q, ptr(res), *ws_args(workspace), stream_ptr(z_e)))
    out = (scal[2 * Q], z_q, scal[Q:2 * Q], idx, hist, scal[:Q])
    return out + (res,) if want_residual else out


def vq_residual_decode(idx: torch.Tensor, codebooks, B: int, H: int, W: int, *, rowmajor: bool = False, shared: bool = False,
                       validate: bool = True) -> torch.Tensor:
    """(Q, N) indices -> the sum of their code rows in stage order, (B,D,H,W) or (B,H,W,D) when rowmajor
    (vqvae_vq_residual_decode_f32).  Indices outside [0, K) raise IndexError (one host sync; skipped with validate=False or while a
    graph is captured: the kernel then writes NaN rows and never reads outside a codebook)."""
    check_dev("idx", idx, torch.int64)
    books, nb = _residual_books(codebooks, shared)
    K, D = books[0].shape
    N = B * H * W
    if idx.numel() % N or idx.numel() == 0:
        raise ValueError("idx must hold Q*B*H*W indices")
    Q = idx.numel() // N
    if nb is not None and Q != nb:
        raise ValueError(f"{Q} stages of indices for {nb} codebooks")
    idx = dense(idx, 8)
    if validate:
        _lib.check_index_range(idx, K, "vq_residual_decode")
    out = _lib.like_map(idx, D, rowmajor, (B, H, W))
    with torch.cuda.device(idx.device):
        _lib.check(_lib.load().vqvae_vq_residual_decode_f32(
            idx.data_ptr(), ptr_array(books), B, D, H, W, K, Q, (VQ_ROWMAJOR if rowmajor else 0) | (VQ_RESIDUAL_SHARED if shared else 0),
            out.data_ptr(), stream_ptr(idx)))
    return out


# ---- grouped (product) vector quantization (csrc/vq_grouped.hip) -----------------------------------------------------------------

def vq_grouped_workspace(N: int, K: int, D: int, G: int, device) -> torch.Tensor:
    """workspace of vq_grouped_forward: one prepared codebook image per group and the G slabs"""
    return _lib.workspace("vqvae_vq_grouped_workspace_bytes", "grouped quantizer",
                          "1 <= G <= 16, D % G == 0, K <= 16384, D <= 256, N < 2^31", dict(N=N, K=K, D=D, G=G), device)


def vq_grouped_forward(z_e: torch.Tensor, codebooks, beta: float, *, rowmajor: bool = False, want_zq: bool = True,
                       want_slabs: bool = False, workspace: torch.Tensor | None = None, prepared: bool = False):
    """Grouped (product) quantization (vqvae_vq_grouped_forward_f32): the D channels of a row are cut into G = len(codebooks) groups of
    d = D / G channels, group g is quantized by the reference quantizer against codebooks[g], a (K, d) tensor.
    z_e: (B,D,H,W), or (B,H,W,D) when rowmajor.
    -> (loss 0-dim: the mean of the group losses, z_q like z_e or None, perplexity (G,), idx (G, N) int64, hist (G, K) int32,
    loss_group (G,)), and with want_slabs a seventh value: the G slabs, (G,B,d,H,W) or (G,B,H,W,d) when rowmajor -- slab g holds the
    group's channels of every row, dense.  prepared: `workspace` holds every group's codebook image from a previous call with the
    same codebooks.  The numeric contract is the header of csrc/vq_grouped.hip."""
    B, D, H, W = map_dims("z_e", z_e, rowmajor)
    books = _lib.books(codebooks, 1, 16, 4)
    G = len(books)
    K, d = books[0].shape
    if d * G != D:
        raise ValueError(f"channel dim {D} != {G} groups of embedding dim {d}")
    books = [dense(c, _lib.vq_align(d)) for c in books]                 # (the groups' quantizer reads the codebooks)
    z_e = dense(z_e, 4)
    dev = z_e.device
    N = B * H * W
    with torch.cuda.device(dev):
        if workspace is None:
            workspace = vq_grouped_workspace(N, K, D, G, dev)
            prepared = False
        z_q = torch.empty_like(z_e) if want_zq else None
        slabs = _lib.like_map(z_e, d, rowmajor, (G * B, H, W)).unflatten(0, (G, B)) if want_slabs else None
        idx = torch.empty((G, N), dtype=torch.int64, device=dev)
        hist = torch.empty((G, K), dtype=torch.int32, device=dev)
        scal = torch.empty((2 * G + 1,), dtype=torch.float32, device=dev)
        flags = (VQ_ROWMAJOR if rowmajor else 0) | (VQ_CODEBOOK_PREPARED if prepared else 0)
        _lib.check(_lib.load().vqvae_vq_grouped_forward_f32(
            z_e.data_ptr(), ptr_array(books), B, D, H, W, K, G, float(beta), flags, ptr(z_q), idx.data_ptr(), hist.data_ptr(),
            scal.data_ptr(), scal.data_ptr() + 4 * G, scal.data_ptr() + 8 * G, ptr(slabs), *ws_args(workspace), stream_ptr(z_e)))
    out = (scal[2 * G], z_q, scal[G:2 * G], idx, hist, scal[:G])
    return out + (slabs,) if want_slabs else out


def vq_grouped_decode(idx: torch.Tensor, codebooks, B: int, H: int, W: int, *, rowmajor: bool = False,
                      validate: bool = True) -> torch.Tensor:
    """(G, N) indices -> their code rows side by side, (B,D,H,W) or (B,H,W,D) when rowmajor (vqvae_vq_grouped_decode_f32).  Indices
    outside [0, K) raise IndexError (one host sync; skipped with validate=False or while a graph is captured: the kernel then writes
    NaN into that group's channels of the row and never reads outside a codebook)."""
    check_dev("idx", idx, torch.int64)
    books = _lib.books(codebooks, 1, 16, 4)
    G = len(books)
    K, d = books[0].shape
    idx = _indices(idx, G * B * H * W, "G*B*H*W (group-major)")
    if validate:
        _lib.check_index_range(idx, K, "vq_grouped_decode")
    out = _lib.like_map(idx, G * d, rowmajor, (B, H, W))
    with torch.cuda.device(idx.device):
        _lib.check(_lib.load().vqvae_vq_grouped_decode_f32(
            idx.data_ptr(), ptr_array(books), B, G * d, H, W, K, G, VQ_ROWMAJOR if rowmajor else 0, out.data_ptr(), stream_ptr(idx)))
    return out


# ---- finite scalar quantization (csrc/vq_fsq.hip) --------------------------------------------------------------------------------

def _fsq_levels(levels):
    """-> (levels tuple, the HOST int array the entries read during the call, K); ValueError outside the kernels' envelope"""
    lv = tuple(int(l) for l in levels)
    K = 1
    for l in lv:
        K *= l
    if not 1 <= len(lv) <= 8 or any(not 2 <= l <= 256 for l in lv) or K > 65536:
        raise ValueError(f"FSQ levels {lv}: 1 to 8 levels, each in [2, 256], with a product of at most 65536")
    return lv, (ctypes.c_int * len(lv))(*lv), K


def _fsq_params(D, d, **params):
    """contiguous fp32 device tensors of nn.Linear's shapes for the names given: w_in (d, D), b_in (d), w_out (D, d), b_out (D)"""
    shapes = {"w_in": (d, D), "b_in": (d,), "w_out": (D, d), "b_out": (D,)}
    out = []
    for name, t in params.items():
        check_dev(name, t)
        if tuple(t.shape) != shapes[name]:
            raise ValueError(f"{name} must be {shapes[name]}, got {tuple(t.shape)}")
        out.append(dense(t, 4))
    return out


def _proj_decode_args(idx, w_out, b_out, d, n):
    """the checked arguments a projected-code decoder (FSQ, LFQ) shares: -> (idx, w_out, b_out, D)"""
    D = _table("w_out", w_out)[0]
    w_out, b_out = _fsq_params(D, d, w_out=w_out, b_out=b_out)
    return _indices(idx, n), w_out, b_out, D


def fsq_forward(z_e: torch.Tensor, w_in: torch.Tensor, b_in: torch.Tensor, w_out: torch.Tensor, b_out: torch.Tensor, levels, *,
                rowmajor: bool = False, want_zq: bool = True, want_hist: bool = True):
    """Finite scalar quantization (vqvae_fsq_forward_f32; arXiv 2309.15505): rows of z_e -> project_in -> tanh bound -> round to
    levels[j] values per channel -> project_out, all inside one kernel.  z_e: (B,D,H,W), or (B,H,W,D) when rowmajor; w_in (d, D),
    b_in (d), w_out (D, d), b_out (D) as nn.Linear holds them.
    -> (z_q like z_e or None, perplexity 0-dim or None, idx (N,1) int64 in [0, prod levels), hist (K,) int32 or None).
    The numeric contract is the header of csrc/vq_fsq.hip."""
    B, D, H, W = map_dims("z_e", z_e, rowmajor)
    lv, c_lv, K = _fsq_levels(levels)
    w_in, b_in, w_out, b_out = _fsq_params(D, len(lv), w_in=w_in, b_in=b_in, w_out=w_out, b_out=b_out)
    z_e = dense(z_e, 4)
    dev = z_e.device
    with torch.cuda.device(dev):
        z_q = torch.empty_like(z_e) if want_zq else None
        idx = torch.empty((B * H * W, 1), dtype=torch.int64, device=dev)
        hist = torch.empty((K,), dtype=torch.int32, device=dev) if want_hist else None
        ppl = torch.empty((), dtype=torch.float32, device=dev) if want_hist else None
        _lib.check(_lib.load().vqvae_fsq_forward_f32(
            z_e.data_ptr(), w_in.data_ptr(), b_in.data_ptr(), w_out.data_ptr(), b_out.data_ptr(), c_lv, len(lv), B, D, H, W,
            VQ_ROWMAJOR if rowmajor else 0, ptr(z_q), idx.data_ptr(), ptr(hist), ptr(ppl), stream_ptr(z_e)))
    return z_q, ppl, idx, hist


def fsq_decode_indices(idx: torch.Tensor, w_out: torch.Tensor, b_out: torch.Tensor, levels, B: int, H: int, W: int, *,
                       rowmajor: bool = False, validate: bool = True) -> torch.Tensor:
    """indices -> z_q (B,D,H,W), or (B,H,W,D) when rowmajor (vqvae_fsq_decode_indices_f32): the forward's z_q of the same indices,
    bit for bit.  Indices outside [0, prod levels) raise IndexError (one host sync; skipped with validate=False or while a graph is
    captured: the kernel then writes NaN rows and reads nothing out of range)."""
    check_dev("idx", idx, torch.int64)
    lv, c_lv, K = _fsq_levels(levels)
    idx, w_out, b_out, D = _proj_decode_args(idx, w_out, b_out, len(lv), B * H * W)
    if validate:
        _lib.check_index_range(idx, K, "fsq_decode_indices")
    out = _lib.like_map(idx, D, rowmajor, (B, H, W))
    with torch.cuda.device(idx.device):
        _lib.check(_lib.load().vqvae_fsq_decode_indices_f32(idx.data_ptr(), w_out.data_ptr(), b_out.data_ptr(), c_lv, len(lv), B, D, H, W,
                                                            VQ_ROWMAJOR if rowmajor else 0, out.data_ptr(), stream_ptr(idx)))
    return out


def fsq_backward_workspace(N: int, D: int, n_levels: int, device) -> torch.Tensor:
    """workspace of training.fsq_backward's parameter gradients: one fp64 record per block of 256 rows"""
    return _lib.workspace("vqvae_fsq_backward_workspace_bytes", "FSQ backward", "1 <= D <= 256, 1 to 8 levels, 1 <= N < 2^31",
                          dict(N=N, D=D, levels=n_levels), device)


# ---- lookup-free quantization (csrc/vq_lfq.hip) ----------------------------------------------------------------------------------

def _lfq_bits(n_e):
    """-> d = log2 n_e; ValueError unless n_e is a power of two in [2, 65536]"""
    n_e = int(n_e)
    if n_e < 2 or n_e > 65536 or n_e & (n_e - 1):
        raise ValueError(f"lookup-free quantization needs a power of two in [2, 65536] codes, got {n_e}")
    return n_e.bit_length() - 1


def lfq_workspace(N: int, D: int, d: int, device) -> torch.Tensor:
    """workspace of lfq_forward's losses and of training.lfq_backward (vqvae_lfq_workspace_bytes: one size for both)"""
    return _lib.workspace("vqvae_lfq_workspace_bytes", "LFQ", "1 <= D <= 256, 1 <= d <= 16, 1 <= N < 2^31", dict(N=N, D=D, d=d), device)


def lfq_forward(z_e: torch.Tensor, w_in: torch.Tensor, b_in: torch.Tensor, w_out: torch.Tensor, b_out: torch.Tensor, n_e: int, *,
                beta: float = 0.25, entropy_weight: float = 0.1, diversity_gamma: float = 1.0, inv_temperature: float = 100.0,
                rowmajor: bool = False, want_zq: bool = True, want_hist: bool = True, want_loss: bool = True, workspace=None):
    """Lookup-free quantization (vqvae_lfq_forward_f32; MAGVIT-v2, arXiv 2310.05737): rows of z_e -> project_in -> sign -> project_out
    inside one kernel, and the commitment and entropy losses from the factorised softmax (no (N, K) array).  z_e: (B,D,H,W), or
    (B,H,W,D) when rowmajor; w_in (d, D), b_in (d), w_out (D, d), b_out (D) as nn.Linear holds them, d = log2 n_e.
    -> (z_q like z_e or None, perplexity 0-dim or None, idx (N,1) int64 in [0, n_e) with the FIRST channel least significant,
        hist (K,) int32 or None, losses (4,) fp32 = (loss, commitment, per-sample entropy, codebook entropy) or None,
        avg (K,) fp64 or None).  The numeric contract is the header of csrc/vq_lfq.hip."""
    B, D, H, W = map_dims("z_e", z_e, rowmajor)
    d = _lfq_bits(n_e)
    w_in, b_in, w_out, b_out = _fsq_params(D, d, w_in=w_in, b_in=b_in, w_out=w_out, b_out=b_out)
    z_e = dense(z_e, 4)
    dev = z_e.device
    with torch.cuda.device(dev):
        z_q = torch.empty_like(z_e) if want_zq else None
        idx = torch.empty((B * H * W, 1), dtype=torch.int64, device=dev)
        hist = torch.empty((n_e,), dtype=torch.int32, device=dev) if want_hist else None
        ppl = torch.empty((), dtype=torch.float32, device=dev) if want_hist else None
        losses = avg = ws = None
        if want_loss:
            losses = torch.empty((4,), dtype=torch.float32, device=dev)
            avg = torch.empty((n_e,), dtype=torch.float64, device=dev)
            ws = workspace if workspace is not None else lfq_workspace(B * H * W, D, d, dev)
        _lib.check(_lib.load().vqvae_lfq_forward_f32(
            z_e.data_ptr(), w_in.data_ptr(), b_in.data_ptr(), w_out.data_ptr(), b_out.data_ptr(), d, B, D, H, W,
            VQ_ROWMAJOR if rowmajor else 0, beta, entropy_weight, diversity_gamma, inv_temperature,
            ptr(z_q), idx.data_ptr(), ptr(hist), ptr(ppl), ptr(losses), ptr(avg), *ws_args(ws), stream_ptr(z_e)))
    return z_q, ppl, idx, hist, losses, avg


def lfq_decode_indices(idx: torch.Tensor, w_out: torch.Tensor, b_out: torch.Tensor, n_e: int, B: int, H: int, W: int, *,
                       rowmajor: bool = False, validate: bool = True) -> torch.Tensor:
    """indices -> z_q (B,D,H,W), or (B,H,W,D) when rowmajor (vqvae_lfq_decode_indices_f32): the forward's z_q of the same indices,
    bit for bit.  Indices outside [0, n_e) raise IndexError (one host sync; skipped with validate=False or while a graph is
    captured: the kernel then writes NaN rows)."""
    check_dev("idx", idx, torch.int64)
    d = _lfq_bits(n_e)
    idx, w_out, b_out, D = _proj_decode_args(idx, w_out, b_out, d, B * H * W)
    if validate:
        _lib.check_index_range(idx, n_e, "lfq_decode_indices")
    out = _lib.like_map(idx, D, rowmajor, (B, H, W))
    with torch.cuda.device(idx.device):
        _lib.check(_lib.load().vqvae_lfq_decode_indices_f32(idx.data_ptr(), w_out.data_ptr(), b_out.data_ptr(), d, B, D, H, W,
                                                            VQ_ROWMAJOR if rowmajor else 0, out.data_ptr(), stream_ptr(idx)))
    return out


# ---- the per-row linear map: a factorized codebook's projections (csrc/vq_linear.hip) --------------------------------------------

def linear_rows(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, *, rowmajor: bool = False) -> torch.Tensor:
    """y = W x + b on every row (vqvae_linear_rows_forward_f32): an fp64 sum from b in ascending channel order, rounded once.
    x: (B,Cin,H,W), (B,H,W,Cin) when rowmajor, or a 2-D (K, Cin) tensor -- rows as they stand; w (Cout, Cin), b (Cout) as nn.Linear
    holds them.  -> y in x's layout with Cout channels.  The numeric contract is the header of csrc/vq_linear.hip."""
    B, Cin, H, W, rm = map_dims("x", x, rowmajor, allow_2d=True)
    Cout = _table("w", w, Cin)[0]                       # (Cout, Cin), as nn.Linear holds it
    check_dev("b", b)
    if tuple(b.shape) != (Cout,):
        raise ValueError(f"b must be ({Cout},), got {tuple(b.shape)}")
    x, w, b = dense(x, 4), dense(w, 4), dense(b, 4)
    with torch.cuda.device(x.device):
        y = _lib.like_map(x, Cout, rm)
        _lib.check(_lib.load().vqvae_linear_rows_forward_f32(x.data_ptr(), w.data_ptr(), b.data_ptr(), B, Cin, H, W, Cout,
                                                             VQ_ROWMAJOR if rm else 0, y.data_ptr(), stream_ptr(x)))
    return y


def linear_rows_backward_workspace(N: int, Cin: int, Cout: int, device) -> torch.Tensor:
    """workspace of linear_rows_backward's parameter gradients: one fp64 record per block of 256 rows"""
    return _lib.workspace("vqvae_linear_rows_backward_workspace_bytes", "linear_rows backward", "1 <= Cin, Cout <= 256, 1 <= N < 2^31",
                          dict(N=N, Cin=Cin, Cout=Cout), device)


def linear_rows_backward(x: torch.Tensor, grad_y: torch.Tensor, w: torch.Tensor, *, rowmajor: bool = False,
                         want=(True, True, True), workspace: torch.Tensor | None = None):
    """Gradients of linear_rows (vqvae_linear_rows_backward_f32) from its input x and the upstream grad_y (y's shape):
    -> (grad_x, grad_w, grad_b), None where `want` says so (not all three).  grad_w and grad_b are fp64 sums over the rows in an
    order that depends on the number of rows alone: the same bits in both layouts and in every run."""
    B, Cin, H, W, rm = map_dims("x", x, rowmajor, allow_2d=True)
    Cout = _table("w", w, Cin)[0]
    grad_y = _lib.same_shape("grad_y", grad_y, _lib.like_map(x, Cout, rm, device="meta"))       # (y's shape)
    x, w = dense(x, 4), dense(w, 4)
    want_x, want_w, want_b = (bool(v) for v in want)
    if not (want_x or want_w or want_b):
        raise ValueError("at least one gradient must be wanted")
    dev = x.device
    with torch.cuda.device(dev):
        gx = torch.empty_like(x) if want_x else None
        gw = torch.empty_like(w) if want_w else None
        gb = torch.empty((Cout,), dtype=torch.float32, device=dev) if want_b else None
        ws = None
        if want_w or want_b:
            ws = workspace if workspace is not None else linear_rows_backward_workspace(B * H * W, Cin, Cout, dev)
        _lib.check(_lib.load().vqvae_linear_rows_backward_f32(
            x.data_ptr(), grad_y.data_ptr(), w.data_ptr(), B, Cin, H, W, Cout, VQ_ROWMAJOR if rm else 0, ptr(gx), ptr(gw), ptr(gb),
            *ws_args(ws), stream_ptr(x)))
    return gx, gw, gb


# ---- orthogonal regularization of a codebook (csrc/vq_orthogonal.hip) ------------------------------------------------------------

def vq_orthogonal_workspace(K: int, D: int, device) -> torch.Tensor:
    """workspace of vq_orthogonal_forward: the K fp64 row sums"""
    return _lib.workspace("vqvae_vq_orthogonal_workspace_bytes", "vq_orthogonal", "1 <= K <= 16384, 1 <= D <= 256", dict(K=K, D=D), device)


def vq_orthogonal_forward(rows: torch.Tensor, hist: torch.Tensor | None = None, *, max_codes: int | None = None,
                          uniforms: torch.Tensor | None = None, want_saved: bool = False, workspace: torch.Tensor | None = None):
    """The orthogonal regularization loss of the rows of a (K, D) table as they stand (vqvae_vq_orthogonal_forward_f32; the caller
    normalises): |E E^T|_F^2 / M^2 - 1 / M over the M selected codes.  hist (K,) int32: only codes with hist > 0 are candidates
    (None: every code).  max_codes with uniforms (K,) fp32 in [0, 1): of more candidates, the max_codes that come first by (u, k)
    are kept.  -> (loss 0-dim, count 0-dim int32 = M, selected (K,) int32 0 / 1, saved (K, D) fp64 for vq_orthogonal_backward, or
    None without want_saved).  No host sync.  The numeric contract is the header of csrc/vq_orthogonal.hip."""
    K, D = _table("rows", rows)
    if hist is not None:
        check_dev("hist", hist, torch.int32)
        if hist.shape != (K,):
            raise ValueError("hist must be (K,)")
        hist = dense(hist, 4)
    if max_codes is not None and uniforms is None:
        raise ValueError("max_codes needs uniforms: one value in [0, 1) per code")
    if uniforms is not None:
        check_dev("uniforms", uniforms)
        if uniforms.shape != (K,):
            raise ValueError("uniforms must be (K,)")
        uniforms = dense(uniforms, 4)
    rows = dense(rows, 4)
    dev = rows.device
    with torch.cuda.device(dev):
        ws = workspace if workspace is not None else vq_orthogonal_workspace(K, D, dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        count = torch.empty((), dtype=torch.int32, device=dev)
        selected = torch.empty((K,), dtype=torch.int32, device=dev)
        saved = torch.empty((K, D), dtype=torch.float64, device=dev) if want_saved else None
        _lib.check(_lib.load().vqvae_vq_orthogonal_forward_f32(
            rows.data_ptr(), ptr(hist), ptr(uniforms), int(max_codes) if max_codes is not None else 0, K, D, 0, loss.data_ptr(),
            count.data_ptr(), selected.data_ptr(), ptr(saved), *ws_args(ws), stream_ptr(rows)))
    return loss, count, selected, saved


def vq_orthogonal_backward(saved: torch.Tensor, selected: torch.Tensor, count: torch.Tensor,
                           grad_loss: torch.Tensor | None = None) -> torch.Tensor:
    """grad_rows (K, D) fp32 of vq_orthogonal_forward's loss from its outputs (vqvae_vq_orthogonal_backward_f32): grad_loss (a device
    scalar; None: 1) times 4 / M^2 times saved in the selected rows, +0.0 elsewhere."""
    check_dev("saved", saved, torch.float64)
    check_dev("selected", selected, torch.int32)
    check_dev("count", count, torch.int32)
    if saved.dim() != 2:
        raise ValueError("saved must be a 2-D (K, D) tensor")
    K, D = saved.shape
    if selected.shape != (K,) or count.numel() != 1:
        raise ValueError("saved must be (K, D), selected (K,), count a scalar")
    grad_loss = _lib.device_scalar("grad_loss", grad_loss)
    saved, selected = dense(saved, 8), dense(selected, 4)
    with torch.cuda.device(saved.device):
        grad_rows = torch.empty((K, D), dtype=torch.float32, device=saved.device)
        _lib.check(_lib.load().vqvae_vq_orthogonal_backward_f32(
            saved.data_ptr(), selected.data_ptr(), count.data_ptr(), ptr(grad_loss), K, D, grad_rows.data_ptr(), stream_ptr(saved)))
    return grad_rows


# ---- the code-entropy loss of a learned codebook (csrc/vq_entropy.hip) --------------------------------------------------------------

def vq_entropy_workspace(N: int, K: int, D: int, device) -> torch.Tensor:
    """workspace of vq_entropy_forward and vq_entropy_backward (vqvae_vq_entropy_workspace_bytes: one size for both)"""
    return _lib.workspace("vqvae_vq_entropy_workspace_bytes", "vq_entropy", "1 <= K <= 16384, 1 <= D <= 256, 1 <= N < 2^31",
                          dict(N=N, K=K, D=D), device)


def vq_entropy_forward(z: torch.Tensor, codebook: torch.Tensor, *, inv_temperature: float, gamma: float, rowmajor: bool = False,
                       want_saved: bool = True, workspace: torch.Tensor | None = None):
    """The code-entropy loss of the rows of z against a (K, D) codebook (vqvae_vq_entropy_forward_f32): with p = softmax_k of
    -inv_temperature * |z_n - e_k|^2, P the mean row entropy and H the entropy of the batch's mean p, term = P - gamma * H.  z:
    (B, D, H, W), or (B, H, W, D) when rowmajor.  -> (losses (3,) fp32 = (term, P, H), avg (K,) fp64, rowstat (N, 2) fp64 = the rows'
    log-sum-exp and entropy for vq_entropy_backward, or None without want_saved).  No (N, K) array, no host sync.  The numeric
    contract is the header of csrc/vq_entropy.hip."""
    B, D, H, W = map_dims("z", z, rowmajor)
    K = _table("codebook", codebook, D)[0]
    z, codebook = dense(z, 4), dense(codebook, 4)
    dev, N = z.device, B * H * W
    with torch.cuda.device(dev):
        ws = workspace if workspace is not None else vq_entropy_workspace(N, K, D, dev)
        losses = torch.empty((3,), dtype=torch.float32, device=dev)
        avg = torch.empty((K,), dtype=torch.float64, device=dev)
        rowstat = torch.empty((N, 2), dtype=torch.float64, device=dev) if want_saved else None
        _lib.check(_lib.load().vqvae_vq_entropy_forward_f32(
            z.data_ptr(), codebook.data_ptr(), B, D, H, W, K, float(inv_temperature), float(gamma), VQ_ROWMAJOR if rowmajor else 0,
            losses.data_ptr(), avg.data_ptr(), ptr(rowstat), *ws_args(ws), stream_ptr(z)))
    return losses, avg, rowstat


def vq_entropy_backward(z: torch.Tensor, codebook: torch.Tensor, avg: torch.Tensor, rowstat: torch.Tensor,
                        grad_loss: torch.Tensor | None = None, *, inv_temperature: float, gamma: float, rowmajor: bool = False,
                        want=(True, True), workspace: torch.Tensor | None = None):
    """The gradients of vq_entropy_forward's term (vqvae_vq_entropy_backward_f32) from its avg and rowstat: grad_loss (a device
    scalar; None: 1) times d term / d z (like z) and d term / d codebook (K, D).  want = (grad_z, grad_codebook): at least one;
    -> (grad_z or None, grad_codebook or None)."""
    B, D, H, W = map_dims("z", z, rowmajor)
    K = _table("codebook", codebook, D)[0]
    check_dev("avg", avg, torch.float64)
    check_dev("rowstat", rowstat, torch.float64)
    N = B * H * W
    if avg.shape != (K,) or rowstat.shape != (N, 2):
        raise ValueError("avg must be (K,) and rowstat (N, 2): vq_entropy_forward's outputs")
    want_z, want_e = bool(want[0]), bool(want[1])
    if not (want_z or want_e):
        raise ValueError("want: at least one of (grad_z, grad_codebook)")
    grad_loss = _lib.device_scalar("grad_loss", grad_loss)
    z, codebook, avg, rowstat = dense(z, 4), dense(codebook, 4), dense(avg, 8), dense(rowstat, 8)
    dev = z.device
    with torch.cuda.device(dev):
        ws = workspace if workspace is not None else vq_entropy_workspace(N, K, D, dev)
        gz = torch.empty_like(z) if want_z else None
        ge = torch.empty_like(codebook) if want_e else None
        _lib.check(_lib.load().vqvae_vq_entropy_backward_f32(
            z.data_ptr(), codebook.data_ptr(), avg.data_ptr(), rowstat.data_ptr(), ptr(grad_loss), B, D, H, W, K,
            float(inv_temperature), float(gamma), VQ_ROWMAJOR if rowmajor else 0, ptr(gz), ptr(ge), *ws_args(ws), stream_ptr(z)))
    return gz, ge
