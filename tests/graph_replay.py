"""Inputs and helpers of the graph-replay tests (tests/test_graph_replay_cpu.py, tests/test_graph_replay_gpu.py).

A replay launches the kernels of the capture with the launch shapes of the capture, so every comparison is bit equality with an
eager call on fresh tensors.  What has to be chosen is the INPUTS: a replay that leaves a histogram, a flag word or a per-image
maximum of the replay before it in place shows only if the two replays' inputs make those words differ.  This module builds such
inputs on the host (numpy only, so the CPU tests can check their properties) and holds the small device-side helpers."""
from __future__ import annotations

import numpy as np

BETA = 0.25
B_VQ = 3

# ---- part 1: the stand-alone quantizer, one case per kernel route ------------------------------------------------------------------
# flags as vqvae_vq_kernel_name takes them: 0x1 = VQVAE_VQ_ROWMAJOR, 0x8 = VQVAE_VQ_BF16_FILTER.  `name` is what that function must
# answer for (K, D, flags); it answers for 8x8 maps, so the 7x7 NCHW case also states what the launch-form query must say at its HW.
VQ_CASES = {
    "track_k512":      dict(K=512,  D=64,  H=8, W=8, rowmajor=True,  bf16=False, name="vq_track_kernel_d64"),
    "track_k1000":     dict(K=1000, D=64,  H=8, W=8, rowmajor=True,  bf16=False, name="vq_track_kernel_d64"),     # 4000-byte histogram
    "track_nchw":      dict(K=512,  D=64,  H=8, W=8, rowmajor=False, bf16=False, name="vq_track_kernel_d64"),
    "chunk_k2048":     dict(K=2048, D=64,  H=8, W=8, rowmajor=True,  bf16=False, name="vq_stream_sweep_kernel"),
    "chunk_d128":      dict(K=512,  D=128, H=8, W=8, rowmajor=True,  bf16=False, name="vq_stream_sweep_kernel"),
    "filter_nchw_7x7": dict(K=100,  D=64,  H=7, W=7, rowmajor=False, bf16=False, name="vq_track_kernel_d64"),     # HW = 49: not the tracker's
    "exact_nchw_d128": dict(K=96,   D=128, H=8, W=8, rowmajor=False, bf16=False, name="vq_exact_kernel"),
    "anyd_d48":        dict(K=100,  D=48,  H=5, W=7, rowmajor=False, bf16=False, name="vq_anyd_kernel"),
    "generic_d3_k5":   dict(K=5,    D=3,   H=8, W=8, rowmajor=True,  bf16=True,  name="vq_generic_kernel"),
}


def vq_flags(case):
    c = VQ_CASES[case]
    return (0x1 if c["rowmajor"] else 0) | (0x8 if c["bf16"] else 0)


def vq_code_ranges(K):
    """-> ((lo, hi) of state b's codes, (lo, hi) of state c's): the first and the last quarter of the codebook; the first two and
    the last two codes at K = 5."""
    q = 2 if K == 5 else K // 4
    return (0, q), (K - q, K)


def vq_codebook(case):
    c = VQ_CASES[case]
    rng = np.random.default_rng(1000 + sorted(VQ_CASES).index(case))
    return rng.standard_normal((c["K"], c["D"])).astype(np.float32)


def _near_codes(rng, cb, lo, hi, n):
    """n rows, each a code of cb[lo:hi] plus noise of 2^-10 of that code's norm"""
    j = rng.integers(lo, hi, n)
    e = cb[j].astype(np.float64)
    noise = rng.standard_normal(e.shape)
    noise *= (2.0 ** -10) * np.linalg.norm(e, axis=1, keepdims=True) / np.linalg.norm(noise, axis=1, keepdims=True)
    return (e + noise).astype(np.float32)


def vq_states(case):
    """-> [a, b, c, a]: four (N, D) fp32 row sets to replay in this order.  a: randn; b: rows next to codes of the first quarter of
    the codebook; c: the same from the last quarter.  b and c fill disjoint parts of the histogram and leave the rest of it zero: a
    histogram, flag or ticket word that a replay does not clear shows in the replay after it."""
    c = VQ_CASES[case]
    n = B_VQ * c["H"] * c["W"]
    cb = vq_codebook(case)
    rng = np.random.default_rng(2000 + sorted(VQ_CASES).index(case))
    a = rng.standard_normal((n, c["D"])).astype(np.float32)
    (b0, b1), (c0, c1) = vq_code_ranges(c["K"])
    return [a, _near_codes(rng, cb, b0, b1, n), _near_codes(rng, cb, c0, c1, n), a]


def vq_layout(case, rows):
    """(N, D) rows -> the case's z layout: (B, H, W, D) row-major or (B, D, H, W)"""
    c = VQ_CASES[case]
    z = rows.reshape(B_VQ, c["H"], c["W"], c["D"])
    return np.ascontiguousarray(z if c["rowmajor"] else z.transpose(0, 3, 1, 2))


def argmin_fp64(rows, cb):
    """the reference's distance (models/quantizer.py:49-51: |z|^2 + |e|^2 - 2 z.e) in fp64, and its argmin"""
    z, e = rows.astype(np.float64), cb.astype(np.float64)
    d = (z * z).sum(1)[:, None] + (e * e).sum(1)[None, :] - 2.0 * (z @ e.T)
    return d.argmin(1)


# ---- part 2: whole-path entries ---------------------------------------------------------------------------------------------------
MODEL_CASES = {
    "fused":      dict(dims=(128, 32, 2, 512, 64),  B=5, HW=32),
    "fused_k1000": dict(dims=(128, 32, 2, 1000, 64), B=5, HW=32),         # the same kernels, a 4000-byte histogram clear
    "per_layer":  dict(dims=(64, 32, 1, 512, 64),   B=3, HW=32),
    "halo_tiles": dict(dims=(128, 32, 2, 512, 64),  B=2, HW=64),
    "generic":    dict(dims=(128, 32, 2, 96, 64),   B=3, HW=24),
}
SCALES = (1.0, 2.0 ** -9, 2.0 ** 6, 0.0)
N_REPLAYS = 5                                # four replays, then the first state again


def image_scale(i, r):
    """factor of image i in replay r (replay 4 repeats replay 0)"""
    return SCALES[(i + r % 4) % 4]


def model_images(case):
    """-> N_REPLAYS arrays (B, 3, HW, HW) fp32: one randn batch whose image i is multiplied by SCALES[(i + r) % 4] in replay r.  The
    maxima that the layers hand to each other are per image: every image's magnitude moves up and down between replays (and through
    an all-zero image), so a maximum left over from the replay before gives that image another scale."""
    c = MODEL_CASES[case]
    rng = np.random.default_rng(3000 + sorted(MODEL_CASES).index(case))
    base = rng.standard_normal((c["B"], 3, c["HW"], c["HW"])).astype(np.float32)
    out = []
    for r in range(N_REPLAYS):
        s = np.array([image_scale(i, r) for i in range(c["B"])], dtype=np.float32)
        out.append(base * s[:, None, None, None])
    return out


def model_indices(case):
    """-> N_REPLAYS index arrays (N, 1) int64 for decode_indices: even replays draw from the lower half of the codebook, odd ones
    from the upper half (disjoint code subsets); replay 4 repeats replay 0."""
    c = MODEL_CASES[case]
    K = c["dims"][3]
    n = c["B"] * (c["HW"] // 4) ** 2
    rng = np.random.default_rng(4000 + sorted(MODEL_CASES).index(case))
    out = []
    for r in range(N_REPLAYS - 1):
        lo, hi = (0, K // 2) if r % 2 == 0 else (K // 2, K)
        out.append(rng.integers(lo, hi, (n, 1)).astype(np.int64))
    return out + [out[0]]


# ---- part 3: the captured training step -------------------------------------------------------------------------------------------
SMALL = (32, 8, 1, 64, 16)
STEP_CASES = {
    "plain":          dict(dims=SMALL, kw={}, B=4, HW=32),
    "plain_clip":     dict(dims=SMALL, kw={}, B=4, HW=32, max_grad_norm=0.01),
    "rotation":       dict(dims=SMALL, kw=dict(rotation_trick=True), B=4, HW=32),
    "cosine":         dict(dims=SMALL, kw=dict(cosine_sim=True), B=4, HW=32),
    "ema":            dict(dims=SMALL, kw=dict(ema_decay=0.99), B=4, HW=32),
    "ema_rot_cos":    dict(dims=SMALL, kw=dict(ema_decay=0.99, rotation_trick=True, cosine_sim=True), B=4, HW=32),
    "rvq2":           dict(dims=SMALL, kw=dict(n_quantizers=2), B=4, HW=32),
    "fsq":            dict(dims=(32, 8, 1, 1000, 16), kw=dict(fsq_levels=(8, 5, 5, 5)), B=4, HW=32),
    "default_b8":     dict(dims=(128, 32, 2, 512, 64), kw={}, B=8, HW=32),       # 8x8-map weight gradients, the hidden-activation path
    "generic_16x16":  dict(dims=(64, 16, 1, 64, 32), kw={}, B=6, HW=16),         # the generic and per-tap kernels
}
X_TRAIN_VAR = 0.06
N_WARMUP = 2


def step_images(case, n):
    c = STEP_CASES[case]
    rng = np.random.default_rng(5000 + sorted(STEP_CASES).index(case))
    return [rng.standard_normal((c["B"], 3, c["HW"], c["HW"])).astype(np.float32) * 0.5 for _ in range(n)]


# ---- device-side helpers (torch is imported where they run) -----------------------------------------------------------------------
def poison(*tensors):
    """Overwrite with 0xFF bytes: NaN for floats, -1 for integers.  A replay whose kernels fail to write an output then shows."""
    import torch
    with torch.no_grad():
        for t in tensors:
            if t is None:
                continue
            t = t.detach()
            assert t.is_contiguous(), "poison() writes through a flat view: the tensor must be contiguous"
            t.reshape(-1).view(torch.uint8).fill_(0xFF)


def same_bits(a, b):
    import torch
    if a is None or b is None:
        return a is None and b is None
    a, b = a.detach(), b.detach()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def differing(a, b):
    """number of elements whose bits differ"""
    import torch
    a, b = a.detach().contiguous().reshape(-1), b.detach().contiguous().reshape(-1)
    it = {4: torch.int32, 8: torch.int64}[a.element_size()]
    return int((a.view(it) != b.view(it)).sum())


class Captured:
    """fn() captured as one linear chain on a private stream, after `warmup` eager calls on that stream (as GraphedForward does).
    The caller sets the grad mode; fn reads static tensors only and returns the static outputs."""

    def __init__(self, fn, device, warmup=2):
        import torch
        from vqvae_amd import _lib
        _lib.load()
        _lib.profile_enable(False)
        self.stream = torch.cuda.Stream(device=device)
        self.graph = torch.cuda.CUDAGraph()
        self.stream.wait_stream(torch.cuda.current_stream(device))
        with torch.cuda.stream(self.stream):
            for _ in range(warmup):
                fn()
        self.stream.synchronize()
        with torch.cuda.graph(self.graph, stream=self.stream):
            self.out = fn()

    def replay(self):
        self.graph.replay()
        return self.out


def make_step(model, opt, x_static):
    """the training step of main.py:74-80 on static tensors"""
    from vqvae_amd import training as T

    def step():
        opt.zero_grad(set_to_none=False)
        el, xh, pp = model(x_static)
        stats = T.step_losses(el, xh, pp, x_static, X_TRAIN_VAR)
        stats[1].backward()
        opt.step()
        return stats
    return step


def make_twins(case, device, seed=0):
    """-> (model_a, opt_a, model_b, opt_b): a model in training mode with the HIP Adam (amsgrad), and its deep copy.  The .grad
    tensors exist from the start (zeros): a captured step accumulates into static gradient tensors."""
    import copy

    import torch
    from vqvae_amd import conv
    from vqvae_amd.modules import VQVAE
    from vqvae_amd.optim import Adam
    conv.set_conv_backend("hip")
    c = STEP_CASES[case]
    torch.manual_seed(seed)
    a = VQVAE(*c["dims"], BETA, **c["kw"]).to(device).train()
    b = copy.deepcopy(a)
    opts = []
    for m in (a, b):
        for p in m.parameters():
            if p.requires_grad:
                p.grad = torch.zeros_like(p)
        opts.append(Adam(m.parameters(), lr=3e-4, amsgrad=True, max_grad_norm=c.get("max_grad_norm")))
    return a, opts[0], b, opts[1]


def state_tensors(model, opt):
    """-> [(name, tensor)]: every parameter and its gradient, every buffer, every optimizer state tensor (`step` included)"""
    out = []
    for k, p in model.named_parameters():
        out.append(("param " + k, p))
        if p.grad is not None:
            out.append(("grad " + k, p.grad))
        for sk, sv in sorted(opt.state.get(p, {}).items()):
            out.append((f"opt {sk} {k}", sv))
    for k, v in model.named_buffers():
        out.append(("buffer " + k, v))
    return out


def assert_same_state(model_a, opt_a, model_b, opt_b, where):
    sa, sb = state_tensors(model_a, opt_a), state_tensors(model_b, opt_b)
    assert [k for k, _ in sa] == [k for k, _ in sb], where
    for (k, ta), (_, tb) in zip(sa, sb):
        assert same_bits(ta, tb), f"{where}: {k} differs in {differing(ta, tb)} of {ta.numel()} elements"


def evaluate(model, x):
    """part 4's evaluation: the eval forward, encode, decode_indices(encode(x)); back to train().  -> list of cloned tensors"""
    import torch
    B, _, H, W = x.shape
    model.eval()
    try:
        with torch.no_grad():
            out = [t.clone() for t in model(x)]
            idx = model.encode(x)
            out += [idx.clone(), model.decode_indices(idx, B, H // 4, W // 4).clone()]
    finally:
        model.train()
    return out
