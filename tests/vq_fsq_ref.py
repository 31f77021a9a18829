"""CPU restatement of finite scalar quantization as vqvae_amd/csrc/vq_fsq.hip's header states it: numpy fp64, one IEEE operation per
written operation, the loops in the contract's order (vectorised over rows only).  Rows are (N, D) fp32; the layouts of the kernels are
views of them.  tanh / atanh are libm's (math.tanh per element): tests/host/fsq_harness.cpp runs the kernels' own text against the
same libm, so it can ask for these bits."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
EPS = 1e-3
BLOCK_ROWS = 256              # kFsqBlockRows: the blocks of the parameter gradients' fixed order

_tanh = np.vectorize(math.tanh, otypes=[F64])


class Consts:
    def __init__(self, levels):
        self.levels = [int(l) for l in levels]
        self.d = len(self.levels)
        self.half_l = np.array([(l - 1) * (1.0 + EPS) / 2.0 for l in self.levels], F64)
        self.offset = np.array([0.5 if l % 2 == 0 else 0.0 for l in self.levels], F64)
        self.shift = np.array([math.atanh(o / h) for o, h in zip(self.offset, self.half_l)], F64)
        self.hw = np.array([l // 2 for l in self.levels], np.int64)
        self.basis = np.array([int(np.prod(self.levels[:j], dtype=np.int64)) for j in range(self.d)], np.int64)
        self.K = int(np.prod(self.levels, dtype=np.int64))


def draw(N, D, levels, seed, scale=1.0):
    """seeded rows, upstream gradient and nn.Linear-shaped parameters (weights large enough that every level is in reach)"""
    rng = np.random.default_rng(seed)
    d = len(levels)
    z = (scale * rng.standard_normal((N, D))).astype(F32)
    g = rng.standard_normal((N, D)).astype(F32)
    w_in = (rng.standard_normal((d, D)) * (1.5 / math.sqrt(D))).astype(F32)
    b_in = (0.1 * rng.standard_normal(d)).astype(F32)
    w_out = (rng.standard_normal((D, d)) / math.sqrt(d)).astype(F32)
    b_out = (0.1 * rng.standard_normal(D)).astype(F32)
    return z, g, w_in, b_in, w_out, b_out


def project_in(z, w_in, b_in):
    """y (N, d) fp32: s = b_in, then the channels in ascending order"""
    N, D = z.shape
    s = np.broadcast_to(b_in.astype(F64), (N, w_in.shape[0])).copy()
    with np.errstate(over="ignore", invalid="ignore"):
        for c in range(D):
            s = s + w_in[:, c].astype(F64)[None, :] * z[:, c].astype(F64)[:, None]
        return s.astype(F32)


def bound_round(y, k):
    """y (N, d) fp32 -> (t, b, q) in fp64; FSQ.bound of vector-quantize-pytorch, then round-half-even"""
    with np.errstate(invalid="ignore"):
        t = _tanh(y.astype(F64) + k.shift[None, :])
        b = t * k.half_l[None, :] - k.offset[None, :]
        return t, b, np.rint(b)


def codes(y, k):
    """-> (c^ (N, d) fp32, idx (N,) int64, t, b): a non-finite y_j gives digit 0 and a NaN code"""
    t, b, q = bound_round(y, k)
    fin = np.isfinite(y)
    with np.errstate(invalid="ignore"):
        chat = np.where(fin, (q / k.hw.astype(F64)[None, :]).astype(F32), F32(np.nan)).astype(F32)
    digit = np.where(fin, np.nan_to_num(q, nan=0.0).astype(np.int64) + k.hw[None, :], 0)
    return chat, (digit * k.basis[None, :]).sum(1), t, b


def project_out(chat, w_out, b_out):
    N = chat.shape[0]
    s = np.broadcast_to(b_out.astype(F64), (N, w_out.shape[0])).copy()
    with np.errstate(invalid="ignore"):
        for j in range(chat.shape[1]):
            s = s + w_out[:, j].astype(F64)[None, :] * chat[:, j].astype(F64)[:, None]
    return s.astype(F32)


class Forward:
    pass


def forward(z, w_in, b_in, w_out, b_out, levels):
    k = Consts(levels)
    f = Forward()
    f.k = k
    f.y = project_in(z, w_in, b_in)
    f.chat, f.idx, f.t, f.b = codes(f.y, k)
    f.z_q = project_out(f.chat, w_out, b_out)
    f.hist = np.bincount(f.idx, minlength=k.K).astype(np.int32)
    f.perplexity = perplexity(f.hist, z.shape[0])
    return f


def clear_rows(f, margin=1e-9):
    """rows whose every b_j lies more than `margin` from a half-integer (and is finite): there a tanh a few ulps off cannot move q"""
    frac = np.abs(f.b - np.floor(f.b) - 0.5)
    return (np.isfinite(f.b) & (frac > margin)).all(1)


def perplexity(hist, N):
    """exp(-sum p log(p + 1e-10)) in the kernel's order: 256 strided sums, a fixed tree, one rounding"""
    p = hist.astype(F64) / F64(N)
    term = p * np.log(p + 1e-10)
    red = np.zeros(256, F64)
    for t in range(min(256, len(term))):
        s = F64(0.0)
        for v in term[t::256]:
            s = s + v
        red[t] = s
    o = 128
    while o > 0:
        red[:o] = red[:o] + red[o:2 * o]
        o >>= 1
    return F32(np.exp(-red[0]))


def decode(idx, w_out, b_out, levels):
    """indices -> z_q; an index outside [0, K) gives a NaN row"""
    k = Consts(levels)
    idx = np.asarray(idx, np.int64)
    ok = (idx >= 0) & (idx < k.K)
    u = np.where(ok, idx, 0)
    q = (u[:, None] // k.basis[None, :]) % np.array(k.levels, np.int64)[None, :] - k.hw[None, :]
    chat = np.where(ok[:, None], (q.astype(F64) / k.hw.astype(F64)[None, :]).astype(F32), F32(np.nan)).astype(F32)
    return project_out(chat, w_out, b_out)


def all_codes(levels):
    """the (K, d) implicit codebook, row idx = the codes of index idx"""
    k = Consts(levels)
    idx = np.arange(k.K, dtype=np.int64)
    q = (idx[:, None] // k.basis[None, :]) % np.array(k.levels, np.int64)[None, :] - k.hw[None, :]
    return (q.astype(F64) / k.hw.astype(F64)[None, :]).astype(F32)


class Backward:
    pass


def backward(z, g, w_in, b_in, w_out, levels):
    """the row-local backward (grad_z, gc, gy) and the per-row terms of the four parameter gradients, in fp64"""
    k = Consts(levels)
    N, D = z.shape
    y = project_in(z, w_in, b_in)
    chat, _, t, _ = codes(y, k)
    r = Backward()
    r.k, r.chat, r.t = k, chat, t
    gc = np.zeros((N, k.d), F64)
    for c in range(D):
        gc = gc + w_out[c, :].astype(F64)[None, :] * g[:, c].astype(F64)[:, None]
    r.gc = gc
    with np.errstate(invalid="ignore"):
        r.gy = gc / k.hw.astype(F64)[None, :] * k.half_l[None, :] * (1.0 - t * t)
        s = np.zeros((N, D), F64)
        for j in range(k.d):
            s = s + w_in[j, :].astype(F64)[None, :] * r.gy[:, j][:, None]
        r.grad_z = s.astype(F32)
        g64, z64 = g.astype(F64), z.astype(F64)
        # terms[n] of every output, fp64: (N, D, d), (N, D), (N, d, D), (N, d)
        r.terms = {"w_out": g64[:, :, None] * chat.astype(F64)[:, None, :], "b_out": g64,
                   "w_in": r.gy[:, :, None] * z64[:, None, :], "b_in": r.gy}
    return r


def param_grads(r):
    """plain fp64 sums over the rows, rounded once -> dict of fp32 arrays, and sum_n |term_n| for the tolerance"""
    with np.errstate(invalid="ignore"):
        return ({n: t.sum(0).astype(F32) for n, t in r.terms.items()}, {n: np.abs(t).sum(0) for n, t in r.terms.items()})


def param_grads_blocked(r):
    """the kernels' order: blocks of 256 rows, inside a block one row after the other from 0.0, then the blocks in order from 0.0"""
    out = {}
    with np.errstate(invalid="ignore"):
        for n, t in r.terms.items():
            total = np.zeros(t.shape[1:], F64)
            for r0 in range(0, t.shape[0], BLOCK_ROWS):
                s = np.zeros(t.shape[1:], F64)
                for row in t[r0:r0 + BLOCK_ROWS]:
                    s = s + row
                total = total + s
            out[n] = total.astype(F32)
    return out


def grad_z_bound(r, w_in):
    """|got - ref| <= 2^-23 |ref| + 2^-48 sum_j |W_in[j][c] gc_j half_l_j / hw_j|.

    gz_c = sum_j W_in[j][c] gy_j with gy_j = gc_j half_l_j / hw_j (1 - t_j^2).  The device's tanh may be off by a few fp64 ulps:
    t (1 + e), |e| <= 4 * 2^-53.  Then 1 - t^2 moves by 2 t^2 e <= 2^-50 in absolute terms (|t| <= 1), so term j moves by at most
    2^-50 |W_in gc half_l / hw|; the fp64 products and the d - 1 additions add a few 2^-53 of the same magnitudes.  2^-48 covers
    both with room; the final rounding to fp32 is the 2^-23 |ref| (half an ulp is 2^-24 |ref|; a value that the fp64 error carries
    across a rounding boundary is off by one ulp)."""
    k = r.k
    mag = np.zeros(r.grad_z.shape, F64)
    for j in range(k.d):
        mag = mag + np.abs(w_in[j, :].astype(F64)[None, :] * (r.gc[:, j] * k.half_l[j] / F64(k.hw[j]))[:, None])
    return 2.0 ** -23 * np.abs(r.grad_z.astype(F64)) + 2.0 ** -48 * mag + 2.0 ** -149


def to_nchw(rows, B, H, W):
    """(N, D) rows -> (B, D, H, W) maps"""
    return np.ascontiguousarray(rows.reshape(B, H, W, -1).transpose(0, 3, 1, 2))


def from_nchw(maps):
    B, D, H, W = maps.shape
    return np.ascontiguousarray(maps.transpose(0, 2, 3, 1)).reshape(B * H * W, D)


# (B, D, H, W, levels) of the GPU tests: the flagship row; odd D, 105 rows, the element path; one row; the widest rows (four chunks);
# 1088 rows: several blocks of the parameter gradients and a ragged last one -- every level list at least once
GPU_CASES = [(4, 64, 8, 8, (8, 5, 5, 5)), (3, 7, 5, 7, (3,)), (3, 7, 5, 7, (8, 5, 5, 5)), (1, 16, 1, 1, (2,)), (2, 256, 4, 4, (4,) * 8),
             (2, 256, 4, 4, (8, 8, 8, 5, 5, 5)), (17, 64, 8, 8, (8, 8, 8, 5, 5, 5)), (17, 64, 8, 8, (8, 5, 5, 5)), (4, 64, 8, 8, (2,))]


def gpu_case_inputs(B, D, H, W, levels):
    """the seeded inputs of a GPU case; tests/test_vq_fsq_cpu.py checks that the restatement leaves out none of their rows"""
    return draw(B * H * W, D, levels, 7000 + 13 * D + B * H * W + len(levels))


def torch_composition(z, w_in, b_in, w_out, b_out, levels, dtype=None, round_y=False):
    """the same function from torch ops under autograd (F.linear, tanh, a straight-through round, F.linear) -> z_q; the inputs are
    torch tensors (of any device) whose gradients the caller reads.  round_y: y takes the contract's rounding to fp32 (straight
    through), so that the indices are the kernels' wherever tanh agrees"""
    import torch
    import torch.nn.functional as F
    k = Consts(levels)
    dt = dtype or z.dtype
    dev = z.device
    half_l = torch.tensor(k.half_l, dtype=dt, device=dev)
    offset = torch.tensor(k.offset, dtype=dt, device=dev)
    shift = torch.tensor(k.shift, dtype=dt, device=dev)
    hw = torch.tensor(k.hw, dtype=dt, device=dev)
    y = F.linear(z, w_in, b_in)
    if round_y:
        y = y + (y.detach().to(torch.float32).to(dt) - y.detach())
    b = torch.tanh(y + shift) * half_l - offset
    q = b + (torch.round(b) - b).detach()
    return F.linear(q / hw, w_out, b_out)
