"""CPU restatement of lookup-free quantization as vqvae_amd/csrc/vq_lfq.hip's header states it: numpy fp64, the loops of the row
operations in the contract's order (vectorised over rows only).  Rows are (N, D) fp32; the layouts of the kernels are views of them.
The sums over the rows (avg, P, C, the parameter gradients) are returned as plain numpy sums together with the sum of the magnitudes
of their terms, from which the tests derive their bounds; `param_grads_blocked` adds in the kernels' order.  `full_softmax` states the
losses a second time through the (N, K) softmax, for small K."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
BLOCK_ROWS = 256              # kLfqBlockRows: the blocks of the parameter gradients' fixed order


def draw(N, D, d, seed, scale=1.0):
    """seeded rows, upstream gradient and nn.Linear-shaped parameters; y has a standard deviation near `scale`"""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((N, D)).astype(F32)
    g = rng.standard_normal((N, D)).astype(F32)
    w_in = (rng.standard_normal((d, D)) * (scale / math.sqrt(D))).astype(F32)
    b_in = (0.1 * scale * rng.standard_normal(d)).astype(F32)
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


def codes(y):
    """-> (c (N, d) fp32: +1 above zero, -1 at and below, NaN for NaN; idx (N,) int64, first channel least significant)"""
    with np.errstate(invalid="ignore"):
        bit = y > 0
    c = np.where(np.isnan(y), F32(np.nan), np.where(bit, F32(1), F32(-1))).astype(F32)
    idx = (bit.astype(np.int64) << np.arange(y.shape[1], dtype=np.int64)[None, :]).sum(1)
    return c, idx


def project_out(c, w_out, b_out):
    N = c.shape[0]
    s = np.broadcast_to(b_out.astype(F64), (N, w_out.shape[0])).copy()
    with np.errstate(invalid="ignore"):
        for j in range(c.shape[1]):
            s = s + w_out[:, j].astype(F64)[None, :] * c[:, j].astype(F64)[:, None]
    return s.astype(F32)


def all_codes(d):
    """(K, d) of +-1: row k = the codes of index k"""
    k = np.arange(1 << d, dtype=np.int64)[:, None]
    return (((k >> np.arange(d)[None, :]) & 1) * 2 - 1).astype(F32)


def decode(idx, w_out, b_out, d):
    """indices -> z_q; an index outside [0, K) gives a NaN row"""
    idx = np.asarray(idx, np.int64)
    ok = (idx >= 0) & (idx < (1 << d))
    u = np.where(ok, idx, 0)
    c = np.where(ok[:, None], all_codes(d)[u], F32(np.nan)).astype(F32)
    return project_out(c, w_out, b_out)


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


class Result:
    pass


def forward(z, w_in, b_in, w_out, b_out):
    f = Result()
    d = w_in.shape[0]
    f.d, f.K = d, 1 << d
    f.y = project_in(z, w_in, b_in)
    f.c, f.idx = codes(f.y)
    f.z_q = project_out(f.c, w_out, b_out)
    f.hist = np.bincount(f.idx, minlength=f.K).astype(np.int32)
    f.perplexity = perplexity(f.hist, z.shape[0])
    return f


def sigmoids(y, s):
    """a = s y -> (p+, p-, h, |a|), each from e = exp(-|a|) as the contract writes it"""
    with np.errstate(invalid="ignore", over="ignore"):
        a = F64(s) * y.astype(F64)
        m = np.abs(a)
        e = np.exp(-m)
        big, small = 1.0 / (1.0 + e), e / (1.0 + e)
        p1 = np.where(a >= 0, big, small)
        p0 = np.where(a >= 0, small, big)
        h = np.log1p(e) + m * small
    return p1, p0, h, m


def code_probs(p1, p0, bits=None):
    """p_n(k) (N, 2^len(bits)) as the product over the channels `bits` in ascending order; entry m holds bit i of m for bits[i]"""
    N, d = p1.shape
    bits = list(range(d)) if bits is None else bits
    tab = np.ones((N, 1), F64)
    for j in bits:
        tab = np.concatenate([tab * p0[:, j:j + 1], tab * p1[:, j:j + 1]], axis=1)
    return tab


def xlogx(a):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(a == 0, 0.0, a * np.log(np.where(a == 0, 1.0, a)))


def losses(y, beta, we, gamma, inv_t):
    """the contract's losses from the factorised form -> Result with C, P, H, loss (fp64), avg (K) and, for the bounds, the sums of the
    magnitudes of the terms: mag_C, mag_P (before the division), mag_H"""
    N, d = y.shape
    r = Result()
    s = 4.0 * F64(inv_t)
    p1, p0, h, _ = sigmoids(y, s)
    c, _ = codes(y)
    with np.errstate(invalid="ignore"):
        cm = (y.astype(F64) - c.astype(F64)) ** 2
    r.C, r.mag_C = cm.sum() / (F64(N) * F64(d)), np.abs(cm).sum() / (F64(N) * F64(d))
    r.P, r.mag_P = h.sum() / F64(N), np.abs(h).sum() / F64(N)
    r.avg = code_probs(p1, p0).sum(0) / F64(N)
    t = xlogx(r.avg)
    r.H, r.mag_H = -t.sum(), np.abs(t).sum()
    r.loss = F64(beta) * r.C + F64(we) * (r.P - F64(gamma) * r.H)
    r.p1, r.p0 = p1, p0
    return r


def full_softmax(y, beta, we, gamma, inv_t):
    """the same losses through the (N, K) softmax with logits 2 inv_t y . c_k (small K only) -> (C, P, H, loss, avg)"""
    N, d = y.shape
    ck = all_codes(d).astype(F64)
    logits = 2.0 * F64(inv_t) * (y.astype(F64) @ ck.T)
    logits = logits - logits.max(1, keepdims=True)
    p = np.exp(logits)
    p = p / p.sum(1, keepdims=True)
    P = -xlogx(p).sum(1).mean()
    avg = p.mean(0)
    H = -xlogx(avg).sum()
    c, _ = codes(y)
    C = ((y.astype(F64) - c.astype(F64)) ** 2).mean()
    return C, P, H, F64(beta) * C + F64(we) * (P - F64(gamma) * H), avg


def insert_bit(m, j, b):
    return ((m >> j) << (j + 1)) | (b << j) | (m & ((1 << j) - 1))


def loss_grad_y(y, avg, beta, we, gamma, inv_t):
    """e (N, d): d loss / d y by the contract's formula, the three terms t1, t2, t3 separately, and mag_T = sum |L[k]| prod (the
    magnitudes of T+ and T- together)"""
    N, d = y.shape
    s = 4.0 * F64(inv_t)
    p1, p0, _, _ = sigmoids(y, s)
    c, _ = codes(y)
    L = np.where(avg == 0, 0.0, np.log(np.where(avg == 0, 1.0, avg)))
    r = Result()
    n = F64(N)
    pq = p1 * p0
    with np.errstate(invalid="ignore"):
        y64 = y.astype(F64)
        r.t1 = F64(beta) * 2.0 * (y64 - c.astype(F64)) / (n * F64(d))
        r.t2 = F64(we) * (s * s / n) * y64 * pq
        T = np.zeros((N, d, 2), F64)
        r.mag_T = np.zeros((N, d), F64)
        m = np.arange(1 << (d - 1), dtype=np.int64)
        for j in range(d):
            tab = code_probs(p1, p0, [i for i in range(d) if i != j])           # (N, K / 2), entry m
            for b in (0, 1):
                Lb = L[insert_bit(m, j, b)]
                T[:, j, b] = tab @ Lb
                r.mag_T[:, j] += tab @ np.abs(Lb)
        r.T = T
        r.pq = pq
        r.t3 = F64(we) * F64(gamma) * (s / n) * pq * (T[:, :, 1] - T[:, :, 0])
        r.e = r.t1 - r.t2 + r.t3
    return r


def backward(z, g, gl, avg, w_in, b_in, w_out, beta, we, gamma, inv_t):
    """the row-local backward (gc, e, gy, grad_z) and the per-row terms of the four parameter gradients, in fp64.  g may be None
    (zero), avg may be None (no loss gradient), gl is the upstream gradient of the loss (a float)"""
    N, D = z.shape
    d = w_in.shape[0]
    y = project_in(z, w_in, b_in)
    c, _ = codes(y)
    r = Result()
    r.y, r.c = y, c
    gc = np.zeros((N, d), F64)
    g64 = np.zeros((N, D), F64) if g is None else g.astype(F64)
    with np.errstate(invalid="ignore"):
        for ch in range(D):
            gc = gc + w_out[ch, :].astype(F64)[None, :] * g64[:, ch][:, None]
    r.gc = gc
    r.lg = loss_grad_y(y, avg, beta, we, gamma, inv_t) if avg is not None else None
    with np.errstate(invalid="ignore"):
        r.gy = gc + F64(gl) * r.lg.e if avg is not None else gc
        s = np.zeros((N, D), F64)
        r.mag_gz = np.zeros((N, D), F64)
        for j in range(d):
            t = w_in[j, :].astype(F64)[None, :] * r.gy[:, j][:, None]
            s = s + t
            r.mag_gz = r.mag_gz + np.abs(t)
        r.grad_z = s.astype(F32)
        z64 = z.astype(F64)
        r.terms = {"w_out": g64[:, :, None] * c.astype(F64)[:, None, :], "b_out": g64,
                   "w_in": r.gy[:, :, None] * z64[:, None, :], "b_in": r.gy}
    return r


def param_grads(r):
    """plain fp64 sums over the rows, rounded once -> dict of fp32 arrays, and sum_n |term_n| for the tolerance"""
    with np.errstate(invalid="ignore"):
        return ({n: t.sum(0).astype(F32) for n, t in r.terms.items()}, {n: np.abs(t).sum(0) for n, t in r.terms.items()})


def param_grads_blocked(r, names=("w_out", "b_out", "w_in", "b_in")):
    """the kernels' order: blocks of 256 rows, inside a block one row after the other from 0.0, then the blocks in order from 0.0"""
    out = {}
    with np.errstate(invalid="ignore"):
        for n in names:
            t = r.terms[n]
            total = np.zeros(t.shape[1:], F64)
            for r0 in range(0, t.shape[0], BLOCK_ROWS):
                s = np.zeros(t.shape[1:], F64)
                for row in t[r0:r0 + BLOCK_ROWS]:
                    s = s + row
                total = total + s
            out[n] = total.astype(F32)
    return out


def partition(N, K):
    """(rows per partition, partitions) of the loss sums: a function of (N, K) alone"""
    pmax = max(16, min(1024, (1 << 20) // K))
    blocks = (N + BLOCK_ROWS - 1) // BLOCK_ROWS
    bpp = (blocks + pmax - 1) // pmax
    return bpp * BLOCK_ROWS, (blocks + bpp - 1) // bpp


def to_nchw(rows, B, H, W):
    """(N, D) rows -> (B, D, H, W) maps"""
    return np.ascontiguousarray(rows.reshape(B, H, W, -1).transpose(0, 3, 1, 2))


def from_nchw(maps):
    B, D, H, W = maps.shape
    return np.ascontiguousarray(maps.transpose(0, 2, 3, 1)).reshape(B * H * W, D)


# ---- the bounds of the GPU tests (derived in tests/test_vq_lfq_gpu.py's docstring) -------------------------------------------------
U = 2.0 ** -53
FN = 8.0                      # allowance, in fp64 ulps, for one device exp / log / log1p and the few operations around it


def avg_bound(ref, N, d):
    return (N + FN * d + 16) * U * ref.avg + 2.0 ** -1000


def loss_bounds(ref, N, d, K, beta, we, gamma):
    """fp64 bounds of (loss, C, P, H) before the fp32 rounding"""
    n_add = N + 1024 + d + 16
    bC = (n_add + 4) * U * ref.mag_C
    bP = (n_add + 2 * FN) * U * ref.mag_P
    with np.errstate(divide="ignore"):
        la = np.where(ref.avg == 0, 0.0, np.abs(np.log(np.where(ref.avg == 0, 1.0, ref.avg))))
    bH = (K / 256 + 8 + FN) * U * ref.mag_H + ((la + 1.0) * avg_bound(ref, N, d)).sum()
    bL = beta * bC + we * (bP + gamma * bH) + 4 * U * (abs(beta * ref.C) + abs(we * ref.P) + abs(we * gamma * ref.H))
    return bL, bC, bP, bH


def e_bound(lg, K, d, we, gamma, s, N):
    """|e_got - e_ref| of loss_grad_y's result"""
    return U * (8 * np.abs(lg.t1) + 3 * FN * np.abs(lg.t2) + 3 * FN * np.abs(lg.t3)) + \
        abs(we * gamma) * (s / N) * lg.pq * (K + FN * d + 16) * U * lg.mag_T
