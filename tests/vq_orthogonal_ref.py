"""CPU restatement of the orthogonal regularization loss as vqvae_amd/csrc/vq_orthogonal.hip's header states it: numpy fp64, one IEEE
operation per written operation, explicit loops over the columns c and the codes j in ascending order (vectorised over the rows i, and
over c where the sums of different c are independent), so that numpy's own summation order never enters."""
import numpy as np

F32, F64, I32 = np.float32, np.float64, np.int32
SUM_BLOCK = 256                   # kOrthSumBlock: the blocks of the total's fixed order


def select(K, hist=None, uniforms=None, max_codes=None):
    """(K) int32 0 / 1: the candidates (every code, or hist > 0); under a cap the max_codes candidates that come first in the order
    (u ascending, then k ascending)"""
    cand = np.ones(K, bool) if hist is None else np.asarray(hist) > 0
    if uniforms is None or max_codes is None or max_codes <= 0:
        return cand.astype(I32)
    order = sorted((float(uniforms[k]), k) for k in range(K) if cand[k])
    sel = np.zeros(K, I32)
    for _, k in order[:max_codes]:
        sel[k] = 1
    return sel


def gram(rows):
    """(K, K) fp64: from 0.0, c ascending; the product of two fp32 values is exact in fp64"""
    n = rows.astype(F64)
    G = np.zeros((n.shape[0], n.shape[0]), F64)
    with np.errstate(over="ignore", invalid="ignore"):
        for c in range(n.shape[1]):
            G = G + n[:, c][:, None] * n[:, c][None, :]
    return G


def row_sums(rows, sel):
    """R (K), V (K, D) fp64: the selected j in ascending order, the product rounded and then added; 0.0 in unselected rows"""
    n, G = rows.astype(F64), gram(rows)
    K, D = n.shape
    R, V = np.zeros(K, F64), np.zeros((K, D), F64)
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(K):
            if not sel[j]:
                continue
            R = R + G[:, j] * G[:, j]
            V = V + G[:, j][:, None] * n[j][None, :]
    R[sel == 0] = 0.0
    V[sel == 0] = 0.0
    return R, V


def total(R):
    """blocks of 256 consecutive codes, ascending inside from 0.0, then the blocks in ascending order from 0.0"""
    T = F64(0.0)
    with np.errstate(over="ignore", invalid="ignore"):
        for b0 in range(0, R.shape[0], SUM_BLOCK):
            s = F64(0.0)
            for i in range(b0, min(R.shape[0], b0 + SUM_BLOCK)):
                s = s + R[i]
            T = T + s
    return T


def forward(rows, hist=None, uniforms=None, max_codes=None):
    """-> loss (fp32 scalar), M, selected (K) int32, V (K, D) fp64"""
    sel = select(rows.shape[0], hist, uniforms, max_codes)
    M = int(sel.sum())
    R, V = row_sums(rows, sel)
    if M == 0:
        return F32(0.0), 0, sel, V
    with np.errstate(over="ignore", invalid="ignore"):
        m = F64(M)
        mm = m * m
        loss = F32(total(R) / mm - F64(1.0) / m)
    return loss, M, sel, V


def backward(V, sel, M, grad_loss=None):
    """(K, D) fp32: float((double(g) (4 / M^2)) V) in selected rows, +0.0 elsewhere"""
    out = np.zeros(V.shape, F32)
    if M == 0:
        return out
    with np.errstate(over="ignore", invalid="ignore"):
        m = F64(M)
        s = F64(1.0 if grad_loss is None else F32(grad_loss)) * (F64(4.0) / (m * m))
        out[sel != 0] = (s * V[sel != 0]).astype(F32)
    return out


# (K, D) of the GPU tests and of the host harness: the degenerate corner; less than a tile, D % 4 != 0; exactly a tile's width and four
# row blocks; one past; ragged row blocks; a width between two classes; three tile steps short of nothing, the widest rows
GPU_SHAPES = [(1, 1), (5, 3), (64, 64), (65, 7), (130, 64), (96, 33), (257, 256)]


def draw_rows(K, D, seed):
    """seeded rows of unit length (normalised in fp32: the entry takes them as they stand)"""
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((K, D)).astype(F32)
    return (e / np.maximum(np.sqrt((e * e).sum(1, keepdims=True)), F32(1e-12))).astype(F32)


def variants(K, D):
    """name -> dict(rows, hist, uniforms, max_codes, grad_loss): every way the entry is called in the tests"""
    rng = np.random.default_rng(77 * K + D)
    rows = draw_rows(K, D, 1000 + 31 * K + D)
    hist = rng.integers(0, 3, K).astype(I32)
    hist[-1] = 2
    if K > 1:
        hist[0] = 0
    one = np.zeros(K, I32)
    one[K // 2] = 5
    u = (rng.integers(0, 8, K) / 8.0).astype(F32)               # eighths: ties in u at every K > 8
    ncand = int((hist > 0).sum())
    v = {
        "plain": dict(rows=rows, hist=None, uniforms=None, max_codes=None, grad_loss=None),
        "hist": dict(rows=rows, hist=hist, uniforms=None, max_codes=None, grad_loss=0.37),
        "hist_all_zero": dict(rows=rows, hist=np.zeros(K, I32), uniforms=None, max_codes=None, grad_loss=None),
        "one_active": dict(rows=rows, hist=one, uniforms=None, max_codes=None, grad_loss=-2.5),
        "cap_below": dict(rows=rows, hist=hist, uniforms=u, max_codes=max(1, ncand // 2), grad_loss=None),
        "cap_above": dict(rows=rows, hist=hist, uniforms=u, max_codes=K + 3, grad_loss=1.5),
        "cap_no_hist": dict(rows=rows, hist=None, uniforms=u, max_codes=max(1, K // 3), grad_loss=None),
    }
    if K >= 5:
        bad = rows.copy()
        bad[0, D // 2] = np.inf                                  # an unselected row (hist[0] = 0): never seen
        bad[K - 1, 0] = np.nan                                   # a selected one: everything selected becomes NaN
        v["non_finite"] = dict(rows=bad, hist=hist, uniforms=None, max_codes=None, grad_loss=None)
    return v


_expected = {}


def expected(shape):
    """name -> (inputs, (loss, M, selected, V, grad_rows)) of a GPU shape: computed once, shared by the tests, never written"""
    if shape not in _expected:
        out = {}
        for name, a in variants(*shape).items():
            loss, M, sel, V = forward(a["rows"], a["hist"], a["uniforms"], a["max_codes"])
            g = backward(V, sel, M, a["grad_loss"])
            for x in (a["rows"], a["hist"], a["uniforms"], sel, V, g):
                if x is not None:
                    x.setflags(write=False)
            out[name] = (a, (loss, M, sel, V, g))
        _expected[shape] = out
    return _expected[shape]


def same_bits(got, want):
    """every element: the same bits, or a NaN in both"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    nan_g = np.isnan(got) if got.dtype.kind == "f" else np.zeros(got.shape, bool)
    nan_w = np.isnan(want) if want.dtype.kind == "f" else np.zeros(want.shape, bool)
    return bool(np.array_equal(nan_g, nan_w) and np.array_equal(got.view(u)[~nan_g], want.view(u)[~nan_w]))
