"""l2-normalisation of rows, forward and backward, restated on the CPU: the arithmetic of vqvae_amd/csrc/vq_cosine.hip's header,
operation by operation.  A loop over the channels, vectorised over the rows; the sums, the square root and the backward are
np.float64 (numpy's +, *, / and sqrt on float64 are one correctly rounded IEEE operation each, and nothing here is fused), the
forward's division is np.float32 / np.float32: compared bitwise with the GPU.

`quantize` is the composed cosine-similarity quantizer: normalise rows and codes, then the reference quantizer on those bits --
tests/rvq_ref.py's one-stage chain, whose indices are the C oracle's.

`torch_normalize` is the independent reference: fp64 torch.nn.functional.normalize and its autograd.

Rows are (N, D) fp32 in the quantizer's row order (tests/rvq_ref.py's to_rows / to_nchw change layouts)."""
import numpy as np

F32 = np.float32
EPS = 1e-12


def l2norm(x, eps=EPS):
    """-> y (N, D) fp32, denom (N,) fp32"""
    x32 = np.ascontiguousarray(x, F32)
    x64 = x32.astype(np.float64)
    eps = F32(eps)
    with np.errstate(all="ignore"):
        s = np.zeros(x32.shape[0])
        for c in range(x32.shape[1]):
            s = s + x64[:, c] * x64[:, c]
        d = np.sqrt(s).astype(F32)
        d = np.where(d < eps, eps, d).astype(F32)               # (a NaN fails the comparison and stays)
        y = (x32 / d[:, None]).astype(F32)
    return y, d


def l2norm_backward(y, denom, g, eps=EPS):
    """-> grad_x (N, D) fp32 from the forward's y and denom"""
    y64, g64 = np.asarray(y, F32).astype(np.float64), np.asarray(g, F32).astype(np.float64)
    d32 = np.asarray(denom, F32)
    d64, e64 = d32.astype(np.float64), np.float64(F32(eps))
    with np.errstate(all="ignore"):
        t = np.zeros(y64.shape[0])
        for c in range(y64.shape[1]):
            t = t + y64[:, c] * g64[:, c]
        off = ((g64 - y64 * t[:, None]) / d64[:, None]).astype(F32)
        on = (g64 / e64).astype(F32)
    return np.where((d32 > F32(eps))[:, None], off, on).astype(F32)


def quantize(z, codebook, beta, eps=EPS):
    """The cosine-similarity quantizer: (z^, E^) = the normalised rows and codes, then tests/rvq_ref.chain on them with one stage.
    -> (z^, E^, chain): chain.idx[0] the indices, chain.z_q = z^ + (e^ - z^), chain.loss / chain.perplexity[0] in fp64"""
    from tests import rvq_ref
    zn, _ = l2norm(z, eps)
    En, _ = l2norm(codebook, eps)
    return zn, En, rvq_ref.chain(zn, [En], beta)


def torch_normalize(x, g, eps=EPS):
    """fp64 torch: -> (normalize(x) (N, D), d/dx sum(normalize(x) * g) (N, D)) as float64 arrays"""
    import torch
    xt = torch.from_numpy(np.asarray(x, F32).astype(np.float64)).requires_grad_(True)
    gt = torch.from_numpy(np.asarray(g, F32).astype(np.float64))
    y = torch.nn.functional.normalize(xt, p=2.0, dim=1, eps=eps)
    (y * gt).sum().backward()
    return y.detach().numpy(), xt.grad.numpy()


def forward_bound(ref):
    """the issue's forward bound: 4 * 2^-24 |y^| plus one fp32 denormal"""
    return 4.0 * 2.0 ** -24 * np.abs(ref) + 2.0 ** -149


def backward_bound(x, g):
    """the issue's backward bound per element of a row off the clamp: 2^-20 ||g||_2 / ||x||_2.  Derivation: y carries <= 2u relative
    error (the rounded norm and the division), the dot t therefore <= 2u ||g||, the numerator g - y t <= 4u ||g||, the division and
    the final rounding <= 2u of the result; with u = 2^-24 that totals 6u ||g|| / ||x||, doubled and rounded up to a power of two."""
    x64, g64 = np.asarray(x, F32).astype(np.float64), np.asarray(g, F32).astype(np.float64)
    with np.errstate(all="ignore"):
        return 2.0 ** -20 * np.sqrt((g64 * g64).sum(1)) / np.sqrt((x64 * x64).sum(1))


def draw(N, D, K, scale, seed):
    """z ~ scale N(0, 1) (N, D), a codebook 0.3 N(0, 1) (K, D) -- its scale has nothing to do with z's, which is the option's point --
    and g ~ N(0, 1)"""
    rng = np.random.default_rng(seed)
    z = (scale * rng.standard_normal((N, D))).astype(F32)
    cb = (0.3 * rng.standard_normal((K, D))).astype(F32)
    g = rng.standard_normal((N, D)).astype(F32)
    return z, cb, g
