"""CPU restatement of the per-row linear map as vqvae_amd/csrc/vq_linear.hip's header states it: numpy fp64, one IEEE operation per
written operation, the loops in the contract's order (vectorised over rows only for the row-local outputs, over the outputs only for
the sums over rows).  Rows are (N, C) fp32; the layouts of the kernels are views of them.  The forward is FSQ's projection
(tests/vq_fsq_ref.py: project_in) and the parameter sums take its blocks."""
import numpy as np

from tests import vq_fsq_ref as FR

F32, F64 = np.float32, np.float64
BLOCK_ROWS = FR.BLOCK_ROWS        # kLinBlockRows: the blocks of the parameter gradients' fixed order
to_nchw, from_nchw = FR.to_nchw, FR.from_nchw


def forward(x, w, b):
    """y (N, Cout) fp32: s = double(b[j]), then the channels in ascending order, one rounding"""
    return FR.project_in(x, w, b)


def grad_x(gy, w):
    """(N, Cin) fp32: s = 0.0, then the output channels j in ascending order, one rounding"""
    N, Cout = gy.shape
    s = np.zeros((N, w.shape[1]), F64)
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(Cout):
            s = s + w[j, :].astype(F64)[None, :] * gy[:, j].astype(F64)[:, None]
        return s.astype(F32)


def param_grads_blocked(x, gy):
    """(grad_w (Cout, Cin), grad_b (Cout)) fp32 in the kernels' order: blocks of 256 rows, inside a block one row after the other from
    0.0, then the blocks in order from 0.0, one rounding"""
    N = x.shape[0]
    x64, g64 = x.astype(F64), gy.astype(F64)
    tw, tb = np.zeros((gy.shape[1], x.shape[1]), F64), np.zeros(gy.shape[1], F64)
    with np.errstate(over="ignore", invalid="ignore"):
        for r0 in range(0, N, BLOCK_ROWS):
            sw, sb = np.zeros_like(tw), np.zeros_like(tb)
            for n in range(r0, min(N, r0 + BLOCK_ROWS)):
                sw = sw + g64[n][:, None] * x64[n][None, :]           # (the product of two fp32 values is exact in fp64)
                sb = sb + g64[n]
            tw = tw + sw
            tb = tb + sb
        return tw.astype(F32), tb.astype(F32)


def param_grads(x, gy):
    """plain fp64 sums over the rows, unrounded: (grad_w, grad_b), and (sum_n |term_n| of each) for the tolerance"""
    x64, g64 = x.astype(F64), gy.astype(F64)
    return (g64.T @ x64, g64.sum(0)), (np.abs(g64).T @ np.abs(x64), np.abs(g64).sum(0))


# (B, H, W, Cin, Cout) of the GPU tests and of the host harness: 98 rows -- less than a block, HW % 4 != 0, Cin % 4 != 0; 405 rows -- a
# block of 256 and a ragged tail; the widening direction with HW % 4 == 0; the degenerate corner; 300 rows at the envelope's corner,
# where the weights exceed LDS; one past the tile widths
GPU_CASES = [(2, 7, 7, 6, 5), (5, 9, 9, 64, 8), (3, 8, 8, 8, 64), (1, 1, 1, 1, 1), (1, 12, 25, 256, 256), (4, 8, 8, 65, 33)]


def draw(N, Cin, Cout, seed):
    """seeded rows, upstream gradient and nn.Linear-shaped parameters; with at least 8 rows, one row of x and one of grad_y carry a NaN
    and another of each an Inf"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((N, Cin)).astype(F32)
    gy = rng.standard_normal((N, Cout)).astype(F32)
    w = (rng.standard_normal((Cout, Cin)) / np.sqrt(Cin)).astype(F32)
    b = (0.1 * rng.standard_normal(Cout)).astype(F32)
    if N >= 8:
        x[1, Cin // 2] = np.nan
        x[N - 2, 0] = np.inf
        gy[1, Cout - 1] = np.nan
        gy[N - 2, 0] = -np.inf
    return x, gy, w, b


def gpu_case_inputs(B, H, W, Cin, Cout):
    return draw(B * H * W, Cin, Cout, 9000 + 17 * Cin + 3 * Cout + B * H * W)


_expected = {}


def expected(case):
    """(x, gy, w, b, y, grad_x, grad_w, grad_b) of a GPU case: computed once, shared by the tests, never written"""
    if case not in _expected:
        x, gy, w, b = gpu_case_inputs(*case)
        gw, gb = param_grads_blocked(x, gy)
        out = (x, gy, w, b, forward(x, w, b), grad_x(gy, w), gw, gb)
        for a in out:
            a.setflags(write=False)
        _expected[case] = out
    return _expected[case]


def same_bits(got, want):
    """every element: the same bits, or a NaN in both"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    return bool(np.array_equal(nan_g, nan_w) and np.array_equal(got.view(np.uint32)[~nan_g], want.view(np.uint32)[~nan_w]))
