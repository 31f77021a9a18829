"""Residual vector quantization on the GPU (vqvae_vq_residual_forward_f32 / _decode_f32 / _backward_f32, functional.vq_residual_*,
training.vq_residual_backward, ResidualVectorQuantizer, VQVAE(n_quantizers=...)) against the CPU restatement tests/rvq_ref.py, whose
operation order is the header of vqvae_amd/csrc/vq_residual.hip.

Exact: indices of every stage, z_q, the last residual, histograms, the decoded sum.  At the quantizer's own contract (rtol 1e-6
against fp64): stage losses, their sum, perplexities.  grad_z: inside 2 (Q + 2) 2^-24 (|grad_zq| + c sum_q |r_q - e_q|) of the fp64
value (the roundings of the chain with a factor two), and bitwise the mirrored fp32 order; codebook gradients at
vqvae_vq_backward_f32's contract (rtol 1e-4, atol 1e-5 max|grad|)."""
import faulthandler
import functools

import numpy as np
import pytest
import torch

from tests import grid_caps as GC
from tests import rvq_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BETA = 0.25

# (K, D) per quantizer route: the resident tracker; a small resident codebook; the four-wave form (row-major only); any-width rows
# twice; the streamed image
KD = [(512, 64), (96, 64), (1024, 64), (64, 48), (5, 3), (2048, 128)]
# (B, H, W): 192 rows, a partial unit; H W = 32; H W = 15 -- NCHW maps that are no multiple of 32 and no multiple of four pixels
SHAPES = [(3, 8, 8), (5, 4, 8), (2, 3, 5)]


def _bits(t):
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return a.view(np.uint32)


def _layout(rows, B, H, W, rowmajor):
    """(N, D) numpy rows -> the device tensor whose rows they are: (B,H,W,D), or (B,D,H,W)"""
    z = torch.from_numpy(np.ascontiguousarray(rows)).view(B, H, W, rows.shape[1])
    return (z if rowmajor else z.permute(0, 3, 1, 2)).contiguous().to(DEV)


def _rows(t, rowmajor):
    """the (N, D) numpy rows of a device tensor in either layout"""
    t = t.detach().cpu()
    t = t if rowmajor else t.permute(0, 2, 3, 1)
    return np.ascontiguousarray(t.contiguous().numpy().reshape(-1, t.shape[-1]))


def _dev(books):
    return [torch.from_numpy(np.ascontiguousarray(E)).to(DEV) for E in books]


def _same_bits_nan_aside(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN positions"
    assert np.array_equal(got.view(np.uint32)[~gn], want.view(np.uint32)[~wn]), f"{what}: bits"


@functools.lru_cache(maxsize=None)
def _case(K, D, B, H, W, shared):
    """rows, the four stages' codebooks (stage q's drawn from r_q) and the chain, computed once and left unchanged"""
    N = B * H * W
    rows = np.random.default_rng(K + D + N).standard_normal((N, D)).astype(np.float32)
    books = R.draw_books(rows, K, 4, shared, K + N)
    return rows, books, R.chain(rows, books, BETA)


def _prefix(rows, books, c4, Q):
    """the chain of the first Q stages (their indices are the four-stage chain's)"""
    return c4 if Q == 4 else R.chain(rows, books[:Q], BETA, idx=c4.idx[:Q])


def _check_forward(out, c, rowmajor, K, what):
    loss, z_q, ppl, idx, hist, loss_stage, res = out
    torch.cuda.synchronize()
    Q = len(c.e)
    assert idx.shape == c.idx.shape and idx.dtype == torch.int64 and hist.shape == (Q, K) and hist.dtype == torch.int32
    assert np.array_equal(idx.cpu().numpy(), c.idx), f"{what}: indices"
    assert np.array_equal(_bits(_rows(z_q, rowmajor)), _bits(c.z_q)), f"{what}: z_q"
    assert np.array_equal(_bits(_rows(res, rowmajor)), _bits(c.r[Q])), f"{what}: residual_out"
    assert np.array_equal(hist.cpu().numpy(), c.hist), f"{what}: hist"
    got = (loss_stage.cpu().numpy().astype(np.float64), float(loss), ppl.cpu().numpy().astype(np.float64))
    print(what, "loss_stage", got[0], "ref", c.loss_stage, "loss", got[1], "ref", c.loss, "perplexity", got[2], "ref", c.perplexity)
    np.testing.assert_allclose(got[0], c.loss_stage, rtol=1e-6, atol=0, err_msg=what)
    np.testing.assert_allclose(got[1], c.loss, rtol=1e-6, atol=0, err_msg=what)
    np.testing.assert_allclose(got[2], c.perplexity, rtol=1e-6, atol=0, err_msg=what)


# ---- 1. forward ------------------------------------------------------------------------------------------------------------------

# ((1024, 64) is the row-major four-wave form's case: no NCHW run of it)
FORWARD_CASES = [(K, D, B, H, W, rm) for K, D in KD for B, H, W in SHAPES for rm in (False, True) if rm or (K, D) != (1024, 64)]


@pytest.mark.parametrize("K,D,B,H,W,rowmajor", FORWARD_CASES)
def test_forward_against_the_restatement(K, D, B, H, W, rowmajor):
    from vqvae_amd import functional as F
    for shared in (False, True):
        rows, books, c4 = _case(K, D, B, H, W, shared)
        z = _layout(rows, B, H, W, rowmajor)
        dbooks = _dev(books[:1] if shared else books)
        if K <= B * H * W:
            assert (~c4.r[1].any(axis=1)).sum() > 0          # rows that equal a code exactly: all zeros for the next stage
        for Q in (1, 2, 4):
            out = F.vq_residual_forward(z, dbooks[:1] if shared else dbooks[:Q], BETA, rowmajor=rowmajor, shared=shared, n_q=Q,
                                        want_residual=True)
            _check_forward(out, _prefix(rows, books, c4, Q), rowmajor, K, f"K={K} D={D} Q={Q} shared={shared}")


def test_forward_without_zq_and_on_a_prepared_workspace():
    from vqvae_amd import functional as F
    rows, books, c4 = _case(96, 64, 3, 8, 8, False)
    z, dbooks = _layout(rows, 3, 8, 8, True), _dev(books)
    ws = F.vq_residual_workspace(192, 96, 64, 4, DEV)
    first = F.vq_residual_forward(z, dbooks, BETA, rowmajor=True, workspace=ws, want_residual=True)
    again = F.vq_residual_forward(z, dbooks, BETA, rowmajor=True, workspace=ws, prepared=True, want_residual=True)
    _check_forward(first, c4, True, 96, "fresh workspace")
    _check_forward(again, c4, True, 96, "prepared workspace")
    out = F.vq_residual_forward(z, dbooks, BETA, rowmajor=True, workspace=ws, prepared=True, want_zq=False)
    torch.cuda.synchronize()
    assert out[1] is None and len(out) == 6 and torch.equal(out[3], first[3]) and torch.equal(out[0], first[0])


def _check_backward(gz, ge, rows, books, idx, grad_zq, gl, rowmajor, what, shared=False):
    """grad_z inside the header's bound of the fp64 value and bitwise the mirrored fp32 order; codebook gradients at
    vqvae_vq_backward_f32's contract"""
    want_gz, bound, _, want_ge = R.grads(rows, books, idx, grad_zq, gl, BETA, shared)
    got = _rows(gz, rowmajor)
    err = np.abs(got.astype(np.float64) - want_gz)
    print(f"{what}: max grad_z error / bound = {float((err / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (err <= bound).all(), what
    assert np.array_equal(_bits(got), _bits(R.grad_z_mirror(rows, books, idx, grad_zq, gl))), f"{what}: grad_z, the header's order"
    assert len(ge) == len(want_ge)
    for a, w in zip(ge, want_ge):
        assert np.abs(w).max() > 0
        np.testing.assert_allclose(a.cpu().numpy(), w, rtol=1e-4, atol=1e-5 * np.abs(w).max(), err_msg=what)


# (B, H, W, D, K) past the launch cap of the element-wise kernels, 65536 workgroups of 256 threads (tests/grid_caps.py reads the
# shapes from here): NCHW maps of 15 pixels go element by element; row-major rows of 8 channels go four elements per thread, so
# the same cap lies four times as many elements out
CAP_SHAPE = (17477, 3, 5, 64, 16)
CAP_SHAPE_WIDE = (8388743, 1, 1, 8, 16)


def test_grid_stride_past_the_launch_cap():
    """more elements than the element-wise kernels' 65536 workgroups of 256 threads cover in one step: the forward, and the backward
    (grad_z and both codebook gradients) into buffers that start as NaNs between guards"""
    from vqvae_amd import functional as F, training as T
    B, H, W, D, K = CAP_SHAPE
    assert B * H * W * D > 65536 * 256
    rows = np.random.default_rng(1).standard_normal((B * H * W, D)).astype(np.float32)
    books = R.draw_books(rows, K, 2, False, 2)
    c = R.chain(rows, books, BETA)
    z, dbooks = _layout(rows, B, H, W, False), _dev(books)
    out = F.vq_residual_forward(z, dbooks, BETA, want_residual=True)
    _check_forward(out, c, False, K, "262155 rows, NCHW")
    del out
    # codes moved off the rows they were drawn from (as _backward_case does), the forward's indices kept: any indices are the entry's input
    g = np.random.default_rng(3)
    moved = [(E + 0.05 * g.standard_normal(E.shape)).astype(np.float32) for E in books]
    grad_zq, gl = g.standard_normal(rows.shape).astype(np.float32), np.float32(0.7)
    with GC.guarded() as guard:
        gz, ge = T.vq_residual_backward(z, _dev(moved), torch.from_numpy(c.idx).to(DEV), _layout(grad_zq, B, H, W, False),
                                        torch.tensor(float(gl), device=DEV), BETA)
    guard.check()
    _check_backward(gz, ge, rows, moved, c.idx, grad_zq, gl, False, "262155 rows, NCHW, backward")


def _wide_case():
    """(z, books, idx, grad_zq) of CAP_SHAPE_WIDE on the device: two stages, indices drawn (decode and backward take any)"""
    B, H, W, D, K = CAP_SHAPE_WIDE
    N = B * H * W
    assert N * D // 4 > 65536 * 256 and (N * D // 4) % 256 != 0
    gen = torch.Generator(device=DEV).manual_seed(4)
    z = torch.randn((B, H, W, D), device=DEV, generator=gen)
    books = [torch.randn((K, D), device=DEV, generator=gen) * 0.5 ** q for q in range(2)]
    idx = torch.randint(0, K, (2, N), device=DEV, generator=gen)
    return z, books, idx, torch.randn((B, H, W, D), device=DEV, generator=gen)


def _wide_blocks(z, books, idx, step=1 << 21):
    """a block of rows at a time: (rows, [e_0, e_1], [r_0, r_1, r_2]) -- the chain of tests/rvq_ref.py in torch's fp32 ops"""
    B, H, W, D, K = CAP_SHAPE_WIDE
    N = B * H * W
    for r0 in range(0, N, step):
        sl = slice(r0, min(N, r0 + step))
        e = [books[q][idx[q, sl]] for q in range(2)]
        r = [z.view(N, D)[sl]]
        for q in range(2):
            r.append(r[q] - e[q])
        yield sl, e, r


def test_grid_stride_past_the_launch_cap_4_wide():
    """the same cap in the kernels' 4-wide forms (row-major rows, D % 4 == 0, aligned tensors), on 67 M elements: rvq_finish_kernel<4>
    through the decode and rvq_gradz_kernel<4> through the backward.  The restatement's arithmetic (tests/rvq_ref.py: chain,
    grad_z_mirror, grads) is evaluated here with torch's elementwise ops on the device, a block of rows at a time -- one IEEE
    operation per op, nothing fused, as numpy's -- because the numpy form would take a minute at this size; the bounds are
    test_backward_against_the_restatement's."""
    from vqvae_amd import functional as F, training as T
    B, H, W, D, K = CAP_SHAPE_WIDE
    N, Q = B * H * W, 2
    z, books, idx, grad_zq = _wide_case()
    gl = np.float32(0.7)
    with GC.guarded() as guard:
        s = F.vq_residual_decode(idx, books, B, H, W, rowmajor=True, validate=False)
        gz, none = T.vq_residual_backward(z, books, idx, grad_zq, torch.tensor(float(gl), device=DEV), BETA, rowmajor=True,
                                          need_codebooks=False)
    guard.check()
    assert none is None and z.data_ptr() % 16 == 0 and gz.data_ptr() % 16 == 0 and s.data_ptr() % 16 == 0
    gs = float(np.float32(gl * np.float32(2.0 / (float(N) * float(D)))))
    cz = float(gl) * 2.0 / (N * D)
    worst = 0.0
    gr, sr, gzr = grad_zq.view(N, D), s.view(N, D), gz.view(N, D)
    for sl, e, r in _wide_blocks(z, books, idx):
        assert torch.equal(sr[sl].view(torch.int32), (e[0] + e[1]).view(torch.int32)), f"decode: rows from {sl.start}"
        mirror = gr[sl] + gs * (r[1] + r[2])
        assert torch.equal(gzr[sl].view(torch.int32), mirror.view(torch.int32)), f"grad_z, the header's order: rows from {sl.start}"
        diffs = [r[q].double() - e[q].double() for q in range(Q)]
        want = gr[sl].double() + cz * (diffs[0] + diffs[1])
        bound = R.grad_z_bound(Q, gr[sl].double().abs(), cz, diffs[0].abs() + diffs[1].abs())
        err = (gzr[sl].double() - want).abs()
        assert bool((err <= bound).all()), f"grad_z against fp64: rows from {sl.start}"
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
    print(f"{N} rows, row-major, 4-wide: max grad_z error / bound = {worst:.3f}")


def test_grid_stride_past_the_launch_cap_4_wide_codebooks():
    """... and rvq_advance_kernel<4> in front of the second stage's segmented sum: both codebook gradients,
    grad_E_q[k] = g 2 beta / (N D) sum_{i: idx_q,i = k} (e_k - r_q,i) in fp64, at vqvae_vq_backward_f32's contract"""
    from vqvae_amd import training as T
    B, H, W, D, K = CAP_SHAPE_WIDE
    N, Q = B * H * W, 2
    z, books, idx, _ = _wide_case()
    gl = 0.7
    with GC.guarded() as guard:
        none, ge = T.vq_residual_backward(z, books, idx, None, torch.tensor(gl, device=DEV), BETA, rowmajor=True, need_z=False)
    guard.check()
    assert none is None and len(ge) == Q
    sums = [torch.zeros((K, D), dtype=torch.float64, device=DEV) for _ in range(Q)]
    for sl, e, r in _wide_blocks(z, books, idx):
        for q in range(Q):                                    # the rows of every code, added up as one product per block
            sums[q] += torch.nn.functional.one_hot(idx[q, sl], K).double().T @ (e[q].double() - r[q].double())
    for a, w in zip(ge, sums):
        w = (gl * 2.0 * BETA / (N * D) * w).cpu().numpy()
        assert np.abs(w).max() > 0
        np.testing.assert_allclose(a.cpu().numpy(), w, rtol=1e-4, atol=1e-5 * np.abs(w).max())


# ---- 2. one stage is the quantizer ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rowmajor", [False, True])
@pytest.mark.parametrize("K,D,B,H,W", [(512, 64, 3, 8, 8), (96, 64, 2, 3, 5), (64, 48, 5, 4, 8), (5, 3, 2, 3, 5), (2048, 128, 3, 8, 8)])
def test_one_stage_has_the_quantizers_bits(K, D, B, H, W, rowmajor):
    from vqvae_amd import functional as F
    rows, books, _ = _case(K, D, B, H, W, False)
    z, cb = _layout(rows, B, H, W, rowmajor), _dev(books[:1])[0]
    loss, z_q, ppl, idx, hist, loss_stage = F.vq_residual_forward(z, [cb], BETA, rowmajor=rowmajor)
    l1, zq1, p1, i1, h1 = F.vq_forward(z, cb, BETA, rowmajor=rowmajor)
    torch.cuda.synchronize()
    assert torch.equal(idx.view(-1), i1.view(-1)) and torch.equal(hist.view(-1), h1)
    assert np.array_equal(_bits(z_q), _bits(zq1))
    assert np.array_equal(_bits(loss), _bits(l1)) and np.array_equal(_bits(loss_stage[0]), _bits(l1))
    assert np.array_equal(_bits(ppl[0]), _bits(p1))


# ---- 3. special values ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rowmajor", [False, True])
@pytest.mark.parametrize("K,D,B,H,W", [(96, 64, 3, 8, 8), (5, 3, 2, 3, 5)])
def test_special_values(K, D, B, H, W, rowmajor):
    from vqvae_amd import functional as F
    N = B * H * W
    rows = np.random.default_rng(N + K).standard_normal((N, D)).astype(np.float32)
    rows[5] = np.nan                                          # an all-NaN row
    rows[11, 1] = np.inf                                      # a row with +Inf
    books = R.draw_books(rows, K, 3, False, 4)               # (finite rows only)
    books[0][2, 0] = -0.0                                     # a codebook entry of -0.0 ...
    rows[17] = books[0][2]                                    # ... in a code that a row equals
    c = R.chain(rows, books, BETA)
    assert np.isnan(c.r[3][5]).all() and np.isinf(c.r[3][11, 1]) and not c.r[1][17].any()
    out = F.vq_residual_forward(_layout(rows, B, H, W, rowmajor), _dev(books), BETA, rowmajor=rowmajor, want_residual=True)
    torch.cuda.synchronize()
    loss, z_q, ppl, idx, hist, loss_stage, res = out
    assert np.array_equal(idx.cpu().numpy(), c.idx)
    assert np.array_equal(hist.cpu().numpy(), c.hist)
    _same_bits_nan_aside(_rows(z_q, rowmajor), c.z_q, "z_q")
    _same_bits_nan_aside(_rows(res, rowmajor), c.r[3], "residual_out")
    np.testing.assert_allclose(ppl.cpu().numpy().astype(np.float64), c.perplexity, rtol=1e-6)
    assert not np.isfinite(c.loss) and not np.isfinite(float(loss))
    assert np.array_equal(np.isfinite(loss_stage.cpu().numpy()), np.isfinite(c.loss_stage))
    dec = F.vq_residual_decode(idx, _dev(books), B, H, W, rowmajor=rowmajor)
    assert np.array_equal(_bits(_rows(dec, rowmajor)), _bits(c.S))          # (finite codes: the sum has no NaN)


# ---- 4. decode -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rowmajor", [False, True])
@pytest.mark.parametrize("K,D,B,H,W", [(96, 64, 3, 8, 8), (64, 48, 2, 3, 5), (5, 3, 5, 4, 8)])
def test_decode_is_the_sum_of_the_code_rows(K, D, B, H, W, rowmajor):
    from vqvae_amd import functional as F
    for shared in (False, True):
        rows, books, c4 = _case(K, D, B, H, W, shared)
        dbooks = _dev(books[:1] if shared else books)
        idx = torch.from_numpy(c4.idx).to(DEV)
        got = F.vq_residual_decode(idx, dbooks, B, H, W, rowmajor=rowmajor, shared=shared)
        assert np.array_equal(_bits(_rows(got, rowmajor)), _bits(c4.S))
        # one index = K: NaN in exactly that row (through the C entry: the front end's check is off), nothing else moves
        bad = idx.clone()
        bad[2, 7] = K
        with pytest.raises(IndexError):
            F.vq_residual_decode(bad, dbooks, B, H, W, rowmajor=rowmajor, shared=shared)
        got = _rows(F.vq_residual_decode(bad, dbooks, B, H, W, rowmajor=rowmajor, shared=shared, validate=False), rowmajor)
        assert np.isnan(got[7]).all()
        keep = np.arange(B * H * W) != 7
        assert np.array_equal(_bits(got[keep]), _bits(c4.S[keep]))


# ---- 5. backward -----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _backward_case(K, D, B, H, W, shared):
    """_case's rows, with every code moved a little off the row it was drawn from: with more codes than rows (30 rows here) every
    row would otherwise equal a code at every stage, and all the gradients under test would be exact zeros"""
    rows, books, _ = _case(K, D, B, H, W, shared)
    g = np.random.default_rng(K + D)
    uniq = [books[0]] if shared else books[:3]
    uniq = [(E + 0.05 * g.standard_normal(E.shape)).astype(np.float32) for E in uniq]
    books = uniq * 3 if shared else uniq
    return rows, books, R.chain(rows, books, BETA)


@pytest.mark.parametrize("rowmajor", [False, True])
@pytest.mark.parametrize("B,H,W", [(3, 8, 8), (2, 3, 5)])
@pytest.mark.parametrize("K,D", [(96, 64), (64, 48)])
def test_backward_against_the_restatement(K, D, B, H, W, rowmajor):
    from vqvae_amd import training as T
    Q, N = 3, B * H * W
    g = np.random.default_rng(K + N)
    grad_zq = g.standard_normal((N, D)).astype(np.float32)
    gl = np.float32(0.7)
    gzq_d, gl_d = _layout(grad_zq, B, H, W, rowmajor), torch.tensor(float(gl), device=DEV)
    for shared in (False, True):
        rows, books, c3 = _backward_case(K, D, B, H, W, shared)
        idx = c3.idx
        z, dbooks, idx_d = _layout(rows, B, H, W, rowmajor), _dev(books[:1] if shared else books), torch.from_numpy(idx).to(DEV)
        gz, ge = T.vq_residual_backward(z, dbooks, idx_d, gzq_d, gl_d, BETA, rowmajor=rowmajor, shared=shared)
        gz2, ge2 = T.vq_residual_backward(z, dbooks, idx_d, gzq_d, gl_d, BETA, rowmajor=rowmajor, shared=shared)
        torch.cuda.synchronize()
        assert np.array_equal(_bits(gz), _bits(gz2)) and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(ge, ge2))
        assert len(ge) == (1 if shared else Q)
        _check_backward(gz, ge, rows, books, idx, grad_zq, gl, rowmajor, f"K={K} D={D} shared={shared}", shared)
        if shared:
            # the shared codebook's gradient is the stage results added in stage order: the same codebook listed per stage gives them
            _, stages = T.vq_residual_backward(z, dbooks * Q, idx_d, gzq_d, gl_d, BETA, rowmajor=rowmajor, need_z=False)
            assert np.array_equal(_bits(ge[0]), _bits((stages[0] + stages[1]) + stages[2]))
        # without an upstream z_q gradient and with g = 1 (NULL pointers)
        gz0, _ = T.vq_residual_backward(z, dbooks, idx_d, None, None, BETA, rowmajor=rowmajor, shared=shared, need_codebooks=False)
        assert np.array_equal(_bits(_rows(gz0, rowmajor)), _bits(R.grad_z_mirror(rows, books, idx, None, np.float32(1.0))))


def test_one_stage_backward_is_the_quantizers():
    from vqvae_amd import training as T
    rows, books, c4 = _case(96, 64, 3, 8, 8, False)
    z, cb, idx = _layout(rows, 3, 8, 8, True), _dev(books[:1])[0], torch.from_numpy(c4.idx[:1]).to(DEV)
    gzq, gl = torch.randn(3, 8, 8, 64, device=DEV), torch.tensor(1.3, device=DEV)
    gz, ge = T.vq_residual_backward(z, [cb], idx, gzq, gl, BETA, rowmajor=True)
    gz1, ge1 = T.vq_backward(z, cb, idx[0], gzq, gl, BETA, rowmajor=True)
    assert np.array_equal(_bits(gz), _bits(gz1)) and np.array_equal(_bits(ge[0]), _bits(ge1))


# ---- 6. module -------------------------------------------------------------------------------------------------------------------------

def _model(**kw):
    from vqvae_amd import conv
    from vqvae_amd.modules import VQVAE
    conv.set_conv_backend("hip")
    torch.manual_seed(0)
    m = VQVAE(32, 8, 1, 64, 64, 0.25, **kw).to(DEV)
    with torch.no_grad():                                     # codes on the scale of what each stage sees
        for q, w in enumerate(m.vector_quantization.codebooks()):
            w.copy_(torch.randn(w.shape, generator=torch.Generator().manual_seed(q)).to(DEV) * 0.5 ** q)
    return m


def test_model_wire_format():
    from vqvae_amd import conv, functional as F
    m = _model(n_quantizers=3).eval()
    vq = m.vector_quantization
    x = torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(1)).to(DEV)
    with torch.no_grad():
        z_e = conv.encoder_forward(m.encoder, x, pre_quant=m.pre_quantization_conv)
        loss, z_q, ppl, idx, hist = vq.quantize(z_e, rowmajor=True)
        code = m.encode(x)
        assert code.shape == (3, 256) and code.dtype == torch.int64 and torch.equal(code, idx)
        books = [w.detach() for w in vq.codebooks()]
        s = F.vq_residual_decode(code, books, 4, 8, 8, rowmajor=True)
        want = conv.decoder_forward(m.decoder, s, rowmajor_in=True)
        got = m.decode_indices(code, 4, 8, 8)
        assert got.shape == (4, 3, 32, 32) and np.array_equal(_bits(got), _bits(want))
        bad = code.clone()
        bad[1, 3] = 64
        with pytest.raises(IndexError):
            m.decode_indices(bad, 4, 8, 8)
        with pytest.raises(ValueError):
            m.decode_indices(code[:2], 4, 8, 8)
        el, x_hat, p = m(x)
        assert p.dim() == 0 and np.array_equal(_bits(p), _bits(ppl.mean())) and np.array_equal(_bits(el), _bits(loss))
        assert np.array_equal(_bits(x_hat), _bits(conv.decoder_forward(m.decoder, z_q, rowmajor_in=True)))
        # the quantizer on its own takes NCHW maps and returns the reference's 5-tuple with stage 0's one-hot
        out = vq(z_e.permute(0, 3, 1, 2).contiguous())
        assert out[1].shape == (4, 64, 8, 8) and torch.equal(out[4], idx) and out[3].shape == (256, 64)
        assert torch.equal(out[3].argmax(1), idx[0])
        # a codebook written in place re-keys the prepared images
        vq.residual_embeddings[0].weight.mul_(0.5)
        fresh = F.vq_residual_forward(z_e, [w.detach() for w in vq.codebooks()], 0.25, rowmajor=True, want_zq=False)[3]
        assert torch.equal(m.encode(x), fresh) and torch.equal(fresh[0], code[0]) and not torch.equal(fresh[1], code[1])


def test_model_training_step():
    from vqvae_amd import training as T
    m = _model(n_quantizers=3).train()
    vq = m.vector_quantization
    x = torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(2)).to(DEV)
    seen = {}

    def hook(mod, args, out):
        seen["z_e"] = args[0].detach().clone()
        seen["idx"] = out[4]
        out[0].register_hook(lambda g: seen.__setitem__("g_loss", g.detach().clone()))
        out[1].register_hook(lambda g: seen.__setitem__("g_zq", g.detach().clone()))

    h = vq.register_forward_hook(hook)
    el, x_hat, p = m(x)
    h.remove()
    assert p.dim() == 0
    T.step_losses(el, x_hat, p, x, 0.06)[1].backward()
    torch.cuda.synchronize()
    for name, prm in m.named_parameters():
        assert prm.grad is not None and torch.isfinite(prm.grad).all(), name
    assert seen["z_e"].shape == (4, 8, 8, 64) and seen["idx"].shape == (3, 256)
    books = [w.detach() for w in vq.codebooks()]
    _, want = T.vq_residual_backward(seen["z_e"], books, seen["idx"], seen["g_zq"], seen["g_loss"], 0.25, rowmajor=True, need_z=False)
    for w, g in zip(vq.codebooks(), want):
        assert np.array_equal(_bits(w.grad), _bits(g)) and float(g.abs().max()) > 0
    # shared: one codebook, one gradient
    s = _model(n_quantizers=3, shared_codebook=True).train()
    el, x_hat, p = s(x)
    T.step_losses(el, x_hat, p, x, 0.06)[1].backward()
    g = s.vector_quantization.embedding.weight.grad
    assert g is not None and torch.isfinite(g).all() and float(g.abs().max()) > 0
    assert s.encode(x).shape == (3, 256)


# ---- 7. init_codebook_ -----------------------------------------------------------------------------------------------------------------

def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


@pytest.mark.parametrize("rowmajor", [False, True])
def test_init_codebook_is_kmeans_stage_by_stage(rowmajor):
    from vqvae_amd import functional as F
    from vqvae_amd.modules import ResidualVectorQuantizer
    B, H, W, D, K, iters = 2, 8, 8, 64, 64, 2
    rows = np.random.default_rng(9).standard_normal((B * H * W, D)).astype(np.float32)
    z = _layout(rows, B, H, W, rowmajor)
    torch.manual_seed(3)
    vq = ResidualVectorQuantizer(3, K, D, 0.25).to(DEV)
    vq.quantize(z, rowmajor=rowmajor)                         # a warm module: prepared images of the old codebooks
    versions = [w._version for w in vq.codebooks()]
    out = vq.init_codebook_(z, iters, _gen(5), rowmajor=rowmajor)
    assert len(out) == 3 and all(w._version > v for w, v in zip(vq.codebooks(), versions))
    gen, r = _gen(5), z
    for q, w in enumerate(vq.codebooks()):
        want, counts = F.vq_kmeans(r, K, iters, generator=gen, rowmajor=rowmajor)
        assert np.array_equal(_bits(w), _bits(want)), f"stage {q}"
        assert torch.equal(out[q][1], counts)
        idx = F.vq_forward(r, want, 0.0, rowmajor=rowmajor, want_zq=False)[3].view(-1)
        e = want[idx].view(B, H, W, D)
        r = r - (e if rowmajor else e.permute(0, 3, 1, 2))
    # the module quantizes against the new codebooks
    got = vq.quantize(z, rowmajor=rowmajor)
    ref = F.vq_residual_forward(z, [w.detach() for w in vq.codebooks()], 0.25, rowmajor=rowmajor)
    assert torch.equal(got[3], ref[3]) and np.array_equal(_bits(got[1]), _bits(ref[1]))
    # shared: k-means of z only
    sh = ResidualVectorQuantizer(3, K, D, 0.25, shared_codebook=True).to(DEV)
    sh.init_codebook_(z, iters, _gen(6), rowmajor=rowmajor)
    want, _ = F.vq_kmeans(z, K, iters, generator=_gen(6), rowmajor=rowmajor)
    assert np.array_equal(_bits(sh.embedding.weight), _bits(want))


# ---- 8. stream capture -----------------------------------------------------------------------------------------------------------------

def test_forward_captures_into_a_graph_as_one_chain():
    from vqvae_amd import _lib, functional as F
    faulthandler.dump_traceback_later(120, exit=True)        # this test's own time limit: a replay that hangs ends the process
    try:
        _lib.load()
        _lib.profile_enable(False)
        rows, books, _ = _case(512, 64, 3, 8, 8, False)
        rows2 = np.random.default_rng(77).standard_normal(rows.shape).astype(np.float32)
        dbooks = _dev(books[:2])
        static_z = _layout(rows, 3, 8, 8, True)
        stream = torch.cuda.Stream(device=DEV)
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            ws = F.vq_residual_workspace(192, 512, 64, 2, DEV)
            F.vq_residual_forward(static_z, dbooks, BETA, rowmajor=True, workspace=ws, want_residual=True)     # prepares the images
        stream.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            out = F.vq_residual_forward(static_z, dbooks, BETA, rowmajor=True, workspace=ws, prepared=True, want_residual=True)
        static_z.copy_(_layout(rows2, 3, 8, 8, True))
        graph.replay()
        torch.cuda.synchronize()
        eager = F.vq_residual_forward(_layout(rows2, 3, 8, 8, True), dbooks, BETA, rowmajor=True, want_residual=True)
        torch.cuda.synchronize()
        for a, b in zip(out, eager):
            assert a.shape == b.shape and np.array_equal(_bits(a) if a.dtype == torch.float32 else a.cpu().numpy(),
                                                         _bits(b) if b.dtype == torch.float32 else b.cpu().numpy())
        _check_forward(out, R.chain(rows2, books[:2], BETA), True, 512, "graph replay")
    finally:
        faulthandler.cancel_dump_traceback_later()


def test_envelope_on_the_device():
    from vqvae_amd import _lib
    L = _lib.load()
    import ctypes
    z = torch.zeros(64 * 260, device=DEV)
    big = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    a, w = z.data_ptr(), big.data_ptr()
    books = (ctypes.c_void_p * 17)(*([a] * 17))
    for D, K, Q in ((257, 16, 2), (4, 16385, 2), (4, 16, 0), (4, 16, 17)):
        assert L.vqvae_vq_residual_workspace_bytes(64, K, D, Q, 0) == 0
        assert L.vqvae_vq_residual_forward_f32(a, books, 1, D, 8, 8, K, Q, 0.25, 0, a, w, w, w, w, w, None, w, big.numel(),
                                               None) == _lib.ERR_UNSUPPORTED
        assert L.vqvae_vq_residual_decode_f32(w, books, 1, D, 8, 8, K, Q, 0, a, None) == _lib.ERR_UNSUPPORTED
        assert L.vqvae_vq_residual_backward_f32(a, books, w, None, None, 1, D, 8, 8, K, Q, 0.25, 0, a, None, w, big.numel(),
                                                None) == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()
