"""Lookup-free quantization on the GPU: functional.lfq_forward / lfq_decode_indices, training.lfq_backward (vqvae_lfq_*_f32), the
LookupFreeQuantizer module and VQVAE(lookup_free=True) against the CPU restatement tests/vq_lfq_ref.py, whose arithmetic is the header
of vqvae_amd/csrc/vq_lfq.hip.

y is a chain of correctly rounded fp64 operations, so z_q, the decode, idx and hist are compared bit for bit on every row.  The losses,
avg and the gradients pass through exp, log and log1p, which the device does not guarantee to round correctly, and through sums whose
order differs from numpy's.  THE BOUNDS (tests/vq_lfq_ref.py: avg_bound, loss_bounds, e_bound; u = 2^-53, FN = 8 ulps allowed for one
device exp / log / log1p together with the one or two correctly rounded operations next to it):

  avg[k]   a sum of N positive terms, each a product of d probabilities.  A probability is exp, one addition and one division
           (<= FN u relative), the product of d of them <= FN d u relative; adding N terms in any order and dividing by N adds at most
           (N + 1) u times the sum of the terms, which is avg[k] itself:  |got - ref| <= (N + FN d + 16) u avg[k] + 2^-1000, the last
           term for products that reach the denormal range.  avg is fp64: no fp32 rounding.
  C, P     sums of N d non-negative terms (C: two exact-to-1-ulp operations a term; P: log1p, exp and three operations, <= 2 FN u),
           added over at most N + 1024 + d values (rows, partitions, channels): (N + 1024 + d + 16 + ..) u times the sum of the terms.
  H        K terms avg log avg.  The sum's order (256 strided sums, a tree) and log give (K / 256 + 8 + FN) u sum |avg log avg|; avg's
           own error moves a term by (|log avg| + 1) times avg's bound.
  loss     beta C + w_e (P - gamma H): the three bounds weighted, plus 4 u of each product.
           Each scalar is rounded to fp32 once: + 2^-23 |ref| (half an ulp is 2^-24 |ref|; an fp64 error that carries the value across
           a rounding boundary makes it one ulp), + 2^-149 where the value is below fp32's normal range.
  e_j      t1 = beta 2 (y - c) / (N d): four operations, 8 u |t1|.  t2 = w_e (s^2 / N) y p+ p-: two probabilities and four operations,
           3 FN u |t2|.  t3 = w_e gamma (s / N) p+ p- (T+ - T-): the same factor, 3 FN u |t3|, and T+-: K / 2 terms each of L[k] (a log:
           FN u) times at most d probabilities, added in another order: (K + FN d + 16) u sum_k |L[k]| prod, which the restatement
           returns as mag_T.  avg is an input of the backward and the same on both sides.
  grad_z   gy_j = gc_j + g e_j (gc_j has the restatement's bits: the same operations in the same order), so gy_j is off by g times e's
           bound plus 4 u (|gc_j| + |g e_j|); grad_z_c = sum_j W_in[j][c] gy_j adds (d + 2) u sum_j |W_in gy_j| and one fp32 rounding.
  grad_W_in, grad_b_in   sums over n of gy z (of gy): gy's bound times |z| summed, (N / 256 + 256 + 4) u sum |term| for the blocked
           order against numpy's, one fp32 rounding.  grad_W_out and grad_b_out involve no transcendental: compared bit for bit with
           the restatement's blocked sums.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import vq_lfq_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BETA, WE, GAMMA, INV_T, GL = 0.25, float(np.float32(0.1)), 0.5, 100.0, 0.75
KW = dict(beta=BETA, entropy_weight=WE, diversity_gamma=GAMMA, inv_temperature=INV_T)

# (B, H, W, D, d, scale of y): 1, 63, 65, 257 and 1025 rows (the wave, the 256-row block and the partition edges); D = 1, 7 (the element
# path), 64, 256 (four chunks); d = 1, 2, 9 (an odd split), 10; saturated rows (|s y| near 400: the library's temperature on y of unit
# scale) and rows on the soft part of the sigmoid; d = 16 at 300 rows, once at D = 64 and once at D = 68: the 16-wide code path with the
# large weight capacity (D > 64), a full chunk plus a ragged one of 4 channels, on the 16-byte path (68 % 4 == 0)
CASES = [(1, 1, 1, 64, 10, 0.02), (3, 3, 7, 7, 2, 0.02), (5, 13, 1, 1, 1, 0.02), (1, 257, 1, 256, 9, 0.02), (5, 5, 41, 64, 10, 1.0),
         (5, 5, 41, 7, 9, 0.02), (1, 257, 1, 64, 2, 0.005), (3, 10, 10, 64, 16, 0.01), (3, 10, 10, 68, 16, 0.01)]
FLAG = (5, 5, 41, 64, 10, 0.02)                                 # the other tests' case: 1025 rows, D = 64, K = 1024


def _dev(a, offset=False):
    """a numpy array on the device; offset: one element into a larger buffer, so that no 16-byte access path takes it"""
    t = torch.from_numpy(np.array(a, order="C"))               # (a copy: the cases' arrays are read-only)
    if not offset:
        return t.to(DEV)
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _layout(rows, B, H, W, rowmajor, offset=False):
    z = np.ascontiguousarray(rows).reshape(B, H, W, rows.shape[1])
    return _dev(z if rowmajor else z.transpose(0, 3, 1, 2), offset)


def _rows(t, rowmajor):
    t = t.detach().cpu()
    t = t if rowmajor else t.permute(0, 2, 3, 1)
    return np.ascontiguousarray(t.contiguous().numpy().reshape(-1, t.shape[-1]))


def _same_bits_nan_aside(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN positions"
    u = np.uint32 if got.dtype == np.float32 else np.uint64
    diff = got.view(u)[~gn] != want.view(u)[~wn]
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} elements differ in their bits"


@functools.lru_cache(maxsize=None)
def _case(B, H, W, D, d, scale):
    """inputs and the restatement (forward, losses, backward, parameter sums), computed once and left unchanged"""
    N = B * H * W
    inp = R.draw(N, D, d, 7000 + 13 * D + N + d, scale=scale)
    z, g, w_in, b_in, w_out, b_out = inp
    f = R.forward(z, w_in, b_in, w_out, b_out)
    ls = R.losses(f.y, BETA, WE, GAMMA, INV_T)
    r = R.backward(z, g, GL, ls.avg, w_in, b_in, w_out, BETA, WE, GAMMA, INV_T)
    pg, mags = R.param_grads(r)
    blocked = R.param_grads_blocked(r, ("w_out", "b_out"))
    st = R.backward(z, g, GL, None, w_in, b_in, w_out, BETA, WE, GAMMA, INV_T)
    for a in (*inp, f.idx, f.z_q, f.hist, ls.avg, r.grad_z, st.grad_z):
        a.setflags(write=False)
    return inp, f, ls, r, pg, mags, blocked, st


def _run(case, B, H, W, d, avg_ref, rowmajor, offset=False):
    """forward, decode of the forward's indices, and backward on the device -> dict of numpy arrays in row order"""
    from vqvae_amd import functional as F, training as T
    z, g, w_in, b_in, w_out, b_out = case
    K = 1 << d
    zt, gt = _layout(z, B, H, W, rowmajor, offset), _layout(g, B, H, W, rowmajor, offset)
    p = [_dev(a, offset) for a in (w_in, b_in, w_out, b_out)]
    gl, avg_in = torch.tensor(GL, dtype=torch.float32, device=DEV), _dev(avg_ref)
    z_q, ppl, idx, hist, losses, avg = F.lfq_forward(zt, *p, K, rowmajor=rowmajor, **KW)
    idx_only = F.lfq_forward(zt, *p, K, rowmajor=rowmajor, want_zq=False, want_hist=False, want_loss=False, **KW)
    assert all(idx_only[i] is None for i in (0, 1, 3, 4, 5))
    dec = F.lfq_decode_indices(idx, p[2], p[3], K, B, H, W, rowmajor=rowmajor)
    gz, gp = T.lfq_backward(zt, gt, gl, avg_in, p[0], p[1], p[2], K, rowmajor=rowmajor, **KW)
    gz_alone, none = T.lfq_backward(zt, gt, gl, avg_in, p[0], p[1], p[2], K, rowmajor=rowmajor, need_params=False, **KW)
    assert none is None
    gz_st, _ = T.lfq_backward(zt, gt, None, None, p[0], p[1], p[2], K, rowmajor=rowmajor, need_params=False, **KW)
    gz_loss, gp_loss = T.lfq_backward(zt, None, gl, avg_in, p[0], p[1], p[2], K, rowmajor=rowmajor, **KW)
    torch.cuda.synchronize()
    assert idx.shape == (B * H * W, 1) and z_q.shape == zt.shape and dec.shape == zt.shape and gz.shape == zt.shape
    assert losses.shape == (4,) and avg.shape == (K,) and avg.dtype == torch.float64
    return dict(z_q=_rows(z_q, rowmajor), ppl=np.float32(ppl.item()), idx=idx.view(-1).cpu().numpy(), idx_only=idx_only[2].view(-1).cpu().numpy(),
                hist=hist.cpu().numpy(), losses=losses.cpu().numpy(), avg=avg.cpu().numpy(), dec=_rows(dec, rowmajor),
                grad_z=_rows(gz, rowmajor), gz_alone=_rows(gz_alone, rowmajor), gz_st=_rows(gz_st, rowmajor), gz_loss=_rows(gz_loss, rowmajor),
                w_in=gp[0].cpu().numpy(), b_in=gp[1].cpu().numpy(), w_out=gp[2].cpu().numpy(), b_out=gp[3].cpu().numpy(),
                w_out_loss=gp_loss[2].cpu().numpy(), b_out_loss=gp_loss[3].cpu().numpy())


FLOATS = ("z_q", "losses", "avg", "dec", "grad_z", "gz_alone", "gz_st", "gz_loss", "w_in", "b_in", "w_out", "b_out")


def _same_run(a, b, what):
    assert np.array_equal(a["idx"], b["idx"]) and np.array_equal(a["hist"], b["hist"]) and a["ppl"].tobytes() == b["ppl"].tobytes(), what
    for n in FLOATS:
        _same_bits_nan_aside(a[n], b[n], f"{what}: {n}")


@pytest.mark.parametrize("B,H,W,D,d,scale", CASES)
def test_against_the_restatement_in_both_layouts_and_on_both_paths(B, H, W, D, d, scale):
    case, f, ls, r, pg, mags, blocked, st = _case(B, H, W, D, d, scale)
    N, K = B * H * W, 1 << d
    if N >= 64:
        assert len(np.unique(f.idx)) > 1                        # more than one code is in use on the seeded inputs
    runs = {(rm, off): _run(case, B, H, W, d, ls.avg, rm, off) for rm in (True, False) for off in (False, True)}
    got = runs[(True, False)]
    # the same bits in both layouts and on both access paths
    for key, other in runs.items():
        _same_run(other, got, f"run {key} against the aligned row-major run")
    # exact: every row's index, the histogram, z_q and the decode
    assert np.array_equal(got["idx"], f.idx) and np.array_equal(got["idx_only"], f.idx) and np.array_equal(got["hist"], f.hist)
    _same_bits_nan_aside(got["z_q"], f.z_q, "z_q")
    _same_bits_nan_aside(got["dec"], f.z_q, "decode")
    assert abs(float(got["ppl"]) - float(f.perplexity)) <= 2.0 ** -22 * float(f.perplexity)
    # avg (fp64) and the four scalars
    print(f"avg: max |got - ref| / bound = {(np.abs(got['avg'] - ls.avg) / R.avg_bound(ls, N, d)).max():.3g}; sum = {got['avg'].sum()!r}")
    assert (np.abs(got["avg"] - ls.avg) <= R.avg_bound(ls, N, d)).all()
    ref = np.array([ls.loss, ls.C, ls.P, ls.H])
    bound = np.array(R.loss_bounds(ls, N, d, K, BETA, WE, GAMMA)) + 2.0 ** -23 * np.abs(ref) + 2.0 ** -149
    print(f"losses: got {got['losses']!r} ref {ref!r} bound {bound!r}")
    assert (np.abs(got["losses"].astype(np.float64) - ref) <= bound).all()
    # the gradients
    be = R.e_bound(r.lg, K, d, WE, GAMMA, 4.0 * INV_T, N)
    bgy = GL * be + 4 * R.U * (np.abs(r.gc) + np.abs(GL * r.lg.e))
    w_abs, z_abs = np.abs(case[2].astype(np.float64)), np.abs(case[0].astype(np.float64))
    b_gz = 2.0 ** -23 * np.abs(r.grad_z.astype(np.float64)) + bgy @ w_abs + (d + 2) * R.U * r.mag_gz + 2.0 ** -149
    err = np.abs(got["grad_z"].astype(np.float64) - r.grad_z)
    print(f"grad_z: max |got - ref| / bound = {(err / b_gz).max():.3g}")
    assert (err <= b_gz).all()
    _same_bits_nan_aside(got["gz_alone"], got["grad_z"], "grad_z without the parameter gradients")
    _same_bits_nan_aside(got["gz_st"], st.grad_z, "grad_z of z_q alone (no loss gradient): exact")
    n_add = N / 256 + 256 + 4
    for n, extra in (("w_in", bgy.T @ z_abs), ("b_in", bgy.sum(0))):
        want = pg[n].astype(np.float64)
        b = 2.0 ** -23 * np.abs(want) + n_add * R.U * mags[n] + extra + 2.0 ** -149
        print(f"grad_{n}: max |got - ref| / bound = {(np.abs(got[n] - want) / b).max():.3g}")
        assert (np.abs(got[n] - want) <= b).all(), n
    for n in ("w_out", "b_out"):
        _same_bits_nan_aside(got[n], blocked[n], f"grad_{n}")
        assert not got[n + "_loss"].any(), f"grad_{n} without grad_zq must be zero"
    # the loss's gradient alone is the difference's source: grad_z(z_q and loss) - grad_z(z_q) ~ grad_z(loss)
    lone = (got["gz_loss"].astype(np.float64) - (r.gy - r.gc) @ case[2].astype(np.float64))
    assert (np.abs(lone) <= 2.0 ** -23 * np.abs(got["gz_loss"]) + bgy @ w_abs + (d + 2) * R.U * (np.abs(r.gy - r.gc) @ w_abs) + 2.0 ** -149).all()


def test_two_runs_and_a_graph_replay_have_the_same_bits():
    """a linear chain on one stream: forward (its histogram cleared by the chain itself), decode, backward; run twice, then captured
    and replayed on new inputs, with other values left in the outputs between the replays"""
    from vqvae_amd import functional as F, training as T
    B, H, W, D, d, scale = FLAG
    K = 1 << d
    case, f, ls, r, pg, mags, blocked, st = _case(*FLAG)
    for rowmajor in (True, False):
        want = _run(case, B, H, W, d, ls.avg, rowmajor)
        _same_run(_run(case, B, H, W, d, ls.avg, rowmajor), want, "second run")
        zs, gs = torch.zeros_like(_layout(case[0], B, H, W, rowmajor)), torch.zeros_like(_layout(case[1], B, H, W, rowmajor))
        p = [_dev(a) for a in case[2:]]
        gl, avg_in = torch.tensor(GL, dtype=torch.float32, device=DEV), _dev(ls.avg)
        ws = F.lfq_workspace(B * H * W, D, d, DEV)

        def chain():
            z_q, ppl, idx, hist, losses, avg = F.lfq_forward(zs, *p, K, rowmajor=rowmajor, workspace=ws, **KW)
            dec = F.lfq_decode_indices(idx, p[2], p[3], K, B, H, W, rowmajor=rowmajor)
            gz, gp = T.lfq_backward(zs, gs, gl, avg_in, p[0], p[1], p[2], K, rowmajor=rowmajor, workspace=ws, **KW)
            gz_st, _ = T.lfq_backward(zs, gs, None, None, p[0], p[1], p[2], K, rowmajor=rowmajor, need_params=False, workspace=ws, **KW)
            gz_loss, _ = T.lfq_backward(zs, None, gl, avg_in, p[0], p[1], p[2], K, rowmajor=rowmajor, need_params=False, workspace=ws, **KW)
            return z_q, ppl, idx, hist, losses, avg, dec, gz, gp, gz_st, gz_loss

        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            chain()
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            z_q, ppl, idx, hist, losses, avg, dec, gz, gp, gz_st, gz_loss = chain()
        zs.copy_(_layout(case[0], B, H, W, rowmajor))
        gs.copy_(_layout(case[1], B, H, W, rowmajor))
        for i in range(2):
            graph.replay()
            torch.cuda.synchronize()
            got = dict(z_q=_rows(z_q, rowmajor), ppl=np.float32(ppl.item()), idx=idx.view(-1).cpu().numpy(), hist=hist.cpu().numpy(),
                       losses=losses.cpu().numpy(), avg=avg.cpu().numpy(), dec=_rows(dec, rowmajor), grad_z=_rows(gz, rowmajor),
                       gz_alone=_rows(gz, rowmajor), gz_st=_rows(gz_st, rowmajor), gz_loss=_rows(gz_loss, rowmajor),
                       w_in=gp[0].cpu().numpy(), b_in=gp[1].cpu().numpy(), w_out=gp[2].cpu().numpy(), b_out=gp[3].cpu().numpy())
            _same_run(got, want, f"replay {i} rowmajor={rowmajor}")
            hist.fill_(1000)
            ppl.fill_(-1.0)
            z_q.fill_(7.0)
            losses.fill_(3.0)
            avg.fill_(0.5)
            ws.fill_(0xFF)


@pytest.mark.parametrize("rowmajor", [True, False])
def test_out_of_range_indices_decode_to_nan_rows(rowmajor):
    from vqvae_amd import functional as F
    B, H, W, D, d, scale = FLAG
    K = 1 << d
    case, f = _case(*FLAG)[:2]
    idx = f.idx.copy()
    bad = [0, 255, 256, 700, 1024]
    idx[bad] = [-1, K, 1 << 40, -(1 << 40), K + 5]
    w_out, b_out = _dev(case[4]), _dev(case[5])
    with pytest.raises(IndexError):
        F.lfq_decode_indices(_dev(idx), w_out, b_out, K, B, H, W, rowmajor=rowmajor)
    dec = _rows(F.lfq_decode_indices(_dev(idx), w_out, b_out, K, B, H, W, rowmajor=rowmajor, validate=False), rowmajor)
    assert np.isnan(dec[bad]).all()
    _same_bits_nan_aside(dec, R.decode(idx, case[4], case[5], d), "decode with bad indices")


@pytest.mark.parametrize("rowmajor", [True, False])
def test_a_nan_stays_in_its_row(rowmajor):
    """one NaN element in row 300 of z: that row of z_q and of grad_z is NaN, every other row has the bits of the clean batch (avg is
    an input of the backward: the clean batch's).  The scalar losses of such a batch are unspecified."""
    from vqvae_amd import functional as F, training as T
    B, H, W, D, d, scale = FLAG
    K = 1 << d
    case, f, ls, r = _case(*FLAG)[:4]
    z = case[0].copy()
    z[300, 17] = np.nan
    zt, gt = _layout(z, B, H, W, rowmajor), _layout(case[1], B, H, W, rowmajor)
    p = [_dev(a) for a in case[2:]]
    clean = _run(case, B, H, W, d, ls.avg, rowmajor)
    z_q, ppl, idx, hist, losses, avg = F.lfq_forward(zt, *p, K, rowmajor=rowmajor, **KW)
    gz, _ = T.lfq_backward(zt, gt, torch.tensor(GL, device=DEV), _dev(ls.avg), p[0], p[1], p[2], K, rowmajor=rowmajor, **KW)
    torch.cuda.synchronize()
    z_q, gz, idx = _rows(z_q, rowmajor), _rows(gz, rowmajor), idx.view(-1).cpu().numpy()
    others = np.arange(B * H * W) != 300
    assert np.isnan(z_q[300]).all() and np.isnan(gz[300]).all() and idx[300] == 0
    assert np.isfinite(z_q[others]).all() and np.isfinite(gz[others]).all()
    _same_bits_nan_aside(z_q[others], clean["z_q"][others], "the other rows of z_q")
    _same_bits_nan_aside(gz[others], clean["grad_z"][others], "the other rows of grad_z")
    assert np.array_equal(idx[others], f.idx[others])


def test_module_against_the_restatement():
    from vqvae_amd.modules import LazyOneHot, LookupFreeQuantizer
    B, H, W, D, d, scale = FLAG
    K = 1 << d
    case, f, ls, r, pg, mags, blocked, st = _case(*FLAG)
    q = LookupFreeQuantizer(K, D, BETA, entropy_weight=WE, diversity_gamma=GAMMA, inv_temperature=INV_T).to(DEV)
    with torch.no_grad():
        for p, a in zip(q._params(), case[2:]):
            p.copy_(_dev(a))
        loss, z_q, ppl, onehot, idx = q(_layout(case[0], B, H, W, False))
        assert isinstance(onehot, LazyOneHot) and onehot.shape == (B * H * W, K) and loss.dim() == 0
        assert abs(float(loss) - ls.loss) <= 1e-6 * abs(ls.loss) and torch.equal(q.last_losses[0], loss)
        _same_bits_nan_aside(_rows(z_q, False), f.z_q, "module z_q")
        assert np.array_equal(idx.view(-1).cpu().numpy(), f.idx)
        assert torch.equal(q.codes().cpu(), torch.from_numpy(R.all_codes(d)))
        _same_bits_nan_aside(q.codebook().cpu().numpy(), R.decode(np.arange(K), case[4], case[5], d), "codebook()")
    z = _layout(case[0], B, H, W, True).requires_grad_(True)
    loss, z_q, ppl, idx, hist = q.quantize(z, rowmajor=True)
    assert z_q.requires_grad and loss.requires_grad and not idx.requires_grad and not hist.requires_grad and not ppl.requires_grad
    assert not q.last_losses.requires_grad
    ((z_q * _layout(case[1], B, H, W, True)).sum() + GL * loss).backward()
    np.testing.assert_allclose(_rows(z.grad, True), r.grad_z, rtol=1e-5, atol=1e-6)
    for n, p in zip(("w_in", "b_in", "w_out", "b_out"), q._params()):
        np.testing.assert_allclose(p.grad.cpu().numpy(), pg[n], rtol=1e-5, atol=1e-6 * float(np.abs(pg[n]).max()), err_msg=n)


def _model(**kw):
    from vqvae_amd import conv
    from vqvae_amd.modules import VQVAE
    conv.set_conv_backend("hip")
    torch.manual_seed(0)
    return VQVAE(16, 8, 1, 64, 16, 0.25, lookup_free=True, **kw).to(DEV)


def _x(B=2):
    return torch.randn(B, 3, 32, 32, generator=torch.Generator().manual_seed(1)).to(DEV)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def test_model_decode_indices_of_encode_equals_the_forward():
    m, x = _model().eval(), _x()
    with torch.no_grad():
        loss, x_hat, ppl = m(x)
        idx = m.encode(x)
        dec = m.decode_indices(idx, 2, 8, 8)
    assert loss.dim() == 0 and np.isfinite(float(loss)) and float(loss) != 0.0            # the loss is computed in eval mode too
    assert x_hat.shape == x.shape and float(ppl) >= 1.0
    assert idx.shape == (128, 1) and int(idx.min()) >= 0 and int(idx.max()) < 64
    assert np.array_equal(_bits(dec), _bits(x_hat))
    with pytest.raises(IndexError):
        m.decode_indices(torch.full_like(idx, 64), 2, 8, 8)


def test_model_training_step_moves_every_projection_tensor():
    from vqvae_amd import training as T
    m, x = _model().train(), _x()
    vq = m.vector_quantization
    before = [p.detach().clone() for p in vq._params()]
    opt = torch.optim.Adam(m.parameters(), lr=2e-3)
    opt.zero_grad(set_to_none=True)
    el, xh, pp = m(x)
    assert el.requires_grad and vq.last_losses.shape == (4,)
    stats = T.step_losses(el, xh, pp, x, 0.06)
    stats[1].backward()
    for p in m.parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all())
    opt.step()
    for b, p in zip(before, vq._params()):
        assert not torch.equal(b, p.detach())
    assert [k for k in m.state_dict() if k.startswith("vector_quantization.")] == [
        "vector_quantization.project_in.weight", "vector_quantization.project_in.bias",
        "vector_quantization.project_out.weight", "vector_quantization.project_out.bias"]


def test_sample_images_with_a_tiny_prior():
    from vqvae_amd.pixelcnn import GatedPixelCNN, sample_images
    m = _model().eval()
    torch.manual_seed(3)
    prior = GatedPixelCNN(64, 16, 3, 10).eval().to(DEV)
    gen = torch.Generator().manual_seed(4)
    label = torch.randint(0, 10, (2,), generator=gen).to(DEV)
    u = torch.rand((2, 8, 8), generator=gen).to(DEV)
    idx, x_hat = sample_images(prior, m, label, (8, 8), 2, uniforms=u)
    assert idx.shape == (2, 8, 8) and x_hat.shape == (2, 3, 32, 32) and int(idx.min()) >= 0 and int(idx.max()) < 64
    with torch.no_grad():
        assert np.array_equal(_bits(x_hat), _bits(m.decode_indices(idx, 2, 8, 8)))
    assert bool(torch.isfinite(x_hat).all())


def test_train_tool_completes_a_run(tmp_path):
    """tools/train_checkpoint.py --lookup_free in a child process: three updates of a small model, the log lines, the checkpoint and
    the evaluation through the per-layer path"""
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train_checkpoint.py"), "--lookup_free", "--lfq_entropy_weight", "0.2",
           "--n_updates", "3", "--batch_size", "8", "--n_train", "64", "--log_interval", "2", "--n_hiddens", "16", "--n_residual_hiddens", "8",
           "--n_residual_layers", "1", "--embedding_dim", "16", "--n_embeddings", "64", "--out", str(tmp_path), "--tag", "t"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    log = open(tmp_path / "t_log.txt").read()
    assert log.count("Update # ") == 2 and "guard: per-layer path" in log
    assert "# eval[per-layer]" in log and "decode_indices(encode(x)) is x_hat: True" in log
    ck = torch.load(tmp_path / "t.pth", weights_only=False)
    assert ck["hyperparameters"]["lookup_free"] is True and ck["hyperparameters"]["lfq_entropy_weight"] == 0.2
    assert len(ck["results"]["loss_vals"]) == 3 and all(np.isfinite(ck["results"]["loss_vals"]))
    assert tuple(ck["model"]["vector_quantization.project_in.weight"].shape) == (6, 16)
