"""The code-entropy loss on the GPU: functional.vq_entropy_forward / vq_entropy_backward (vqvae_vq_entropy_*_f32), training.
CodeEntropyLoss, the quantizer modules' entropy_weight option and VQVAE(entropy_weight=) against the CPU restatement
tests/vq_entropy_ref.py, whose arithmetic is the header of vqvae_amd/csrc/vq_entropy.hip.

Every output passes through exp and log, which the device does not guarantee to round correctly, and through sums whose order differs
from numpy's: the comparison is by THE BOUNDS below (tests/vq_entropy_ref.py: fwd_bounds, bwd_bounds, f32_round).  u = 2^-53; FN = 8
ulps are allowed for one device exp / log together with the correctly rounded operations next to it.  Each bound is derived for one
side and used twice (SIDES = 2): the restatement's numpy sums and libm calls carry an error of the same form.  s = inv_temperature.

  l_nk     zz, ee and dot are sums of D exact products, added with one rounding each in some order: D u sum |products| each, and
           sum_c |z_c e_kc| <= (zz + ee) / 2.  With the two additions and the two multiplications:
           |dl_nk| <= (2 D + 8) u s (zz_n + ee_k + 2 sum_c |z_c e_kc|) <= el_n := (2 D + 8) u 2 s (zz_n + max_k ee_k), absolute.
  S_n      sum_k e^x, x = l - max <= 0.  dx <= 2 el_n + u |x|; a term's relative error is FN u + dx; the u |x| part sums to
           u sum p |x| = u (H_n - log S) <= u log K; K additions.  Relative: eps_n := 3 el_n + (FN + K + 12) u (one el_n to spare).
  lse_n    max + log S: the maximum's el_n (inside eps_n), S's eps_n, the log and the addition: eps_n + (FN + 2) u (|lse_n| + log K).
  H_n      log S - T / S, T = sum e^x x, X := T / S in [-log K, 0].  T's terms carry (FN + 2) u + dx relative and e^x dx absolute, K
           additions, the division by S its eps_n: |dH_n| <= (1 + |X|)(eps_n + 2 el_n) + |X| (FN + K + 4) u + FN u log K + ..
           <= 4 (1 + log K) eps_n.
  P        the mean of H_n: the mean of their bounds, and N + 16 additions of non-negative terms in any order: (N + 16) u P.
  avg_k    p_nk = exp(l - lse): relative el_n + lse's bound + (FN + 2) u, and u |l - lse| p = u p |log p| absolute; N additions of
           non-negative terms and the division: (N + 2) u avg_k; + 2^-1000 for terms in the denormal range.  avg is fp64.
  H        K terms avg log avg: a term moves by (|log avg| + 1) times avg's bound; the sum's order and the log:
           (K + FN + 8) u sum |avg log avg|.
  term     P - gamma H: the two bounds weighted, 4 u (|P| + |gamma H|).
  losses   each scalar is rounded to fp32 once: + 2^-23 |ref| (an fp64 error that carries the value across a rounding boundary makes
           the half ulp a whole one) + 2^-149.

  The backward reads the restatement's avg and rowstat: they are the same on both sides.
  L_k      one log: FN u |L_k|.        p_nk, log p_nk = l - lse: dp <= p (el_n + (FN + 1) u) + u p |log p|;  dlogp <= el_n + u |log p|.
  M_n      sum_k p L: (el_n + (2 FN + K + 8) u) sum_k p |L_k| + u max |L| H_n   (sum_k p |log p| = H_n).
  a_nk     (g / N) p br, br = -(log p + H_n) + gamma (L_k - M_n):
           dbr <= el_n + 3 u |log p| + 2 u H_n + |gamma| ((FN + 2) u |L_k| + dM_n + 2 u |M_n|) + 2 u |br|;
           da <= (|g| / N)(dp |br| + p dbr) + 4 u |a|.
  grad_z   -2 s (z_c A_n - G_nc), A_n = sum_k a_nk, G_nc = sum_k a_nk e_kc -- the contract's sum_k a_nk (z_c - e_kc) grouped as two
           contractions, so the magnitudes are |a| (|z_c| + |e_kc|): 2 s sum_k (da + (K + 4) u |a|)(|z_c| + |e_kc|), one fp32 rounding.
  grad_E   2 s (sum_n a_nk z_nc - e_kc sum_n a_nk): 2 s sum_n (da + (N + 4) u |a|)(|z_nc| + |e_kc|), one fp32 rounding.

Between the two layouts, the aligned and the 4-byte-offset pointers, two runs, and an eager call and a graph replay every output has
the same bits.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import vq_entropy_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, GAMMA, GL = 100.0, 0.5, 0.75

# (B, H, W, D, K, regime): 1, 63, 257 and 1025 rows (the wave, the block of 256 rows and the partition edges); D = 1, 7, 64, 68 (the
# 128-wide class, one chunk ragged), 256 (sixteen chunks); K = 1, 2, 5, 96, 512 and 65 (one past the tile of 64 codes)
CASES = [(1, 1, 1, 64, 512, "soft"), (3, 3, 7, 7, 2, "soft"), (1, 257, 1, 256, 5, "saturated"), (1, 257, 1, 1, 1, "soft"),
         (3, 3, 7, 68, 96, "saturated"), (1, 257, 1, 64, 65, "onehot"), (5, 5, 41, 7, 96, "saturated"), (1, 63, 1, 1, 5, "soft"),
         # partitions of more than one block of 256 rows: avg's at 259 blocks (256 partitions at most), grad_E's at K D = 2^20 (4)
         (1, 257, 257, 7, 5, "soft"), (5, 5, 41, 256, 4096, "saturated")]
FLAG = (5, 5, 41, 64, 512, "soft")                                  # 1025 rows, D = 64, K = 512
NAMES = ("losses", "avg", "rowstat", "grad_z", "grad_E")


def _dev(a, offset=False):
    """a numpy array on the device; offset: one fp32 element (4 bytes) into a larger 16-byte aligned buffer"""
    t = torch.from_numpy(np.array(a, order="C"))
    if not offset:
        return t.to(DEV)
    assert t.dtype == torch.float32
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


@functools.lru_cache(maxsize=None)
def _case(B, H, W, D, K, regime):
    """inputs, the restatement and the bounds, computed once and left unchanged"""
    N = B * H * W
    z, E = R.draw(N, D, K, 7000 + 13 * D + N + K, regime)
    f = R.forward(z, E, S, GAMMA)
    r = R.backward(z, E, f.avg, f.rowstat, GL, S, GAMMA)
    fb = R.fwd_bounds(f, N, K, D, S, GAMMA)
    b_gz, b_gE = R.bwd_bounds(r, f, z, E, GL, S, GAMMA)
    ref_l = np.array([f.term, f.P, f.H])
    ref = dict(losses=ref_l, avg=f.avg, rowstat=f.rowstat, grad_z=r.grad_z64, grad_E=r.grad_E64)
    bound = dict(losses=R.SIDES * np.array([fb["term"], fb["P"], fb["H"]]) + R.f32_round(ref_l), avg=R.SIDES * fb["avg"],
                 rowstat=R.SIDES * np.stack([fb["lse"], fb["Hn"]], 1), grad_z=R.SIDES * b_gz + R.f32_round(r.grad_z64),
                 grad_E=R.SIDES * b_gE + R.f32_round(r.grad_E64))
    for a in (z, E, *ref.values(), *bound.values()):
        a.setflags(write=False)
    return z, E, ref, bound


def _run(case, B, H, W, rowmajor, offset=False, ws=None):
    """forward, then backward from the RESTATEMENT's avg and rowstat, on the device -> dict of numpy arrays, gradients in row order"""
    from vqvae_amd import functional as F
    z, E, ref, _ = case
    zt, Et = _layout(z, B, H, W, rowmajor, offset), _dev(E, offset)
    gl = torch.tensor(GL, dtype=torch.float32, device=DEV)
    kw = dict(inv_temperature=S, gamma=GAMMA, rowmajor=rowmajor, workspace=ws)
    losses, avg, rowstat = F.vq_entropy_forward(zt, Et, **kw)
    gz, gE = F.vq_entropy_backward(zt, Et, _dev(ref["avg"]), _dev(ref["rowstat"]), gl, **kw)
    torch.cuda.synchronize()
    assert losses.shape == (3,) and avg.shape == (E.shape[0],) and rowstat.shape == (z.shape[0], 2) and gz.shape == zt.shape
    return dict(losses=losses.cpu().numpy(), avg=avg.cpu().numpy(), rowstat=rowstat.cpu().numpy(), grad_z=_rows(gz, rowmajor),
                grad_E=gE.cpu().numpy())


def _same(a, b, what):
    for n in NAMES:
        assert a[n].dtype == b[n].dtype and a[n].tobytes() == b[n].tobytes(), f"{what}: {n} differs in its bits"


def _within(got, case, what):
    _, _, ref, bound = case
    for n in NAMES:
        err = np.abs(got[n].astype(np.float64) - ref[n])
        print(f"{what} {n}: max |got - ref| / bound = {(err / bound[n]).max():.3g}")
        assert np.isfinite(got[n]).all() and (err <= bound[n]).all(), f"{what}: {n}"


@pytest.mark.parametrize("B,H,W,D,K,regime", CASES + [FLAG])
def test_against_the_restatement_in_both_layouts_aligned_and_offset(B, H, W, D, K, regime):
    case = _case(B, H, W, D, K, regime)
    if regime == "soft" and K >= 5:
        assert (R.forward(case[0], case[1], S, GAMMA).p > 0.1 / K).sum(1).min() >= 3      # several codes carry mass in every row
    runs = {(rm, off): _run(case, B, H, W, rm, off) for rm in (True, False) for off in (False, True)}
    got = runs[(True, False)]
    for key, other in runs.items():
        _same(other, got, f"run {key} against the aligned row-major run")
    _within(got, case, f"{(B * H * W, D, K, regime)}")


def test_two_runs_and_a_graph_replay_have_the_same_bits():
    """both chains are linear chains of launches on one stream: run twice, then captured and replayed on new inputs, with other
    values left in the outputs and in the workspace between the replays"""
    from vqvae_amd import functional as F
    B, H, W, D, K, regime = FLAG
    case = _case(*FLAG)
    z, E, ref, _ = case
    N = B * H * W
    for rowmajor in (True, False):
        ws = F.vq_entropy_workspace(N, K, D, DEV)
        want = _run(case, B, H, W, rowmajor, ws=ws)
        ws.fill_(7)
        _same(_run(case, B, H, W, rowmajor, ws=ws), want, "second run")
        zt, Et = torch.zeros_like(_layout(z, B, H, W, rowmajor)), torch.zeros_like(_dev(E))
        avg_in, rs_in = torch.ones(K, dtype=torch.float64, device=DEV), torch.zeros(N, 2, dtype=torch.float64, device=DEV)
        gl = torch.tensor(GL, dtype=torch.float32, device=DEV)
        kw = dict(inv_temperature=S, gamma=GAMMA, rowmajor=rowmajor, workspace=ws)

        def chain():
            losses, avg, rowstat = F.vq_entropy_forward(zt, Et, **kw)
            gz, gE = F.vq_entropy_backward(zt, Et, avg_in, rs_in, gl, **kw)
            return losses, avg, rowstat, gz, gE

        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            chain()
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = chain()
        zt.copy_(_layout(z, B, H, W, rowmajor))
        Et.copy_(_dev(E))
        avg_in.copy_(_dev(ref["avg"]))
        rs_in.copy_(_dev(ref["rowstat"]))
        for i in range(2):
            graph.replay()
            torch.cuda.synchronize()
            got = dict(losses=outs[0].cpu().numpy(), avg=outs[1].cpu().numpy(), rowstat=outs[2].cpu().numpy(),
                       grad_z=_rows(outs[3], rowmajor), grad_E=outs[4].cpu().numpy())
            _same(got, want, f"replay {i}")
            for o in outs:
                o.fill_(7)
            ws.fill_(7)


def test_argument_combinations():
    from vqvae_amd import functional as F
    B, H, W, D, K, regime = CASES[4]
    case = _case(*CASES[4])
    z, E, ref, _ = case
    for rowmajor in (True, False):
        want = _run(case, B, H, W, rowmajor)
        zt, Et = _layout(z, B, H, W, rowmajor), _dev(E)
        avg_in, rs_in = _dev(ref["avg"]), _dev(ref["rowstat"])
        gl = torch.tensor(GL, dtype=torch.float32, device=DEV)
        kw = dict(inv_temperature=S, gamma=GAMMA, rowmajor=rowmajor)
        losses, avg, none = F.vq_entropy_forward(zt, Et, want_saved=False, **kw)                  # rowstat NULL
        assert none is None and losses.cpu().numpy().tobytes() == want["losses"].tobytes()
        assert avg.cpu().numpy().tobytes() == want["avg"].tobytes()
        gz, none = F.vq_entropy_backward(zt, Et, avg_in, rs_in, gl, want=(True, False), **kw)     # only grad_z
        assert none is None and _rows(gz, rowmajor).tobytes() == want["grad_z"].tobytes()
        none, gE = F.vq_entropy_backward(zt, Et, avg_in, rs_in, gl, want=(False, True), **kw)     # only grad_codebook
        assert none is None and gE.cpu().numpy().tobytes() == want["grad_E"].tobytes()
        one = torch.tensor(1.0, dtype=torch.float32, device=DEV)                                   # grad_loss NULL is grad_loss = 1
        a, b = F.vq_entropy_backward(zt, Et, avg_in, rs_in, None, **kw), F.vq_entropy_backward(zt, Et, avg_in, rs_in, one, **kw)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and not torch.equal(a[0], gz)
        with pytest.raises(ValueError):
            F.vq_entropy_backward(zt, Et, avg_in, rs_in, gl, want=(False, False), **kw)


def test_envelope_and_alias_errors_come_back_without_a_launch():
    from vqvae_amd import _lib, functional as F
    L = _lib.load()
    N, D, K = 6, 3, 5
    z, E = torch.full((N, D), 0.5, device=DEV), torch.full((K, D), 0.25, device=DEV)
    losses, avg = torch.full((3,), 7.0, device=DEV), torch.full((K,), 7.0, dtype=torch.float64, device=DEV)
    rs = torch.full((N, 2), 7.0, dtype=torch.float64, device=DEV)
    gz, gE = torch.full((N, D), 7.0, device=DEV), torch.full((K, D), 7.0, device=DEV)
    ws = F.vq_entropy_workspace(N, K, D, DEV)
    ws.fill_(7)
    st = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    UNSUPPORTED, WORKSPACE, NULL = -3, -4, -1

    def fw(K_=K, D_=D, s=100.0, gamma=1.0, flags=1, z_=p(z), losses_=p(losses), avg_=p(avg), rs_=p(rs), ws_=p(ws), n=ws.numel()):
        return L.vqvae_vq_entropy_forward_f32(z_, p(E), N, D_, 1, 1, K_, s, gamma, flags, losses_, avg_, rs_, ws_, n, st)

    def bw(K_=K, D_=D, s=100.0, gamma=1.0, flags=1, gz_=p(gz), gE_=p(gE), avg_=p(avg), ws_=p(ws), n=ws.numel()):
        return L.vqvae_vq_entropy_backward_f32(p(z), p(E), avg_, p(rs), None, N, D_, 1, 1, K_, s, gamma, flags, gz_, gE_, ws_, n, st)

    for call in (fw, bw):
        assert call(K_=16385) == UNSUPPORTED and call(K_=0) == UNSUPPORTED and call(D_=257) == UNSUPPORTED and call(D_=0) == UNSUPPORTED
        assert call(s=0.0) == UNSUPPORTED and call(s=-1.0) == UNSUPPORTED and call(s=float("inf")) == UNSUPPORTED
        assert call(s=float("nan")) == UNSUPPORTED and call(gamma=float("nan")) == UNSUPPORTED and call(gamma=float("inf")) == UNSUPPORTED
        assert call(flags=2) == UNSUPPORTED and call(ws_=None) == WORKSPACE and call(n=ws.numel() - 8) == WORKSPACE
        assert call(ws_=p(ws) + 4) == UNSUPPORTED and call(avg_=p(avg) + 4) == UNSUPPORTED
    assert fw(z_=p(z) + 2) == UNSUPPORTED and fw(losses_=p(z)) == UNSUPPORTED and fw(rs_=p(avg)) == UNSUPPORTED
    assert fw(losses_=None) == NULL and fw(avg_=None) == NULL
    assert bw(gz_=p(z)) == UNSUPPORTED and bw(gE_=p(E)) == UNSUPPORTED and bw(gE_=p(gz)) == UNSUPPORTED and bw(gz_=None, gE_=None) == NULL
    assert L.vqvae_vq_entropy_workspace_bytes(N, 16385, D) == 0 and L.vqvae_vq_entropy_workspace_bytes(N, K, 257) == 0
    assert L.vqvae_vq_entropy_workspace_bytes(2 ** 31, K, D) == 0 and L.vqvae_vq_entropy_workspace_bytes(0, K, D) == 0
    torch.cuda.synchronize()
    for t in (losses, avg, rs, gz, gE, ws):                        # nothing was launched: nothing was written
        assert (t == 7).all()
    assert fw() == 0 and bw(avg_=p(torch.full((K,), 0.2, dtype=torch.float64, device=DEV))) == 0       # and the same calls do run
    torch.cuda.synchronize()
    assert torch.isfinite(losses).all() and torch.isfinite(gz).all() and torch.isfinite(gE).all()


def test_a_non_finite_batch_returns():
    """the values are unspecified; the call returns and a finite batch afterwards is right again"""
    from vqvae_amd import functional as F
    B, H, W, D, K, regime = CASES[1]
    case = _case(*CASES[1])
    z = np.array(case[0])
    z[5, 3], z[17, 0] = np.nan, np.inf
    zt, Et = _layout(z, B, H, W, True), _dev(case[1])
    losses, avg, rowstat = F.vq_entropy_forward(zt, Et, inv_temperature=S, gamma=GAMMA, rowmajor=True)
    F.vq_entropy_backward(zt, Et, avg, rowstat, None, inv_temperature=S, gamma=GAMMA, rowmajor=True)
    torch.cuda.synchronize()
    _within(_run(case, B, H, W, True), case, "after a non-finite batch")


# ---- the modules ------------------------------------------------------------------------------------------------------------------

WEIGHT = 0.3
CONFIGS = {"plain": {}, "cosine_sim": dict(cosine_sim=True), "codebook_dim": dict(codebook_dim=8), "rotation_trick": dict(rotation_trick=True),
           "ema_decay": dict(ema_decay=0.99)}


def _quantizers(opts):
    """the option's quantizer and its twin without the option: the same bits in every parameter and buffer"""
    from vqvae_amd.modules import VQVAE
    out = []
    for ent in (dict(entropy_weight=WEIGHT, entropy_diversity_gamma=GAMMA, entropy_inv_temperature=50.0), {}):
        torch.manual_seed(5)
        q = VQVAE(16, 8, 1, 32, 16, 0.25, **opts, **ent).vector_quantization.to(DEV).train()
        with torch.no_grad():
            q.embedding.weight.mul_(3.0)                           # codes of the rows' scale: several carry mass, the term has a gradient
        out.append(q)
    return out


def _grads(q, z):
    return [None if p.grad is None else p.grad.clone() for p in q.parameters()] + [z.grad.clone()]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_module_loss_and_gradients_are_the_hand_written_chain(name):
    """loss = the loss without the option + weight * term, and every gradient is the twin's own backward with the term's gradients
    -- functional.vq_entropy_backward at grad_loss = weight -- added at the operands the search ran on, bit for bit"""
    from vqvae_amd import functional as F
    on, off = _quantizers(CONFIGS[name])
    torch.manual_seed(9)
    x = 0.1 * torch.randn(3, 16, 5, 7, device=DEV)
    z_on, z_off = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    out_on = on.quantize(z_on)
    seen = []
    # (a codebook without a gradient is copied where it is seen: the EMA update that follows writes it in place)
    off._with_entropy = lambda out, z, codes, rowmajor: (seen.append((z, codes if codes.requires_grad else codes.clone(), rowmajor)), out)[1]
    out_off = off.quantize(z_off)
    (zop, codes, rowmajor), = seen
    kw = dict(inv_temperature=50.0, gamma=GAMMA, rowmajor=rowmajor)
    losses, avg, rowstat = F.vq_entropy_forward(zop.detach(), codes.detach(), **kw)
    assert torch.equal(on.last_entropy_losses, losses) and off.last_entropy_losses is None
    assert torch.equal(out_on[0], out_off[0] + WEIGHT * losses[0])
    for a, b in zip(out_on[1:], out_off[1:]):
        assert torch.equal(a, b)
    assert float(losses[1]) > 1e-6 and np.isfinite(losses.cpu().numpy()).all()
    ema = name == "ema_decay"
    gz, gE = F.vq_entropy_backward(zop.detach(), codes.detach(), avg, rowstat, torch.tensor(WEIGHT, device=DEV),
                                   want=(True, not ema), **kw)
    assert gz.abs().max() > 0
    g_out = torch.randn_like(out_on[1])
    (out_on[0] + (out_on[1] * g_out).sum()).backward()
    roots, grads = [out_off[0] + (out_off[1] * g_out).sum(), zop], [None, gz]
    if not ema:
        roots, grads = roots + [codes], grads + [gE]
    torch.autograd.backward(roots, grads)
    for a, b in zip(_grads(on, z_on), _grads(off, z_off)):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b))
    if ema:
        assert on.embedding.weight.grad is None and torch.equal(on.embedding.weight, off.embedding.weight)
        assert torch.equal(on.ema_w, off.ema_w) and torch.equal(on.ema_cluster_size, off.ema_cluster_size)
    else:
        assert on.embedding.weight.grad.abs().max() > 0


@pytest.mark.parametrize("name", list(CONFIGS))
def test_eval_no_grad_encode_and_decode_are_the_option_off(name):
    from vqvae_amd.modules import VQVAE
    models = []
    for ent in (dict(entropy_weight=WEIGHT), {}):
        torch.manual_seed(5)
        models.append(VQVAE(16, 8, 1, 32, 16, 0.25, **CONFIGS[name], **ent).to(DEV))
    on, off = models
    x = torch.randn(2, 3, 32, 32, device=DEV)
    with torch.no_grad():
        for mode in ("train", "eval"):
            getattr(on, mode)(), getattr(off, mode)()
            for a, b in zip(on(x), off(x)):
                assert torch.equal(a, b), mode
        idx = on.encode(x)
        assert torch.equal(idx, off.encode(x)) and torch.equal(on.decode_indices(idx, 2, 8, 8), off.decode_indices(idx, 2, 8, 8))
    on.eval()
    for a, b in zip(on(x), off.eval()(x)):                         # eval with grad enabled: still nothing launched
        assert torch.equal(a, b)
    assert on.vector_quantization.last_entropy_losses is None


def test_one_train_checkpoint_step_saves_no_new_key(tmp_path):
    """tools/train_checkpoint.py --entropy_weight in a child process: two updates of a small model; the checkpoint has the keys of a
    model without the option"""
    from vqvae_amd.modules import VQVAE
    cmd = [sys.executable, os.path.join(ROOT, "tools", "train_checkpoint.py"), "--entropy_weight", "0.1", "--entropy_inv_temperature", "50",
           "--cosine_sim", "--n_updates", "2", "--batch_size", "8", "--n_train", "64", "--log_interval", "1", "--n_hiddens", "16",
           "--n_residual_hiddens", "8", "--n_residual_layers", "1", "--embedding_dim", "16", "--n_embeddings", "64", "--out", str(tmp_path),
           "--tag", "t"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    ck = torch.load(tmp_path / "t.pth", weights_only=False)
    assert ck["hyperparameters"]["entropy_weight"] == 0.1 and ck["hyperparameters"]["entropy_inv_temperature"] == 50.0
    assert len(ck["results"]["loss_vals"]) == 2 and all(np.isfinite(ck["results"]["loss_vals"]))
    assert list(ck["model"]) == list(VQVAE(16, 8, 1, 64, 16, 0.25, cosine_sim=True).state_dict())
