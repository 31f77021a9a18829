"""Lookup-free quantization without a GPU: the CPU restatement (tests/vq_lfq_ref.py) against fp64 torch autograd of the full-softmax
composition, the factorised losses against the (N, K) form, the index <-> bits round trip, the rules for y == 0, +-Inf and NaN, the C
ABI's four entries (declared, bound, argument errors before any launch, ABI still 9), the front ends' refusal of CPU tensors, the
constructor rules, the train tool's option, and the kernels' own text on the host under the sanitizers."""
import os
import re
import struct

import numpy as np
import pytest
import torch

from tests import vq_lfq_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = lambda v: float(np.float32(v))
BETA, WE, GAMMA = 0.25, f32(0.1), 0.5


def torch_composition(t, g, gl, d, beta, we, gamma, inv_t):
    """what a user would write: F.linear, sign with a straight-through gradient, the (N, K) softmax entropy loss, F.linear.  y takes
    the contract's rounding to fp32 (straight through).  -> (z_q, (loss, C, P, H), avg); the caller reads the inputs' gradients."""
    import torch.nn.functional as F
    y = F.linear(t["z"], t["w_in"], t["b_in"])
    y = y + (y.detach().to(torch.float32).to(torch.float64) - y.detach())
    c = torch.where(y > 0, 1.0, -1.0).to(torch.float64)
    zq = F.linear(y + (c - y).detach(), t["w_out"], t["b_out"])
    C = ((y - c.detach()) ** 2).mean()
    ck = torch.from_numpy(R.all_codes(d).astype(np.float64))
    prob = torch.softmax(2.0 * inv_t * (y @ ck.T), dim=1)
    P = -(prob * torch.log(prob)).sum(1).mean()
    avg = prob.mean(0)
    H = -(avg * torch.log(avg)).sum()
    loss = beta * C + we * (P - gamma * H)
    ((zq * g).sum() + gl * loss).backward()
    return zq.detach().numpy(), [v.item() for v in (loss, C, P, H)], avg.detach().numpy()


@pytest.mark.parametrize("inv_t", [1.0, 100.0])
@pytest.mark.parametrize("d", [1, 2, 5])
@pytest.mark.parametrize("D", [1, 7, 64])
def test_restatement_agrees_with_fp64_torch_autograd(D, d, inv_t):
    """|s y| <= 30 (y scaled with the temperature), so that no probability of the (N, K) softmax underflows: autograd of p log p is NaN
    at p = 0, the contract gives 0.  Both sides are fp64 on the same fp32 y, so they agree to a few hundred ulps of the terms'
    magnitudes (1e-12 relative to them); z_q and grad_z carry the restatement's one fp32 rounding."""
    N, gl = 300, 0.75
    z, g, w_in, b_in, w_out, b_out = R.draw(N, D, d, 1000 * D + d, scale=1.5 / inv_t)
    f = R.forward(z, w_in, b_in, w_out, b_out)
    assert np.abs(4.0 * inv_t * f.y).max() <= 30.0
    ls = R.losses(f.y, BETA, WE, GAMMA, inv_t)
    r = R.backward(z, g, gl, ls.avg, w_in, b_in, w_out, BETA, WE, GAMMA, inv_t)
    t = {n: torch.from_numpy(v.astype(np.float64)).requires_grad_(True) for n, v in dict(z=z, w_in=w_in, b_in=b_in, w_out=w_out, b_out=b_out).items()}
    zq, scal, avg = torch_composition(t, torch.from_numpy(g.astype(np.float64)), gl, d, BETA, WE, GAMMA, inv_t)
    assert (np.abs(f.z_q - zq) <= 2.0 ** -23 * np.abs(zq) + 2.0 ** -149).all()
    for got, want in zip((ls.loss, ls.C, ls.P, ls.H), scal):
        assert abs(got - want) <= 1e-12 * (1.0 + abs(want))
    assert (np.abs(ls.avg - avg) <= 1e-12 * avg + 1e-300).all()
    gz = t["z"].grad.numpy()
    assert (np.abs(r.grad_z - gz) <= 2.0 ** -23 * np.abs(gz) + 1e-11 * r.mag_gz + 1e-300).all()
    got, mags = R.param_grads(r)
    for n in ("w_out", "b_out", "w_in", "b_in"):
        want = t[n].grad.numpy()
        assert (np.abs(got[n] - want) <= 2.0 ** -23 * np.abs(want) + 1e-11 * mags[n] + 1e-300).all(), n
        blocked = R.param_grads_blocked(r)[n]
        assert (np.abs(blocked.astype(np.float64) - got[n]) <= 2.0 ** -23 * np.abs(got[n]) + 2.0 ** -40 * mags[n] + 1e-300).all(), n


@pytest.mark.parametrize("d,inv_t,scale", [(1, 100.0, 1.0), (3, 100.0, 1.0), (8, 100.0, 0.01), (6, 1.0, 1.0), (10, 100.0, 0.02)])
def test_factorised_losses_equal_the_full_softmax_form(d, inv_t, scale):
    """avg, P and H from the d binary channels against the (N, K) softmax of the logits 2 inv_t y . c_k, saturated rows included
    (there the full form's probabilities underflow to 0 and its entropy terms are taken as 0, as the contract's are)."""
    N, D = 200, 16
    z, _, w_in, b_in, w_out, b_out = R.draw(N, D, d, 31 * d, scale=scale)
    y = R.project_in(z, w_in, b_in)
    ls = R.losses(y, BETA, WE, GAMMA, inv_t)
    C, P, H, loss, avg = R.full_softmax(y, BETA, WE, GAMMA, inv_t)
    assert abs(ls.C - C) <= 1e-13 * (1 + C) and abs(ls.P - P) <= 1e-12 * (1 + P) and abs(ls.H - H) <= 1e-12 * (1 + H)
    assert abs(ls.loss - loss) <= 1e-12 * (1 + abs(loss))
    assert (np.abs(ls.avg - avg) <= 1e-12 * avg + 1e-300).all() and abs(ls.avg.sum() - 1.0) < 1e-12
    # the gradient's two forms: p+ p- (T+ - T-) is sum_k L_k p(k) (bit_j(k) - p+)
    lg = R.loss_grad_y(y, ls.avg, BETA, WE, GAMMA, inv_t)
    pk = R.code_probs(ls.p1, ls.p0)
    L = np.where(ls.avg == 0, 0.0, np.log(np.where(ls.avg == 0, 1.0, ls.avg)))
    bits = ((np.arange(1 << d)[:, None] >> np.arange(d)[None, :]) & 1).astype(np.float64)
    other = ((pk * L[None, :])[:, :, None] * (bits[None, :, :] - ls.p1[:, None, :])).sum(1)
    mine = lg.pq * (lg.T[:, :, 1] - lg.T[:, :, 0])
    assert (np.abs(mine - other) <= 1e-12 * (np.abs(pk * L[None, :]).sum(1)[:, None]) + 1e-300).all()


@pytest.mark.parametrize("d", [1, 9, 16])
def test_index_bits_round_trip_over_all_K(d):
    K = 1 << d
    codes = R.all_codes(d)
    assert codes.shape == (K, d) and set(np.unique(codes).tolist()) == {-1.0, 1.0}
    c, idx = R.codes(codes * np.float32(0.5))                    # y = +-0.5: the forward's own index
    assert np.array_equal(idx, np.arange(K)) and np.array_equal(c, codes)
    assert idx[1] == 1 and codes[1, 0] == 1.0 and (codes[1, 1:] == -1.0).all()        # the FIRST channel is the least significant bit
    eye = np.eye(d, dtype=np.float32)
    assert np.array_equal(R.decode(np.arange(K), eye, np.zeros(d, np.float32), d), codes)
    from vqvae_amd.modules import LookupFreeQuantizer
    assert torch.equal(LookupFreeQuantizer(K, 8, 0.25).codes(), torch.from_numpy(codes))


def test_zero_inf_and_nan_follow_the_rules():
    y = np.array([[0.0, -0.0, 1e-45], [np.inf, -np.inf, 1.0], [np.nan, 2.0, -3.0], [1.0, 1.0, 1.0]], np.float32)
    c, idx = R.codes(y)
    assert np.array_equal(c[0], [-1, -1, 1]) and idx[0] == 4      # y == 0 (either sign) gives -1, the smallest denormal +1
    assert np.array_equal(c[1], [1, -1, 1]) and idx[1] == 5       # +-Inf keep their sign
    assert np.isnan(c[2, 0]) and np.array_equal(c[2, 1:], [1, -1]) and idx[2] == 2        # NaN: bit 0, a NaN code
    w_out = np.ones((2, 3), np.float32)
    zq = R.project_out(c, w_out, np.zeros(2, np.float32))
    assert np.isnan(zq[2]).all() and np.isfinite(zq[[0, 1, 3]]).all()                    # the NaN stays in its row
    assert np.isnan(R.decode([-1, 8, 3], w_out, np.zeros(2, np.float32), 3)[:2]).all()


NAMES = ("vqvae_lfq_workspace_bytes", "vqvae_lfq_forward_f32", "vqvae_lfq_decode_indices_f32", "vqvae_lfq_backward_f32")


def test_entries_are_declared_and_bound_and_the_abi_stays_9():
    import ctypes
    from vqvae_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    src = open(os.path.join(ROOT, "include", "vqvae_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert re.search(r"VQVAE_API\s+(int|size_t)\s+" + name + r"\s*\(", src)
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [3, 24, 11, 25]
    assert _lib.load().vqvae_abi_version() == 9 and re.search(r"#define VQVAE_HIP_ABI_VERSION 9\b", src)
    assert "LFQ" not in "".join(re.findall(r"#define\s+(VQVAE_VQ_\w+)", src))         # no new flag: the entries take ROWMAJOR only


def test_argument_errors_come_back_before_any_launch():
    from vqvae_amd import _lib
    L = _lib.load()
    M = 1 << 26                                                # fake, aligned, disjoint "device pointers" (never dereferenced)
    names = "z wi bi wo bo zq ix hs pp ls av ws g gl gz gwi gbi gwo gbo".split()
    P = {n: M * (i + 1) for i, n in enumerate(names)}
    fw, dec, bw, size = L.vqvae_lfq_forward_f32, L.vqvae_lfq_decode_indices_f32, L.vqvae_lfq_backward_f32, L.vqvae_lfq_workspace_bytes
    big = 1 << 26
    for flags in (0, 1):
        def F(**k):
            a = dict(P, d=10, B=2, D=64, H=8, W=8, n=big)
            a.update(k)
            return fw(a["z"], a["wi"], a["bi"], a["wo"], a["bo"], a["d"], a["B"], a["D"], a["H"], a["W"], flags, 0.25, 0.1, 1.0, 100.0,
                      a["zq"], a["ix"], a["hs"], a["pp"], a["ls"], a["av"], a["ws"], a["n"], None)

        def Dc(**k):
            a = dict(P, d=10, B=2, D=64, H=8, W=8)
            a.update(k)
            return dec(a["ix"], a["wo"], a["bo"], a["d"], a["B"], a["D"], a["H"], a["W"], flags, a["zq"], None)

        def Bk(**k):
            a = dict(P, d=10, B=2, D=64, H=8, W=8, n=big)
            a.update(k)
            return bw(a["z"], a["g"], a["gl"], a["av"], a["wi"], a["bi"], a["wo"], a["d"], a["B"], a["D"], a["H"], a["W"], flags, 0.25, 0.1, 1.0,
                      100.0, a["gz"], a["gwi"], a["gbi"], a["gwo"], a["gbo"], a["ws"], a["n"], None)

        # NULLs
        for name in ("z", "wi", "bi", "wo", "bo", "ix"):
            assert F(**{name: None}) == -1, name
        assert F(hs=None) == -1                                  # perplexity needs hist
        assert F(ls=None) == -1 and F(av=None) == -1             # losses and avg come together
        for name in ("ix", "wo", "bo", "zq"):
            assert Dc(**{name: None}) == -1, name
        for name in ("z", "wi", "bi", "wo"):
            assert Bk(**{name: None}) == -1, name
        assert Bk(gz=None, gwi=None, gbi=None, gwo=None, gbo=None) == -1
        assert Bk(g=None, av=None) == -1                         # no upstream gradient at all
        for call in (F, Dc, Bk):
            # shapes, then the envelope: d = 0 and d = 17, D = 0 and D = 257, N = 2^32
            assert call(B=0) == -2 and call(H=0) == -2 and call(W=-1) == -2
            assert call(d=0) == -3 and call(d=17) == -3
            assert call(D=257) == -3 and call(D=0) == -3
            assert call(B=1 << 20, H=64, W=64) == -3
        a = P
        assert fw(a["z"], a["wi"], a["bi"], a["wo"], a["bo"], 10, 2, 64, 8, 8, flags | 2, 0.25, 0.1, 1.0, 100.0, a["zq"], a["ix"], a["hs"],
                  a["pp"], a["ls"], a["av"], a["ws"], big, None) == -3
        # misaligned pointers
        for name in ("z", "wi", "bi", "wo", "bo", "zq", "hs", "pp", "ls"):
            assert F(**{name: P["z"] + 2 + M * 40}) == -3, name
        assert F(ix=P["ix"] + 4) == -3 and F(av=P["av"] + 4) == -3 and F(ws=P["ws"] + 4) == -3
        assert Dc(zq=P["zq"] + 2) == -3 and Dc(wo=P["wo"] + 1) == -3 and Dc(ix=P["ix"] + 4) == -3
        for name in ("z", "g", "gl", "wi", "bi", "wo", "gz", "gwi", "gbi", "gwo", "gbo"):
            assert Bk(**{name: P["z"] + 2 + M * 40}) == -3, name
        assert Bk(ws=P["ws"] + 4) == -3 and Bk(av=P["av"] + 4) == -3
        # an output on an input
        assert F(zq=P["z"]) == -3 and F(zq=P["z"] + 400) == -3 and F(zq=P["wo"]) == -3 and F(ix=P["z"]) == -3 and F(hs=P["wi"]) == -3
        assert F(pp=P["bi"]) == -3 and F(ls=P["bo"]) == -3 and F(av=P["z"]) == -3 and F(ws=P["z"]) == -3
        assert Dc(zq=P["ix"]) == -3 and Dc(zq=P["wo"]) == -3
        assert Bk(gz=P["z"]) == -3 and Bk(gz=P["g"] + 64) == -3 and Bk(gwi=P["wi"]) == -3 and Bk(gwo=P["wo"]) == -3 and Bk(gbi=P["bi"]) == -3
        assert Bk(ws=P["z"]) == -3 and Bk(ws=P["av"]) == -3 and Bk(gz=P["gl"]) == -3
        # the workspace
        need = size(128, 64, 10)
        assert F(ws=None) == -4 and F(n=need - 8) == -4 and Bk(ws=None) == -4 and Bk(n=need - 8) == -4
        assert F(d=16, ws=None) == -4                            # (K = 65536 is inside the envelope)
    # the sizing call: y, then the larger of the forward's and the backward's needs; 0 outside the envelope
    y_bytes = 128 * 10 * 4
    fwd = 1 * 1024 * 8 + 1 * 32 * 8
    bwd = 1024 * 8 + 128 * 10 * 8 + 1 * (2 * 64 * 10 + 64 + 10) * 8
    assert size(128, 64, 10) == y_bytes + max(fwd, bwd)
    assert size(1 << 20, 64, 16) < 700 << 20 and R.partition(1 << 20, 65536) == (256 * 256, 16)   # 16 partitions of K doubles: 8 MiB
    assert R.partition(1025, 1024) == (256, 5) and R.partition(262144, 1024) == (256, 1024) and R.partition(300, 2) == (256, 2)
    assert size(1 << 32, 64, 4) == 0 and size(0, 64, 4) == 0 and size(128, 257, 4) == 0 and size(128, 64, 0) == 0 and size(128, 64, 17) == 0


def test_front_ends_reject_cpu_tensors():
    from vqvae_amd import _lib, functional as F, training as T
    from vqvae_amd.modules import LookupFreeQuantizer
    z = torch.zeros(2, 16, 3, 3)
    w_in, b_in, w_out, b_out = torch.zeros(4, 16), torch.zeros(4), torch.zeros(16, 4), torch.zeros(16)
    with pytest.raises(_lib.VqvaeHipError):
        F.lfq_forward(z, w_in, b_in, w_out, b_out, 16)
    with pytest.raises(_lib.VqvaeHipError):
        F.lfq_decode_indices(torch.zeros(18, dtype=torch.int64), w_out, b_out, 16, 2, 3, 3)
    with pytest.raises(_lib.VqvaeHipError):
        T.lfq_backward(z, z, None, None, w_in, b_in, w_out, 16)
    with pytest.raises(_lib.VqvaeHipError):
        T.LFQStraightThrough.apply(z.requires_grad_(True), w_in, b_in, w_out, b_out, 16, (0.25, 0.1, 1.0, 100.0), False)
    with pytest.raises(_lib.VqvaeHipError):
        F.lfq_workspace(1 << 32, 16, 4, "cpu")
    q = LookupFreeQuantizer(16, 16, 0.25)
    with pytest.raises(_lib.VqvaeHipError):
        q(z)
    with pytest.raises(_lib.VqvaeHipError):
        q.quantize(z.detach())
    for bad in (0, 1, 3, 1000, 1 << 17):
        with pytest.raises(ValueError):
            F._lfq_bits(bad)
    assert F.lfq_forward.__kwdefaults__["inv_temperature"] == 100.0 and F.lfq_forward.__kwdefaults__["want_loss"] is True


def test_the_module_and_its_state():
    from vqvae_amd.modules import LookupFreeQuantizer
    torch.manual_seed(0)
    q = LookupFreeQuantizer(1024, 16, 0.25)
    assert list(q.state_dict()) == ["project_in.weight", "project_in.bias", "project_out.weight", "project_out.bias"]
    assert q.n_e == 1024 and q.e_dim == 16 and q.bits == 10 and q.last_losses is None
    assert (q.entropy_weight, q.diversity_gamma, q.inv_temperature) == (0.1, 1.0, 100.0)
    assert q.project_in.weight.shape == (10, 16) and q.project_out.weight.shape == (16, 10)
    assert torch.equal(q.codes(), torch.from_numpy(R.all_codes(10)))
    for bad in (1, 3, 1000, 1 << 17):
        with pytest.raises(ValueError):
            LookupFreeQuantizer(bad, 16, 0.25)
    with pytest.raises(ValueError):
        LookupFreeQuantizer(16, 257, 0.25)


def test_constructor_rules_and_the_default_is_todays_model():
    from vqvae_amd._lib import VqvaeHipError
    from vqvae_amd.modules import VQVAE, LookupFreeQuantizer, VectorQuantizer
    m = VQVAE(32, 8, 1, 1024, 16, 0.25, lookup_free=True, lfq_entropy_weight=0.2, lfq_diversity_gamma=0.5, lfq_inv_temperature=10.0)
    vq = m.vector_quantization
    assert type(vq) is LookupFreeQuantizer and (vq.beta, vq.entropy_weight, vq.diversity_gamma, vq.inv_temperature) == (0.25, 0.2, 0.5, 10.0)
    assert [k for k in m.state_dict() if k.startswith("vector_quantization.")] == [
        "vector_quantization.project_in.weight", "vector_quantization.project_in.bias",
        "vector_quantization.project_out.weight", "vector_quantization.project_out.bias"]
    for kw in (dict(ema_decay=0.99), dict(ema_decay=0.99, restart_threshold=1.0), dict(restart_threshold=1.0), dict(n_quantizers=2),
               dict(n_quantizers=2, shared_codebook=True), dict(shared_codebook=True), dict(rotation_trick=True), dict(cosine_sim=True),
               dict(fsq_levels=(4, 4, 4, 4, 4)), dict(codebook_groups=2)):
        with pytest.raises(ValueError):
            VQVAE(32, 8, 1, 1024, 16, 0.25, lookup_free=True, **kw)
    for bad in (1, 1000, 24, 1 << 17):
        with pytest.raises(ValueError):
            VQVAE(32, 8, 1, bad, 16, 0.25, lookup_free=True)
    assert VQVAE(32, 8, 1, 2, 16, 0.25, lookup_free=True).vector_quantization.bits == 1
    with pytest.raises(TypeError):
        VQVAE(32, 8, 1, 1024, 16, 0.25, False, None, 1e-5, None, 1, False, False, False, None, 1, True)      # keyword-only
    with pytest.raises(VqvaeHipError):
        m.init_codebook_(torch.zeros(1, 3, 32, 32))
    with pytest.raises(VqvaeHipError):
        m._c_weights()
    # without the option: today's model, its keys and its bits at a fixed seed, and no random number drawn on the way
    torch.manual_seed(0)
    a = VQVAE(32, 8, 1, 64, 16, 0.25)
    after_a = torch.rand(4)
    torch.manual_seed(0)
    b = VQVAE(32, 8, 1, 64, 16, 0.25, lookup_free=False, lfq_entropy_weight=0.3)
    after_b = torch.rand(4)
    assert type(b.vector_quantization) is VectorQuantizer and torch.equal(after_a, after_b)
    assert list(a.state_dict()) == list(b.state_dict())
    for k_, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k_]), k_
    # the codebook's bits at seed 0 are those of the reference's initialisation drawn after the encoder's and the 1x1 conv's
    torch.manual_seed(0)
    from vqvae_amd.modules import Encoder
    Encoder(3, 32, 1, 8)
    torch.nn.Conv2d(32, 16, kernel_size=1, stride=1)
    e = torch.nn.Embedding(64, 16)
    e.weight.data.uniform_(-1.0 / 64, 1.0 / 64)
    assert torch.equal(e.weight, a.vector_quantization.embedding.weight)


def test_train_tool_options_are_absent_unless_given():
    src = open(os.path.join(ROOT, "tools", "train_checkpoint.py")).read()
    for opt in ('"--lookup_free"', '"--lfq_entropy_weight"', '"--lfq_diversity_gamma"', '"--lfq_inv_temperature"'):
        line = next(l for l in src.splitlines() if opt in l)
        assert "argparse.SUPPRESS" in line, opt


# ---- the kernels' own text on the host --------------------------------------------------------------------------------------------

# (B, HW, D, d, clean, nwg, inv_t, scale): one row; odd D on the element path, d = 1; the flagship split (5 + 5 bits) over two blocks;
# an odd split (5 + 4) with rows wider than one chunk; special rows (losses unspecified, nothing faults); d = 16: 64 code tiles, log avg
# read from memory; the LDS table's largest form (K = 4096); d = 16 with the large weight capacity (D = 68 > 64: a full chunk and a
# ragged one, the 16-byte path) at the GPU test's 300 rows
HOST_CASES = [(1, 1, 16, 4, 1, 1, 100.0, 1.0), (3, 35, 7, 1, 1, 7, 100.0, 0.01), (5, 64, 64, 10, 1, 13, 100.0, 0.02),
              (2, 150, 68, 9, 1, 64, 1.0, 1.0), (9, 36, 12, 3, 0, 5, 100.0, 1.0), (1, 6, 12, 16, 1, 3, 100.0, 0.01),
              (1, 70, 8, 12, 1, 9, 100.0, 0.02), (3, 100, 68, 16, 1, 16, 100.0, 0.01)]


def host_case_bytes(B, HW, D, d, clean, nwg, inv_t, scale, seed):
    """one case of tests/host/lfq_harness.cpp's input: the inputs and every expected output or its reference value and bound"""
    N, K, gl = B * HW, 1 << d, 0.75
    z, g, w_in, b_in, w_out, b_out = R.draw(N, D, d, seed, scale=scale)
    if not clean:
        b_in[0] = 0.0
        z[1] = 1e4
        z[2] = -1e4
        z[3] = 0.0                                               # y[3, 0] == 0 exactly
        z[4, D // 2] = np.nan
        z[5] = np.inf
        z[6, 0] = -np.inf
        g[7, D - 1] = np.nan
    f = R.forward(z, w_in, b_in, w_out, b_out)
    if not clean:
        assert f.y[3, 0] == 0 and f.c[3, 0] == -1 and np.isnan(f.z_q[4]).all() and np.isfinite(f.z_q[[0, 1, 2, 3, 7]]).all()
        assert ((f.idx >= 0) & (f.idx < K)).all()
    ls = R.losses(f.y, BETA, WE, GAMMA, inv_t)
    avg_in = ls.avg if clean else np.full(K, 1.0 / K)
    st = R.backward(z, g, gl, None, w_in, b_in, w_out, BETA, WE, GAMMA, inv_t)
    st_p = R.param_grads_blocked(st)
    wl = R.backward(z, g, gl, avg_in, w_in, b_in, w_out, BETA, WE, GAMMA, inv_t)
    wl_p, wl_m = R.param_grads(wl)
    dec_idx = f.idx.copy()
    if N >= 8:
        dec_idx[0], dec_idx[N - 1], dec_idx[2] = -1, K, 1 << 40
    dec = R.decode(dec_idx, w_out, b_out, d)
    if N >= 8:
        assert np.isnan(dec[[0, N - 1, 2]]).all() and np.isfinite(dec[1]).all()
    # the bounds: tests/test_vq_lfq_gpu.py derives them; here libm's exp / log replace the device's
    bL, bC, bP, bH = R.loss_bounds(ls, N, d, K, BETA, WE, GAMMA)
    scal = np.array([ls.loss, ls.C, ls.P, ls.H], np.float64)
    b_scal = np.array([bL, bC, bP, bH]) + 2.0 ** -23 * np.abs(scal) + 2.0 ** -149     # (fp32 outputs: below 2^-126 the step is 2^-149)
    with np.errstate(invalid="ignore"):
        be = R.e_bound(wl.lg, K, d, WE, GAMMA, 4.0 * inv_t, N)
        bgy = gl * be + 4 * R.U * (np.abs(wl.gc) + np.abs(gl * wl.lg.e))
        b_gz = 2.0 ** -23 * np.abs(wl.grad_z.astype(np.float64)) + bgy @ np.abs(w_in.astype(np.float64)) + (d + 2) * R.U * wl.mag_gz + 2.0 ** -149
        n_add = N / 256 + 256 + 4
        b_gwi = 2.0 ** -23 * np.abs(wl_p["w_in"]) + n_add * R.U * wl_m["w_in"] + bgy.T @ np.abs(z.astype(np.float64)) + 2.0 ** -149
        b_gbi = 2.0 ** -23 * np.abs(wl_p["b_in"]) + n_add * R.U * wl_m["b_in"] + bgy.sum(0) + 2.0 ** -149
    head = np.array([B, HW, D, d, clean, nwg], np.int32)
    scalars = np.array([BETA, WE, GAMMA, inv_t, gl], np.float64)
    d64 = lambda v: np.asarray(v, np.float64)
    parts = [head, scalars, z, g, w_in, b_in, w_out, b_out, f.idx.astype(np.int64), f.hist.astype(np.int32), f.z_q, f.y, dec_idx.astype(np.int64),
             dec, scal, b_scal, d64(avg_in), d64(R.avg_bound(ls, N, d)),
             st.grad_z, st_p["w_out"], st_p["b_out"], st_p["w_in"], st_p["b_in"],
             d64(wl.lg.e), d64(be), d64(wl.grad_z), d64(b_gz), d64(wl_p["w_in"]), d64(b_gwi), d64(wl_p["b_in"]), d64(b_gbi)]
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


def test_kernel_text_on_the_host(tmp_path):
    """tests/host/lfq_harness.cpp compiles csrc/vq_lfq.h -- the per-row operations and the whole bodies of the kernels -- for the host
    with AddressSanitizer and UBSan and -ffp-contract=off and runs both launch chains in both layouts and on both access paths (a
    workgroup runs as host threads with a barrier).  z_q, idx, hist, y, decode and the straight-through gradients must have the
    restatement's bits; the losses, avg and the loss's gradients must lie inside the bounds of the GPU tests: zero, saturated, NaN and
    Inf rows, out-of-range indices, odd D, wide rows, ragged last blocks, odd bit splits and d = 16 among the cases."""
    import shutil
    import subprocess
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe, data = str(tmp_path / "lfq_harness"), str(tmp_path / "cases.bin")
    with open(data, "wb") as fh:
        fh.write(struct.pack("<i", len(HOST_CASES)))
        for i, case in enumerate(HOST_CASES):
            fh.write(host_case_bytes(*case, 77 + i))
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-pthread", "-o", exe, os.path.join(ROOT, "tests", "host", "lfq_harness.cpp")])
    out = subprocess.run([exe, data], capture_output=True, text=True)
    assert out.returncode == 0 and "emulation ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
