"""The code-entropy loss without a GPU: the CPU restatement (tests/vq_entropy_ref.py) against fp64 torch autograd of the (N, K)
composition, two analytic cases, the bounds of the GPU test shown to tell a broken gradient from a right one, the C ABI's three
entries (declared, bound, ABI still 9), the constructor rules of the modules and of VQVAE, the train tool's option, and the kernels'
own text on the host under the sanitizers (tests/host/entropy_harness.cpp)."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest
import torch

from tests import vq_entropy_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAG = dict(N=1025, D=64, K=512, regime="soft", s=100.0, gamma=0.5, g=0.75)        # the GPU test's flag case


def torch_composition(z, E, s, gamma, g):
    """what a user would write, in fp64: zz + ee - 2 z E^T, log_softmax, the two entropies"""
    z = torch.from_numpy(z.astype(np.float64)).requires_grad_(True)
    E = torch.from_numpy(E.astype(np.float64)).requires_grad_(True)
    d = (z * z).sum(1, keepdim=True) + (E * E).sum(1)[None, :] - 2.0 * z @ E.T
    logp = torch.log_softmax(-s * d, dim=1)
    p = logp.exp()
    P = -(p * logp).sum(1).mean()
    avg = p.mean(0)
    H = -(avg * torch.log(avg)).sum()
    term = P - gamma * H
    (g * term).backward()
    return [v.item() for v in (term, P, H)], avg.detach().numpy(), z.grad.numpy(), E.grad.numpy()


@pytest.mark.parametrize("s,gamma", [(1.0, 1.0), (100.0, 0.5)])
@pytest.mark.parametrize("K", [1, 2, 5, 65])
@pytest.mark.parametrize("D", [1, 7, 64])
def test_restatement_agrees_with_fp64_torch_autograd(D, K, s, gamma):
    """The soft regime, so that no probability of the (N, K) softmax underflows (autograd of p log p is NaN at p = 0, the contract
    gives 0).  Both sides are fp64 on the same fp32 inputs: tests/test_vq_lfq_cpu.py's like-for-like tolerances -- 1e-12 relative for
    the scalars and avg, one fp32 rounding plus 1e-11 of the terms' magnitudes for the gradients."""
    N, g = 300, 0.75
    z, E = R.draw(N, D, K, 1000 * D + K, "soft")
    if s == 1.0:
        z, E = (10.0 * z).astype(np.float32), (10.0 * E).astype(np.float32)
    f = R.forward(z, E, s, gamma)
    r = R.backward(z, E, f.avg, f.rowstat, g, s, gamma)
    scal, avg, gz, gE = torch_composition(z, E, s, gamma, g)
    for got, want in zip((f.term, f.P, f.H), scal):
        assert abs(got - want) <= 1e-12 * (1.0 + abs(want))
    assert (np.abs(f.avg - avg) <= 1e-12 * avg + 1e-300).all() and abs(f.avg.sum() - 1.0) < 1e-12
    az, aE, aa = np.abs(z.astype(np.float64)), np.abs(E.astype(np.float64)), np.abs(r.a)
    mag_z = 2.0 * s * (aa @ aE + az * aa.sum(1)[:, None])
    mag_E = 2.0 * s * (aa.T @ az + aE * aa.sum(0)[:, None])
    assert (np.abs(r.grad_z - gz) <= 2.0 ** -23 * np.abs(gz) + 1e-11 * mag_z + 1e-300).all()
    assert (np.abs(r.grad_E - gE) <= 2.0 ** -23 * np.abs(gE) + 1e-11 * mag_E + 1e-300).all()


def test_equal_codes_give_log_K_and_no_gradient():
    N, D, K = 50, 7, 12
    z, E = R.draw(N, D, K, 5, "soft")
    E = np.repeat(E[:1], K, 0)
    f = R.forward(z, E, 100.0, 1.0)
    assert abs(f.P - np.log(K)) <= 1e-12 and abs(f.H - np.log(K)) <= 1e-12 and abs(f.term) <= 1e-12
    r = R.backward(z, E, f.avg, f.rowstat, 1.0, 100.0, 1.0)
    scale = 2.0 * 100.0 * (np.abs(z).max() + np.abs(E).max())
    assert np.abs(r.grad_z64).max() <= 1e-12 * scale and np.abs(r.grad_E64).max() <= 1e-12 * scale


def test_rows_on_far_apart_codes_are_confident():
    N, D, K = 64, 7, 16
    rng = np.random.default_rng(3)
    E = (10.0 * rng.standard_normal((K, D))).astype(np.float32)
    idx = np.arange(N) % K
    f = R.forward(E[idx], E, 100.0, 1.0)
    assert 0.0 <= f.P <= 1e-30                                    # every row sits on its code: p is one-hot
    assert abs(f.H - np.log(K)) <= 1e-12                          # and the batch uses every code equally often
    assert np.array_equal(f.p.argmax(1), idx)
    assert np.isfinite(f.rowstat).all() and np.isfinite(f.losses).all()


def test_the_bounds_tell_a_broken_gradient_from_the_right_one():
    """On the flag case: leaving out either bracket term of a_nk, or flipping gamma's sign, moves grad_z and grad_E outside the
    bound the GPU test allows (both sides' fp64 error and one fp32 rounding), in most elements."""
    c = FLAG
    z, E = R.draw(c["N"], c["D"], c["K"], 77, c["regime"])
    f = R.forward(z, E, c["s"], c["gamma"])
    r = R.backward(z, E, f.avg, f.rowstat, c["g"], c["s"], c["gamma"])
    assert (f.p > 1e-4).sum(1).min() >= 3                         # the soft regime: several codes carry mass in every row
    b_gz, b_gE = R.bwd_bounds(r, f, z, E, c["g"], c["s"], c["gamma"])
    b_gz, b_gE = R.SIDES * b_gz + R.f32_round(r.grad_z64), R.SIDES * b_gE + R.f32_round(r.grad_E64)
    assert (np.abs(r.grad_z - r.grad_z64) <= b_gz).all() and (np.abs(r.grad_E - r.grad_E64) <= b_gE).all()
    # the bound is about one fp32 ulp of the element plus a billionth of the largest gradient
    assert (b_gz <= 2.0 ** -22 * np.abs(r.grad_z64) + 1e-9 * np.abs(r.grad_z64).max()).all()
    assert (b_gE <= 2.0 ** -22 * np.abs(r.grad_E64) + 1e-9 * np.abs(r.grad_E64).max()).all()
    for drop in ("confidence", "diversity", "sign"):
        bad = R.backward(z, E, f.avg, f.rowstat, c["g"], c["s"], c["gamma"], drop=drop)
        out_z = np.abs(bad.grad_z - r.grad_z64) > b_gz
        out_E = np.abs(bad.grad_E - r.grad_E64) > b_gE
        assert out_z.mean() > 0.9 and out_E.mean() > 0.9, drop


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------

def test_entries_are_declared_and_bound():
    from vqvae_amd import _lib
    header = open(os.path.join(ROOT, "include", "vqvae_hip.h")).read()
    for name in ("vqvae_vq_entropy_workspace_bytes", "vqvae_vq_entropy_forward_f32", "vqvae_vq_entropy_backward_f32"):
        assert name in header and name in _lib.SIGNATURES
    assert re.search(r"#define VQVAE_HIP_ABI_VERSION 9\b", header)


def test_front_ends_refuse_cpu_tensors():
    from vqvae_amd import _lib, functional as F
    z, E = torch.zeros(1, 4, 2, 2), torch.zeros(3, 4)
    with pytest.raises(_lib.VqvaeHipError):
        F.vq_entropy_forward(z, E, inv_temperature=100.0, gamma=1.0)
    with pytest.raises(_lib.VqvaeHipError):
        F.vq_entropy_backward(z, E, torch.zeros(3, dtype=torch.float64), torch.zeros(4, 2, dtype=torch.float64), inv_temperature=100.0,
                              gamma=1.0)


# ---- construction rules -----------------------------------------------------------------------------------------------------------

def test_modules_are_off_by_default_and_add_no_state():
    from vqvae_amd import modules as M
    makers = [lambda **kw: M.VectorQuantizer(16, 8, 0.25, **kw), lambda **kw: M.VectorQuantizerEMA(16, 8, 0.25, **kw),
              lambda **kw: M.FactorizedVectorQuantizer(16, 8, 4, 0.25, **kw), lambda **kw: M.FactorizedVectorQuantizerEMA(16, 8, 4, 0.25, **kw)]
    for make in makers:
        torch.manual_seed(3)
        off = make()
        torch.manual_seed(3)
        on = make(entropy_weight=0.1, entropy_diversity_gamma=0.5, entropy_inv_temperature=50.0)
        assert off.entropy_weight == 0.0 and off.entropy_diversity_gamma == 1.0 and off.entropy_inv_temperature == 100.0
        assert (on.entropy_weight, on.entropy_diversity_gamma, on.entropy_inv_temperature) == (0.1, 0.5, 50.0)
        assert off.last_entropy_losses is None and on.last_entropy_losses is None
        assert list(off.state_dict()) == list(on.state_dict())
        assert [n for n, _ in off.named_parameters()] == [n for n, _ in on.named_parameters()]
        for (n, a), (_, b) in zip(off.state_dict().items(), on.state_dict().items()):
            assert torch.equal(a, b), n
    import inspect
    for cls in (M.VectorQuantizer, M.VectorQuantizerEMA, M.FactorizedVectorQuantizer, M.FactorizedVectorQuantizerEMA):
        params = inspect.signature(cls.__init__).parameters
        for n in ("entropy_weight", "entropy_diversity_gamma", "entropy_inv_temperature"):
            assert params[n].kind is inspect.Parameter.KEYWORD_ONLY, (cls.__name__, n)
    for bad in (dict(entropy_weight=-0.1), dict(entropy_weight=float("nan")), dict(entropy_inv_temperature=0.0),
                dict(entropy_inv_temperature=-1.0), dict(entropy_inv_temperature=float("inf")), dict(entropy_diversity_gamma=float("nan"))):
        with pytest.raises(ValueError):
            M.VectorQuantizer(16, 8, 0.25, **bad)


def test_vqvae_keywords():
    import inspect
    from vqvae_amd.modules import VQVAE, VectorQuantizer, VectorQuantizerEMA, FactorizedVectorQuantizer, FactorizedVectorQuantizerEMA
    names = list(inspect.signature(VQVAE.__init__).parameters)
    i = names.index("codebook_dim")
    assert names[i - 3:i] == ["entropy_weight", "entropy_diversity_gamma", "entropy_inv_temperature"] and names[-1] == "codebook_dim"
    for n in names[i - 3:i]:
        assert inspect.signature(VQVAE.__init__).parameters[n].kind is inspect.Parameter.KEYWORD_ONLY
    args = (16, 8, 1, 32, 8, 0.25)
    torch.manual_seed(11)
    off = VQVAE(*args)
    torch.manual_seed(11)
    on = VQVAE(*args, entropy_weight=0.1)
    assert list(off.state_dict()) == list(on.state_dict())
    for (n, a), (_, b) in zip(off.state_dict().items(), on.state_dict().items()):
        assert torch.equal(a, b), n
    assert type(on.vector_quantization) is VectorQuantizer and on.vector_quantization.entropy_weight == 0.1
    assert off.vector_quantization.entropy_weight == 0.0
    for kw, cls in ((dict(ema_decay=0.99), VectorQuantizerEMA), (dict(codebook_dim=4), FactorizedVectorQuantizer),
                    (dict(codebook_dim=4, ema_decay=0.99), FactorizedVectorQuantizerEMA), (dict(cosine_sim=True), VectorQuantizer),
                    (dict(rotation_trick=True), VectorQuantizer)):
        m = VQVAE(*args, entropy_weight=0.2, entropy_diversity_gamma=0.5, entropy_inv_temperature=50.0, **kw)
        q = m.vector_quantization
        assert type(q) is cls and (q.entropy_weight, q.entropy_diversity_gamma, q.entropy_inv_temperature) == (0.2, 0.5, 50.0)
    for kw in (dict(n_quantizers=2), dict(n_quantizers=2, shared_codebook=True), dict(codebook_groups=2), dict(fsq_levels=(8, 4)),
               dict(lookup_free=True)):
        with pytest.raises(ValueError, match="entropy_weight > 0 does not combine"):
            VQVAE(*args, entropy_weight=0.1, **kw)
        VQVAE(*args, **kw)                                        # and at weight 0 the combination is what it always was
    for kw in (dict(entropy_weight=-1.0), dict(entropy_weight=0.1, entropy_inv_temperature=0.0), dict(entropy_inv_temperature=-2.0)):
        with pytest.raises(ValueError):
            VQVAE(*args, **kw)


def test_train_tool_parses_the_option():
    from tools import train_checkpoint as tc
    args, kw = tc.parse(["--entropy_weight", "0.1", "--entropy_diversity_gamma", "0.5", "--entropy_inv_temperature", "50"])[:2]
    assert kw["entropy_weight"] == 0.1 and kw["entropy_diversity_gamma"] == 0.5 and kw["entropy_inv_temperature"] == 50.0
    assert "entropy_weight" not in tc.parse([])[1]


# ---- the kernels' text on the host ------------------------------------------------------------------------------------------------

HOST_CASES = [  # N, D, K, HW, regime, s, gamma, grad_loss or None
    (70, 7, 5, 7, "soft", 100.0, 0.5, 0.75),
    (257, 20, 65, 1, "saturated", 100.0, 1.0, None),
    (66, 3, 9, 1, "onehot", 100.0, 1.0, None),
    (130, 68, 3, 13, "soft", 100.0, -0.25, 0.75),
]


def test_kernel_text_on_the_host_under_the_sanitizers(tmp_path):
    """tests/host/entropy_harness.cpp compiles csrc/vq_entropy.h for the host (ASan + UBSan, -ffp-contract=off) and runs both launch
    chains in both layouts; its outputs lie within the GPU test's bounds of the restatement, and are the same bits in both layouts."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    blob = [struct.pack("<i", len(HOST_CASES))]
    for i, (N, D, K, HW, regime, s, gamma, g) in enumerate(HOST_CASES):
        assert N % HW == 0
        z, E = R.draw(N, D, K, 900 + i, regime)
        f = R.forward(z, E, s, gamma)
        gv = 1.0 if g is None else g
        r = R.backward(z, E, f.avg, f.rowstat, gv, s, gamma)
        fb = R.fwd_bounds(f, N, K, D, s, gamma)
        b_gz, b_gE = R.bwd_bounds(r, f, z, E, gv, s, gamma)
        ref_l = np.array([f.term, f.P, f.H])
        b_l = R.SIDES * np.array([fb["term"], fb["P"], fb["H"]]) + R.f32_round(ref_l)
        blob += [struct.pack("<5i", N, D, K, HW, 0 if g is None else 1), struct.pack("<2d", s, gamma), struct.pack("<f", gv),
                 z.tobytes(), E.tobytes(), ref_l.tobytes(), b_l.tobytes(), f.avg.tobytes(), (R.SIDES * fb["avg"]).tobytes(),
                 f.rowstat.tobytes(), (R.SIDES * np.stack([fb["lse"], fb["Hn"]], 1)).tobytes(),
                 r.grad_z64.tobytes(), (R.SIDES * b_gz + R.f32_round(r.grad_z64)).tobytes(),
                 r.grad_E64.tobytes(), (R.SIDES * b_gE + R.f32_round(r.grad_E64)).tobytes()]
    cases = tmp_path / "cases.bin"
    cases.write_bytes(b"".join(blob))
    exe = str(tmp_path / "entropy_harness")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-pthread", "-o", exe,
                           os.path.join(ROOT, "tests", "host", "entropy_harness.cpp")])
    out = subprocess.run([exe, str(cases)], capture_output=True, text=True)
    assert out.returncode == 0 and "emulation ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
