"""The cosine-similarity codebook without a GPU: the CPU restatement (tests/vq_cosine_ref.py) against fp64 torch (F.normalize and its
autograd), its clamp and NaN / Inf rows, the C ABI's two entries (declared, bound, argument errors before any launch, ABI still 9),
the modules' option (no state, today's model by default) and the kernels' own text on the host under the sanitizers."""
import os
import re

import numpy as np
import pytest
import torch

from tests import vq_cosine_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("scale", [0.05, 1.0])
@pytest.mark.parametrize("D", [1, 3, 48, 64, 256])
def test_restatement_agrees_with_fp64_torch(D, scale):
    """forward |y - y^| <= 4 2^-24 |y^| + one fp32 denormal; backward |grad_x - ref| <= 2^-20 ||g|| / ||x|| per element
    (vq_cosine_ref.backward_bound has the derivation).  Measured when the option was written: forward at most 0.49 of its bound,
    backward at most 0.17 of its bound (D = 3; 0.02 at D = 256)."""
    x, _, g = R.draw(4096, D, 1, scale, 100 * D + int(scale * 100))
    y, d = R.l2norm(x)
    gx = R.l2norm_backward(y, d, g)
    ref_y, ref_gx = R.torch_normalize(x, g)
    assert (d > R.F32(R.EPS)).all()
    ef, bf = np.abs(y.astype(np.float64) - ref_y), R.forward_bound(ref_y)
    print(f"D={D} scale={scale}: forward max err / bound = {(ef / bf).max():.4f}")
    assert (ef <= bf).all()
    eb, bb = np.abs(gx.astype(np.float64) - ref_gx), R.backward_bound(x, g)[:, None]
    print(f"D={D} scale={scale}: backward max err / bound = {(eb / bb).max():.4f}")
    assert (eb <= bb).all()
    n = np.sqrt((y.astype(np.float64) ** 2).sum(1))
    assert np.abs(n - 1.0).max() <= 2.0 ** -22


def test_clamp_rows_and_nan_rows():
    x, _, g = R.draw(16, 8, 1, 1.0, 3)
    x[0] = 0.0                                               # an all-zero row
    x[1] = np.array([1e-20, -1e-21] * 4, R.F32)              # a norm below eps
    x[3, 4] = np.nan
    x[4, 7] = np.inf
    g[5, 0] = np.nan
    y, d = R.l2norm(x)
    gx = R.l2norm_backward(y, d, g)
    eps = R.F32(R.EPS)
    assert d[0] == eps and d[1] == eps and np.isnan(d[3]) and np.isinf(d[4])
    assert (y[0] == 0).all() and np.array_equal(y[1], x[1] / eps)
    # the clamp rows' gradient is g / eps: what autograd gives clamp_min there
    for r in (0, 1):
        assert np.array_equal(gx[r], (g[r].astype(np.float64) / np.float64(eps)).astype(R.F32))
    xt = torch.from_numpy(x[:2].astype(np.float64)).requires_grad_(True)
    (torch.nn.functional.normalize(xt, dim=1, eps=R.EPS) * torch.from_numpy(g[:2].astype(np.float64))).sum().backward()
    # (on the zero row exactly; below eps torch adds a term of relative size ||x||^2 / eps^2 = 1e-16 ... 1e-15)
    np.testing.assert_allclose(gx[:2].astype(np.float64), xt.grad.numpy(), rtol=2.0 ** -23)
    assert np.isnan(y[3]).all()                              # a NaN reaches all of its row ...
    assert np.isnan(y[4, 7]) and (np.delete(y[4], 7) == 0).all()          # inf / inf, and finite / inf
    assert np.isnan(gx[5]).all()
    keep = [r for r in range(16) if r not in (3, 4, 5)]
    assert np.isfinite(y[keep]).all() and np.isfinite(gx[keep]).all()     # ... and no other
    # the comparison is written out: fmaxf would have returned eps for the NaN norm
    assert np.isnan(R.l2norm(np.full((1, 4), np.nan, R.F32))[1][0])


def test_composed_quantizer_searches_by_angle():
    """the restated quantizer's index is the fp64 argmax of cosine similarity wherever the top two are 1e-4 apart, and z_q has unit rows"""
    z, cb, _ = R.draw(512, 16, 32, 1.0, 11)
    zn, En, c = R.quantize(z, cb, 0.25)
    z64, c64 = z.astype(np.float64), cb.astype(np.float64)
    cos = (z64 / np.linalg.norm(z64, axis=1, keepdims=True)) @ (c64 / np.linalg.norm(c64, axis=1, keepdims=True)).T
    top = np.sort(cos, axis=1)
    clear = top[:, -1] - top[:, -2] >= 1e-4
    assert clear.mean() >= 0.98
    assert np.array_equal(c.idx[0][clear], cos.argmax(1)[clear])
    assert np.abs(np.linalg.norm(c.z_q.astype(np.float64), axis=1) - 1.0).max() <= 2.0 ** -22
    assert np.array_equal(c.z_q, (zn + (En[c.idx[0]] - zn).astype(R.F32)).astype(R.F32))


def test_entries_are_declared_and_bound_and_the_abi_stays_9():
    import ctypes
    from vqvae_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    src = open(os.path.join(ROOT, "include", "vqvae_hip.h")).read()
    for name in ("vqvae_l2norm_forward_f32", "vqvae_l2norm_backward_f32"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert re.search(r"VQVAE_API\s+int\s+" + name + r"\s*\(", src)
    assert len(_lib.SIGNATURES["vqvae_l2norm_forward_f32"][1]) == 10 and len(_lib.SIGNATURES["vqvae_l2norm_backward_f32"][1]) == 11
    assert _lib.load().vqvae_abi_version() == 9
    assert "COSINE" not in "".join(re.findall(r"#define\s+(VQVAE_VQ_\w+)", src))      # no new flag: the entries take ROWMAJOR only


def test_argument_errors_come_back_before_any_launch():
    from vqvae_amd import _lib
    L = _lib.load()
    a, b, c, d = 1 << 20, 2 << 20, 3 << 20, 4 << 20           # fake, aligned, disjoint "device pointers" (never dereferenced)
    fw, bw = L.vqvae_l2norm_forward_f32, L.vqvae_l2norm_backward_f32
    eps = 1e-12
    for flags in (0, 1):
        assert fw(None, 2, 64, 8, 8, eps, flags, b, c, None) == -1
        assert fw(a, 2, 64, 8, 8, eps, flags, None, c, None) == -1
        assert fw(a, 2, 64, 8, 8, eps, flags, b, None, None) == -1
        assert fw(a, 0, 64, 8, 8, eps, flags, b, c, None) == -2
        assert fw(a, 2, 64, 0, 8, eps, flags, b, c, None) == -2
        assert fw(a, 2, 64, 8, -1, eps, flags, b, c, None) == -2
        assert fw(a, 2, 257, 8, 8, eps, flags, b, c, None) == -3
        assert fw(a, 2, 0, 8, 8, eps, flags, b, c, None) == -3
        assert fw(a + 2, 2, 64, 8, 8, eps, flags, b, c, None) == -3
        assert fw(a, 2, 64, 8, 8, eps, flags, b + 2, c, None) == -3
        assert fw(a, 2, 64, 8, 8, eps, flags, a, c, None) == -3                       # y == x
        assert fw(a, 2, 64, 8, 8, eps, flags, a + 4 * 100, c, None) == -3             # y inside x
        assert fw(a, 1 << 20, 64, 64, 64, eps, flags, b, c, None) == -3               # N = 2^32
        assert bw(None, b, c, 2, 64, 8, 8, eps, flags, d, None) == -1
        assert bw(a, None, c, 2, 64, 8, 8, eps, flags, d, None) == -1
        assert bw(a, b, None, 2, 64, 8, 8, eps, flags, d, None) == -1
        assert bw(a, b, c, 2, 64, 8, 8, eps, flags, None, None) == -1
        assert bw(a, b, c, 0, 64, 8, 8, eps, flags, d, None) == -2
        assert bw(a, b, c, 2, 257, 8, 8, eps, flags, d, None) == -3
        assert bw(a, b, c + 2, 2, 64, 8, 8, eps, flags, d, None) == -3
        assert bw(a, b, c, 2, 64, 8, 8, eps, flags, a, None) == -3                    # grad_x == y
        assert bw(a, b, c, 2, 64, 8, 8, eps, flags, c, None) == -3                    # grad_x == grad_y


def test_front_ends_reject_cpu_and_other_tensors():
    from vqvae_amd import _lib, functional as F, training as T
    x = torch.zeros(2, 4, 3, 3)
    with pytest.raises(_lib.VqvaeHipError):
        F.l2norm_rows(x)
    with pytest.raises(_lib.VqvaeHipError):
        F.l2norm_rows(torch.zeros(5, 4))
    with pytest.raises(_lib.VqvaeHipError):
        F.l2norm_rows_backward(x, torch.zeros(18), x)
    with pytest.raises(_lib.VqvaeHipError):
        T.L2NormRows.apply(x.requires_grad_(True))
    assert F.l2norm_rows.__kwdefaults__ == {"rowmajor": False, "eps": 1e-12}
    assert F.l2norm_rows_backward.__kwdefaults__ == {"rowmajor": False, "eps": 1e-12}


def test_the_option_adds_no_state_and_the_default_is_todays_model():
    from vqvae_amd.modules import VQVAE, VectorQuantizer, VectorQuantizerEMA
    torch.manual_seed(0)
    a = VQVAE(32, 8, 1, 64, 16, 0.25)
    torch.manual_seed(0)
    b = VQVAE(32, 8, 1, 64, 16, 0.25, cosine_sim=True)
    torch.manual_seed(0)
    c = VQVAE(32, 8, 1, 64, 16, 0.25, cosine_sim=False)
    assert type(a.vector_quantization) is VectorQuantizer and a.vector_quantization.cosine_sim is False
    assert b.vector_quantization.cosine_sim is True and c.vector_quantization.cosine_sim is False
    for m in (b, c):
        assert list(a.state_dict()) == list(m.state_dict())
        for k, v in a.state_dict().items():
            assert torch.equal(v, m.state_dict()[k]), k
        assert [n for n, _ in a.named_buffers()] == [n for n, _ in m.named_buffers()]
        assert [n for n, _ in a.named_parameters()] == [n for n, _ in m.named_parameters()]
    assert list(VectorQuantizer(64, 16, 0.25, cosine_sim=True).state_dict()) == list(VectorQuantizer(64, 16, 0.25).state_dict())
    e0, e1 = VectorQuantizerEMA(64, 16, 0.25), VectorQuantizerEMA(64, 16, 0.25, cosine_sim=True)
    assert list(e0.state_dict()) == list(e1.state_dict()) and e1.cosine_sim and not e0.cosine_sim
    ema = VQVAE(32, 8, 1, 64, 16, 0.25, ema_decay=0.99, cosine_sim=True, rotation_trick=True)
    assert type(ema.vector_quantization) is VectorQuantizerEMA and ema.vector_quantization.cosine_sim
    assert ema.vector_quantization.rotation_trick
    with pytest.raises(TypeError):
        VectorQuantizer(64, 16, 0.25, False, True)          # keyword-only
    with pytest.raises(TypeError):
        VQVAE(32, 8, 1, 64, 16, 0.25, False, None, 1e-5, None, 1, False, False, True)
    with pytest.raises(ValueError):
        VQVAE(32, 8, 1, 64, 16, 0.25, n_quantizers=2, cosine_sim=True)
    VQVAE(32, 8, 1, 64, 16, 0.25, n_quantizers=2)           # (residual quantization itself is as it was)


def test_train_tool_option_is_absent_unless_given():
    src = open(os.path.join(ROOT, "tools", "train_checkpoint.py")).read()
    line = next(l for l in src.splitlines() if '"--cosine_sim"' in l)
    assert "argparse.SUPPRESS" in line


def test_kernel_text_on_the_host(tmp_path):
    """tests/host/cosine_harness.cpp compiles csrc/vq_cosine.h -- the per-row operations and the whole bodies of the kernels,
    forward and backward -- for the host with AddressSanitizer and UBSan and -ffp-contract=off, and compares them bit for bit with a
    scalar loop: both layouts, both access widths, the register forms, the re-reading form and the LDS forms (a workgroup runs as
    256 host threads with a barrier), D in {1, 3, 48, 64, 256} and others, HW % 4 != 0, zero rows, rows below eps, NaN and Inf rows
    (no NaN outside its row)."""
    import shutil
    import subprocess
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "cosine_harness")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "host", "cosine_harness.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "emulation ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
