"""The rotation-trick gradient without a GPU: the CPU restatement (tests/vq_rotation_ref.py) against fp64 torch autograd of the
paper's forward, its fallback rows, the C ABI's flag (defined, free of collisions, argument error before any launch), the modules'
option (no state, today's model by default) and the kernel's own text on the host under the sanitizers."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import vq_rotation_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _nearest(z, cb):
    z64, c64 = z.astype(np.float64), cb.astype(np.float64)
    d = (z64 * z64).sum(1)[:, None] - 2.0 * z64 @ c64.T + (c64 * c64).sum(1)[None, :]
    return d.argmin(1)


@pytest.mark.parametrize("scale", [0.05, 1.0])
@pytest.mark.parametrize("D", [1, 3, 48, 64, 256])
def test_restatement_agrees_with_fp64_autograd_of_the_papers_forward(D, scale):
    """elementwise within 2^-24 |ref| + 2^-40 lam ||g|| on every rotated row (measured when the option was written: at most 0.9997
    of the bound -- the fp32 rounding just below a power of two), and ||rot|| = lam ||g|| to the fp32 rounding of the elements
    (2^-24 each, so 2^-24 of the norm; measured at most 6e-8).  D = 1 produces antipodal rows by itself: sign flips."""
    z, cb, g = R.draw(4096, D, 64, scale, 100 * D + int(scale * 100), plant=False)
    idx = _nearest(z, cb)
    q = cb[idx]
    rot, rotate = R.rot(z, q, g)
    if D == 1:
        assert (~rotate).sum() > 0 and rotate.sum() > 0
    else:
        assert rotate.all()
    with np.errstate(all="ignore"):
        ref, lam_g, value_err = R.autograd_rot(z, q, g)
    ok = rotate
    assert value_err[ok].max() < 1e-12                      # the forward the reference differentiates does land on q
    err = np.abs(rot.astype(np.float64) - ref)[ok]
    bnd = R.bound(ref, lam_g)[ok]
    print(f"D={D} scale={scale}: max err / bound = {(err / bnd).max():.4f}")
    assert (err <= bnd).all()
    ratio = np.sqrt((rot.astype(np.float64) ** 2).sum(1))[ok] / lam_g[ok] - 1.0
    print(f"D={D} scale={scale}: max | ||rot|| / (lam ||g||) - 1 | = {np.abs(ratio).max():.3g}")
    assert np.abs(ratio).max() <= 2.0 ** -24 + 2.0 ** -40


def test_fallback_rows_return_g_bit_for_bit_and_a_nan_stays_in_its_row():
    z, cb, g = R.draw(64, 16, 8, 1.0, 7)
    cb, idx = R.plant_codes(z, cb, _nearest(z, cb))
    q = cb[idx]
    rot, rotate = R.rot(z, q, g)
    assert not rotate[0] and not rotate[1] and not rotate[2] and rotate[3]
    assert np.array_equal(rot[~rotate].view(np.uint32), g[~rotate].view(np.uint32))
    assert np.isnan(rot[3]).all()                           # the NaN of g's row 3 reaches all of that row's gradient ...
    assert np.isfinite(np.delete(rot, 3, axis=0)).all()     # ... and no other row
    z2 = z.copy()
    z2[5, 2] = np.nan                                       # a NaN in z: the row is not rotated
    rot2, rotate2 = R.rot(z2, q, g)
    assert not rotate2[5] and np.array_equal(rot2[5].view(np.uint32), g[5].view(np.uint32))
    q2 = q.copy()
    q2[6] = np.inf                                          # a non-finite norm
    assert not R.rot(z, q2, g)[1][6]
    # the threshold: ns2 just below 2^-20 falls back, just above rotates
    e = np.zeros((2, 2), np.float32)
    e[:, 0] = 1.0
    th = np.array([np.pi - 2.0 ** -10.5, np.pi - 2.0 ** -9.5])            # ns2 = 2 + 2 cos(th) ~ (pi - th)^2
    qq = np.stack([np.cos(th), np.sin(th)], 1).astype(np.float32)
    assert R.rot(e, qq, np.ones((2, 2), np.float32))[1].tolist() == [False, True]


def _flags():
    src = open(os.path.join(ROOT, "include", "vqvae_hip.h")).read()
    return {m.group(1): int(m.group(2), 16) for m in re.finditer(r"#define\s+(VQVAE_VQ_\w+)\s+(0x[0-9a-fA-F]+)", src)}


def test_the_flag_is_defined_and_collides_with_nothing_and_the_abi_stays_9():
    from vqvae_amd import _lib, build, functional as F
    lib = ctypes.CDLL(build.build())
    assert hasattr(lib, "vqvae_vq_backward_f32")
    assert _lib.load().vqvae_abi_version() == 9
    flags = _flags()
    rot = flags["VQVAE_VQ_BWD_ROTATION"]
    assert rot == F.VQ_BWD_ROTATION and rot > 0 and rot & (rot - 1) == 0
    for name, v in flags.items():
        if name != "VQVAE_VQ_BWD_ROTATION":
            assert not (v & rot), name
    assert "VQVAE_VQ_BWD_COMMITMENT" in flags and len(flags) >= 12


def test_flag_without_grad_z_is_a_null_error_before_any_launch():
    from vqvae_amd import _lib, functional as F
    L = _lib.load()
    a, big = 256, 1 << 40                      # a fake, aligned "device pointer" (never dereferenced)
    bw = L.vqvae_vq_backward_f32

    def call(flags, gz, ge, gzq=a):
        return bw(a, a, a, gzq, None, 1, 64, 8, 8, 16, 0.25, flags, gz, ge, a, big, None)

    assert call(F.VQ_BWD_ROTATION, None, a) == -1
    assert call(F.VQ_BWD_ROTATION | F.VQ_ROWMAJOR, None, a) == -1
    assert call(F.VQ_BWD_ROTATION | F.VQ_BWD_COMMITMENT, None, None) == -1
    assert call(F.VQ_BWD_ROTATION | F.VQ_BWD_COMMITMENT, a, a) == -3          # the commitment form has no codebook gradient


def test_front_end_rejects_cpu_tensors_and_rotation_without_grad_z():
    from vqvae_amd import _lib, training as T
    z, cb, idx = torch.zeros(1, 4, 2, 2), torch.zeros(3, 4), torch.zeros(4, dtype=torch.int64)
    with pytest.raises(_lib.VqvaeHipError):
        T.vq_backward(z, cb, idx, z, None, 0.25, rotation=True)
    with pytest.raises(_lib.VqvaeHipError):
        T.vq_backward(z, cb, idx, z, None, 0.25)
    with pytest.raises(ValueError):
        T.vq_backward(z, cb, idx, z, None, 0.25, rotation=True, need_z=False)


def test_the_option_adds_no_state_and_the_default_is_todays_model():
    from vqvae_amd.modules import VQVAE, VectorQuantizer, VectorQuantizerEMA
    torch.manual_seed(0)
    a = VQVAE(32, 8, 1, 64, 16, 0.25)
    torch.manual_seed(0)
    b = VQVAE(32, 8, 1, 64, 16, 0.25, rotation_trick=True)
    torch.manual_seed(0)
    c = VQVAE(32, 8, 1, 64, 16, 0.25, rotation_trick=False)
    assert type(a.vector_quantization) is VectorQuantizer and a.vector_quantization.rotation_trick is False
    assert b.vector_quantization.rotation_trick is True
    for m in (b, c):
        assert list(a.state_dict()) == list(m.state_dict())
        for k, v in a.state_dict().items():
            assert torch.equal(v, m.state_dict()[k]), k
        assert [n for n, _ in a.named_buffers()] == [n for n, _ in m.named_buffers()]
    assert list(VectorQuantizer(64, 16, 0.25, rotation_trick=True).state_dict()) == list(VectorQuantizer(64, 16, 0.25).state_dict())
    e0, e1 = VectorQuantizerEMA(64, 16, 0.25), VectorQuantizerEMA(64, 16, 0.25, rotation_trick=True)
    assert list(e0.state_dict()) == list(e1.state_dict()) and e1.rotation_trick and not e0.rotation_trick
    ema = VQVAE(32, 8, 1, 64, 16, 0.25, ema_decay=0.99, rotation_trick=True)
    assert type(ema.vector_quantization) is VectorQuantizerEMA and ema.vector_quantization.rotation_trick
    with pytest.raises(TypeError):
        VectorQuantizer(64, 16, 0.25, True)                 # keyword-only
    with pytest.raises(ValueError):
        VQVAE(32, 8, 1, 64, 16, 0.25, n_quantizers=2, rotation_trick=True)
    VQVAE(32, 8, 1, 64, 16, 0.25, n_quantizers=2)           # (residual quantization itself is as it was)


def test_train_tool_option_is_absent_unless_given():
    src = open(os.path.join(ROOT, "tools", "train_checkpoint.py")).read()
    line = next(l for l in src.splitlines() if '"--rotation_trick"' in l)
    assert "argparse.SUPPRESS" in line


def test_kernel_text_on_the_host(tmp_path):
    """tests/host/rotation_harness.cpp compiles csrc/vq_rotation.h -- the per-row coefficients and the whole body of the kernel -- for
    the host with AddressSanitizer and UBSan and -ffp-contract=off, and compares it bit for bit with a scalar loop: both layouts,
    both access widths, the register forms and the re-reading form, zero rows, zero codes, antipodal rows, NaNs in g and z and
    indices of K and -1 among the rows (no read outside the codebook, no NaN outside its row)."""
    import shutil
    import subprocess
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "rotation_harness")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "host", "rotation_harness.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "emulation ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
