"""The orthogonal regularization loss without a GPU: the CPU restatement (tests/vq_orthogonal_ref.py) against fp64 torch autograd of
the library's formula, the selection rule, the kernels' own text on the host under the sanitizers, the C ABI's three entries (declared,
bound, argument errors before any launch, ABI still 9), the front ends' refusal of CPU tensors, the constructor rules, the unchanged
default model and the train tool's options."""
import os
import re
import struct

import numpy as np
import pytest
import torch

from tests import vq_orthogonal_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("K,D,mode", [(300, 64, "all"), (300, 64, "hist"), (130, 7, "cap"), (40, 256, "all"), (5, 3, "hist")])
def test_restatement_agrees_with_fp64_torch_autograd(K, D, mode):
    """The library's formula in fp64 torch: E = rows[selected], G = E E^T, loss = sum(G^2) / M^2 - 1 / M, and its autograd.

    The rows have unit length up to fp32 rounding, so |G_ij| <= 1 + 2^-22 and sum_c |n_ic n_jc| <= 1 + 2^-22.  Write s^2 = T / M^2.
    G: a sum of D exact products; either implementation is off by at most D 2^-53 (1 + ...), the two differ by dG <= 2 D 2^-53.
    T / M^2: (a) dG moves a term G^2 by 2 |G| dG, the mean of |G| is at most s (Jensen): 4 D 2^-53 s; (b) each product G G is
    rounded, and M^2 non-negative terms are added in some order with at most K + 256 + 64 additions on the path of any term and
    the product's rounding and one more for slack: (K + 322) 2^-53 s^2 on each side, 2 (K + 322) 2^-53 s^2 together; (c) the
    division, 1 / M and the subtraction: 3 roundings of values <= max(s^2, 1), 4 2^-53 max(s^2, 1) with slack.  The subtraction of 1 / M makes the bound
    absolute, in units of s^2, not relative to the loss.  Last, the restatement rounds to fp32: 2^-24 |loss|.

    grad[i][c] = (4 g / M^2) sum_j G_ij n_jc over the selected j: with mag_c = (4 |g| / M^2) sum_j |n_jc|, dG moves it by 2 D 2^-53
    mag_c, the products' and the sum's roundings (at most K additions) by (K + 2) 2^-53 mag_c (1 + 2^-22) on each side, the scale's
    three roundings by 3 2^-53 |grad|; the rounding to fp32 by 2^-24 |grad|.  Used: 2^-24 |ref| + (2 D + 2 K + 8) 2^-53 mag_c."""
    rng = np.random.default_rng(100 * K + D)
    rows = R.draw_rows(K, D, 7 + K + D)
    hist = None if mode == "all" else rng.integers(0, 2, K).astype(np.int32)
    if hist is not None:
        hist[K // 2] = 1
    u = rng.random(K).astype(np.float32) if mode == "cap" else None
    max_codes = 37 if mode == "cap" else None
    g = 0.75
    loss, M, sel, V = R.forward(rows, hist, u, max_codes)
    grad = R.backward(V, sel, M, g)
    assert M == int(sel.sum()) and M >= 1 and (mode != "cap" or M == 37)
    n = torch.from_numpy(rows.astype(np.float64)).requires_grad_(True)
    E = n[torch.from_numpy(sel.astype(bool))]
    G = E @ E.T
    s2 = (G ** 2).sum() / (M * M)
    ref = s2 - 1.0 / M
    (g * ref).backward()
    s2, ref = float(s2.detach()), float(ref.detach())
    bound = 2.0 ** -24 * abs(ref) + 2.0 ** -53 * (4 * D * np.sqrt(s2) + 2 * (K + 322) * s2 + 4 * max(s2, 1.0))
    assert loss.dtype == np.float32 and abs(float(loss) - ref) <= bound
    want = n.grad.numpy()
    mag = (4 * abs(g) / (M * M)) * np.abs(rows.astype(np.float64))[sel != 0].sum(0)[None, :]
    assert grad.dtype == np.float32 and (np.abs(grad - want) <= 2.0 ** -24 * np.abs(want) + (2 * D + 2 * K + 8) * 2.0 ** -53 * mag + 2.0 ** -149).all()
    assert not grad[sel == 0].any() and not np.signbit(grad[sel == 0]).any()


def test_the_loss_of_an_orthonormal_set_is_zero_and_of_equal_rows_is_the_largest():
    eye = np.eye(8, 16, dtype=np.float32)
    loss, M, sel, V = R.forward(eye)
    assert M == 8 and float(loss) == 0.0 and np.array_equal(V, eye.astype(np.float64))
    same = np.tile(eye[:1], (8, 1))
    assert float(R.forward(same)[0]) == np.float32(1.0 - 1.0 / 8)


def test_the_selection_rule():
    K = 12
    hist = np.array([3, 0, 1, 1, 0, 2, 9, 1, 0, 1, 1, 4], np.int32)
    u = np.array([.5, .0, .25, .5, .0, .25, .75, .25, .0, .5, .125, .5], np.float32)
    cand = [0, 2, 3, 5, 6, 7, 9, 10, 11]
    assert list(np.flatnonzero(R.select(K, hist))) == cand
    assert R.select(K).all() and R.select(K).dtype == np.int32
    # the order (u, k): 10 (.125), 2, 5, 7 (.25 by k), 0, 3, 9, 11 (.5 by k), 6
    order = [10, 2, 5, 7, 0, 3, 9, 11, 6]
    for m in range(1, 12):
        assert sorted(np.flatnonzero(R.select(K, hist, u, m))) == sorted(order[:m]), m
    # no cap: max_codes None or <= 0, or no uniforms
    for kw in (dict(uniforms=u, max_codes=None), dict(uniforms=u, max_codes=0), dict(uniforms=None, max_codes=3)):
        assert list(np.flatnonzero(R.select(K, hist, **kw))) == cand
    # without hist every code is a candidate; ties at u = 0: 1, 4, 8 by k
    assert sorted(np.flatnonzero(R.select(K, None, u, 4))) == [1, 4, 8, 10]


def test_no_code_and_one_code():
    rows = R.draw_rows(9, 5, 3)
    loss, M, sel, V = R.forward(rows, np.zeros(9, np.int32))
    g = R.backward(V, sel, M, 2.0)
    assert M == 0 and loss.dtype == np.float32 and float(loss) == 0.0 and not sel.any() and not V.any() and not g.any()
    assert not np.signbit(g).any()
    one = np.zeros(9, np.int32)
    one[4] = 1
    loss, M, sel, V = R.forward(rows, one)
    n = rows[4].astype(np.float64)
    G = np.float64(0.0)
    for c in range(5):
        G = G + n[c] * n[c]
    assert M == 1 and list(np.flatnonzero(sel)) == [4] and float(loss) == float(np.float32(G * G / 1.0 - 1.0))
    assert np.array_equal(V[4], G * n) and not np.delete(V, 4, 0).any()
    assert np.array_equal(R.backward(V, sel, M)[4], (4.0 * V[4]).astype(np.float32))


def test_a_non_finite_value_stays_out_of_unselected_rows():
    a, (loss, M, sel, V, g) = R.expected((5, 3))["non_finite"]
    assert sel[0] == 0 and sel[4] == 1 and not np.isfinite(a["rows"][0]).all()
    assert np.isnan(loss) and np.isnan(V[sel != 0]).all() and np.isnan(g[sel != 0]).all()
    assert not V[sel == 0].any() and not g[sel == 0].any()


# ---- the kernels' own text on the host --------------------------------------------------------------------------------------------

def host_case_bytes(a, want):
    loss, M, sel, V, g = want
    K, D = a["rows"].shape
    head = np.array([K, D, a["hist"] is not None, a["uniforms"] is not None, a["max_codes"] or 0, a["grad_loss"] is not None], np.int32)
    parts = [head, np.array([a["grad_loss"] or 0.0], np.float32), a["rows"]]
    parts += [p for p in (a["hist"], a["uniforms"]) if p is not None]
    parts += [np.array([loss], np.float32), np.array([M], np.int32), sel, V, g]
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


def test_kernel_text_on_the_host(tmp_path):
    """tests/host/orthogonal_harness.cpp compiles csrc/vq_orthogonal.h -- the whole bodies of the kernels -- for the host with
    AddressSanitizer and UBSan and -ffp-contract=off, runs the selection, the main kernel, the total and the backward over the GPU
    test's shapes and calls (a workgroup runs as 256 host threads with a barrier) and compares loss, count, selected, V and grad_rows
    bit for bit with the restatement's values written here.  (Of the four larger shapes, whose every workgroup costs the host
    thousands of barrier waits, three calls each: every code, a capped selection, a non-finite row.)"""
    import shutil
    import subprocess
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe, data = str(tmp_path / "orthogonal_harness"), str(tmp_path / "cases.bin")
    cases = []
    for shape in R.GPU_SHAPES:
        for name, c in R.expected(shape).items():
            if shape[0] * shape[1] <= 1000 or name in ("plain", "cap_below", "non_finite"):
                cases.append(c)
    with open(data, "wb") as fh:
        fh.write(struct.pack("<i", len(cases)))
        for a, want in cases:
            fh.write(host_case_bytes(a, want))
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-pthread", "-o", exe,
                           os.path.join(ROOT, "tests", "host", "orthogonal_harness.cpp")])
    out = subprocess.run([exe, data], capture_output=True, text=True)
    assert out.returncode == 0 and "emulation ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


# ---- header and binding -----------------------------------------------------------------------------------------------------------

NAMES = ("vqvae_vq_orthogonal_workspace_bytes", "vqvae_vq_orthogonal_forward_f32", "vqvae_vq_orthogonal_backward_f32")


def test_entries_are_declared_and_bound_and_the_abi_stays_9():
    import ctypes
    from vqvae_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    src = open(os.path.join(ROOT, "include", "vqvae_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert re.search(r"VQVAE_API\s+(int|size_t)\s+" + name + r"\s*\(", src)
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [2, 14, 8]
    assert _lib.load().vqvae_abi_version() == 9 and re.search(r"#define VQVAE_HIP_ABI_VERSION 9\b", src)


def test_the_sizing_call_and_the_argument_errors_come_back_before_any_launch():
    from vqvae_amd import _lib
    L = _lib.load()
    size = L.vqvae_vq_orthogonal_workspace_bytes
    assert size(512, 64) == 512 * 8 and size(16384, 256) == 16384 * 8 and size(1, 1) == 8
    for bad in ((0, 64), (16385, 64), (512, 0), (512, 257), (-1, 64)):
        assert size(*bad) == 0, bad
    M = 1 << 24                                                # fake, aligned, disjoint "device pointers" (never dereferenced)
    rows, hist, u, loss, count, sel, saved, ws, gl, grad = [M * (i + 1) for i in range(10)]
    fw, bw = L.vqvae_vq_orthogonal_forward_f32, L.vqvae_vq_orthogonal_backward_f32

    def F(**k):
        a = dict(rows=rows, hist=hist, u=u, m=8, K=64, D=16, flags=0, loss=loss, count=count, sel=sel, saved=saved, ws=ws, n=64 * 8)
        a.update(k)
        return fw(a["rows"], a["hist"], a["u"], a["m"], a["K"], a["D"], a["flags"], a["loss"], a["count"], a["sel"], a["saved"],
                  a["ws"], a["n"], None)

    def B(**k):
        a = dict(saved=saved, sel=sel, count=count, gl=gl, K=64, D=16, grad=grad)
        a.update(k)
        return bw(a["saved"], a["sel"], a["count"], a["gl"], a["K"], a["D"], a["grad"], None)

    for name in ("rows", "loss", "count", "sel"):
        assert F(**{name: None}) == -1, name
    for name in ("saved", "sel", "count", "grad"):
        assert B(**{name: None}) == -1, name
    for call in (F, B):
        assert call(K=0) == -2 and call(D=0) == -2 and call(K=-5) == -2
        assert call(K=16385) == -3 and call(D=257) == -3
    assert F(flags=1) == -3 and F(flags=-1) == -3
    for name in ("rows", "hist", "u", "loss", "count", "sel"):
        assert F(**{name: rows + 2 + M * 20}) == -3, name                          # not 4-byte aligned
    assert F(saved=saved + 4) == -3 and F(ws=ws + 4) == -3                          # not 8-byte aligned
    assert B(saved=saved + 4) == -3 and B(grad=grad + 2) == -3
    # an output on an input, or on another output
    assert F(sel=rows) == -3 and F(saved=rows + 64) == -3 and F(loss=hist + 8) == -3 and F(count=u) == -3 and F(ws=rows) == -3
    assert F(loss=count) == -3 and F(saved=ws) == -3 and F(sel=saved + 8) == -3
    assert B(grad=saved) == -3 and B(grad=sel) == -3 and B(grad=count) == -3 and B(grad=gl) == -3
    assert F(ws=None) == -4 and F(n=64 * 8 - 8) == -4


def test_front_ends_reject_cpu_tensors():
    from vqvae_amd import _lib, functional as F, training as T
    rows = torch.zeros(8, 4)
    with pytest.raises(_lib.VqvaeHipError):
        F.vq_orthogonal_forward(rows)
    with pytest.raises(_lib.VqvaeHipError):
        F.vq_orthogonal_backward(torch.zeros(8, 4, dtype=torch.float64), torch.zeros(8, dtype=torch.int32), torch.zeros((), dtype=torch.int32))
    with pytest.raises(_lib.VqvaeHipError):
        T.OrthogonalLoss.apply(rows.requires_grad_(True), None, None, None, None)
    with pytest.raises(_lib.VqvaeHipError):
        F.vq_orthogonal_workspace(1 << 20, 4, "cpu")
    assert F.vq_orthogonal_forward.__kwdefaults__ == {"max_codes": None, "uniforms": None, "want_saved": False, "workspace": None}


# ---- construction on the CPU ------------------------------------------------------------------------------------------------------

DIMS = (32, 8, 1, 64, 16, 0.25)


def test_the_option_constructs_on_the_gradient_trained_one_stage_quantizers():
    from vqvae_amd.modules import VQVAE, FactorizedVectorQuantizer, VectorQuantizer
    for kw, cls in ((dict(), VectorQuantizer), (dict(rotation_trick=True), VectorQuantizer), (dict(cosine_sim=True), VectorQuantizer),
                    (dict(codebook_dim=4), FactorizedVectorQuantizer), (dict(codebook_dim=4, cosine_sim=True), FactorizedVectorQuantizer)):
        plain = VQVAE(*DIMS, **kw)
        m = VQVAE(*DIMS, orthogonal_reg_weight=10.0, orthogonal_reg_active_codes_only=True, orthogonal_reg_max_codes=32, **kw)
        vq = m.vector_quantization
        assert type(vq) is cls and list(m.state_dict()) == list(plain.state_dict())
        assert (vq.orthogonal_reg_weight, vq.orthogonal_reg_active_codes_only, vq.orthogonal_reg_max_codes) == (10.0, True, 32)
        assert vq.last_orthogonal_loss is None and vq.generator is None
    g = torch.Generator()
    assert VectorQuantizer(64, 16, 0.25, orthogonal_reg_weight=1.0, generator=g).generator is g
    assert FactorizedVectorQuantizer(64, 16, 4, 0.25, orthogonal_reg_weight=1.0, generator=g).generator is g


def test_excluded_combinations_raise():
    from vqvae_amd.modules import VQVAE, VectorQuantizer
    for kw in (dict(ema_decay=0.99), dict(ema_decay=0.99, codebook_dim=4), dict(n_quantizers=2), dict(codebook_groups=2),
               dict(fsq_levels=(4, 4, 4)), dict(lookup_free=True)):
        with pytest.raises(ValueError):
            VQVAE(*DIMS, orthogonal_reg_weight=1.0, **kw)
        VQVAE(*DIMS, orthogonal_reg_weight=0.0, orthogonal_reg_max_codes=8, **kw)      # at weight 0 the option is off: nothing to refuse
    for bad in (-1.0, -1e-9, float("nan")):
        with pytest.raises(ValueError):
            VQVAE(*DIMS, orthogonal_reg_weight=bad)
        with pytest.raises(ValueError):
            VectorQuantizer(64, 16, 0.25, orthogonal_reg_weight=bad)
    for bad in (0, -3, 2.5, True):
        with pytest.raises(ValueError):
            VQVAE(*DIMS, orthogonal_reg_weight=1.0, orthogonal_reg_max_codes=bad)
    with pytest.raises(TypeError):                                                  # keyword-only
        VectorQuantizer(64, 16, 0.25, False, False, 1.0)


def test_the_default_is_todays_model():
    from vqvae_amd.modules import VQVAE, VectorQuantizer
    torch.manual_seed(0)
    a = VQVAE(*DIMS)
    after_a = torch.rand(4)
    torch.manual_seed(0)
    b = VQVAE(*DIMS, orthogonal_reg_weight=0.0, orthogonal_reg_active_codes_only=False, orthogonal_reg_max_codes=None)
    after_b = torch.rand(4)
    torch.manual_seed(0)
    c = VQVAE(*DIMS, orthogonal_reg_weight=5.0, orthogonal_reg_max_codes=16)
    after_c = torch.rand(4)
    for m, after in ((b, after_b), (c, after_c)):
        assert type(m.vector_quantization) is VectorQuantizer and torch.equal(after_a, after)    # no random number drawn on the way
        assert list(a.state_dict()) == list(m.state_dict())
        for k, v in a.state_dict().items():
            assert torch.equal(v, m.state_dict()[k]), k
    assert b.vector_quantization.orthogonal_reg_weight == 0.0 and b.vector_quantization.last_orthogonal_loss is None


def test_train_tool_options_are_absent_unless_given():
    src = open(os.path.join(ROOT, "tools", "train_checkpoint.py")).read()
    for opt in ("--orthogonal_reg_weight", "--orthogonal_reg_active_codes_only", "--orthogonal_reg_max_codes"):
        line = next(l for l in src.splitlines() if f'"{opt}"' in l)
        assert "argparse.SUPPRESS" in line
    from tools import train_checkpoint as tc
    assert tc.parse([])[1] == {}
    assert tc.parse(["--orthogonal_reg_weight", "10", "--orthogonal_reg_active_codes_only", "--orthogonal_reg_max_codes", "128"])[1] == \
        dict(orthogonal_reg_weight=10.0, orthogonal_reg_active_codes_only=True, orthogonal_reg_max_codes=128)
