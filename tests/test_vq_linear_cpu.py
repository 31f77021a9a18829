"""The per-row linear map and the factorized quantizer without a GPU: the CPU restatement (tests/vq_linear_ref.py) against fp64 torch
autograd of F.linear, the kernels' own text on the host under the sanitizers, the C ABI's three entries (declared, bound, argument
errors before any launch, ABI still 9), the front ends' refusal of CPU tensors, the constructor rules and the train tool's option."""
import os
import re
import struct

import numpy as np
import pytest
import torch

from tests import vq_linear_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("N,Cin,Cout", [(300, 64, 8), (300, 8, 64), (700, 7, 5), (1, 1, 1), (260, 33, 65)])
def test_restatement_agrees_with_fp64_torch_autograd(N, Cin, Cout):
    """y and grad_x: the restatement is an fp64 sum rounded once, compared with torch's UNROUNDED fp64 value: the rounding moves it
    by at most half an fp32 ulp, 2^-24 |ref|, and the two fp64 sums (other orders, at most 256 exact products) differ by a few
    2^-53 of the terms' magnitudes, for which 2^-48 sum |term| leaves room: 2^-24 |ref| + 2^-48 sum |term|.  The parameter
    gradients are sums of up to 700 terms in another order: 2^-23 |ref| +
    2^-40 sum |term|, the bound tests/test_vq_fsq_cpu.py derives for the same sums (N <= 2^11 additions of 2^-53 relative error each)."""
    rng = np.random.default_rng(5 * N + Cin)
    x = rng.standard_normal((N, Cin)).astype(np.float32)
    gy = rng.standard_normal((N, Cout)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin)) / np.sqrt(Cin)).astype(np.float32)
    b = (0.1 * rng.standard_normal(Cout)).astype(np.float32)
    t = {n: torch.from_numpy(v.astype(np.float64)).requires_grad_(True) for n, v in dict(x=x, w=w, b=b).items()}
    y = torch.nn.functional.linear(t["x"], t["w"], t["b"])
    y.backward(torch.from_numpy(gy.astype(np.float64)))
    a64 = lambda v: np.abs(v.astype(np.float64))
    ref = y.detach().numpy()
    mag = a64(x) @ a64(w).T + a64(b)[None, :]
    assert (np.abs(R.forward(x, w, b) - ref) <= 2.0 ** -24 * np.abs(ref) + 2.0 ** -48 * mag + 2.0 ** -149).all()
    ref = t["x"].grad.numpy()
    mag = a64(gy) @ a64(w)
    assert (np.abs(R.grad_x(gy, w) - ref) <= 2.0 ** -24 * np.abs(ref) + 2.0 ** -48 * mag + 2.0 ** -149).all()
    (_, _), (mw, mb) = R.param_grads(x, gy)
    gw, gb = R.param_grads_blocked(x, gy)
    for got, want, m in ((gw, t["w"].grad.numpy(), mw), (gb, t["b"].grad.numpy(), mb)):
        assert got.dtype == np.float32 and (np.abs(got - want) <= 2.0 ** -23 * np.abs(want) + 2.0 ** -40 * m + 2.0 ** -149).all()


def test_the_restatement_keeps_a_non_finite_value_in_its_row():
    x, gy, w, b, y, gx, gw, gb = R.expected((2, 7, 7, 6, 5))
    assert np.isnan(y[1]).all() and not np.isfinite(y[96]).any() and np.isfinite(np.delete(y, [1, 96], 0)).all()
    assert np.isnan(gx[1]).all() and not np.isfinite(gx[96]).any() and np.isfinite(np.delete(gx, [1, 96], 0)).all()
    assert np.isnan(gw[4]).all() and np.isnan(gw[:, 3]).all() and np.isnan(gb[4]) and np.isfinite(gw[1:4, 1:3]).all()


# ---- the kernels' own text on the host --------------------------------------------------------------------------------------------

def host_case_bytes(case):
    B, H, W, Cin, Cout = case
    x, gy, w, b, y, gx, gw, gb = R.expected(case)
    parts = [np.array([B, H * W, Cin, Cout], np.int32), x, gy, w, b, y, gx, gw, gb]
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


def test_kernel_text_on_the_host(tmp_path):
    """tests/host/linear_harness.cpp compiles csrc/vq_linear.h -- the whole bodies of the kernels -- for the host with AddressSanitizer
    and UBSan and -ffp-contract=off, runs forward, grad_x, the parameter gradients' block kernel and their second launch over the GPU
    test's shapes in both layouts and on both access paths (a workgroup runs as 256 host threads with a barrier), and compares every
    output bit for bit with the restatement's values written here: NaN and Inf rows, odd widths, ragged last blocks, the envelope's
    corner among them."""
    import shutil
    import subprocess
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe, data = str(tmp_path / "linear_harness"), str(tmp_path / "cases.bin")
    with open(data, "wb") as fh:
        fh.write(struct.pack("<i", len(R.GPU_CASES)))
        for case in R.GPU_CASES:
            fh.write(host_case_bytes(case))
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-pthread", "-o", exe, os.path.join(ROOT, "tests", "host", "linear_harness.cpp")])
    out = subprocess.run([exe, data], capture_output=True, text=True)
    assert out.returncode == 0 and "emulation ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


# ---- header and binding -----------------------------------------------------------------------------------------------------------

NAMES = ("vqvae_linear_rows_forward_f32", "vqvae_linear_rows_backward_workspace_bytes", "vqvae_linear_rows_backward_f32")


def test_entries_are_declared_and_bound_and_the_abi_stays_9():
    import ctypes
    from vqvae_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    src = open(os.path.join(ROOT, "include", "vqvae_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert re.search(r"VQVAE_API\s+(int|size_t)\s+" + name + r"\s*\(", src)
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [11, 3, 15]
    assert _lib.load().vqvae_abi_version() == 9 and re.search(r"#define VQVAE_HIP_ABI_VERSION 9\b", src)


def test_the_sizing_call_and_the_argument_errors_come_back_before_any_launch():
    from vqvae_amd import _lib
    L = _lib.load()
    size = L.vqvae_linear_rows_backward_workspace_bytes
    assert size(128, 64, 8) == (8 * 64 + 8) * 8                                    # one block of 256 rows
    assert size(256, 64, 8) == size(128, 64, 8) and size(257, 64, 8) == 2 * size(128, 64, 8)
    assert size(300, 256, 256) == 2 * (256 * 256 + 256) * 8
    for bad in ((0, 64, 8), (1 << 31, 64, 8), (128, 0, 8), (128, 257, 8), (128, 64, 0), (128, 64, 257)):
        assert size(*bad) == 0, bad
    M = 1 << 24                                                # fake, aligned, disjoint "device pointers" (never dereferenced)
    x, w, b, y, g, gx, gw, gb, ws = [M * (i + 1) for i in range(9)]
    fw, bw = L.vqvae_linear_rows_forward_f32, L.vqvae_linear_rows_backward_f32
    big = 1 << 30
    for flags in (0, 1):
        def F(**k):
            a = dict(x=x, w=w, b=b, B=2, Cin=64, H=8, W=8, Cout=8, y=y)
            a.update(k)
            return fw(a["x"], a["w"], a["b"], a["B"], a["Cin"], a["H"], a["W"], a["Cout"], flags, a["y"], None)

        def Bk(**k):
            a = dict(x=x, g=g, w=w, B=2, Cin=64, H=8, W=8, Cout=8, gx=gx, gw=gw, gb=gb, ws=ws, n=big)
            a.update(k)
            return bw(a["x"], a["g"], a["w"], a["B"], a["Cin"], a["H"], a["W"], a["Cout"], flags, a["gx"], a["gw"], a["gb"], a["ws"],
                      a["n"], None)

        for name in ("x", "w", "b", "y"):
            assert F(**{name: None}) == -1, name
        for name in ("x", "g", "w"):
            assert Bk(**{name: None}) == -1, name
        assert Bk(gx=None, gw=None, gb=None) == -1
        for call in (F, Bk):
            assert call(B=0) == -2 and call(H=0) == -2 and call(W=-1) == -2 and call(Cin=0) == -2 and call(Cout=0) == -2
            assert call(Cout=257) == -3 and call(Cin=257) == -3 and call(B=1 << 20, H=64, W=64) == -3
        assert fw(x, w, b, 2, 64, 8, 8, 8, flags | 2, y, None) == -3
        for name in ("x", "w", "b", "y"):
            assert F(**{name: x + 2 + M * 20}) == -3, name
        for name in ("x", "g", "w", "gx", "gw", "gb"):
            assert Bk(**{name: x + 2 + M * 20}) == -3, name
        assert Bk(ws=ws + 4) == -3
        assert F(y=x) == -3 and F(y=x + 400) == -3 and F(y=w) == -3 and F(y=b) == -3
        assert Bk(gx=x) == -3 and Bk(gx=g + 64) == -3 and Bk(gw=w) == -3 and Bk(gb=g) == -3 and Bk(ws=x) == -3 and Bk(gw=gx) == -3
        need = size(128, 64, 8)
        assert Bk(ws=None) == -4 and Bk(n=need - 8) == -4 and Bk(gx=None, gw=None, ws=None) == -4
    # (grad_x alone needs no workspace: with fake pointers that would launch, so the GPU test covers it)


def test_front_ends_reject_cpu_tensors():
    from vqvae_amd import _lib, functional as F, training as T
    x, w, b = torch.zeros(2, 16, 3, 3), torch.zeros(4, 16), torch.zeros(4)
    with pytest.raises(_lib.VqvaeHipError):
        F.linear_rows(x, w, b)
    with pytest.raises(_lib.VqvaeHipError):
        F.linear_rows_backward(x, torch.zeros(2, 4, 3, 3), w)
    with pytest.raises(_lib.VqvaeHipError):
        T.LinearRows.apply(x.requires_grad_(True), w, b, False)
    with pytest.raises(_lib.VqvaeHipError):
        F.linear_rows_backward_workspace(1 << 32, 16, 4, "cpu")
    assert F.linear_rows.__kwdefaults__ == {"rowmajor": False}
    assert F.linear_rows_backward.__kwdefaults__ == {"rowmajor": False, "want": (True, True, True), "workspace": None}


# ---- construction on the CPU ------------------------------------------------------------------------------------------------------

DIMS = (32, 8, 1, 64, 16, 0.25)


def _vq_state(m):
    return {k[len("vector_quantization."):]: tuple(v.shape) for k, v in m.state_dict().items() if k.startswith("vector_quantization.")}


def test_the_factorized_model_constructs_with_exactly_its_state():
    from vqvae_amd.modules import VQVAE, FactorizedVectorQuantizer, FactorizedVectorQuantizerEMA
    plain = {"embedding.weight": (64, 4), "project_in.weight": (4, 16), "project_in.bias": (4,), "project_out.weight": (16, 4),
             "project_out.bias": (16,)}
    m = VQVAE(*DIMS, codebook_dim=4)
    vq = m.vector_quantization
    assert type(vq) is FactorizedVectorQuantizer and _vq_state(m) == plain
    assert (vq.n_e, vq.e_dim, vq.dim, vq.codebook_dim) == (64, 4, 16, 4) and vq.embedding.weight.requires_grad
    assert float(vq.embedding.weight.detach().abs().max()) <= 1.0 / 64
    for kw in (dict(rotation_trick=True), dict(cosine_sim=True), dict(rotation_trick=True, cosine_sim=True)):
        q = VQVAE(*DIMS, codebook_dim=4, **kw).vector_quantization
        assert type(q) is FactorizedVectorQuantizer and (q.rotation_trick, q.cosine_sim) == (kw.get("rotation_trick", False), kw.get("cosine_sim", False))
    e = VQVAE(*DIMS, codebook_dim=4, ema_decay=0.99, ema_eps=1e-4, restart_threshold=1.0, cosine_sim=True)
    vq = e.vector_quantization
    assert type(vq) is FactorizedVectorQuantizerEMA and isinstance(vq, FactorizedVectorQuantizer)
    assert _vq_state(e) == dict(plain, ema_cluster_size=(64,), ema_w=(64, 4))
    assert not vq.embedding.weight.requires_grad and vq.project_in.weight.requires_grad and vq.project_out.bias.requires_grad
    assert (vq.decay, vq.eps, vq.restart_threshold, vq.cosine_sim) == (0.99, 1e-4, 1.0, True)
    assert torch.equal(vq.ema_w, vq.embedding.weight) and not vq.ema_cluster_size.any()
    assert VQVAE(*DIMS, codebook_dim=16).vector_quantization.project_in.weight.shape == (16, 16)
    # the order the three are drawn in: the codebook as VectorQuantizer draws it, then project_in, then project_out
    torch.manual_seed(3)
    q = FactorizedVectorQuantizer(64, 16, 4, 0.25)
    torch.manual_seed(3)
    emb = torch.nn.Embedding(64, 4)
    emb.weight.data.uniform_(-1.0 / 64, 1.0 / 64)
    p_in, p_out = torch.nn.Linear(16, 4), torch.nn.Linear(4, 16)
    for got, want in ((q.embedding.weight, emb.weight), (q.project_in.weight, p_in.weight), (q.project_in.bias, p_in.bias),
                      (q.project_out.weight, p_out.weight), (q.project_out.bias, p_out.bias)):
        assert torch.equal(got, want)


def test_excluded_combinations_raise():
    from vqvae_amd.modules import VQVAE
    for kw in (dict(n_quantizers=2), dict(n_quantizers=2, shared_codebook=True), dict(shared_codebook=True), dict(codebook_groups=2),
               dict(fsq_levels=(4, 4, 4)), dict(lookup_free=True), dict(restart_threshold=1.0)):
        with pytest.raises(ValueError):
            VQVAE(*DIMS, codebook_dim=4, **kw)
    for bad in (0, 257, -1, 2.5, True):
        with pytest.raises(ValueError):
            VQVAE(*DIMS, codebook_dim=bad)
    with pytest.raises(TypeError):
        VQVAE(32, 8, 1, 64, 16, 0.25, False, None, 1e-5, None, 1, False, False, False, None, 1, False, 0.1, 1.0, 100.0, 4)   # keyword-only
    import inspect
    assert list(inspect.signature(VQVAE.__init__).parameters)[-1] == "codebook_dim"


def test_the_default_is_todays_model():
    from vqvae_amd.modules import VQVAE, VectorQuantizer
    torch.manual_seed(0)
    a = VQVAE(*DIMS)
    after_a = torch.rand(4)
    torch.manual_seed(0)
    b = VQVAE(*DIMS, codebook_dim=None)
    after_b = torch.rand(4)
    assert type(b.vector_quantization) is VectorQuantizer and torch.equal(after_a, after_b)      # no random number drawn on the way
    assert list(a.state_dict()) == list(b.state_dict())
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]), k


def test_the_fused_entries_never_see_a_low_dimensional_codebook():
    from vqvae_amd._lib import VqvaeHipError
    from vqvae_amd.modules import VQVAE
    for kw in ({}, dict(ema_decay=0.99)):
        with pytest.raises(VqvaeHipError):
            VQVAE(*DIMS, codebook_dim=4, **kw)._c_weights()


def test_train_tool_option_is_absent_unless_given():
    src = open(os.path.join(ROOT, "tools", "train_checkpoint.py")).read()
    line = next(l for l in src.splitlines() if '"--codebook_dim"' in l)
    assert "argparse.SUPPRESS" in line
