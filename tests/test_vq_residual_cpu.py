"""Residual vector quantization without a GPU: the C ABI's new entries (exported, bound, sized, argument errors before any launch),
the CPU restatement (tests/rvq_ref.py) against the reference port at Q = 1 and against torch autograd of the composition, and the
modules' state_dict layout."""
import ctypes

import numpy as np
import pytest
import torch

from tests import rvq_ref as R

NEW = ("vqvae_vq_residual_workspace_bytes", "vqvae_vq_residual_forward_f32", "vqvae_vq_residual_decode_f32",
       "vqvae_vq_residual_backward_workspace_bytes", "vqvae_vq_residual_backward_f32")


def test_new_symbols_are_exported_and_bound_and_the_abi_stays_9():
    from vqvae_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    for s in NEW:
        assert hasattr(lib, s)
        assert s in _lib.SIGNATURES
        assert getattr(_lib.load(), s).argtypes is not None
    assert _lib.load().vqvae_abi_version() == 9


def test_workspace_sizing_envelope():
    from vqvae_amd import _lib
    L = _lib.load()
    f, b = L.vqvae_vq_residual_workspace_bytes, L.vqvae_vq_residual_backward_workspace_bytes
    one = L.vqvae_vq_workspace_bytes(192, 512, 64)
    assert f(192, 512, 64, 1, 0) >= one                                     # one stage: the quantizer's own workspace
    assert f(192, 512, 64, 4, 0) >= 4 * one + 192 * 64 * 4                  # an image per codebook and the residual map
    assert one + 192 * 64 * 4 <= f(192, 512, 64, 4, 1) < 2 * one            # shared: one image
    assert b(192, 512, 64, 3) >= L.vqvae_vq_backward_workspace_bytes(192, 512, 64) + 192 * 64 * 4
    assert f(1, 16384, 256, 16, 0) > 0 and b(1, 16384, 256, 16) > 0
    for N, K, D, Q in ((0, 512, 64, 2), (2 ** 31, 512, 64, 2), (192, 16385, 64, 2), (192, 512, 257, 2), (192, 0, 64, 2),
                       (192, 512, 0, 2), (192, 512, 64, 0), (192, 512, 64, 17)):
        assert f(N, K, D, Q, 0) == 0 and f(N, K, D, Q, 1) == 0 and b(N, K, D, Q) == 0, (N, K, D, Q)


def test_argument_errors_without_gpu():
    from vqvae_amd import _lib
    L = _lib.load()
    a, big = 256, 1 << 40                      # a fake, aligned "device pointer" (never dereferenced)
    books = (ctypes.c_void_p * 16)(*([a] * 16))
    hole = (ctypes.c_void_p * 16)(*([a, None] + [a] * 14))
    fw, de, bw = L.vqvae_vq_residual_forward_f32, L.vqvae_vq_residual_decode_f32, L.vqvae_vq_residual_backward_f32

    def forward(z=a, cb=books, B=1, D=64, H=8, W=8, K=16, Q=2, flags=0, zq=a, idx=a, hist=a, ls=a, pp=a, loss=a, res=None, ws=a,
                nws=big):
        return fw(z, cb, B, D, H, W, K, Q, 0.25, flags, zq, idx, hist, ls, pp, loss, res, ws, nws, None)

    for kw in ({"z": None}, {"cb": None}, {"idx": None}, {"hist": None}, {"ls": None}, {"pp": None}, {"loss": None}, {"cb": hole}):
        assert forward(**kw) == -1, kw
    assert forward(B=0) == -2 and forward(H=0) == -2
    for kw in ({"Q": 0}, {"Q": 17}, {"D": 257}, {"D": 0}, {"K": 16385}, {"K": 0}, {"B": 2 ** 31, "H": 1, "W": 1},
               {"flags": 0x800}, {"flags": 0x20000}):
        assert forward(**kw) == -3, kw
    assert forward(ws=None) == -4 and forward(nws=16) == -4
    assert forward(cb=hole, flags=0x10000, ws=None) == -4                    # shared: only codebooks[0] is read

    def decode(idx=a, cb=books, B=1, D=64, H=8, W=8, K=16, Q=2, flags=0, zq=a):
        return de(idx, cb, B, D, H, W, K, Q, flags, zq, None)

    for kw in ({"idx": None}, {"cb": None}, {"zq": None}, {"cb": hole}):
        assert decode(**kw) == -1, kw
    assert decode(W=0) == -2
    for kw in ({"Q": 0}, {"Q": 17}, {"D": 257}, {"K": 16385}, {"flags": 0x2}):
        assert decode(**kw) == -3, kw

    def backward(z=a, cb=books, idx=a, B=1, D=64, H=8, W=8, K=16, Q=2, flags=0, gz=a, ge=books, ws=a, nws=big):
        return bw(z, cb, idx, None, None, B, D, H, W, K, Q, 0.25, flags, gz, ge, ws, nws, None)

    for kw in ({"z": None}, {"cb": None}, {"idx": None}, {"gz": None, "ge": None}, {"cb": hole}, {"ge": hole}):
        assert backward(**kw) == -1, kw
    assert backward(B=0) == -2
    for kw in ({"Q": 0}, {"Q": 17}, {"D": 257}, {"K": 0}, {"flags": 0x2}):
        assert backward(**kw) == -3, kw
    assert backward(ws=None) == -4 and backward(nws=16) == -4


def test_front_end_rejects_cpu_tensors_and_bad_shapes():
    from vqvae_amd import _lib, functional as F, training as T
    z, cb = torch.zeros(1, 4, 2, 2), torch.zeros(3, 4)
    with pytest.raises(_lib.VqvaeHipError):
        F.vq_residual_forward(z, [cb, cb], 0.25)
    with pytest.raises(_lib.VqvaeHipError):
        F.vq_residual_decode(torch.zeros(2, 4, dtype=torch.int64), [cb, cb], 1, 2, 2)
    with pytest.raises(_lib.VqvaeHipError):
        T.vq_residual_backward(z, [cb, cb], torch.zeros(2, 4, dtype=torch.int64), None, None, 0.25)


@pytest.mark.parametrize("B,D,H,W,K", [(2, 64, 8, 8, 96), (2, 3, 3, 5, 5), (1, 48, 4, 8, 64)])
def test_one_stage_is_the_reference_quantizer(B, D, H, W, K):
    from oracle import torch_port
    g = np.random.default_rng(B * D + K)
    z = g.standard_normal((B, D, H, W)).astype(np.float32)
    rows = R.to_rows(z)
    cb = R.draw_books(rows, K, 1, False, 1)[0]
    loss, z_q, ppl, _, idx = torch_port.quantize(torch.from_numpy(z), torch.from_numpy(cb), 0.25)
    c = R.chain(rows, [cb], 0.25)
    assert np.array_equal(c.idx[0], idx.view(-1).numpy())
    assert np.array_equal(R.to_nchw(c.z_q, B, H, W).view(np.uint32), z_q.numpy().view(np.uint32))
    np.testing.assert_allclose(c.loss, float(loss), rtol=1e-5)
    np.testing.assert_allclose(c.perplexity[0], float(ppl), rtol=1e-5)
    assert np.array_equal(c.r[1], rows - cb[c.idx[0]])


def test_the_chain_shrinks_and_hits_codes_exactly():
    rows = np.random.default_rng(0).standard_normal((192, 64)).astype(np.float32)
    for shared in (False, True):
        books = R.draw_books(rows, 96, 4, shared, 2)
        c = R.chain(rows, books, 0.25)
        norms = [float((r.astype(np.float64) ** 2).sum()) for r in c.r]
        # (a stage shrinks the residual when its codes lie on the residual's own scale: the drawn codebooks do, stage by stage;
        # a shared one -- drawn from z -- only at stage 0)
        assert norms[1] < norms[0] and (shared or all(b <= a for a, b in zip(norms, norms[1:]))), norms
        assert (~c.r[1].any(axis=1)).sum() > 0                # rows that equal a code: all zeros for the next stage
        # the stage losses are the partial-sum commitment terms: ||r_q - e_q||^2 = ||z - sum_{i<=q} e_i||^2 up to fp32 rounding
        part = np.zeros_like(rows, dtype=np.float64)
        for q in range(4):
            part += c.e[q]
            want = 1.25 * ((rows - part) ** 2).mean()
            np.testing.assert_allclose(c.loss_stage[q], want, rtol=1e-4, atol=1e-12)
        assert c.loss == pytest.approx(c.loss_stage.sum(), rel=1e-12)


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("B,D,H,W,K,Q", [(3, 64, 8, 8, 96, 3), (2, 48, 3, 5, 64, 3), (2, 3, 4, 4, 5, 4)])
def test_closed_form_gradients_equal_autograd_of_the_composition(B, D, H, W, K, Q, shared):
    g = np.random.default_rng(B + D + Q)
    z = g.standard_normal((B, D, H, W)).astype(np.float32)
    rows = R.to_rows(z)
    books = R.draw_books(rows, K, Q, shared, 3)
    # (drawn rows make exact hits; a little noise on the codes keeps every stage's gradient away from zero)
    uniq = [books[0]] if shared else books
    uniq = [(E + 0.05 * g.standard_normal(E.shape)).astype(np.float32) for E in uniq]
    zt = torch.from_numpy(z).requires_grad_(True)
    ut = [torch.from_numpy(E).requires_grad_(True) for E in uniq]
    bt = [ut[0]] * Q if shared else ut
    loss, z_q, idx = R.autograd_chain(zt, bt, 0.25)
    grad_zq = g.standard_normal((B, D, H, W)).astype(np.float32)
    gl = 0.7
    (gl * loss + (z_q * torch.from_numpy(grad_zq)).sum()).backward()
    books_np = [uniq[0]] * Q if shared else uniq
    c = R.chain(rows, books_np, 0.25)
    assert np.array_equal(c.idx, idx.numpy())                 # torch's argmin and the C oracle's agree on these rows
    np.testing.assert_allclose(c.loss, float(loss.detach()), rtol=1e-5)
    assert np.array_equal(R.to_nchw(c.z_q, B, H, W).view(np.uint32), z_q.detach().numpy().view(np.uint32))
    gz, bound, per_stage, ge = R.grads(rows, books_np, c.idx, R.to_rows(grad_zq), gl, 0.25, shared)
    np.testing.assert_allclose(R.to_nchw(gz, B, H, W), zt.grad.numpy(), rtol=1e-4, atol=1e-6)
    assert len(ge) == len(ut)
    for want, t in zip(ge, ut):
        np.testing.assert_allclose(want, t.grad.numpy(), rtol=1e-4, atol=1e-5 * np.abs(want).max())
        assert np.abs(want).max() > 0
    # the mirrored fp32 order stays inside the stated bound of the fp64 value
    mirror = R.grad_z_mirror(rows, books_np, c.idx, R.to_rows(grad_zq), np.float32(gl))
    assert (np.abs(mirror.astype(np.float64) - gz) <= bound).all()


def test_residual_quantizer_state_dict_layout():
    from oracle import torch_port
    from vqvae_amd.modules import ResidualVectorQuantizer, VectorQuantizer
    torch.manual_seed(0)
    m = ResidualVectorQuantizer(3, 32, 8, 0.25)
    assert list(m.state_dict()) == ["embedding.weight", "residual_embeddings.0.weight", "residual_embeddings.1.weight"]
    for v in m.state_dict().values():
        assert v.shape == (32, 8) and float(v.abs().max()) <= 1.0 / 32
    assert len({v.data_ptr() for v in m.state_dict().values()}) == 3
    s = ResidualVectorQuantizer(3, 32, 8, 0.25, shared_codebook=True)
    assert list(s.state_dict()) == ["embedding.weight"] and len(s.codebooks()) == 1
    # a one-stage (reference-layout) quantizer's state dict fills stage 0
    ref = VectorQuantizer(32, 8, 0.25).state_dict()
    missing, unexpected = m.load_state_dict(ref, strict=False)
    assert sorted(missing) == ["residual_embeddings.0.weight", "residual_embeddings.1.weight"] and not unexpected
    assert torch.equal(m.embedding.weight, ref["embedding.weight"])
    one = ResidualVectorQuantizer(1, 32, 8, 0.25)
    one.load_state_dict(ref)                                  # strict: exactly the reference's keys
    with pytest.raises(ValueError):
        ResidualVectorQuantizer(0, 32, 8, 0.25)
    with pytest.raises(ValueError):
        ResidualVectorQuantizer(17, 32, 8, 0.25)
    # a reference checkpoint (the port's state dict) loads into a residual model's stage 0
    from vqvae_amd.modules import VQVAE
    torch.manual_seed(1)
    sd = torch_port.init_state_dict(h_dim=32, res_h_dim=8, n_embeddings=32, embedding_dim=16)
    v = VQVAE(32, 8, 2, 32, 16, 0.25, n_quantizers=3)
    missing, unexpected = v.load_state_dict(sd, strict=False)
    assert sorted(missing) == [f"vector_quantization.residual_embeddings.{i}.weight" for i in range(2)] and not unexpected
    assert torch.equal(v.vector_quantization.embedding.weight, sd["vector_quantization.embedding.weight"])
    assert VQVAE._RAW["codebook"] in dict(v.named_parameters())


def test_one_quantizer_constructs_todays_model():
    from vqvae_amd.modules import VQVAE, ResidualVectorQuantizer, VectorQuantizer, VectorQuantizerEMA
    torch.manual_seed(0)
    a = VQVAE(32, 8, 1, 64, 16, 0.25)
    torch.manual_seed(0)
    b = VQVAE(32, 8, 1, 64, 16, 0.25, n_quantizers=1)
    assert type(b.vector_quantization) is VectorQuantizer
    assert list(a.state_dict()) == list(b.state_dict())
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]), k
    assert type(VQVAE(32, 8, 1, 64, 16, 0.25, n_quantizers=1, ema_decay=0.99).vector_quantization) is VectorQuantizerEMA
    r = VQVAE(32, 8, 1, 64, 16, 0.25, n_quantizers=2)
    assert type(r.vector_quantization) is ResidualVectorQuantizer and r.vector_quantization.n_q == 2
    assert [k for k in r.state_dict() if k not in a.state_dict()] == ["vector_quantization.residual_embeddings.0.weight"]
    assert "vector_quantization.residual_embeddings.0.weight" not in VQVAE(32, 8, 1, 64, 16, 0.25, n_quantizers=2,
                                                                          shared_codebook=True).state_dict()
    with pytest.raises(ValueError):
        VQVAE(32, 8, 1, 64, 16, 0.25, n_quantizers=2, ema_decay=0.99)
    with pytest.raises(ValueError):
        VQVAE(32, 8, 1, 64, 16, 0.25, n_quantizers=0)


def test_train_tool_options_are_absent_unless_given():
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "train_checkpoint.py")).read()
    for opt in ("--n_quantizers", "--shared_codebook"):
        line = next(l for l in src.splitlines() if f'"{opt}"' in l)
        assert "argparse.SUPPRESS" in line, opt


def test_element_wise_kernels_on_the_host(tmp_path):
    """tests/host/rvq_harness.cpp compiles csrc/vq_residual.h -- the text of the advance, finish and grad_z kernels -- for the host
    with AddressSanitizer and UBSan and compares it bit for bit with a scalar loop: both layouts, both access widths, in place,
    Q up to 16, indices of K and -1 among the rows (NaN rows, no read outside a codebook)."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "rvq_harness")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(root, "tests", "host", "rvq_harness.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "emulation ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
