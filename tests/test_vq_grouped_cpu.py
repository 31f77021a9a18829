"""Grouped (product) quantization without a GPU: the CPU restatement tests/vq_grouped_ref.py against a plain numpy formulation, the
modules' state_dict layout, codebook_groups=1 as the model it always was, the entries' argument checks (they come before any
launch), the train tool's option, and the element-wise kernels' text compiled for the host under the sanitizers."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import vq_grouped_ref as GR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPED = ["vqvae_vq_grouped_workspace_bytes", "vqvae_vq_grouped_forward_f32", "vqvae_vq_grouped_decode_f32",
           "vqvae_vq_grouped_backward_workspace_bytes", "vqvae_vq_grouped_backward_f32"]


def _near_codes(rng, books, N):
    """rows whose group g lies next to a code of books[g]: every argmin is decided by a wide margin"""
    parts = []
    for E in books:
        j = rng.integers(0, E.shape[0], N)
        parts.append(E[j] + 0.01 * rng.standard_normal((N, E.shape[1])))
    return np.concatenate(parts, axis=1).astype(np.float32)


@pytest.mark.parametrize("K,D,G", [(16, 12, 3), (7, 8, 1), (5, 16, 16), (32, 64, 2)])
def test_restatement_against_plain_numpy(K, D, G):
    rng = np.random.default_rng(K + D + G)
    d, N, beta = D // G, 90, 0.25
    books = [rng.standard_normal((K, d)).astype(np.float32) for _ in range(G)]
    rows = _near_codes(rng, books, N)
    c = GR.forward(rows, books, beta)
    # plain formulation: reshape to (N, G, d), fp64 distances, argmin, concatenate the codes
    z = rows.reshape(N, G, d).astype(np.float64)
    idx = np.stack([((z[:, g, None, :] - books[g].astype(np.float64)[None]) ** 2).sum(-1).argmin(1) for g in range(G)])
    assert np.array_equal(c.idx, idx)
    e = np.concatenate([books[g][idx[g]] for g in range(G)], axis=1)
    assert np.array_equal(c.e.view(np.uint32), e.view(np.uint32))
    assert np.array_equal(c.z_q.view(np.uint32), (rows + (e - rows)).view(np.uint32))
    assert np.array_equal(c.slabs, rows.reshape(N, G, d).transpose(1, 0, 2))
    # the mean of the group losses is the reference's loss formula on the whole rows: a mean over N D elements
    mse = ((e.astype(np.float64) - rows.astype(np.float64)) ** 2).mean()
    np.testing.assert_allclose(c.loss, mse + beta * mse, rtol=1e-12)
    assert np.array_equal(c.hist, np.stack([np.bincount(idx[g], minlength=K) for g in range(G)]))
    p = c.hist / N
    np.testing.assert_allclose(c.perplexity, np.exp(-(p * np.log(p + 1e-10)).sum(1)), rtol=1e-12)
    # the device's combination of fp32 group losses
    lg = c.loss_group.astype(np.float32)
    acc = lg[0]
    for g in range(1, G):
        acc = np.float32(acc + lg[g])
    assert GR.mean_loss(lg) == np.float32(acc / np.float32(G))
    # an index outside [0, K): NaN in that group's segment only
    bad = c.idx.copy()
    bad[G - 1, 4], bad[0, 9] = K, -1
    got = GR.gather(books, bad, K)
    want_nan = np.zeros((N, D), bool)
    want_nan[4, (G - 1) * d:], want_nan[9, :d] = True, True
    assert np.array_equal(np.isnan(got), want_nan) and np.array_equal(got[~want_nan], c.e[~want_nan])
    # gradients: the mirror against fp64, and the codebook gradients against autograd of the formula
    gzq = rng.standard_normal((N, D)).astype(np.float32)
    gm = GR.grad_z_mirror(rows, books, c.idx, gzq, 0.7)
    want = gzq.astype(np.float64) + 0.7 / G * 2.0 / (N * d) * (rows.astype(np.float64) - e)
    np.testing.assert_allclose(gm, want, rtol=1e-5, atol=1e-7)
    zt = torch.from_numpy(rows).double().requires_grad_(True)
    bt = [torch.from_numpy(E).double().requires_grad_(True) for E in books]
    et = torch.cat([bt[g][torch.from_numpy(idx[g])] for g in range(G)], dim=1)
    loss = ((et.detach() - zt) ** 2).mean() + beta * ((et - zt.detach()) ** 2).mean()          # models/quantizer.py:63-64
    (0.7 * loss).backward()
    for g, w in zip(bt, GR.codebook_grads(rows, books, c.idx, 0.7, beta)):
        np.testing.assert_allclose(w, g.grad.numpy(), rtol=1e-9, atol=1e-15)
    np.testing.assert_allclose(GR.grad_z_mirror(rows, books, c.idx, None, 0.7), zt.grad.numpy(), rtol=1e-5, atol=1e-8)
    np.testing.assert_allclose(GR.grad_z_mirror(rows, books, c.idx, None, 0.7, beta=beta), beta * zt.grad.numpy(), rtol=1e-5, atol=1e-8)


def test_state_dict_keys_and_shapes():
    from vqvae_amd.modules import GroupedVectorQuantizer, GroupedVectorQuantizerEMA, VQVAE
    torch.manual_seed(0)
    vq = GroupedVectorQuantizer(4, 32, 16, 0.25)
    sd = vq.state_dict()
    assert list(sd) == ["embedding.weight", "group_embeddings.0.weight", "group_embeddings.1.weight", "group_embeddings.2.weight"]
    assert all(tuple(v.shape) == (32, 4) for v in sd.values())
    assert all(float(w.detach().abs().max()) <= 1.0 / 32 and w.requires_grad for w in vq.codebooks())
    # drawn in group order: the same uniforms as drawing them one after the other
    torch.manual_seed(0)
    torch.nn.Embedding(32, 4)                                  # (nn.Embedding's own initial draw comes before each group's)
    want = [torch.empty(32, 4).uniform_(-1.0 / 32, 1.0 / 32)]
    for _ in range(3):
        torch.nn.Embedding(32, 4)
    want += [torch.empty(32, 4).uniform_(-1.0 / 32, 1.0 / 32) for _ in range(3)]
    assert all(torch.equal(w.detach(), u) for w, u in zip(vq.codebooks(), want))
    ema = GroupedVectorQuantizerEMA(2, 32, 16, 0.25, decay=0.9, restart_threshold=1.0)
    sd = ema.state_dict()
    assert sorted(sd) == ["ema_cluster_size", "ema_w", "embedding.weight", "group_embeddings.0.weight"]
    assert tuple(sd["ema_cluster_size"].shape) == (2, 32) and tuple(sd["ema_w"].shape) == (2, 32, 8)
    assert not sd["ema_cluster_size"].any() and all(not w.requires_grad for w in ema.codebooks())
    assert torch.equal(sd["ema_w"], torch.stack([w.detach() for w in ema.codebooks()]))
    m = VQVAE(32, 8, 1, 64, 16, 0.25, codebook_groups=2)
    assert type(m.vector_quantization) is GroupedVectorQuantizer
    keys = [k for k in m.state_dict() if k.startswith("vector_quantization.")]
    assert keys == ["vector_quantization.embedding.weight", "vector_quantization.group_embeddings.0.weight"]
    assert tuple(m.state_dict()[keys[0]].shape) == (64, 8)
    m = VQVAE(32, 8, 1, 64, 16, 0.25, codebook_groups=4, ema_decay=0.99, restart_threshold=0.5)
    assert type(m.vector_quantization) is GroupedVectorQuantizerEMA and m.vector_quantization.restart_threshold == 0.5
    assert tuple(m.state_dict()["vector_quantization.ema_w"].shape) == (4, 64, 4)
    m2 = VQVAE(32, 8, 1, 64, 16, 0.25, codebook_groups=4, ema_decay=0.99)
    m2.load_state_dict(m.state_dict())


def test_one_group_is_the_model_as_it_always_was():
    from vqvae_amd.modules import VectorQuantizer, VectorQuantizerEMA, VQVAE
    for kw in ({}, {"ema_decay": 0.99}):
        torch.manual_seed(5)
        a = VQVAE(32, 8, 1, 64, 16, 0.25, **kw)
        ra = torch.rand(3)
        torch.manual_seed(5)
        b = VQVAE(32, 8, 1, 64, 16, 0.25, codebook_groups=1, **kw)
        rb = torch.rand(3)
        assert type(a.vector_quantization) is type(b.vector_quantization) is (VectorQuantizerEMA if kw else VectorQuantizer)
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa) == list(sb)
        assert all(torch.equal(sa[k], sb[k]) for k in sa) and torch.equal(ra, rb)          # same keys, bits and random draws


def test_bindings_and_sizing_calls():
    from vqvae_amd import _lib
    L = _lib.load()
    assert all(n in _lib.SIGNATURES for n in GROUPED)
    assert L.vqvae_abi_version() == 9
    one = L.vqvae_vq_workspace_bytes(4096, 512, 16)
    n = L.vqvae_vq_grouped_workspace_bytes(4096, 512, 64, 4)
    assert n >= 4 * one + 4096 * 64 * 4                        # one prepared image per group and the slabs
    assert L.vqvae_vq_grouped_backward_workspace_bytes(4096, 512, 64, 4) >= L.vqvae_vq_backward_workspace_bytes(4096, 512, 16) + 4096 * 16 * 4
    for N, K, D, G in ((4096, 512, 64, 0), (4096, 512, 64, 17), (4096, 512, 64, 3), (4096, 16385, 64, 2), (4096, 512, 258, 2),
                       (1 << 31, 512, 64, 2), (0, 512, 64, 2)):
        assert L.vqvae_vq_grouped_workspace_bytes(N, K, D, G) == 0, (N, K, D, G)
        assert L.vqvae_vq_grouped_backward_workspace_bytes(N, K, D, G) == 0, (N, K, D, G)
    assert L.vqvae_vq_grouped_workspace_bytes(64, 16384, 256, 16) > 0 and L.vqvae_vq_grouped_workspace_bytes(64, 5, 16, 16) > 0


def test_argument_errors_come_before_any_launch():
    """fake pointers, never dereferenced: every call here must return before it launches anything"""
    from vqvae_amd import _lib
    L = _lib.load()
    MB = 1 << 20
    z, zq, idx, hist, sc, sl, cb0, cb1, gz, ge0, ge1 = (MB * i for i in range(1, 12))     # 1 MiB apart: nothing overlaps
    ws, big = 16 * MB, 1 << 24                                                               # (above everything else)
    books = (ctypes.c_void_p * 2)(cb0, cb1)

    def fwd(z=z, books=books, zq=zq, idx=idx, hist=hist, lg=sc, pp=sc + 64, loss=sc + 128, sl=sl, ws=ws, nws=big, D=64, K=96, G=2, B=1, flags=0):
        return L.vqvae_vq_grouped_forward_f32(z, books, B, D, 8, 8, K, G, 0.25, flags, zq, idx, hist, lg, pp, loss, sl, ws, nws, None)
    assert fwd(z=None) == -1 and fwd(idx=None) == -1 and fwd(books=(ctypes.c_void_p * 2)(cb0, None)) == -1
    assert fwd(B=0) == -2
    assert fwd(G=3) == -3 and fwd(G=0) == -3 and fwd(G=17) == -3 and fwd(D=258) == -3 and fwd(K=16385) == -3
    assert fwd(nws=1024) == -4 and fwd(ws=None) == -4
    assert fwd(z=z + 2) == -3 and fwd(zq=zq + 1) == -3 and fwd(idx=idx + 4) == -3 and fwd(ws=ws + 4) == -3 and fwd(sl=sl + 2) == -3
    assert fwd(books=(ctypes.c_void_p * 2)(cb0, cb1 + 2)) == -3
    assert fwd(zq=z) == -3 and fwd(zq=z + 64) == -3 and fwd(sl=z) == -3     # an output on top of z_e
    assert fwd(hist=cb1) == -3 and fwd(zq=cb0 - 64 * 64 * 4 + 16) == -3     # ... and on top of a codebook
    assert fwd(ws=z - 4096) == -3                                            # the workspace's end reaches into z_e

    def dec(idx=idx, books=books, zq=zq, D=64, K=96, G=2, flags=1):
        return L.vqvae_vq_grouped_decode_f32(idx, books, 1, D, 8, 8, K, G, flags, zq, None)
    assert dec(idx=None) == -1 and dec(zq=None) == -1 and dec(G=3) == -3 and dec(flags=2) == -3
    assert dec(idx=idx + 4) == -3 and dec(zq=zq + 2) == -3 and dec(zq=idx) == -3 and dec(zq=cb1) == -3

    gbooks = (ctypes.c_void_p * 2)(ge0, ge1)

    def bwd(z=z, books=books, idx=idx, gzq=zq, gl=sc, gz=gz, ge=gbooks, ws=ws, nws=big, D=64, K=96, G=2, flags=0):
        return L.vqvae_vq_grouped_backward_f32(z, books, idx, gzq, gl, 1, D, 8, 8, K, G, 0.25, flags, gz, ge, ws, nws, None)
    assert bwd(z=None) == -1 and bwd(gz=None, ge=None) == -1 and bwd(ge=(ctypes.c_void_p * 2)(ge0, None)) == -1
    assert bwd(G=3) == -3 and bwd(flags=0x800) == -3                        # the commitment form has no codebook gradient
    assert bwd(flags=0x800, gz=None, ge=None) == -1
    assert bwd(nws=64) == -4 and bwd(gz=gz + 2) == -3 and bwd(gzq=zq + 1) == -3 and bwd(gl=sc + 2) == -3
    assert bwd(gz=z) == -3 and bwd(gz=zq) == -3 and bwd(ge=(ctypes.c_void_p * 2)(cb0, ge1)) == -3


def test_train_tool_option_is_absent_unless_given():
    """the tool's own argument parsing, and the model it builds from what was given"""
    from tools import train_checkpoint as tc
    from vqvae_amd.modules import GroupedVectorQuantizer, GroupedVectorQuantizerEMA, VectorQuantizer, VQVAE

    def model(args, kw):
        return VQVAE(args.n_hiddens, args.n_residual_hiddens, args.n_residual_layers, args.n_embeddings, args.embedding_dim, args.beta, **kw)
    args, kw = tc.parse([])
    assert not hasattr(args, "codebook_groups") and kw == {} and "codebook_groups" not in vars(args)
    assert type(model(args, kw).vector_quantization) is VectorQuantizer
    args, kw = tc.parse(["--codebook_groups", "4"])
    assert kw == {"codebook_groups": 4}
    vq = model(args, kw).vector_quantization
    assert type(vq) is GroupedVectorQuantizer and vq.n_g == 4 and tuple(vq.embedding.weight.shape) == (512, 16)
    args, kw = tc.parse(["--codebook_groups", "2", "--ema_decay", "0.9", "--restart_threshold", "1"])
    vq = model(args, kw).vector_quantization
    assert type(vq) is GroupedVectorQuantizerEMA and vq.decay == 0.9 and vq.restart_threshold == 1.0


def test_element_wise_kernels_on_the_host(tmp_path):
    """tests/host/grouped_harness.cpp compiles csrc/vq_grouped.h -- the text of the split, finish / decode and grad_z kernels -- for
    the host with AddressSanitizer and UBSan and compares it bit for bit with scalar loops: both layouts, both access widths, G up
    to 16, d = 1, indices of K and -1 among the rows (NaN in that group's segment, no read outside a codebook)."""
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe = str(tmp_path / "grouped_harness")
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe, os.path.join(ROOT, "tests", "host", "grouped_harness.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "emulation ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
