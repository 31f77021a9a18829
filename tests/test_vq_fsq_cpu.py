"""Finite scalar quantization without a GPU: the CPU restatement (tests/vq_fsq_ref.py) against fp64 torch autograd, the index <-> digits
round trip, the reach and the bounds of the levels, the C ABI's four entries (declared, bound, argument errors before any launch, ABI
still 9), the front ends' refusal of CPU tensors, the constructor rules, the train tool's option, and the kernels' own text on the host
under the sanitizers."""
import os
import re
import struct

import numpy as np
import pytest
import torch

from tests import vq_fsq_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = [(8, 5, 5, 5), (2,), (3,), (8, 8, 8, 5, 5, 5), (4,) * 8]


@pytest.mark.parametrize("levels", LEVELS)
@pytest.mark.parametrize("D", [1, 7, 64])
def test_restatement_agrees_with_fp64_torch_autograd(levels, D):
    """The restatement rounds y to fp32 (2^-24 |y|), the composition does not: rows whose b lies within 1e-5 of a half-integer are
    left out (the rounding moves b by at most half_l 2^-24 |y| < 1e-5 for |y| < 40); on the others the indices' codes agree, so z_q
    agrees to its own fp32 rounding, and grad_z and the parameter gradients agree to the rounding of y carried through 1 - t^2:
    a relative 2 |t| |y| 2^-24 <= 2^-23 |y| per term, plus one fp32 rounding of the result."""
    N = 300
    z, g, w_in, b_in, w_out, b_out = R.draw(N, D, levels, 1000 * D + len(levels))
    f = R.forward(z, w_in, b_in, w_out, b_out, levels)
    r = R.backward(z, g, w_in, b_in, w_out, levels)
    assert np.abs(f.y).max() < 40
    keep = R.clear_rows(f, 1e-5)
    assert keep.mean() > 0.9
    t = {n: torch.from_numpy(v.astype(np.float64)).requires_grad_(True)
         for n, v in dict(z=z[keep], w_in=w_in, b_in=b_in, w_out=w_out, b_out=b_out).items()}
    zq = R.torch_composition(t["z"], t["w_in"], t["b_in"], t["w_out"], t["b_out"], levels)
    zq.backward(torch.from_numpy(g[keep].astype(np.float64)))
    ref = zq.detach().numpy()
    assert (np.abs(f.z_q[keep] - ref) <= 2.0 ** -23 * np.abs(ref) + 2.0 ** -149).all()
    k = r.k
    ymag = 1.0 + np.abs(f.y[keep].astype(np.float64))
    mag = np.zeros((keep.sum(), D))
    for j in range(k.d):
        mag += np.abs(w_in[j].astype(np.float64)[None, :] * (r.gy[keep][:, j] * ymag[:, j])[:, None])
    gz_ref = t["z"].grad.numpy()
    assert (np.abs(r.grad_z[keep] - gz_ref) <= 2.0 ** -23 * np.abs(gz_ref) + 2.0 ** -22 * mag + 1e-300).all()
    # the parameter gradients, as plain sums over the kept rows
    rk = R.backward(z[keep], g[keep], w_in, b_in, w_out, levels)
    got, mags = R.param_grads(rk)
    ymax = 1.0 + np.abs(f.y[keep]).max()
    for n in ("w_out", "b_out", "w_in", "b_in"):
        want = t[n].grad.numpy()
        tol = 2.0 ** -23 * np.abs(want) + 2.0 ** -22 * ymax * mags[n] + 1e-300
        assert (np.abs(got[n] - want) <= tol).all(), n
        blocked = R.param_grads_blocked(rk)[n]
        assert (np.abs(blocked.astype(np.float64) - got[n]) <= 2.0 ** -23 * np.abs(got[n]) + 2.0 ** -40 * mags[n] + 1e-300).all(), n


@pytest.mark.parametrize("levels", LEVELS)
def test_index_digits_round_trip_over_all_K(levels):
    k = R.Consts(levels)
    assert k.K == int(np.prod(levels)) <= 65536
    codes = R.all_codes(levels)                                  # (K, d): the codes of every index
    assert codes.shape == (k.K, k.d) and len({tuple(c) for c in codes.tolist()}) == k.K
    q = np.rint(codes.astype(np.float64) * k.hw[None, :]).astype(np.int64)
    assert ((q >= -k.hw) & (q <= np.array(levels) - 1 - k.hw)).all()
    assert np.array_equal(((q + k.hw) * k.basis).sum(1), np.arange(k.K))
    # ... and through the forward's own index: y chosen so that b lands on each level exactly
    b = q.astype(np.float64)
    y = np.arctanh((b + k.offset) / k.half_l) - k.shift
    chat, idx, _, _ = R.codes(y.astype(np.float32), k)
    assert np.array_equal(idx, np.arange(k.K)) and np.array_equal(chat, codes)
    eye = np.eye(k.d, dtype=np.float32)
    assert np.array_equal(R.decode(np.arange(k.K), eye, np.zeros(k.d, np.float32), levels), codes)


@pytest.mark.parametrize("L", [2, 3, 4, 5, 8, 255, 256])
def test_every_level_is_reached_and_none_outside(L):
    k = R.Consts((L,))
    y = np.concatenate([np.linspace(-12, 12, 200001), [-1e4, 1e4, -np.inf, np.inf, -40.0, 40.0]]).astype(np.float32)[:, None]
    _, _, q = R.bound_round(y, k)
    lo, hi = -(L // 2), L - 1 - L // 2
    assert q.min() == lo and q.max() == hi
    assert set(np.unique(q).astype(int).tolist()) == set(range(lo, hi + 1))
    # the forward's rule for a non-finite y: digit 0, a NaN code
    chat, idx, _, _ = R.codes(np.array([[np.inf], [-np.inf], [np.nan]], np.float32), k)
    assert np.isnan(chat).all() and (idx == 0).all()


@pytest.mark.parametrize("B,D,H,W,levels", R.GPU_CASES)
def test_the_gpu_cases_leave_out_no_row(B, D, H, W, levels):
    """the GPU tests compare indices on rows whose every b lies more than 1e-9 from a half-integer: on their seeded inputs that is
    every row, and every level list's range of codes is in use"""
    z, g, w_in, b_in, w_out, b_out = R.gpu_case_inputs(B, D, H, W, levels)
    f = R.forward(z, w_in, b_in, w_out, b_out, levels)
    assert R.clear_rows(f, 1e-9).all()
    if B * H * W >= 64:
        assert len(np.unique(f.idx)) > 1


NAMES = ("vqvae_fsq_forward_f32", "vqvae_fsq_decode_indices_f32", "vqvae_fsq_backward_workspace_bytes", "vqvae_fsq_backward_f32")


def test_entries_are_declared_and_bound_and_the_abi_stays_9():
    import ctypes
    from vqvae_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    src = open(os.path.join(ROOT, "include", "vqvae_hip.h")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert re.search(r"VQVAE_API\s+(int|size_t)\s+" + name + r"\s*\(", src)
    assert [len(_lib.SIGNATURES[n][1]) for n in NAMES] == [17, 12, 3, 20]
    assert _lib.load().vqvae_abi_version() == 9 and re.search(r"#define VQVAE_HIP_ABI_VERSION 9\b", src)
    assert "FSQ" not in "".join(re.findall(r"#define\s+(VQVAE_VQ_\w+)", src))         # no new flag: the entries take ROWMAJOR only


def _lv(*levels):
    import ctypes
    return (ctypes.c_int * len(levels))(*levels), len(levels)


def test_argument_errors_come_back_before_any_launch():
    from vqvae_amd import _lib
    L = _lib.load()
    M = 1 << 24                                                # fake, aligned, disjoint "device pointers" (never dereferenced)
    z, wi, bi, wo, bo, zq, ix, hs, pp, g, gz, gwi, gbi, gwo, gbo, ws = [M * (i + 1) for i in range(16)]
    fw, dec, bw, size = L.vqvae_fsq_forward_f32, L.vqvae_fsq_decode_indices_f32, L.vqvae_fsq_backward_f32, L.vqvae_fsq_backward_workspace_bytes
    lv, d = _lv(8, 5, 5, 5)
    big = 1 << 30
    for flags in (0, 1):
        def F(**k):
            a = dict(z=z, wi=wi, bi=bi, wo=wo, bo=bo, lv=lv, d=d, B=2, D=64, H=8, W=8, zq=zq, ix=ix, hs=hs, pp=pp)
            a.update(k)
            return fw(a["z"], a["wi"], a["bi"], a["wo"], a["bo"], a["lv"], a["d"], a["B"], a["D"], a["H"], a["W"], flags, a["zq"], a["ix"],
                      a["hs"], a["pp"], None)

        def Dc(**k):
            a = dict(ix=ix, wo=wo, bo=bo, lv=lv, d=d, B=2, D=64, H=8, W=8, zq=zq)
            a.update(k)
            return dec(a["ix"], a["wo"], a["bo"], a["lv"], a["d"], a["B"], a["D"], a["H"], a["W"], flags, a["zq"], None)

        def Bk(**k):
            a = dict(z=z, g=g, wi=wi, bi=bi, wo=wo, lv=lv, d=d, B=2, D=64, H=8, W=8, gz=gz, gwi=gwi, gbi=gbi, gwo=gwo, gbo=gbo, ws=ws, n=big)
            a.update(k)
            return bw(a["z"], a["g"], a["wi"], a["bi"], a["wo"], a["lv"], a["d"], a["B"], a["D"], a["H"], a["W"], flags, a["gz"], a["gwi"],
                      a["gbi"], a["gwo"], a["gbo"], a["ws"], a["n"], None)

        # NULLs
        for name in ("z", "wi", "bi", "wo", "bo", "lv", "ix"):
            assert F(**{name: None}) == -1, name
        assert F(hs=None) == -1                                  # perplexity needs hist
        for name in ("ix", "wo", "bo", "lv", "zq"):
            assert Dc(**{name: None}) == -1, name
        for name in ("z", "g", "wi", "bi", "wo", "lv"):
            assert Bk(**{name: None}) == -1, name
        assert Bk(gz=None, gwi=None, gbi=None, gwo=None, gbo=None) == -1
        # shapes
        for call in (F, Dc, Bk):
            assert call(B=0) == -2 and call(H=0) == -2 and call(W=-1) == -2
            # the envelope: d = 0 and d = 9, L = 1 and L = 257, K > 65536, D = 0 and D = 257, N = 2^32, another flag
            assert call(d=0) == -3
            assert call(lv=_lv(*(2,) * 9)[0], d=9) == -3
            assert call(lv=_lv(8, 1, 5)[0], d=3) == -3
            assert call(lv=_lv(257)[0], d=1) == -3
            assert call(lv=_lv(256, 256, 2)[0], d=3) == -3       # K = 131072
            assert call(D=257) == -3 and call(D=0) == -3
            assert call(B=1 << 20, H=64, W=64) == -3
        assert fw(z, wi, bi, wo, bo, lv, d, 2, 64, 8, 8, flags | 2, zq, ix, hs, pp, None) == -3
        # misaligned pointers
        for name in ("z", "wi", "bi", "wo", "bo", "zq", "hs", "pp"):
            assert F(**{name: z + 2 + M * 20}) == -3, name
        assert F(ix=ix + 4) == -3
        assert Dc(zq=zq + 2) == -3 and Dc(wo=wo + 1) == -3 and Dc(ix=ix + 4) == -3
        for name in ("z", "g", "wi", "bi", "wo", "gz", "gwi", "gbi", "gwo", "gbo"):
            assert Bk(**{name: z + 2 + M * 20}) == -3, name
        assert Bk(ws=ws + 4) == -3
        # an output on an input
        assert F(zq=z) == -3 and F(zq=z + 400) == -3 and F(zq=wo) == -3 and F(ix=z) == -3 and F(hs=wi) == -3 and F(pp=bi) == -3
        assert Dc(zq=ix) == -3 and Dc(zq=wo) == -3
        assert Bk(gz=z) == -3 and Bk(gz=g + 64) == -3 and Bk(gwi=wi) == -3 and Bk(gwo=wo) == -3 and Bk(gbi=bi) == -3 and Bk(ws=z) == -3
        # the workspace
        need = size(128, 64, 4)
        assert need == (2 * 64 * 4 + 64 + 4) * 8                 # one block of 256 rows
        assert size(257, 64, 4) == 2 * need
        assert Bk(ws=None) == -4 and Bk(n=need - 8) == -4
        assert Bk(lv=_lv(256, 256)[0], d=2, ws=None) == -4       # (K = 65536 is inside the envelope)
    assert size(1 << 32, 64, 4) == 0 and size(0, 64, 4) == 0 and size(128, 257, 4) == 0 and size(128, 64, 0) == 0 and size(128, 64, 9) == 0


def test_front_ends_reject_cpu_tensors():
    from vqvae_amd import _lib, functional as F, training as T
    from vqvae_amd.modules import FiniteScalarQuantizer
    levels = (8, 5, 5, 5)
    z = torch.zeros(2, 16, 3, 3)
    w_in, b_in, w_out, b_out = torch.zeros(4, 16), torch.zeros(4), torch.zeros(16, 4), torch.zeros(16)
    with pytest.raises(_lib.VqvaeHipError):
        F.fsq_forward(z, w_in, b_in, w_out, b_out, levels)
    with pytest.raises(_lib.VqvaeHipError):
        F.fsq_decode_indices(torch.zeros(18, dtype=torch.int64), w_out, b_out, levels, 2, 3, 3)
    with pytest.raises(_lib.VqvaeHipError):
        T.fsq_backward(z, z, w_in, b_in, w_out, levels)
    with pytest.raises(_lib.VqvaeHipError):
        T.FSQStraightThrough.apply(z.requires_grad_(True), w_in, b_in, w_out, b_out, levels, False)
    with pytest.raises(_lib.VqvaeHipError):
        F.fsq_backward_workspace(1 << 32, 16, 4, "cpu")
    q = FiniteScalarQuantizer(levels, 16)
    with pytest.raises(_lib.VqvaeHipError):
        q(z)
    with pytest.raises(_lib.VqvaeHipError):
        q.quantize(z.detach())
    assert F.fsq_forward.__kwdefaults__ == {"rowmajor": False, "want_zq": True, "want_hist": True}


def test_the_module_and_its_state():
    from vqvae_amd.modules import FiniteScalarQuantizer
    torch.manual_seed(0)
    q = FiniteScalarQuantizer((8, 5, 5, 5), 16)
    assert list(q.state_dict()) == ["project_in.weight", "project_in.bias", "project_out.weight", "project_out.bias"]
    assert q.n_e == 1000 and q.e_dim == 16 and q.levels == (8, 5, 5, 5)
    assert q.project_in.weight.shape == (4, 16) and q.project_out.weight.shape == (16, 4)
    assert torch.equal(q.codes(), torch.from_numpy(R.all_codes((8, 5, 5, 5))))
    for bad in ((), (2,) * 9, (1, 4), (257,), (256, 256, 2)):
        with pytest.raises(ValueError):
            FiniteScalarQuantizer(bad, 16)
    with pytest.raises(ValueError):
        FiniteScalarQuantizer((4, 4), 257)


def test_constructor_rules_and_the_default_is_todays_model():
    from vqvae_amd.modules import VQVAE, FiniteScalarQuantizer, VectorQuantizer
    lv = (8, 5, 5, 5)
    m = VQVAE(32, 8, 1, 1000, 16, 0.25, fsq_levels=lv)
    assert type(m.vector_quantization) is FiniteScalarQuantizer and m.vector_quantization.levels == lv
    assert [k for k in m.state_dict() if k.startswith("vector_quantization.")] == [
        "vector_quantization.project_in.weight", "vector_quantization.project_in.bias",
        "vector_quantization.project_out.weight", "vector_quantization.project_out.bias"]
    assert VQVAE(32, 8, 1, 64, 16, 0.25, fsq_levels=[4, 4, 4]).vector_quantization.levels == (4, 4, 4)
    for kw in (dict(ema_decay=0.99), dict(ema_decay=0.99, restart_threshold=1.0), dict(restart_threshold=1.0), dict(n_quantizers=2),
               dict(n_quantizers=2, shared_codebook=True), dict(shared_codebook=True), dict(rotation_trick=True), dict(cosine_sim=True)):
        with pytest.raises(ValueError):
            VQVAE(32, 8, 1, 1000, 16, 0.25, fsq_levels=lv, **kw)
    with pytest.raises(ValueError):
        VQVAE(32, 8, 1, 512, 16, 0.25, fsq_levels=lv)          # n_embeddings != prod levels
    with pytest.raises(TypeError):
        VQVAE(32, 8, 1, 1000, 16, 0.25, False, None, 1e-5, None, 1, False, False, False, lv)      # keyword-only
    with pytest.raises(VqvaeErr()):
        m.init_codebook_(torch.zeros(1, 3, 32, 32))
    # without the option: today's model, its keys and its bits at a fixed seed, and no random number drawn on the way
    torch.manual_seed(0)
    a = VQVAE(32, 8, 1, 64, 16, 0.25)
    after_a = torch.rand(4)
    torch.manual_seed(0)
    b = VQVAE(32, 8, 1, 64, 16, 0.25, fsq_levels=None)
    after_b = torch.rand(4)
    assert type(b.vector_quantization) is VectorQuantizer and torch.equal(after_a, after_b)
    assert list(a.state_dict()) == list(b.state_dict()) == EXPECTED_DEFAULT_KEYS
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


def VqvaeErr():
    from vqvae_amd._lib import VqvaeHipError
    return VqvaeHipError


EXPECTED_DEFAULT_KEYS = [
    "encoder.conv_stack.0.weight", "encoder.conv_stack.0.bias", "encoder.conv_stack.2.weight", "encoder.conv_stack.2.bias",
    "encoder.conv_stack.4.weight", "encoder.conv_stack.4.bias", "encoder.conv_stack.5.stack.0.res_block.1.weight",
    "encoder.conv_stack.5.stack.0.res_block.3.weight", "pre_quantization_conv.weight", "pre_quantization_conv.bias",
    "vector_quantization.embedding.weight", "decoder.inverse_conv_stack.0.weight", "decoder.inverse_conv_stack.0.bias",
    "decoder.inverse_conv_stack.1.stack.0.res_block.1.weight", "decoder.inverse_conv_stack.1.stack.0.res_block.3.weight",
    "decoder.inverse_conv_stack.2.weight", "decoder.inverse_conv_stack.2.bias", "decoder.inverse_conv_stack.4.weight",
    "decoder.inverse_conv_stack.4.bias"]


def test_train_tool_option_is_absent_unless_given():
    src = open(os.path.join(ROOT, "tools", "train_checkpoint.py")).read()
    line = next(l for l in src.splitlines() if '"--fsq_levels"' in l)
    assert "argparse.SUPPRESS" in line


# ---- the kernels' own text on the host --------------------------------------------------------------------------------------------

# (B, HW, D, levels): one row; odd D on the element path; several chunks; a ragged last block of several; every level list
HOST_CASES = [(1, 1, 16, (8, 5, 5, 5)), (3, 35, 7, (3,)), (4, 64, 64, (8, 5, 5, 5)), (2, 16, 256, (4,) * 8), (5, 60, 68, (8, 8, 8, 5, 5, 5)),
              (9, 36, 12, (2,)), (1, 300, 130, (5, 4))]


def host_case_bytes(B, HW, D, levels, seed):
    """one case of tests/host/fsq_harness.cpp's input: the inputs, the constants and every expected output"""
    N = B * HW
    z, g, w_in, b_in, w_out, b_out = R.draw(N, D, levels, seed)
    if N >= 8:
        z[1] = 1e4
        z[2] = -1e4
        z[3] = 0.0
        z[4, D // 2] = np.nan
        z[5] = np.inf
        z[6, 0] = -np.inf
        g[7, D - 1] = np.nan
    f = R.forward(z, w_in, b_in, w_out, b_out, levels)
    k = f.k
    r = R.backward(z, g, w_in, b_in, w_out, levels)
    pg = R.param_grads_blocked(r)
    dec_idx = f.idx.copy()
    if N >= 8:
        dec_idx[0], dec_idx[N - 1], dec_idx[2] = -1, k.K, 1 << 40
    dec = R.decode(dec_idx, w_out, b_out, levels)
    if N >= 8:                                                   # what the special rows must look like, whatever else is compared
        assert np.isnan(f.z_q[[4, 5, 6]]).all() and np.isfinite(f.z_q[[0, 1, 2, 3, 7]]).all() and ((f.idx >= 0) & (f.idx < k.K)).all()
        assert np.isnan(dec[[0, N - 1, 2]]).all() and np.isnan(r.grad_z[7]).all() and np.isfinite(r.grad_z[[0, 1, 2, 3]]).all()
    pad = lambda v, dt: np.concatenate([np.asarray(v, dt), np.zeros(8 - len(v), dt)])
    head = np.concatenate([np.array([B, HW, D, k.d, k.K], np.int32), pad(k.levels, np.int32), pad(k.hw, np.int32), pad(k.basis, np.int32)])
    cst = np.concatenate([pad(k.half_l, np.float64), pad(k.shift, np.float64), pad(k.offset, np.float64)])
    parts = [head, cst, z, g, w_in, b_in, w_out, b_out, f.idx.astype(np.int64), f.hist.astype(np.int32), f.z_q, dec_idx.astype(np.int64), dec,
             r.grad_z, pg["w_out"], pg["b_out"], pg["w_in"], pg["b_in"]]
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


def test_kernel_text_on_the_host(tmp_path):
    """tests/host/fsq_harness.cpp compiles csrc/vq_fsq.h -- the per-row operations and the whole bodies of the kernels -- for the host
    with AddressSanitizer and UBSan and -ffp-contract=off, runs forward (with and without z_q), decode, backward (with and without the
    parameter gradients) and the partials' second launch in both layouts and on both access paths (a workgroup runs as 256 host threads
    with a barrier), and compares every output bit for bit with the restatement's values written here: saturated, zero, NaN and Inf
    rows, out-of-range indices, odd D, wide rows and ragged last blocks among them."""
    import shutil
    import subprocess
    gxx = shutil.which("g++")
    assert gxx, "g++ is part of the image"
    exe, data = str(tmp_path / "fsq_harness"), str(tmp_path / "cases.bin")
    with open(data, "wb") as fh:
        fh.write(struct.pack("<i", len(HOST_CASES)))
        for i, (B, HW, D, levels) in enumerate(HOST_CASES):
            fh.write(host_case_bytes(B, HW, D, levels, 77 + i))
    subprocess.check_call([gxx, "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-pthread", "-o", exe, os.path.join(ROOT, "tests", "host", "fsq_harness.cpp")])
    out = subprocess.run([exe, data], capture_output=True, text=True)
    assert out.returncode == 0 and "emulation ok" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
