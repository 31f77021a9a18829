"""GPU tests (-m gpu) of the three-launch forward: on the default 32x32 shapes vqvae_forward_f32 runs the decoder's head (conv-transpose
3x3 + residual stack) INSIDE the kernel that quantizes -- the wave that quantized an image keeps its z_q rows on chip and goes on with
them -- and takes loss / perplexity from the decoder's last kernel.  z_q is neither stored nor loaded, nothing runs between the big
kernels.

The yardstick is the VQVAE_FWD_DEBUG_ZE route of the same entry point, which keeps the separate launches (quantizing kernel -> z_q in
the workspace -> finalize -> decoder head -> decoder tail).  Same operands in the same order per accumulator, the same two reduction
trees: x_hat, loss, perplexity and the indices must agree BIT FOR BIT -- no tolerance anywhere in this file.

Model: 32x32x3, h_dim 128, res_h 32, two residual layers, D = 64 (the default-init construction of tests/cases.py: torch.manual_seed(0)
right before the model)."""
import numpy as np
import pytest
import torch

from tests import cases, synthdata

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def _model(K, seed=0):
    from vqvae_amd import conv
    from vqvae_amd.modules import VQVAE
    conv.set_conv_backend("hip")
    torch.manual_seed(seed)
    return VQVAE(128, 32, 2, K, 64, 0.25).eval().to(dev())


def _both(m, x):
    """-> (default route, debug route), each (loss, x_hat, perplexity, idx) on the host; the debug route gets the caller's idx buffer"""
    from vqvae_amd import functional as F
    with torch.no_grad():
        a = m._forward_c(x, want_idx=True, parts=1, fwd_flags=0)
        b = m._forward_c(x, want_idx=True, parts=1, fwd_flags=F.FWD_DEBUG_ZE)
    torch.cuda.synchronize()
    return [t.cpu() for t in a], [t.cpu() for t in b]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_same_bits(a, b, what=""):
    assert torch.equal(a[3], b[3]), f"{what}: {int((a[3] != b[3]).sum())} indices differ"
    assert torch.equal(_bits(a[1]), _bits(b[1])), f"{what}: {int((_bits(a[1]) != _bits(b[1])).sum())} x_hat elements differ in their bits"
    assert torch.equal(_bits(a[0].view(1)), _bits(b[0].view(1))), f"{what}: loss {a[0].item()!r} vs {b[0].item()!r}"
    assert torch.equal(_bits(a[2].view(1)), _bits(b[2].view(1))), f"{what}: perplexity {a[2].item()!r} vs {b[2].item()!r}"


def test_the_default_route_is_three_launches_and_the_debug_route_is_not():
    """What the other tests compare really are two different routes: the profiler's hooks see no stand-alone quantizer on either, one
    residual-kernel launch on the default route (the quantizing kernel carries the decoder's head) and two on the debug route."""
    from vqvae_amd import _lib, functional as F
    m = _model(512)
    x = torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(11)).to(dev())
    with torch.no_grad():
        m._forward_c(x, want_idx=True, parts=1, fwd_flags=0)          # (packs the weights, prepares the codebook)
        torch.cuda.synchronize()
        _lib.profile_enable(True)
        m._forward_c(x, want_idx=True, parts=1, fwd_flags=0)
        n_default = _lib.profile_collect('res_layer')[1]
        m._forward_c(x, want_idx=True, parts=1, fwd_flags=F.FWD_DEBUG_ZE)
        n_debug = _lib.profile_collect('res_layer')[1]
        _lib.profile_enable(False)
    assert (n_default, n_debug) == (1, 2), (n_default, n_debug)


@pytest.mark.parametrize("K", [256, 512, 1024])          # 2, 4 and 8 codebook stages; 1024: the eight-part streamed path
@pytest.mark.parametrize("B", [1, 3, 4, 5, 9])           # workgroups with idle waves, a partial last workgroup
def test_routes_agree_bit_for_bit(B, K):
    m = _model(K)
    x = torch.randn(B, 3, 32, 32, generator=torch.Generator().manual_seed(100 + B)).to(dev())
    a, b = _both(m, x)
    assert torch.isfinite(a[1]).all() and a[1].shape == x.shape
    _assert_same_bits(a, b, f"B={B} K={K}")


@pytest.mark.parametrize("cluster", [32, 420], ids=["cluster_32_rescan", "cluster_420_overflows_the_task_table"])
def test_second_screen_path(cluster):
    """The construction of tests/test_model_gpu.py's hard-row test (what a trained checkpoint's dead codes are: a cluster of near-identical
    codes, tests/test_trained_ckpt_gpu.py): rows whose candidates the stream x cell products do not cover make the workgroup vote and
    stream the codebook stages AGAIN through the weight buffers -- the buffers that afterwards hold half of the z_q rows and then the
    decoder's weights.  420 codes overflow the task table (the wave-wide argmin)."""
    m = _model(512, seed=1)
    with torch.no_grad():
        cb = m.vector_quantization.embedding.weight
        cb[8:16] = cb[0:8]                                   # exact duplicates: ties, first index wins
        cb[16:16 + cluster] = cb[0:1] + 1e-9 * torch.randn(cluster, 64, device=dev())    # a cluster of near-ties around code 0
        cb[450:500] = cb[300:301] * (1 + 1e-7 * torch.arange(50, device=dev()).view(-1, 1))
    m.invalidate_caches()
    x = torch.randn(9, 3, 32, 32, generator=torch.Generator().manual_seed(4)).to(dev())
    a, b = _both(m, x)
    assert torch.isfinite(a[1]).all()
    _assert_same_bits(a, b, f"cluster {cluster}")


def test_trained_checkpoint_with_its_dead_code_cluster():
    """A committed trained checkpoint (~450 of its 512 codes never left their init: one point at the scale of a trained z_e) on structured
    images, B = 5."""
    from vqvae_amd import conv
    from vqvae_amd.modules import VQVAE
    conv.set_conv_backend("hip")
    name = "trained_main_defaults"
    h, rh, nl, K, D, beta, _, seed = cases.TRAINED_CASES[name]
    m = VQVAE(h, rh, nl, K, D, beta).eval()
    m.load_state_dict(cases.trained_state(name), strict=True)
    m = m.to(dev())
    cb = m.vector_quantization.embedding.weight.detach()
    assert int((cb.norm(dim=1) < 0.05).sum()) > 300          # the cluster exists
    x = synthdata.normalised(5, seed + 7).to(dev())
    a, b = _both(m, x)
    assert torch.isfinite(a[1]).all()
    _assert_same_bits(a, b, name)


def test_nan_pixel_same_pattern_and_clean_images_same_bits():
    """One image with a NaN pixel among finite ones: the NaN travels encoder -> z_e -> z_q (in LDS and registers here, through memory on the
    debug route) -> decoder.  The same NaN pattern in x_hat, the same bits wherever it is finite; the clean images stay finite."""
    m = _model(512)
    B = 5
    x = torch.randn(B, 3, 32, 32, generator=torch.Generator().manual_seed(21))
    x[2, 1, 7, 9] = float("nan")
    a, b = _both(m, x.to(dev()))
    nan_a, nan_b = torch.isnan(a[1]), torch.isnan(b[1])
    assert torch.equal(nan_a, nan_b)
    assert nan_a[2].any() and not nan_a[[0, 1, 3, 4]].any()
    assert torch.equal(_bits(a[1])[~nan_a], _bits(b[1])[~nan_b])
    for i in (0, 1, 3, 4):
        assert torch.equal(_bits(a[1][i]), _bits(b[1][i]))
    assert torch.equal(a[3], b[3])
    assert torch.isnan(a[0]) == torch.isnan(b[0]) and (torch.isnan(a[0]) or torch.equal(_bits(a[0].view(1)), _bits(b[0].view(1))))
    assert torch.equal(_bits(a[2].view(1)), _bits(b[2].view(1)))


def test_no_read_of_the_workspace_z_q_and_warm_alternation():
    """The main workspace filled with 0xFF bytes (every float a NaN, z_q's region included) before a default-route call: x_hat is finite and
    equals the other route's, so the fused kernel reads no stale z_q.  The quantizer workspace carries the prepared codebook images and is
    left alone.  Then the two routes alternate twice on that one workspace (warm state)."""
    from vqvae_amd import _lib, functional as F
    m = _model(512)
    B = 5
    x = torch.randn(B, 3, 32, 32, generator=torch.Generator().manual_seed(31)).to(dev())
    L = _lib.load()
    with torch.no_grad():
        ref = [t.cpu() for t in m._forward_c(x, want_idx=True, parts=1, fwd_flags=F.FWD_DEBUG_ZE)]
        cw, _keep = m._c_weights()
        ws, _stream = m._c_workspace(L, cw, B, 32, 32, dev())
        ws.fill_(0xFF)
        got = [t.cpu() for t in m._forward_c(x, want_idx=True, parts=1, fwd_flags=0)]
        ws2, _ = m._c_workspace(L, cw, B, 32, 32, dev())
        assert ws2.data_ptr() == ws.data_ptr()               # the call used the workspace that was filled
    assert torch.isfinite(got[1]).all()
    _assert_same_bits(got, ref, "0xFF-filled workspace")
    for rnd in range(2):
        a, b = _both(m, x)
        _assert_same_bits(a, ref, f"warm round {rnd}, default route")
        _assert_same_bits(b, ref, f"warm round {rnd}, debug route")
