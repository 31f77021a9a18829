"""GPU tests (-m gpu): a standing guard for WHEN the three-launch forward reads its arguments.  Today every kernel of the forward
fetches its arguments at entry.  Reading the quantizer's and the decoder head's arguments of
conv_res_pair8_h2_kernel<2, true, false, false, true> from the kernel-argument segment at the start of the phase that uses them was
built, measured and taken out again (profiles/mid_stream_ab.txt: the kernel got slower); these tests are what such a change -- or a
parameter block in device memory, which would be wrong -- has to pass.  Every launch carries its own copy of its arguments, so
forwards of DIFFERENT models queued on one stream with no synchronisation in between must each see their own weights, codebook,
buffers and sizes.  They pass on the code as it stands; what came with them (the kernels' wave reductions through
v_permlane32_swap / ds_swizzle) is covered bit for bit by them and by tests/test_forward_midfused_gpu.py.

No tolerance anywhere: x_hat (as int32), loss, perplexity and the indices are compared bit for bit -- against the model's own
isolated, synchronised call, and (second half) the three-launch route against the VQVAE_FWD_DEBUG_ZE route of the same entry point
(tests/test_forward_midfused_gpu.py), for K = 256 / 512 / 1024 -- 2, 4 and 8 stages of 128 codes through the weight buffers, the
kernel's `nvq` = K32 / 128 (the K the request names; its "1, 4 and 8 stages" would need K = 128, which it does not list) -- with and
without a caller's index buffer, and for a single partial workgroup (B = 1, 3)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _model(K, seed=0):
    from vqvae_amd import conv
    from vqvae_amd.modules import VQVAE
    conv.set_conv_backend("hip")
    torch.manual_seed(seed)
    return VQVAE(128, 32, 2, K, 64, 0.25).eval().to(dev())


def _images(B, seed):
    return torch.randn(B, 3, 32, 32, generator=torch.Generator().manual_seed(seed)).to(dev())


def _bits(t):
    return t.contiguous().view(torch.int32)


def _assert_same_bits(a, b, what):
    """a, b: (loss, x_hat, perplexity[, idx]) on the host; the indices are compared where both have them"""
    assert torch.equal(_bits(a[1]), _bits(b[1])), f"{what}: {int((_bits(a[1]) != _bits(b[1])).sum())} x_hat elements differ in their bits"
    assert torch.equal(_bits(a[0].view(1)), _bits(b[0].view(1))), f"{what}: loss {a[0].item()!r} vs {b[0].item()!r}"
    assert torch.equal(_bits(a[2].view(1)), _bits(b[2].view(1))), f"{what}: perplexity {a[2].item()!r} vs {b[2].item()!r}"
    if len(a) > 3 and len(b) > 3:
        assert torch.equal(a[3], b[3]), f"{what}: {int((a[3] != b[3]).sum())} indices differ"


def _isolated(m, x):
    with torch.no_grad():
        out = m._forward_c(x, want_idx=True, parts=1, fwd_flags=0)
    torch.cuda.synchronize()
    return [t.cpu() for t in out]


def _enqueue(m, x):
    """vqvae_forward_f32 on the current stream with output, index and workspace buffers of this call's own; nothing waits.
    -> (loss, x_hat, perplexity, idx, keep-alive) still on the device"""
    from vqvae_amd import _lib, functional as F
    L = _lib.load()
    B, _, H, W = x.shape
    cw, keep = m._c_weights()
    nws = L.vqvae_workspace_bytes(cw.dims, B, H, W)
    assert nws > 0
    ws = torch.empty(nws, dtype=torch.uint8, device=x.device)
    vws, prepared, key, slot = m.vector_quantization._workspace()
    assert prepared                                          # (the isolated call in front has prepared the codebook's images)
    x_hat = torch.empty_like(x)
    scal = torch.empty(2, dtype=torch.float32, device=x.device)
    idx = torch.empty((B * (H // 4) * (W // 4), 1), dtype=torch.int64, device=x.device)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    _lib.check(L.vqvae_forward_f32(cw, x.data_ptr(), B, H, W, F.VQ_CODEBOOK_PREPARED, x_hat.data_ptr(), scal.data_ptr(),
                                   scal.data_ptr() + 4, idx.data_ptr(), ws.data_ptr(), nws, vws.data_ptr(), vws.numel(), stream))
    slot[1] = key
    return scal[0], x_hat, scal[1], idx, (ws, keep, x)


@pytest.mark.parametrize("B", [5, 9])                      # a full workgroup of four images plus a ragged one; three workgroups
def test_two_models_in_flight_on_one_stream(B):
    """A (K = 512), B (K = 256, other weights), A again: queued back to back, one synchronisation at the end.  A launch that read
    another launch's arguments -- a parameter block shared between launches would do that -- gives the wrong model's bits."""
    ma, mb = _model(512, 0), _model(256, 1)
    xa, xb = _images(B, 200 + B), _images(B, 300 + B)
    ref_a, ref_b = _isolated(ma, xa), _isolated(mb, xb)
    assert torch.isfinite(ref_a[1]).all() and torch.isfinite(ref_b[1]).all()
    assert not torch.equal(ref_a[1], ref_b[1]) and int(ref_b[3].max()) < 256
    with torch.no_grad():
        q = [_enqueue(ma, xa), _enqueue(mb, xb), _enqueue(ma, xa)]
    torch.cuda.synchronize()
    got = [[t.cpu() for t in r[:4]] for r in q]
    _assert_same_bits(got[0], ref_a, f"B={B}: A, first in the queue")
    _assert_same_bits(got[1], ref_b, f"B={B}: B, between the two A")
    _assert_same_bits(got[2], ref_a, f"B={B}: A, behind B")


@pytest.mark.parametrize("want_idx", [True, False], ids=["idx_buffer", "no_idx_buffer"])
@pytest.mark.parametrize("K", [256, 512, 1024])            # 2, 4 and 8 codebook stages
@pytest.mark.parametrize("B", [1, 3, 5])                    # a single partial workgroup (1, 3); a full one plus a ragged one (5)
def test_three_launch_route_against_the_debug_route(B, K, want_idx):
    from vqvae_amd import functional as F
    m = _model(K, 0)
    x = _images(B, 400 + 10 * B + K // 256)
    with torch.no_grad():
        a = m._forward_c(x, want_idx=want_idx, parts=1, fwd_flags=0)
        b = m._forward_c(x, want_idx=True, parts=1, fwd_flags=F.FWD_DEBUG_ZE)
    torch.cuda.synchronize()
    a, b = [t.cpu() for t in a], [t.cpu() for t in b]
    assert torch.isfinite(a[1]).all() and a[1].shape == x.shape
    assert len(a) == (4 if want_idx else 3)
    _assert_same_bits(a, b, f"B={B} K={K} want_idx={want_idx}")
