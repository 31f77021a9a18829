"""CPU side of the cached GatedPixelCNN sampler: the fp64 recurrence it implements agrees with the reference's forward at every
position of teacher-forced maps (the dependency analysis, checked before any kernel runs), and the new C entries are exported and
validate their arguments without a device."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import pixelcnn_port
from tests import pixelcnn_sample_ref as R

# (K, dim, n_layers, n_classes, B, H, W): the two models of tests/test_pixelcnn.py and a 12 x 12 map
CASES = {"k512_dim64_l15": (512, 64, 15, 10, 2, 8, 8), "k64_dim32_l3": (64, 32, 3, 5, 3, 6, 6), "k32_dim16_l4_12x12": (32, 16, 4, 3, 2, 12, 12)}


def _model(K, dim, nl, ncls, seed=0):
    from vqvae_amd.pixelcnn import GatedPixelCNN
    torch.manual_seed(seed)
    m = GatedPixelCNN(K, dim, nl, ncls).eval()
    with torch.no_grad():
        for n_, p in m.named_parameters():
            if n_.endswith("bias"):
                p.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(len(n_))) * 0.05)
    return m


@pytest.mark.parametrize("name", list(CASES))
def test_recurrence_matches_reference_forward(name):
    torch.set_num_threads(4)
    K, dim, nl, ncls, B, H, W = CASES[name]
    m = _model(K, dim, nl, ncls)
    g = torch.Generator().manual_seed(5)
    x = torch.randint(0, K, (B, H, W), generator=g)
    label = torch.randint(0, ncls, (B,), generator=g)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        sd["layers.0.vert_stack.weight"][:, :, -1] = 0.7             # junk in the masked taps: the recurrence never reads them
        sd["layers.0.horiz_stack.weight"][:, :, :, -1] = -0.7
        rec = R.recurrence_logits(sd, x, label, nl).numpy()
        ref = pixelcnn_port.forward(sd, x, label, nl).double().numpy()
    scale = np.abs(ref).max()
    err = np.abs(rec - ref).max()
    assert err <= 2e-6 * scale + 1e-6, f"max |recurrence - forward| = {err:.3g} (logit scale {scale:.3g})"


def test_inverse_cdf_is_the_documented_draw():
    lg = np.log(np.array([0.1, 0.2, 0.3, 0.4]))[None, :, None, None]
    for u, k in ((0.0, 0), (0.0999, 0), (0.1001, 1), (0.55, 2), (0.61, 3), (0.999999, 3)):
        idx, near = R.inverse_cdf(lg, np.full((1, 1, 1), u))
        assert int(idx[0, 0, 0]) == k, (u, k)
    assert R.inverse_cdf(lg, np.full((1, 1, 1), 0.3 + 1e-7))[1].all()


def _lib():
    from vqvae_amd import _lib
    return _lib.load()


def test_entries_declared_and_exported():
    from tests.test_capi import declared_symbols
    from vqvae_amd import _lib as binding
    L = _lib()
    for s in ("vqvae_pixelcnn_sample_packed_bytes", "vqvae_pixelcnn_sample_pack_f32", "vqvae_pixelcnn_sample_workspace_bytes",
              "vqvae_pixelcnn_sample_f32"):
        assert s in declared_symbols() and s in binding.SIGNATURES and hasattr(L, s)
    assert L.vqvae_abi_version() == 9


def test_bytes_functions():
    L = _lib()
    assert L.vqvae_pixelcnn_sample_packed_bytes(512, 64, 15, 10) > 512 * 512 * 4
    assert L.vqvae_pixelcnn_sample_packed_bytes(2, 4, 1, 1) > 0
    assert L.vqvae_pixelcnn_sample_packed_bytes(4096, 128, 15, 10) > 0
    assert L.vqvae_pixelcnn_sample_packed_bytes(512, 62, 15, 10) == 0          # dim % 4
    assert L.vqvae_pixelcnn_sample_packed_bytes(512, 260, 15, 10) == 0         # dim > 256
    assert L.vqvae_pixelcnn_sample_packed_bytes(1, 64, 15, 10) == 0            # K < 2
    assert L.vqvae_pixelcnn_sample_packed_bytes(8193, 64, 15, 10) == 0         # K > 8192
    assert L.vqvae_pixelcnn_sample_packed_bytes(512, 64, 0, 10) == 0
    assert L.vqvae_pixelcnn_sample_packed_bytes(512, 64, 15, 0) == 0
    assert L.vqvae_pixelcnn_sample_workspace_bytes(64, 8, 8, 64, 15) > 0
    assert L.vqvae_pixelcnn_sample_workspace_bytes(1, 1, 1, 4, 1) > 0
    assert L.vqvae_pixelcnn_sample_workspace_bytes(64, 64, 64, 128, 15) > 0
    assert L.vqvae_pixelcnn_sample_workspace_bytes(64, 8, 6, 64, 15) == 0      # not square
    assert L.vqvae_pixelcnn_sample_workspace_bytes(64, 129, 129, 64, 15) == 0  # larger than 128 x 128
    assert L.vqvae_pixelcnn_sample_workspace_bytes(64, 8, 8, 62, 15) == 0
    assert L.vqvae_pixelcnn_sample_workspace_bytes(0, 8, 8, 64, 15) == 0
    # the workspace grows linearly with the batch
    assert L.vqvae_pixelcnn_sample_workspace_bytes(64, 8, 8, 64, 15) == 64 * L.vqvae_pixelcnn_sample_workspace_bytes(1, 8, 8, 64, 15)


def test_entries_reject_bad_arguments_without_gpu():
    L = _lib()
    a = 256
    nb = L.vqvae_pixelcnn_sample_packed_bytes(512, 64, 2, 10)
    nws = L.vqvae_pixelcnn_sample_workspace_bytes(4, 8, 8, 64, 2)
    f = L.vqvae_pixelcnn_sample_f32
    #      packed, bytes, label, u, B, H, W, K, dim, nl, ncls, samples, logits, status, ws, ws_bytes, stream
    assert f(None, nb, a, a, 4, 8, 8, 512, 64, 2, 10, a, None, a, a, nws, None) == -1
    assert f(a, nb, a, a, 4, 8, 8, 512, 64, 2, 10, a, None, None, a, nws, None) == -1      # status is required
    assert f(a, nb, a, a, 4, 8, 8, 512, 64, 2, 10, a, None, a, None, nws, None) == -1
    assert f(a, nb, a, a, 0, 8, 8, 512, 64, 2, 10, a, None, a, a, nws, None) == -2
    assert f(a, nb, a, a, 4, 0, 0, 512, 64, 2, 10, a, None, a, a, nws, None) == -2
    assert f(a, nb, a, a, 4, 8, 8, 512, 64, 0, 10, a, None, a, a, nws, None) == -2
    assert f(a, nb, a, a, 4, 8, 6, 512, 64, 2, 10, a, None, a, a, nws, None) == -3         # not square
    assert f(a, nb, a, a, 4, 8, 8, 512, 66, 2, 10, a, None, a, a, nws, None) == -3         # dim % 4
    assert f(a, nb, a, a, 4, 8, 8, 1, 64, 2, 10, a, None, a, a, nws, None) == -3           # K = 1
    assert f(a, nb, a, a, 4, 8, 8, 9000, 64, 2, 10, a, None, a, a, nws, None) == -3
    assert f(a, nb, a, a, 4, 200, 200, 512, 64, 2, 10, a, None, a, a, nws, None) == -3
    assert f(a + 4, nb, a, a, 4, 8, 8, 512, 64, 2, 10, a, None, a, a, nws, None) == -3     # misaligned image
    assert f(a, nb - 4, a, a, 4, 8, 8, 512, 64, 2, 10, a, None, a, a, nws, None) == -4
    assert f(a, nb, a, a, 4, 8, 8, 512, 64, 2, 10, a, None, a, a, nws - 4, None) == -4
    p = L.vqvae_pixelcnn_sample_pack_f32
    ptrs = (ctypes.c_void_p * 23)(*([a] * 23))
    assert p(None, 23, 512, 64, 2, 10, a, nb, None) == -1
    assert p(ptrs, 23, 512, 64, 2, 10, None, nb, None) == -1
    assert p(ptrs, 22, 512, 64, 2, 10, a, nb, None) == -2                                   # 9 n_layers + 5 parameters
    assert p(ptrs, 23, 512, 62, 2, 10, a, nb, None) == -3
    assert p(ptrs, 23, 512, 64, 2, 10, a, nb - 4, None) == -4
    ptrs[7] = None
    assert p(ptrs, 23, 512, 64, 2, 10, a, nb, None) == -1


def test_python_rejects_cpu_and_bad_shapes_without_gpu():
    from vqvae_amd._lib import VqvaeHipError
    m = _model(16, 8, 2, 3)
    with pytest.raises(VqvaeHipError):
        m.generate_cached(torch.zeros(2, dtype=torch.int64), (4, 4), 2)
