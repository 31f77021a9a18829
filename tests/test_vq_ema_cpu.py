"""EMA codebook updates without a GPU: the fp64 restatement (tests/vq_ema_ref.py) against a per-row loop, the C ABI's new entries
(exported, bound, sized, argument errors before any launch) and the module layer's state (state_dict keys, pickle, deepcopy)."""
import copy
import io

import pytest
import torch

from tests import cases
from tests import vq_ema_ref as R


def _state(K, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(K, generator=g) * 3, (torch.rand(K, D, generator=g) * 2 - 1) / K


@pytest.mark.parametrize("threshold", [None, 0.5])
def test_restatement_matches_a_per_row_loop(threshold):
    g = torch.Generator().manual_seed(1)
    N, K, D = 300, 24, 5
    z = torch.randn(N, D, generator=g)
    idx = torch.randint(0, 6, (N,), generator=g)          # most codes get no row: some fall below the threshold
    cs, w = _state(K, D, 2)
    u = torch.rand(K, generator=g)
    a = R.ema_update(z, idx, cs, w, 0.9, 1e-5, threshold, u if threshold is not None else None)
    b = R.ema_update_loop(z, idx, cs, w, 0.9, 1e-5, threshold, u if threshold is not None else None)
    for k in ("N", "m", "e", "n"):
        torch.testing.assert_close(a[k], b[k], rtol=1e-12, atol=1e-14)
    if threshold is not None:
        assert a["dead"].any() and not a["dead"].all()
    # the Laplace-smoothed counts keep the total
    torch.testing.assert_close(a["smoothed"].sum(), a["n"], rtol=1e-12, atol=0)


def test_restart_rows_are_in_range():
    u = torch.tensor([0.0, 0.5, 0.99999994, 1.0 - 2.0 ** -24], dtype=torch.float32)
    r = R.restart_rows(u, 7)
    assert r.tolist() == [0, 3, 6, 6]


def test_new_symbols_are_exported_and_bound():
    import ctypes
    from vqvae_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    for s in ("vqvae_vq_ema_workspace_bytes", "vqvae_vq_ema_update_f32"):
        assert hasattr(lib, s)
        assert s in _lib.SIGNATURES
        assert getattr(_lib.load(), s).argtypes is not None
    from vqvae_amd import functional as F
    assert F.VQ_BWD_COMMITMENT == 0x800


def test_workspace_sizing_envelope():
    from vqvae_amd import _lib
    L = _lib.load()
    assert L.vqvae_vq_ema_workspace_bytes(2048, 512, 64) >= L.vqvae_vq_backward_workspace_bytes(2048, 512, 64) + 512 * 8
    assert L.vqvae_vq_ema_workspace_bytes(1, 16384, 256) > 0
    for N, K, D in ((0, 512, 64), (2 ** 31, 512, 64), (2048, 16385, 64), (2048, 512, 257), (2048, 0, 64), (2048, 512, 0)):
        assert L.vqvae_vq_ema_workspace_bytes(N, K, D) == 0, (N, K, D)


def test_argument_errors_without_gpu():
    from vqvae_amd import _lib
    L = _lib.load()
    a = 256                                   # a fake, aligned "device pointer" (never dereferenced)
    big = 1 << 30
    f = L.vqvae_vq_ema_update_f32
    assert f(None, a, 1, 64, 8, 8, 512, 0.99, 1e-5, -1.0, None, 0, a, a, a, a, big, None) == -1
    assert f(a, a, 1, 64, 8, 8, 512, 0.99, 1e-5, -1.0, None, 0, a, None, a, a, big, None) == -1
    assert f(a, a, 1, 64, 8, 8, 512, 0.99, 1e-5, -1.0, None, 0, a, a, None, a, big, None) == -1
    assert f(a, a, 0, 64, 8, 8, 512, 0.99, 1e-5, -1.0, None, 0, a, a, a, a, big, None) == -2
    assert f(a, a, 1, 64, 8, 8, 0, 0.99, 1e-5, -1.0, None, 0, a, a, a, a, big, None) == -2
    assert f(a, a, 1, 257, 8, 8, 512, 0.99, 1e-5, -1.0, None, 0, a, a, a, a, big, None) == -3
    assert f(a, a, 1, 64, 8, 8, 16385, 0.99, 1e-5, -1.0, None, 0, a, a, a, a, big, None) == -3
    assert f(a, a, 2 ** 31, 64, 1, 1, 512, 0.99, 1e-5, -1.0, None, 0, a, a, a, a, big, None) == -3
    assert f(a, a, 1, 64, 8, 8, 512, 0.99, 1e-5, -1.0, None, 0x2, a, a, a, a, big, None) == -3       # only VQVAE_VQ_ROWMAJOR
    assert f(a, a, 1, 64, 8, 8, 512, 1.5, 1e-5, -1.0, None, 0, a, a, a, a, big, None) == -3          # decay outside [0, 1]
    assert f(a, a, 1, 64, 8, 8, 512, 0.99, 0.0, -1.0, None, 0, a, a, a, a, big, None) == -3          # eps must be positive
    assert f(a, a, 1, 64, 8, 8, 512, 0.99, 1e-5, -1.0, None, 0, a, a, a, a, 16, None) == -4
    assert f(a, a, 1, 64, 8, 8, 512, 0.99, 1e-5, -1.0, None, 0, a, a, a, None, 0, None) == -4
    # the commitment-only z gradient: grad_z only
    b = L.vqvae_vq_backward_f32
    assert b(a, a, a, None, None, 1, 64, 8, 8, 512, 0.25, 0x800, None, a, a, big, None) == -1
    assert b(a, a, a, None, None, 1, 64, 8, 8, 512, 0.25, 0x800, a, a, a, big, None) == -3


def test_default_model_keeps_the_reference_state_dict_and_ema_adds_two_buffers(golden_models):
    from vqvae_amd.modules import VQVAE, VectorQuantizer, VectorQuantizerEMA
    for name, (h, rh, nl, K, D, beta, *_shape) in cases.MODEL_CASES.items():
        keys = list(golden_models[f"{name}/keys"])
        torch.manual_seed(0)
        m = VQVAE(h, rh, nl, K, D, beta)
        assert list(m.state_dict().keys()) == keys
        assert type(m.vector_quantization) is VectorQuantizer
        torch.manual_seed(0)
        e = VQVAE(h, rh, nl, K, D, beta, ema_decay=0.99)
        sd, sd0 = e.state_dict(), m.state_dict()
        assert isinstance(e.vector_quantization, VectorQuantizerEMA)
        assert [k for k in sd if k not in sd0] == ["vector_quantization.ema_cluster_size", "vector_quantization.ema_w"]
        assert all(k in sd for k in keys)
        # same random initialisation; the EMA state starts at (0, the initial codebook)
        for k in keys:
            assert torch.equal(sd[k], sd0[k]), k
        vq = e.vector_quantization
        assert not vq.embedding.weight.requires_grad
        assert torch.equal(vq.ema_cluster_size, torch.zeros(K)) and torch.equal(vq.ema_w, vq.embedding.weight.detach())
    with pytest.raises(ValueError):
        VQVAE(128, 32, 2, 512, 64, 0.25, restart_threshold=1.0)


@pytest.mark.parametrize("kw", [{}, {"ema_decay": 0.99}, {"ema_decay": 0.9, "restart_threshold": 1.0}])
def test_models_pickle_and_deepcopy(kw):
    from vqvae_amd.modules import VQVAE
    torch.manual_seed(0)
    m = VQVAE(128, 32, 2, 512, 64, 0.25, **kw)
    buf = io.BytesIO()
    torch.save(m, buf)
    buf.seek(0)
    for a in (torch.load(buf, weights_only=False), copy.deepcopy(m)):
        assert type(a.vector_quantization) is type(m.vector_quantization)
        assert list(a.state_dict()) == list(m.state_dict())
        for k, v in m.state_dict().items():
            assert torch.equal(a.state_dict()[k], v)
        if kw:
            assert a.vector_quantization.decay == kw["ema_decay"]
            assert a.vector_quantization.restart_threshold == kw.get("restart_threshold")
