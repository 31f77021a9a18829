"""CPU side of the cached sampler's sampling controls: the fp64 reference of the filtered draw on hand-computed cases, the new C
entry's declaration, export and argument checks without a device, and generate_cached's checks that need none."""
import numpy as np
import pytest
import torch

from tests import pixelcnn_sample_filter_ref as F
from tests import pixelcnn_sample_ref as R


def _lg(p):
    return np.asarray(p, dtype=np.float32)[None, :, None, None]


def _draw(lg, u, **kw):
    idx, near = F.filtered_draw(lg, np.full((1, 1, 1), u), **kw)
    return int(idx[0, 0, 0]), bool(near[0, 0, 0])


def test_top_p_keeps_the_documented_nucleus():
    logits = np.log(np.array([0.5, 0.25, 0.125, 0.125]))
    # masses ranked before the codes: 0, 0.5, 0.75, 0.875
    assert F.surviving(logits, top_p=0.6) == [0, 1]
    assert F.surviving(logits, top_p=0.76) == [0, 1, 2]
    assert not _draw(_lg(logits), 0.3, top_p=0.6)[1] and not _draw(_lg(logits), 0.3, top_p=0.76)[1]
    # top_p = 0.5: the mass before code 1 is exactly the bound, so the rule (strictly less) drops it -- and the position is near
    assert F.surviving(logits, top_p=0.5) == [0]
    assert _draw(_lg(logits), 0.3, top_p=0.5)[1]
    # within the nucleus the draw is the renormalised CDF: {0, 1} at 2/3, 1/3
    assert _draw(_lg(logits), 0.66, top_p=0.6)[0] == 0 and _draw(_lg(logits), 0.67, top_p=0.6)[0] == 1
    # a nucleus out of index order: the ranking is by logit, the draw by index
    perm = np.log(np.array([0.125, 0.5, 0.125, 0.25]))
    assert F.surviving(perm, top_p=0.6) == [1, 3]
    assert F.surviving(perm, top_p=0.76) == [0, 1, 3]                  # of the tied 0.125s the lower index ranks first


def test_top_k_ties_go_to_the_lower_index():
    tied = np.array([1.0, 1.0, 1.0, 0.0])
    assert F.surviving(tied, top_k=2) == [0, 1]
    assert F.surviving(tied, top_k=3) == [0, 1, 2]
    assert F.surviving(tied, top_k=1) == [0]                          # greedy: the argmax with the lowest index
    assert F.surviving(np.array([0.0, 2.0, 2.0, 1.0]), top_k=1) == [1]
    assert F.surviving(np.array([0.0, -0.0, -1.0]), top_k=1) == [0]   # -0 ranks as +0
    assert F.surviving(tied, top_k=4) == [0, 1, 2, 3] and F.surviving(tied, top_k=0) == [0, 1, 2, 3]     # >= K, 0: off
    for u in (0.0, 0.3, 0.999):
        assert _draw(_lg([0.3, 0.1, 2.0, 1.9]), u, top_k=1)[0] == 2


def test_temperature_limit_and_order():
    lg = np.array([0.2, 1.0, 0.9, -1.0])
    for u in (1e-6, 0.5, 0.9999):                                    # exp(-80) of the mass before code 1, exp(-10) = 4.5e-5 after it
        assert _draw(_lg(lg), u, temperature=0.01)[0] == 1
    # top-k before the temperature, the nucleus after it: at T = 0.5 the probabilities of (0, 1) are 1 / (1 + e^2), e^2 / (1 + e^2)
    lg2 = np.array([0.0, 1.0, -3.0])
    p0 = 1.0 / (1.0 + np.exp(2.0))
    assert _draw(_lg(lg2), p0 - 1e-3, temperature=0.5, top_k=2)[0] == 0
    assert _draw(_lg(lg2), p0 + 1e-3, temperature=0.5, top_k=2)[0] == 1
    assert F.surviving(lg2, temperature=0.5, top_p=0.85) == [1]       # 0.88 of the mass on code 1 at T = 0.5 ...
    assert F.surviving(lg2, temperature=1.0, top_p=0.85) == [0, 1]    # ... 0.72 at T = 1


def test_everything_off_is_the_plain_inverse_cdf():
    g = np.random.default_rng(0)
    lg = g.normal(size=(3, 37, 4, 5)).astype(np.float32) * 2
    u = g.random((3, 4, 5))
    want, wnear = R.inverse_cdf(lg, u)
    for kw in ({}, {"top_k": 37}, {"top_k": None, "top_p": None}, {"temperature": 1.0, "top_k": 0, "top_p": 1.0}):
        got, near = F.filtered_draw(lg, u, **kw)
        assert np.array_equal(got, want) and np.array_equal(near, wnear)


def _lib():
    from vqvae_amd import _lib
    return _lib.load()


def test_entry_declared_and_exported():
    from tests.test_capi import declared_symbols
    from vqvae_amd import _lib as binding
    L = _lib()
    s = "vqvae_pixelcnn_sample_ex_f32"
    assert s in declared_symbols() and s in binding.SIGNATURES and hasattr(L, s)
    assert L.vqvae_abi_version() == 9
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vqvae_hip.h")).read()
    assert "#define VQVAE_SAMPLE_GIVEN_RANGE 2" in hdr
    from vqvae_amd import pixelcnn
    assert (pixelcnn.SAMPLE_NONFINITE, pixelcnn.SAMPLE_GIVEN_RANGE) == (1, 2)


def test_entry_rejects_bad_arguments_without_gpu():
    L = _lib()
    a = 256
    nb = L.vqvae_pixelcnn_sample_packed_bytes(512, 64, 2, 10)
    nws = L.vqvae_pixelcnn_sample_workspace_bytes(4, 8, 8, 64, 2)
    f = L.vqvae_pixelcnn_sample_ex_f32
    nan, inf = float("nan"), float("inf")

    def call(T=1.0, k=0, p=1.0, given=None, packed=a, pbytes=nb, B=4, H=8, W=8, K=512, dim=64, nl=2, status=a, ws=a, wbytes=nws):
        return f(packed, pbytes, a, a, B, H, W, K, dim, nl, 10, T, k, p, given, a, None, status, ws, wbytes, None)

    for T in (0.0, -1.0, nan, inf, -inf):
        assert call(T=T) == -2, T
    assert call(k=-1) == -2
    for p in (0.0, 1.5, nan, -0.5):
        assert call(p=p) == -2, p
    for kw in ({"T": 0.0, "given": a}, {"k": -1, "T": 0.7}, {"p": nan, "k": 5}):
        assert call(**kw) == -2, kw
    # the plain entry's cases, with valid options and with given codes
    for opt in ({}, {"T": 0.7, "k": 5, "p": 0.9, "given": a}):
        assert call(packed=None, **opt) == -1
        assert call(status=None, **opt) == -1
        assert call(ws=None, **opt) == -1
        assert call(B=0, **opt) == -2
        assert call(H=0, W=0, **opt) == -2
        assert call(nl=0, **opt) == -2
        assert call(W=6, **opt) == -3                      # not square
        assert call(dim=66, **opt) == -3                   # dim % 4
        assert call(K=1, **opt) == -3
        assert call(K=9000, **opt) == -3
        assert call(H=200, W=200, **opt) == -3
        assert call(packed=a + 4, **opt) == -3             # misaligned image
        assert call(pbytes=nb - 4, **opt) == -4
        assert call(wbytes=nws - 4, **opt) == -4
    # a NULL pointer is reported before a bad option, a bad option before an unsupported shape
    assert call(packed=None, T=0.0) == -1
    assert call(W=6, T=0.0) == -2


def test_python_checks_without_gpu():
    from vqvae_amd._lib import VqvaeHipError
    from vqvae_amd.pixelcnn import GatedPixelCNN
    torch.manual_seed(0)
    m = GatedPixelCNN(16, 8, 2, 3).eval()
    lab = torch.zeros(2, dtype=torch.int64)
    with pytest.raises(VqvaeHipError):
        m.generate_cached(lab, (4, 4), 2, temperature=0.7, top_k=5, top_p=0.9, given=torch.full((2, 4, 4), -1))
    for kw in ({"temperature": 0}, {"temperature": -1.0}, {"temperature": float("nan")}, {"temperature": float("inf")},
               {"top_k": -1}, {"top_p": 0}, {"top_p": 1.5}, {"top_p": float("nan")}):
        with pytest.raises(ValueError):
            m.generate_cached(lab, (4, 4), 2, **kw)
    with pytest.raises(TypeError):
        m.generate_cached(lab, (4, 4), 2, None, None, False, 0.7)     # the options are keyword-only
