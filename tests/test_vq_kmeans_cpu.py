"""k-means initialisation without a GPU: the fp64 restatement (tests/kmeans_ref.py) vectorised against its plain loops, the
properties the GPU tests rely on (zero-weight rows are never picked, repeated points, separated blobs), and the C ABI's new entries
(exported, bound, sized, argument errors before any launch)."""
import numpy as np
import pytest
import torch

from tests import kmeans_ref as R

U_TOP = np.float32(1.0) - np.float32(2.0 ** -24)          # the largest fp32 below 1


def _uniforms(K, seed):
    return np.random.default_rng(seed).random(K, dtype=np.float32)


@pytest.mark.parametrize("N,D,K", [(600, 5, 12), (256, 3, 7), (1, 4, 3), (257, 1, 9)])
def test_vectorised_seeding_matches_the_plain_loops(N, D, K):
    g = np.random.default_rng(N + K)
    z = g.standard_normal((N, D)).astype(np.float32)
    z[N // 2] = z[0]                                        # a repeated row
    for seed in range(3):
        u = _uniforms(K, seed)
        u[1 % K] = 0.0
        u[K - 1] = U_TOP
        a, b = R.seed(z, K, u), R.seed_loop(z, K, u)
        assert np.array_equal(a, b)
        assert a.min() >= 0 and a.max() < N


def test_groups_of_several_blocks_match_the_plain_loops():
    # more than 256 blocks: groups hold two blocks, the last group is partial
    N = 256 * 300 + 17
    z = np.random.default_rng(0).standard_normal((N, 2)).astype(np.float32)
    u = np.array([0.3, 0.0, U_TOP, 0.5, 0.999], dtype=np.float32)
    a = R.seed(z, 5, u)
    assert np.array_equal(a, R.seed_loop(z, 5, u))
    assert len(set(a.tolist())) == 5 and a.max() >= 256 * 256           # distinct rows, one beyond the first group


def test_every_chosen_row_has_positive_weight_while_the_total_is_positive():
    z, _ = R.repeated_points(40, 9, 6, 1)                   # 360 rows, 40 distinct
    for seed in range(4):
        u = _uniforms(48, seed)
        u[3], u[4] = 0.0, U_TOP
        trace = []
        rows = R.seed(z, 48, u, trace)
        for k, (w, T) in enumerate(trace, start=1):
            assert (w >= 0).all()
            if T > 0:
                assert w[rows[k]] > 0, (seed, k)
            else:
                assert k >= 40 and rows[k] == R.uniform_row(u[k], len(z))
            assert (w[rows[:k]] == 0).all()                 # chosen centres (and their copies) weigh exactly nothing


@pytest.mark.parametrize("M,r,D", [(16, 8, 64), (5, 60, 3), (300, 2, 4)])
def test_repeated_points_are_each_hit_once(M, r, D):
    z, which = R.repeated_points(M, r, D, M)
    N = M * r
    for u in (np.zeros(M, np.float32), np.full(M, U_TOP, np.float32), _uniforms(M, 1), _uniforms(M, 2)):
        rows = R.seed(z, M, u)
        assert sorted(which[rows].tolist()) == list(range(M))
    # more codes than distinct rows: the surplus follows the T = 0 rule
    u = _uniforms(M + 6, 3)
    rows = R.seed(z, M + 6, u)
    assert sorted(which[rows[:M]].tolist()) == list(range(M))
    assert rows[M:].tolist() == [R.uniform_row(v, N) for v in u[M:]]


@pytest.mark.parametrize("K,n,D", [(8, 32, 64), (16, 16, 8), (5, 51, 3)])
def test_separated_blobs_get_one_code_each_and_equal_counts(K, n, D):
    z, which, sep = R.blobs(K, n, D, K)
    assert sep >= 100.0
    for seed in range(5):
        u = _uniforms(K, 10 + seed)
        rows = R.seed(z, K, u)
        assert sorted(which[rows].tolist()) == list(range(K)), seed
        cb, counts, rows2 = R.kmeans(z, K, 1, u)
        assert np.array_equal(rows, rows2)
        assert counts.tolist() == [n] * K
        # every code is the mean of its blob
        for k in range(K):
            m = z[which == which[rows[k]]].astype(np.float64).mean(0)
            np.testing.assert_allclose(cb[k], m, rtol=1e-6, atol=1e-7)


def test_update_matches_a_per_row_loop():
    g = np.random.default_rng(5)
    N, K, D = 300, 24, 5
    z = g.standard_normal((N, D)).astype(np.float32)
    idx = g.integers(0, 6, N)                               # most codes get no row
    cb = g.standard_normal((K, D)).astype(np.float32)
    u = _uniforms(K, 6)
    for uu in (None, u):
        a, ca = R.update(z, idx, cb, uu)
        b, cbn = R.update_loop(z, idx, cb, uu)
        assert np.array_equal(ca, cbn) and ca.sum() == N
        np.testing.assert_allclose(a, b, rtol=1e-13, atol=1e-15)
        empty = ca == 0
        assert empty.sum() == K - 6
        want = z[[R.uniform_row(v, N) for v in u[empty]]] if uu is not None else cb[empty]
        assert np.array_equal(a[empty], want.astype(np.float64))


def test_new_symbols_are_exported_and_bound():
    import ctypes
    from vqvae_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    for s in ("vqvae_vq_kmeans_workspace_bytes", "vqvae_vq_kmeans_seed_f32", "vqvae_vq_kmeans_update_f32"):
        assert hasattr(lib, s)
        assert s in _lib.SIGNATURES
        assert getattr(_lib.load(), s).argtypes is not None
    assert _lib.load().vqvae_abi_version() == 9


def test_workspace_sizing_envelope():
    from vqvae_amd import _lib
    L = _lib.load()
    f = L.vqvae_vq_kmeans_workspace_bytes
    assert f(2048, 512, 64) >= max(2048 * 8 + 8 * 8, L.vqvae_vq_backward_workspace_bytes(2048, 512, 64))
    assert f(1 << 20, 16, 4) >= (1 << 20) * 8 + 4096 * 8    # the weights and the block sums of the seeding
    assert f(1, 16384, 256) > 0 and f(2 ** 31 - 1, 1, 1) > 0
    for N, K, D in ((0, 512, 64), (2 ** 31, 512, 64), (2048, 16385, 64), (2048, 512, 257), (2048, 0, 64), (2048, 512, 0)):
        assert f(N, K, D) == 0, (N, K, D)


def test_argument_errors_without_gpu():
    from vqvae_amd import _lib
    L = _lib.load()
    a, big = 256, 1 << 30                     # a fake, aligned "device pointer" (never dereferenced)
    s, u = L.vqvae_vq_kmeans_seed_f32, L.vqvae_vq_kmeans_update_f32
    assert s(None, 1, 64, 8, 8, 16, a, 0, a, a, a, big, None) == -1
    assert s(a, 1, 64, 8, 8, 16, None, 0, a, a, a, big, None) == -1          # the seeding needs its uniforms
    assert s(a, 1, 64, 8, 8, 16, a, 0, None, a, a, big, None) == -1
    assert s(a, 1, 64, 8, 8, 16, a, 0, a, None, a, big, None) == -1
    assert s(a, 0, 64, 8, 8, 16, a, 0, a, a, a, big, None) == -2
    assert s(a, 1, 64, 8, 0, 16, a, 0, a, a, a, big, None) == -2
    assert s(a, 1, 257, 8, 8, 16, a, 0, a, a, a, big, None) == -3
    assert s(a, 1, 64, 8, 8, 16385, a, 0, a, a, a, big, None) == -3
    assert s(a, 1, 64, 8, 8, 0, a, 0, a, a, a, big, None) == -3
    assert s(a, 2 ** 31, 64, 1, 1, 16, a, 0, a, a, a, big, None) == -3
    assert s(a, 1, 64, 8, 8, 16, a, 0x2, a, a, a, big, None) == -3           # only VQVAE_VQ_ROWMAJOR
    assert s(a, 1, 64, 8, 8, 16, a, 0, a, a, a, 16, None) == -4
    assert s(a, 1, 64, 8, 8, 16, a, 1, a, a, None, 0, None) == -4
    assert u(None, a, 1, 64, 8, 8, 16, None, 0, a, a, a, big, None) == -1
    assert u(a, None, 1, 64, 8, 8, 16, None, 0, a, a, a, big, None) == -1
    assert u(a, a, 1, 64, 8, 8, 16, None, 0, None, a, a, big, None) == -1
    assert u(a, a, 1, 64, 8, 8, 16, None, 0, a, None, a, big, None) == -1
    assert u(a, a, 0, 64, 8, 8, 16, None, 0, a, a, a, big, None) == -2
    assert u(a, a, 1, 257, 8, 8, 16, None, 0, a, a, a, big, None) == -3
    assert u(a, a, 1, 64, 8, 8, 16385, None, 0, a, a, a, big, None) == -3
    assert u(a, a, 1, 64, 8, 8, 0, None, 0, a, a, a, big, None) == -3
    assert u(a, a, 1, 64, 8, 8, 16, None, 0x4, a, a, a, big, None) == -3
    assert u(a, a, 1, 64, 8, 8, 16, None, 0, a, a, a, 16, None) == -4


def test_front_end_rejects_cpu_tensors_and_bad_shapes():
    from vqvae_amd import _lib, functional as F
    z = torch.zeros(1, 4, 2, 2)
    with pytest.raises(_lib.VqvaeHipError):
        F.vq_kmeans_seed(z, 2, torch.zeros(2))
    with pytest.raises(_lib.VqvaeHipError):
        F.vq_kmeans_update(z, torch.zeros(4, dtype=torch.int64), torch.zeros(2, 4))
    with pytest.raises(_lib.VqvaeHipError):
        F.vq_kmeans(z, 2)


def test_modules_are_unchanged_until_the_call():
    """construction draws what it always drew: init_codebook_ is opt-in"""
    from oracle import torch_port
    from vqvae_amd.modules import VQVAE, VectorQuantizer, VectorQuantizerEMA
    torch.manual_seed(0)
    m = VQVAE(128, 32, 2, 512, 64, 0.25)
    torch.manual_seed(0)
    ref = torch_port.init_state_dict()
    sd = m.state_dict()
    assert set(ref) <= set(sd) and "vector_quantization.embedding.weight" in ref
    for k, v in ref.items():
        assert torch.equal(sd[k], v), k
    assert float(sd["vector_quantization.embedding.weight"].abs().max()) <= 1.0 / 512
    for cls in (VectorQuantizer, VectorQuantizerEMA):
        assert callable(getattr(cls, "init_codebook_"))
    assert callable(VQVAE.init_codebook_)
