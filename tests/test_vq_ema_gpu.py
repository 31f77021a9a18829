"""EMA codebook updates on the GPU (vqvae_vq_ema_update_f32, VectorQuantizerEMA, VQVAE(..., ema_decay=...)) against the fp64
restatement of tests/vq_ema_ref.py, the C oracle and the plain VQVAE.

Tolerances: ema_cluster_size / ema_w within 1 ulp of the fp64 restatement rounded to fp32, the codebook within 2 ulp (one
update; the GPU's fp64 sums run in another fixed order); restarted rows bit-exact; dz rtol 1e-5; 30-update trajectories rtol 1e-5."""
import copy

import numpy as np
import pytest
import torch

from tests import vq_ema_ref as R
from tests.test_training_gpu import CASES

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _ulps(got, ref64):
    """|got - round32(ref)| in units of fp32 spacing at round32(ref)"""
    ref = ref64.float().cpu().numpy()
    got = got.detach().float().cpu().numpy()
    sp = np.spacing(np.maximum(np.abs(ref), np.float32(np.finfo(np.float32).tiny))).astype(np.float64)
    return np.abs(got.astype(np.float64) - ref.astype(np.float64)) / sp


def _layout(z_nchw, rowmajor):
    return z_nchw.permute(0, 2, 3, 1).contiguous() if rowmajor else z_nchw.contiguous()


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.uint32)


def _update(z, idx, cs, w, rowmajor, decay=0.99, eps=1e-5, threshold=None, uniforms=None):
    from vqvae_amd import functional as F
    cs_d, w_d = cs.to(DEV).clone(), w.to(DEV).clone()
    cb = torch.empty_like(w_d)
    F.vq_ema_update(z, idx, cs_d, w_d, cb, decay, eps, threshold=threshold, uniforms=uniforms, rowmajor=rowmajor)
    torch.cuda.synchronize()
    return cs_d, w_d, cb


def _histograms(K, N, cb, z_nchw):
    """idx variants: every row on one code, a 420-code cluster, and the forward's indices against a freshly initialised codebook"""
    from vqvae_amd import functional as F
    g = torch.Generator().manual_seed(N + K)
    out = {"one code": torch.full((N, 1), K // 3, dtype=torch.int64),
           "cluster": torch.randint(0, min(420, K), (N, 1), generator=g)}
    _, _, _, idx, _ = F.vq_forward(z_nchw.to(DEV), cb.to(DEV), 0.25)
    out["fresh"] = idx.cpu()
    return out


@pytest.mark.parametrize("B,D,H,W,K", CASES + [(2, 128, 8, 8, 8192)])
@pytest.mark.parametrize("rowmajor", [False, True])
def test_one_update_against_the_restatement(B, D, H, W, K, rowmajor):
    g = torch.Generator().manual_seed(B * 7 + K)
    z = torch.randn(B, D, H, W, generator=g) * 0.05
    cb0 = (torch.rand(K, D, generator=g) * 2 - 1) / K
    cs0 = torch.rand(K, generator=g) * 2 * (torch.rand(K, generator=g) < 0.5)     # a warm state: half the codes have counts
    w0 = cb0 * cs0[:, None] + (torch.rand(K, D, generator=g) - 0.5) * 1e-3
    zd = _layout(z, rowmajor).to(DEV)
    rows = R.rows_of(z.permute(0, 2, 3, 1), True)
    for name, idx in _histograms(K, B * H * W, cb0, z).items():
        for cs, w in ((torch.zeros(K), cb0.clone()), (cs0, w0)):
            cs_d, w_d, cb = _update(zd, idx.to(DEV), cs, w, rowmajor)
            ref = R.ema_update(rows, idx, cs, w, 0.99, 1e-5)
            assert _ulps(cs_d, ref["N"]).max() <= 1, name
            assert _ulps(w_d, ref["m"]).max() <= 1, name
            assert _ulps(cb, ref["e"]).max() <= 2, name
            again = _update(zd, idx.to(DEV), cs, w, rowmajor)
            for a, b in zip((cs_d, w_d, cb), again):
                assert np.array_equal(_bits(a), _bits(b)), f"{name}: not bit-reproducible"


@pytest.mark.parametrize("rowmajor", [False, True])
def test_restart_takes_the_rows_the_uniforms_pick(rowmajor):
    B, D, H, W, K = 4, 64, 8, 8, 512
    g = torch.Generator().manual_seed(11)
    z = torch.randn(B, D, H, W, generator=g) * 0.05
    N = B * H * W
    idx = torch.randint(0, 40, (N, 1), generator=g)            # 40 codes share 256 rows: every other code is dead
    cs, w = torch.zeros(K), (torch.rand(K, D, generator=g) * 2 - 1) / K
    u = torch.rand(K, generator=g)
    tau = 0.01 * 6                                             # one update from 0: N_k = 0.01 c_k -> dead below 6 rows
    cs_d, w_d, cb = _update(_layout(z, rowmajor).to(DEV), idx.to(DEV), cs, w, rowmajor, threshold=tau, uniforms=u.to(DEV))
    rows = R.rows_of(z.permute(0, 2, 3, 1), True)
    ref = R.ema_update(rows, idx, cs, w, 0.99, 1e-5, tau, u)
    dead = ref["dead"]
    assert 0 < int(dead[:40].sum()) < 40 and bool(dead[40:].all())
    r = R.restart_rows(u, N)
    assert np.array_equal(_bits(cb)[dead.numpy()], _bits(rows[r[dead]])), "restarted codes must hold their rows bit for bit"
    assert _ulps(cb[~dead.to(DEV)], ref["e"][~dead]).max() <= 2
    assert _ulps(cs_d, ref["N"]).max() <= 1 and _ulps(w_d, ref["m"]).max() <= 1       # N and m stay as updated


@pytest.mark.parametrize("rowmajor", [False, True])
def test_gradients_and_the_in_place_update(rowmajor):
    from vqvae_amd.modules import VectorQuantizerEMA
    torch.manual_seed(3)
    vq = VectorQuantizerEMA(512, 64, 0.25).to(DEV).train()
    w = vq.embedding.weight
    e_before = w.detach().clone()
    v0 = w._version
    z_cpu = torch.randn(8, 64, 8, 8) * 0.05
    z = _layout(z_cpu, rowmajor).to(DEV).requires_grad_(True)
    g_zq = torch.randn_like(z)
    loss, z_q, ppl, idx, hist = vq.quantize(z, rowmajor=rowmajor)
    assert w._version > v0 and not torch.equal(w.detach(), e_before), "the training forward updates the codebook in place"
    (0.7 * loss + (z_q * g_zq).sum()).backward()                   # must not trip autograd's version check
    assert w.grad is None
    e_idx = e_before[idx.view(-1)]
    e_idx = e_idx.view(8, 8, 8, 64) if rowmajor else e_idx.view(8, 8, 8, 64).permute(0, 3, 1, 2)
    # z_q is the reference's straight-through z + (e_idx - z) (models/quantizer.py:67), of the codebook before the update
    zd = z.detach()
    assert torch.equal(z_q.detach(), zd + (e_idx.contiguous() - zd)), "z_q comes from the codebook before the update"
    mse = ((e_idx.double() - z.detach().double()) ** 2).mean()
    torch.testing.assert_close(loss.double().cpu(), (0.25 * mse).cpu(), rtol=1e-6, atol=0)
    ref = R.commitment_grad(z.detach().cpu(), e_idx.cpu(), g_zq.cpu(), 0.7, 0.25)
    torch.testing.assert_close(z.grad.cpu().double(), ref, rtol=1e-5, atol=1e-9)


def test_trajectory_of_30_updates():
    from vqvae_amd.modules import VectorQuantizerEMA
    torch.manual_seed(5)
    K, D = 256, 32
    vq = VectorQuantizerEMA(K, D, 0.25, decay=0.9).to(DEV).train()
    cs, w = torch.zeros(K, dtype=torch.float64), vq.ema_w.detach().double().cpu()
    g = torch.Generator().manual_seed(6)
    with torch.no_grad():
        for t in range(30):
            z = (torch.randn(4, 8, 8, D, generator=g) * 0.1 + 0.02 * t)
            _, _, _, idx, _ = vq.quantize(z.to(DEV), rowmajor=True)
            ref = R.ema_update(z.reshape(-1, D), idx.cpu(), cs, w, 0.9, 1e-5)
            cs, w = ref["N"], ref["m"]
            torch.testing.assert_close(vq.embedding.weight.detach().cpu().double(), ref["e"], rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(vq.ema_cluster_size.cpu().double(), cs, rtol=1e-5, atol=1e-7)
    torch.testing.assert_close(vq.ema_w.cpu().double(), w, rtol=1e-5, atol=1e-7)


def _trained_codebook(restart):
    from vqvae_amd.modules import VectorQuantizerEMA
    torch.manual_seed(7)
    vq = VectorQuantizerEMA(512, 64, 0.25, decay=0.99, restart_threshold=1.0 if restart else None,
                            generator=torch.Generator(device=DEV).manual_seed(8) if restart else None).to(DEV).train()
    g = torch.Generator().manual_seed(9)
    used = torch.zeros(512, dtype=torch.bool)
    with torch.no_grad():
        for _ in range(50):
            z = torch.randn(4, 8, 8, 64, generator=g) * 0.05
            _, _, _, idx, _ = vq.quantize(z.to(DEV), rowmajor=True)
            used[idx.view(-1).cpu()] = True
    return vq.embedding.weight.detach().cpu().clone(), used


@pytest.mark.parametrize("restart", [False, True])
def test_quantizer_forms_on_ema_codebooks(restart):
    from oracle import c_oracle
    from tests.test_vq_gpu import ALL_FORMS, _run
    cb, used = _trained_codebook(restart)
    if not restart:
        # codes no row picks: N_k -> 0, so the smoothed count is ~eps and e_k ~ decay^t m_0 / eps, far from the data
        assert (~used).any()
        assert float(cb[~used].abs().amax(1).min()) > 1.0
    g = torch.Generator().manual_seed(10)
    for z in (torch.randn(4, 64, 8, 8, generator=g) * 0.05, torch.randn(4, 64, 8, 8, generator=g) * 2.0):
        ref = c_oracle.vq_forward(z.numpy(), cb.numpy(), 0.25)
        for name, kw in ALL_FORMS:
            loss, zq, ppl, idx, hist = _run(z, cb, 0.25, **kw)
            assert np.array_equal(idx, ref["idx"]), f"{name}: indices"
            assert np.array_equal(zq.view(np.uint32), ref["z_q"].view(np.uint32)), f"{name}: z_q"


def _models(**kw):
    from vqvae_amd import conv
    from vqvae_amd.modules import VQVAE
    conv.set_conv_backend("hip")
    torch.manual_seed(0)
    return VQVAE(128, 32, 2, 512, 64, 0.25, ema_decay=0.99, **kw).to(DEV)


def test_whole_path_in_eval_equals_the_plain_model():
    from vqvae_amd.modules import VQVAE
    m = _models()
    x = torch.randn(8, 3, 32, 32, device=DEV)
    with torch.no_grad():
        m.train()
        for _ in range(3):
            m(torch.randn(8, 3, 32, 32, device=DEV))        # move the codebook
        m.eval()
        el, xh, pp = m(x)
        idx = m.encode(x)
    plain = VQVAE(128, 32, 2, 512, 64, 0.25).to(DEV).eval()
    missing, unexpected = plain.load_state_dict(m.state_dict(), strict=False)
    assert not missing and sorted(unexpected) == ["vector_quantization.ema_cluster_size", "vector_quantization.ema_w"]
    with torch.no_grad():
        el0, xh0, pp0 = plain(x)
        idx0 = plain.encode(x)
    assert np.array_equal(_bits(xh), _bits(xh0)) and np.array_equal(_bits(pp), _bits(pp0))
    assert torch.equal(idx, idx0)
    mse = el0.double() / 1.25                                   # the plain model's loss is (1 + beta) mse
    torch.testing.assert_close(el.double(), 0.25 * mse, rtol=1e-6, atol=0)


def test_warm_state_after_an_update_equals_a_fresh_module():
    from vqvae_amd.modules import VQVAE
    m = _models()
    x1, x2 = torch.randn(8, 3, 32, 32, device=DEV), torch.randn(8, 3, 32, 32, device=DEV)
    z = torch.randn(8, 64, 8, 8, device=DEV) * 0.05
    vq = m.vector_quantization
    with torch.no_grad():
        m.eval()
        m(x2)                                                  # packs the whole-path weights and prepares the codebook image
        vq(z)
        sd0 = copy.deepcopy(m.state_dict())
        m(x1)                                                  # eval: no update
        for k, v in m.state_dict().items():
            assert torch.equal(v, sd0[k]), f"eval forward changed {k}"
        m.train()
        m(x1)                                                  # train mode under no_grad: updates
        assert not torch.equal(vq.embedding.weight, sd0["vector_quantization.embedding.weight"])
        assert not torch.equal(vq.ema_cluster_size, sd0["vector_quantization.ema_cluster_size"])
        m.eval()
        out, outq = m(x2), vq(z)
    fresh = VQVAE(128, 32, 2, 512, 64, 0.25, ema_decay=0.99).to(DEV).eval()
    fresh.load_state_dict(m.state_dict())
    with torch.no_grad():
        ref, refq = fresh(x2), fresh.vector_quantization(z)
    for a, b in zip(out, ref):
        assert np.array_equal(_bits(a), _bits(b)), "whole path after the update"
    for i in (0, 1, 2, 4):
        assert np.array_equal(_bits(outq[i]) if outq[i].dtype == torch.float32 else outq[i].cpu().numpy(),
                              _bits(refq[i]) if refq[i].dtype == torch.float32 else refq[i].cpu().numpy()), "prepared image"


def test_state_dict_round_trip_continues_training_bitwise():
    from vqvae_amd import training as T
    from vqvae_amd.modules import VQVAE
    m = _models().train()
    xs = [torch.randn(8, 3, 32, 32, device=DEV) for _ in range(3)]
    m(xs[0])[0].backward()
    m2 = VQVAE(128, 32, 2, 512, 64, 0.25, ema_decay=0.99).to(DEV).train()
    m2.load_state_dict(m.state_dict())
    for x in xs[1:]:
        outs = []
        for mm in (m, m2):
            mm.zero_grad(set_to_none=True)
            el, xh, pp = mm(x)
            st = T.step_losses(el, xh, pp, x, 0.06)
            st[1].backward()
            outs.append((st.detach().clone(), mm.encoder.conv_stack[0].weight.grad.clone()))
        assert np.array_equal(_bits(outs[0][0]), _bits(outs[1][0])) and np.array_equal(_bits(outs[0][1]), _bits(outs[1][1]))
        for k, v in m.state_dict().items():
            assert np.array_equal(_bits(v), _bits(m2.state_dict()[k])), k


def test_training_step_graph_replays_to_the_eager_bits():
    from vqvae_amd import training as T
    a = _models().train()
    b = copy.deepcopy(a)
    x = torch.randn(16, 3, 32, 32, device=DEV)

    def step(m):
        m.zero_grad(set_to_none=False)
        el, xh, pp = m(x)
        st = T.step_losses(el, xh, pp, x, 0.06)
        st[1].backward()
        return st

    for m in (a, b):                       # materialise the .grad buffers the capture accumulates into
        for p in m.parameters():
            if p.requires_grad:
                p.grad = torch.zeros_like(p)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step(b)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        step(a)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st_b = step(b)
    torch.cuda.synchronize()
    for _ in range(3):
        st_a = step(a)
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(_bits(st_a), _bits(st_b))
        for k, v in a.state_dict().items():
            assert np.array_equal(_bits(v), _bits(b.state_dict()[k])), k
        assert np.array_equal(_bits(a.encoder.conv_stack[0].weight.grad), _bits(b.encoder.conv_stack[0].weight.grad))
