"""GPU parity tests (-m gpu) on REALLY TRAINED checkpoints (VERDICT r5 "next round" item 1).

Every other weight set in tests/ is the default init (torch.manual_seed(0)) or a synthetic "trained-like" construction
(tests/hetero.py).  These two were trained: tools/train_checkpoint.py ran the loop of main.py:67-98 (Adam amsgrad lr 3e-4,
recon / x_train_var + embedding loss) on the HIP training path over structured synthetic 32x32x3 images (tests/synthdata.py) --
5 000 updates at batch 32 (main.py's defaults; perplexity 2.7 -> 42) and 20 000 at batch 128 (perplexity -> 115) -- the state_dicts
came back from the GPU box (tests/golden/<name>_state.npz) and the UNMODIFIED reference, loaded with them in the build container,
produced tests/golden/trained_cases.npz (oracle/gen_golden.py trained; tests/test_oracle.py re-runs it where /root/reference is).

Checked here, through the C ABI:
  * P0: the quantizer on the REFERENCE's z_e bits -- indices and z_q bit-exact (z_e of a trained encoder: |z| up to 6, a codebook
    that moved to where z_e lives, 57 / 125 codes in use; the init's U(+-1/K) codebook exercises none of that);
  * P1: the whole forward in ALL THREE product schemes and the guard's own choice -- z_e and x_hat per output channel
    (|got - ref| <= 1e-5 max|ref channel| + 1e-4 |ref|), the decoder on the reference's z_q bits, index flips counted and each one
    explained by the z_e tolerance, loss / perplexity;
  * what vqvae_weights_range_check_f32 measures on a trained checkpoint (printed: <= 1.5 binades on both; the limit is 10) and
    that the module's default call therefore IS the two-term fp16 path, bit for bit;
  * BASELINE config-3 size (B = 4096 validation images, every one of the 262 144 rows) against oracle/torch_port.py.
"""
import os

import numpy as np
import pytest
import torch

from tests import cases, hetero, synthdata

pytestmark = pytest.mark.gpu

NAMES = list(cases.TRAINED_CASES)


def dev():
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden_trained():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trained_cases.npz"))


def _model(name):
    from vqvae_amd import conv
    from vqvae_amd.modules import VQVAE
    conv.set_conv_backend("hip")
    h, rh, nl, K, D, beta, B, seed = cases.TRAINED_CASES[name]
    m = VQVAE(h, rh, nl, K, D, beta).eval()
    m.load_state_dict(cases.trained_state(name), strict=True)
    return m.to(dev())


def _flags(scheme):
    from vqvae_amd import functional as F
    return {"guard": None, "fp16x2": 0, "bf16x3": F.FWD_CONV_BF16_SPLIT, "fp32": F.FWD_CONV_EXACT_FP32}[scheme]


@pytest.mark.parametrize("name", NAMES)
def test_quantizer_bit_exact_on_the_reference_ze_bits(name, golden_trained):
    h, rh, nl, K, D, beta, B, seed = cases.TRAINED_CASES[name]
    m = _model(name)
    g_ze = torch.from_numpy(golden_trained[f"{name}/z_e"]).to(dev())
    sha = golden_trained[f"{name}/sha"]
    with torch.no_grad():
        loss, z_q, ppl, onehot, idx = m.vector_quantization(g_ze)                                      # the module's NCHW boundary
        l2, zq2, p2, idx2, _ = m.vector_quantization.quantize(g_ze.permute(0, 2, 3, 1).contiguous(), rowmajor=True)   # the fused path's rows
    np.testing.assert_array_equal(idx.cpu().numpy().reshape(-1), golden_trained[f"{name}/idx"])
    np.testing.assert_array_equal(idx2.cpu().numpy().reshape(-1), golden_trained[f"{name}/idx"])
    assert cases.sha(z_q) == sha[2], "z_q (NCHW) not bit-exact"
    assert cases.sha(zq2.permute(0, 3, 1, 2).contiguous()) == sha[2], "z_q (rows) not bit-exact"
    np.testing.assert_allclose(loss.item(), golden_trained[f"{name}/loss"], rtol=1e-6)
    np.testing.assert_allclose(ppl.item(), golden_trained[f"{name}/perplexity"], rtol=1e-6)
    assert onehot.shape == (B * 64, K) and float(onehot.sum()) == B * 64
    # the decoder on the quantizer's (= the reference's) z_q bits
    with torch.no_grad():
        x_hat = m.decoder(z_q)
    hetero.per_channel_check(x_hat.cpu().numpy(), golden_trained[f"{name}/x_hat"], "x_hat(decoder on reference z_q)", per_image=False)


@pytest.mark.parametrize("scheme", ["guard", "fp16x2", "bf16x3", "fp32"])
@pytest.mark.parametrize("name", NAMES)
def test_whole_forward_vs_reference_golden(name, scheme, golden_trained, capsys):
    from vqvae_amd import _lib
    h, rh, nl, K, D, beta, B, seed = cases.TRAINED_CASES[name]
    m = _model(name)
    L = _lib.load()
    x = torch.from_numpy(golden_trained[f"{name}/x"])          # (committed beside the outputs: tests/synthdata.py rounds per host ISA)
    assert cases.sha(x) == golden_trained[f"{name}/sha"][0]
    xd = x.to(dev())
    flags = _flags(scheme)
    with torch.no_grad():
        loss, x_hat, ppl, idx = m._forward_c(xd, want_idx=True, fwd_flags=flags)
        cw, _keep = m._c_weights()
        eff = m.scheme_hint()[0] if flags is None else flags
        nws = L.vqvae_workspace_bytes(cw.dims, B, 32, 32)
        ws = torch.empty(nws, dtype=torch.uint8, device=dev())
        st = torch.cuda.current_stream().cuda_stream
        z_e = torch.empty(B, 8, 8, D, device=dev())
        _lib.check(L.vqvae_encoder_ex_f32(cw, xd.data_ptr(), B, 32, 32, eff, z_e.data_ptr(), ws.data_ptr(), nws, st))
        idx_enc = m.encode(xd) if flags is None else None
    torch.cuda.synchronize()
    g_ze = golden_trained[f"{name}/z_e"]
    ze = z_e.permute(0, 3, 1, 2).cpu().numpy()
    w_ze = hetero.per_channel_check(ze, g_ze, f"z_e [{scheme}]", per_image=False)
    got = idx.cpu().numpy().reshape(-1)
    want = golden_trained[f"{name}/idx"].astype(np.int64)
    cb64 = m.vector_quantization.embedding.weight.detach().cpu().double().numpy()
    zr = np.transpose(g_ze, (0, 2, 3, 1)).reshape(-1, D).astype(np.float64)
    cmax = np.abs(g_ze).max(axis=(0, 2, 3))
    flips, worst = hetero.explain_flips(got, want, zr, cb64, cmax)
    assert worst <= 1.0, f"an index flip is not explained by the z_e tolerance: gap = {worst:.3g} x the bound"
    assert len(flips) <= max(1, int(1e-3 * got.size)), f"{len(flips)} flips in {got.size} rows"
    clean = np.setdiff1d(np.arange(B), np.unique(flips // 64))
    w_xh = hetero.per_channel_check(x_hat.cpu().numpy()[clean], golden_trained[f"{name}/x_hat"][clean], f"x_hat [{scheme}]", per_image=False)
    if len(flips) == 0:
        np.testing.assert_allclose(loss.item(), golden_trained[f"{name}/loss"], rtol=2e-5)
        np.testing.assert_allclose(ppl.item(), golden_trained[f"{name}/perplexity"], rtol=1e-5)
    if idx_enc is not None:
        assert torch.equal(idx_enc, idx)
    with capsys.disabled():
        print(f"\n   [{name} / {scheme}] worst error in units of the channel maximum: z_e {w_ze:.2e}, x_hat {w_xh:.2e}; "
              f"{len(flips)} index flips / {got.size} rows (worst {worst:.2f} x the bound)")


@pytest.mark.parametrize("name", NAMES)
def test_range_guard_on_a_trained_checkpoint(name, capsys):
    """What the 10-binade limit of vqvae_weights_range_check_f32 (include/vqvae_hip.h) means for checkpoints training actually
    produces: the largest per-layer input-channel spread is 1.3-1.5 binades (default init: 0.1; tests/hetero.py's constructions:
    16-19), the guard recommends nothing, and the module's default call is the two-term fp16 path bit for bit."""
    h, rh, nl, K, D, beta, B, seed = cases.TRAINED_CASES[name]
    m = _model(name)
    flags, spreads = m.scheme_hint()
    xd = synthdata.normalised(64, seed + 100).to(dev())
    with torch.no_grad():
        auto = m._forward_c(xd, want_idx=True)
        named = m._forward_c(xd, want_idx=True, fwd_flags=0)
    torch.cuda.synchronize()
    with capsys.disabled():
        print(f"\n   [{name}] input-channel spread per layer (binades): " + " ".join(f"{v:.2f}" for v in spreads)
              + f" -> {'bf16x3' if flags else 'fp16x2'}")
    assert flags == 0, (flags, spreads)
    assert max(spreads) < 3.0, spreads                      # 7 binades of room below the limit
    assert torch.equal(auto[3], named[3]) and torch.equal(auto[1].view(torch.int32), named[1].view(torch.int32))


@pytest.mark.parametrize("scheme", ["guard", "bf16x3"])
@pytest.mark.parametrize("name", NAMES)
def test_config3_batch_every_row_vs_reference_port(name, scheme, capsys):
    """B = 4096 validation images, every one of the 262 144 latent rows against oracle/torch_port.py (bitwise the imported
    reference, tests/test_oracle.py)."""
    from oracle import torch_port
    h, rh, nl, K, D, beta, _, seed = cases.TRAINED_CASES[name]
    B = 4096
    m = _model(name)
    sd = cases.trained_state(name)
    x = synthdata.normalised(B, seed + 7)
    xd = x.to(dev())
    with torch.no_grad():
        loss, x_hat, ppl, idx = m._forward_c(xd, want_idx=True, fwd_flags=_flags(scheme))
        z_e_ref = torch.cat([torch_port.encode(sd, x[i:i + 512].clone(), nl) for i in range(0, B, 512)])
        cbk = sd["vector_quantization.embedding.weight"]
        outs = [torch_port.quantize(z_e_ref[i:i + 512], cbk, beta) for i in range(0, B, 512)]
        z_q_ref = torch.cat([o[1] for o in outs])
        idx_ref = torch.cat([o[4] for o in outs])
        x_hat_ref = torch.cat([torch_port.decode(sd, z_q_ref[i:i + 512].clone(), nl) for i in range(0, B, 512)])
    got, want = idx.cpu().numpy().reshape(-1), idx_ref.numpy().reshape(-1)
    zr = z_e_ref.permute(0, 2, 3, 1).reshape(-1, D).double().numpy()
    cmax = z_e_ref.abs().amax(dim=(0, 2, 3)).double().numpy()
    flips, worst = hetero.explain_flips(got, want, zr, cbk.double().numpy(), cmax)
    assert worst <= 1.0, f"an index flip is not explained by the z_e tolerance: gap = {worst:.3g} x the bound"
    assert len(flips) <= int(1e-4 * got.size), f"{len(flips)} flips in {got.size} rows (SURVEY 8c expects <= 1e-4)"
    clean = np.setdiff1d(np.arange(B), np.unique(flips // 64))
    w_xh = hetero.per_channel_check(x_hat.cpu().numpy()[clean], x_hat_ref.numpy()[clean], f"x_hat [{scheme}]", per_image=False)
    # merged scalars of the reference's 512-image slabs: loss = mean of slab losses (equal sizes); perplexity from the index histogram
    loss_ref = float(np.mean([o[0].item() for o in outs]))
    if len(flips) == 0:
        np.testing.assert_allclose(loss.item(), loss_ref, rtol=2e-5)
    p = np.bincount(want, minlength=K).astype(np.float64) / want.size
    ppl_ref = float(np.exp(-(p * np.log(p + 1e-10)).sum()))
    np.testing.assert_allclose(ppl.item(), ppl_ref, rtol=1e-4)
    with capsys.disabled():
        print(f"\n   [{name} / {scheme} / B=4096] {len(flips)} index flips / {got.size} rows (worst {worst:.2f} x the bound); x_hat worst "
              f"{w_xh:.2e} of its channel maximum; perplexity {ppl.item():.3f}, {len(np.unique(got))} codes in use")


@pytest.mark.parametrize("name", NAMES)
def test_wire_format_and_checkpoint_file_on_a_trained_checkpoint(name, golden_trained, tmp_path):
    """encode -> indices -> decode_indices on trained weights, and the checkpoint FILE layout of utils.py:109-113
    ({'model', 'results', 'hyperparameters'}) round-trips through torch.save / load_state_dict."""
    h, rh, nl, K, D, beta, B, seed = cases.TRAINED_CASES[name]
    m = _model(name)
    path = tmp_path / "vqvae_data_test.pth"
    torch.save({"model": m.state_dict(), "results": {"n_updates": 0}, "hyperparameters": {}}, path)
    from vqvae_amd.modules import VQVAE
    m2 = VQVAE(h, rh, nl, K, D, beta).eval()
    m2.load_state_dict(torch.load(path, map_location="cpu")["model"])
    m2 = m2.to(dev())
    xd = synthdata.normalised(B, seed).to(dev())
    with torch.no_grad():
        idx = m2.encode(xd)
        x_dec = m2.decode_indices(idx, B, 8, 8)
        _, x_hat, _, idx_f = m._forward_c(xd, want_idx=True)
    assert torch.equal(idx, idx_f)
    # decode_indices gathers e_k itself, forward decodes z + (e_k - z): equal up to that rounding of z_q
    scale = float(x_hat.abs().max())
    np.testing.assert_allclose(x_dec.cpu().numpy(), x_hat.cpu().numpy(), atol=2e-6 * scale, rtol=1e-5)


@pytest.mark.parametrize("form", [0, 8, 16], ids=["default_form", "units64_8waves", "units32_16waves"])
@pytest.mark.parametrize("rowmajor", [False, True], ids=["nchw", "rows"])
@pytest.mark.parametrize("name", NAMES)
def test_rows_at_the_dead_code_cluster_bit_exact(name, rowmajor, form, golden_trained):
    """What training leaves behind and no synthetic codebook of tests/ had: ~450 of the 512 codes never moved from their U(+-1/K)
    init -- at the scale of a trained |z| ~ 10 they are ONE point, so a row near the origin finds hundreds of codes above the
    screen's threshold, the task table (64 entries) overflows and the row takes torch.argmin over all codes.  Round 6 gave that
    path to the whole wave (it was one lane: 33 such rows made the kernel 14x slower).  Half of these rows are aimed at the cluster;
    indices and z_q against the C oracle, bit for bit."""
    from oracle import c_oracle
    from vqvae_amd import functional as F
    h, rh, nl, K, D, beta, B, seed = cases.TRAINED_CASES[name]
    cb = cases.trained_state(name)["vector_quantization.embedding.weight"]
    g = torch.Generator().manual_seed(99)
    z = torch.from_numpy(golden_trained[f"{name}/z_e"]).clone()                 # (32, 64, 8, 8)
    zr = z.permute(0, 2, 3, 1).reshape(-1, D)
    n = zr.shape[0]
    pick = torch.rand(n, generator=g) < 0.5
    scale = 10.0 ** (torch.rand(n, 1, generator=g) * 3 - 3)                     # |z| element scale 1e-3 .. 1
    zr[pick] = (torch.randn(n, D, generator=g) * scale)[pick]
    zr[::97] = 0.0                                                               # the origin itself
    z = zr.view(32, 8, 8, D).permute(0, 3, 1, 2).contiguous()
    ref = c_oracle.vq_forward(z.numpy(), cb.numpy(), beta)
    dead = (cb.norm(dim=1) < 0.05).numpy()
    assert dead.sum() > 300 and dead[ref["idx"].reshape(-1)].mean() > 0.2       # the cluster exists and wins many rows
    zd = z.to(dev())
    if rowmajor:
        zd = zd.permute(0, 2, 3, 1).contiguous()
    loss, zq, ppl, idx, hist = F.vq_forward(zd, cb.to(dev()), beta, rowmajor=rowmajor, form=form)
    torch.cuda.synchronize()
    if rowmajor:
        zq = zq.permute(0, 3, 1, 2).contiguous()
    np.testing.assert_array_equal(idx.cpu().numpy(), ref["idx"])
    assert np.array_equal(zq.cpu().numpy().view(np.uint32), ref["z_q"].view(np.uint32))
    np.testing.assert_allclose(loss.item(), ref["loss"], rtol=1e-6)
    np.testing.assert_array_equal(hist.cpu().numpy(), ref["hist"])


@pytest.mark.parametrize("name", NAMES)
def test_quantizer_time_on_trained_z_e_stays_near_the_init_models(name, capsys):
    """The stand-alone quantizer's time is data-dependent (open / hard / wide rows take the exact part).  On a trained checkpoint's
    own z_e (B = 4096: 262 144 rows) it must stay within 2x of the default-init model's (measured 1.1-1.3x; it was 14x before
    round 6's wave-wide path)."""
    from vqvae_amd import _lib, conv_hip, functional as F
    from vqvae_amd.modules import VQVAE
    h, rh, nl, K, D, beta, _, seed = cases.TRAINED_CASES[name]

    def time_vq(model, x):
        with torch.no_grad():
            z_e = conv_hip.encoder_forward(model.encoder, x, model.pre_quantization_conv)
            cbw = model.vector_quantization.embedding.weight.detach()
            ws = F.vq_workspace(K, D, dev())
            F.vq_forward(z_e, cbw, beta, rowmajor=True, workspace=ws)
            for _ in range(3):
                F.vq_forward(z_e, cbw, beta, rowmajor=True, workspace=ws, prepared=True)
            torch.cuda.synchronize()
            _lib.profile_enable(True)
            for _ in range(20):
                F.vq_forward(z_e, cbw, beta, rowmajor=True, workspace=ws, prepared=True)
            ms, cnt = _lib.profile_collect("vq_main")
            _lib.profile_enable(False)
        return ms / cnt * 1e3

    torch.manual_seed(0)
    init = VQVAE(h, rh, nl, K, D, beta).eval().to(dev())
    t_init = time_vq(init, torch.randn(4096, 3, 32, 32, generator=torch.Generator().manual_seed(1000)).to(dev()))
    t_tr = time_vq(_model(name), synthdata.normalised(4096, seed + 7).to(dev()))
    with capsys.disabled():
        print(f"\n   [{name}] stand-alone quantizer, 262 144 rows: {t_tr:.1f} us on the trained z_e, {t_init:.1f} us on the default-init model's")
    assert t_tr <= 2.0 * t_init


@pytest.mark.parametrize("name", NAMES)
def test_dead_code_cluster_on_the_two_sweep_filter_kernel(name, golden_trained):
    """NCHW maps whose pixel count is not a multiple of 32 (7x7, 14x14 ...) run vq_filter_kernel_d64, whose candidate lists overflow on a
    trained codebook the same way: those rows take vq_wave_argmin (round 6; one lane per row before: 1.8 ms instead of 75 us).  Bit-exact
    against the C oracle, half of the rows aimed at the cluster."""
    from oracle import c_oracle
    from vqvae_amd import functional as F
    h, rh, nl, K, D, beta, B, seed = cases.TRAINED_CASES[name]
    cb = cases.trained_state(name)["vector_quantization.embedding.weight"]
    g = torch.Generator().manual_seed(7)
    zr = torch.from_numpy(golden_trained[f"{name}/z_e"]).permute(0, 2, 3, 1).reshape(-1, D)[:36 * 49].clone()
    pick = torch.rand(zr.shape[0], generator=g) < 0.5
    zr[pick] = (torch.randn(zr.shape[0], D, generator=g) * 10.0 ** (torch.rand(zr.shape[0], 1, generator=g) * 3 - 3))[pick]
    z = zr.view(36, 7, 7, D).permute(0, 3, 1, 2).contiguous()
    ref = c_oracle.vq_forward(z.numpy(), cb.numpy(), beta)
    for bf in (False, True):
        loss, zq, ppl, idx, hist = F.vq_forward(z.to(dev()), cb.to(dev()), beta, rowmajor=False, bf16_filter=bf)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(idx.cpu().numpy(), ref["idx"])
        assert np.array_equal(zq.cpu().numpy().view(np.uint32), ref["z_q"].view(np.uint32))


def test_retraining_reproduces_the_committed_checkpoint_bit_for_bit(capsys):
    """main.py:67-98's loop on the HIP training path is deterministic (no floating-point atomics anywhere; the quantizer's indices are
    exact by contract): 5 000 updates of tools/train_checkpoint.py's loop on the same data must give the committed
    trained_main_defaults checkpoint BIT FOR BIT -- with every kernel change since it was made (round 6: NaN-keeping ReLUs, the wave-wide
    argmin, the ballot-prefix second screen) in the path.  ~10 s.  Skipped where the host's CPU makes other synthetic images
    (tests/synthdata.py's bicubic / sin / exp round per ISA)."""
    import hashlib
    from vqvae_amd import conv, training as T
    from vqvae_amd.modules import VQVAE
    x01 = synthdata.images01(50000, 2026)
    got_sha = hashlib.sha256(x01[:4096].numpy().tobytes()).hexdigest()[:16]
    if got_sha != "f32cbcd26e5039ae":                # the images the GPU boxes' host CPU (EPYC 9575F) makes: what the checkpoint was trained on
        pytest.skip(f"this host generates other synthetic training images ({got_sha}) than the checkpoint's host: another model would come out")
    want = cases.trained_state("trained_main_defaults")
    conv.set_conv_backend("hip")
    x_train_var = synthdata.train_var(x01)
    data = ((x01 - 0.5) / 0.5).to(dev())
    torch.manual_seed(0)
    model = VQVAE(128, 32, 2, 512, 64, 0.25).to(dev())
    opt = torch.optim.Adam(model.parameters(), lr=3e-4, amsgrad=True)
    model.train()
    g = torch.Generator().manual_seed(1)
    for i in range(5000):
        sel = torch.randint(0, 50000, (32,), generator=g).to(dev())
        x = data[sel].contiguous()
        opt.zero_grad()
        el, xh, pp = model(x)
        stats = T.step_losses(el, xh, pp, x, x_train_var)
        stats[1].backward()
        opt.step()
    torch.cuda.synchronize()
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    diff = {k: float((sd[k] - want[k]).abs().max()) for k in want if not torch.equal(sd[k].view(torch.int32), want[k].view(torch.int32))}
    assert not diff, f"retrained checkpoint differs from the committed one in {len(diff)} tensors: {diff}"
    with capsys.disabled():
        print("\n   5 000 updates on the HIP training path reproduce tests/golden/trained_main_defaults_state.npz bit for bit")
