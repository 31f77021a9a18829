"""The 32x32 whole-path kernels at every width their plan accepts (fwd_plan, vqvae_amd/csrc/model.hip), against oracle/torch_port.py.

Every other forward test that reaches enc_front8_h2_kernel / conv_res_pair8_h2_kernel / dec_tail8_h2_kernel uses res_h_dim = 32 and
D = 64.  The fourteen models of tests/forward_widths.py reach what those leave out: hidden tiles with 1 to 31 padded channels (also
inside the quantizing and the decoder-head instances), the 1x1 post conv's <1> and <4> instances, the front conv and the gathering
instance at Cin = 32 / 96 / 128 / 256, and the mixed plans (D = 96 / 256: layerwise encoder middle, fused decoder head, 0xFF-filled
per-image maxima next to kernels that store theirs plainly).  Two codebooks per model; x seeds on which the oracle has no row within
rounding of a tie (forward_widths.fragile_rows), so the indices are asserted exactly.

Tolerances are the project's tiers, none is new: z_e atol 2e-6; x_hat atol 1e-5 + rtol 1e-4; loss rtol 1e-4, perplexity rtol 1e-5
(tests/test_model_gpu.py).  The first two tests check the inputs and the case table and run without a GPU."""
import numpy as np
import pytest
import torch

from tests import forward_widths as fw

gpu = pytest.mark.gpu
ALL = [(n, c) for n in fw.CASES for c in fw.CODEBOOKS]
ALL_IDS = [f"{n}-{c}" for n, c in ALL]


def dev():
    return torch.device("cuda:0")


def _report(what, got, ref, atol, rtol):
    """print worst |err| / tolerance (the table in DESIGN.md section 3 is made of these lines), then assert"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    ratio = float((np.abs(got - ref) / (atol + rtol * np.abs(ref))).max())
    print(f"widths: {what}: worst |err| / tolerance = {ratio:.3f}")
    np.testing.assert_allclose(got, ref, atol=atol, rtol=rtol, err_msg=what)
    return ratio


_models = {}


def _device_model(name, codebook):
    """the row's model on the GPU with the reference's state (one per row and codebook, shared by the tests that do not change it)"""
    from vqvae_amd import conv
    conv.set_conv_backend("hip")
    key = (name, codebook)
    if key not in _models:
        m = fw.model(name)
        m.load_state_dict(fw.reference(name, codebook)["sd"], strict=True)
        _models[key] = m.to(dev())
    return _models[key]


def _entries(m, B):
    from vqvae_amd import _lib
    L = _lib.load()
    cw, keep = m._c_weights()
    ws, st = m._c_workspace(L, cw, B, 32, 32, dev())
    return L, cw, keep, ws, st


def _encoder_entry(m, x):
    """vqvae_encoder_f32 -> z_e as (B, D, 8, 8) on the host"""
    from vqvae_amd import _lib
    B = x.shape[0]
    L, cw, _keep, ws, st = _entries(m, B)
    xd = x.to(dev()).contiguous()
    z = torch.empty(B, 8, 8, cw.dims.embedding_dim, device=dev())
    _lib.check(L.vqvae_encoder_f32(cw, xd.data_ptr(), B, 32, 32, z.data_ptr(), ws.data_ptr(), ws.numel(), st))
    return z.permute(0, 3, 1, 2).cpu()


def _decoder_entry(m, z_q_rows):
    """vqvae_decoder_f32 on row-major latents (B, 8, 8, D) on the device -> x_hat on the device"""
    from vqvae_amd import _lib
    B = z_q_rows.shape[0]
    L, cw, _keep, ws, st = _entries(m, B)
    x_hat = torch.empty(B, 3, 32, 32, device=dev())
    _lib.check(L.vqvae_decoder_f32(cw, z_q_rows.data_ptr(), B, 8, 8, x_hat.data_ptr(), ws.data_ptr(), ws.numel(), st))
    return x_hat


def _rows(z_nchw):
    return z_nchw.to(dev()).permute(0, 2, 3, 1).contiguous()


# ---- the inputs: no row of the reference may sit within rounding of a tie (CPU) ---------------------------------------------------

@pytest.mark.parametrize("name,codebook", ALL, ids=ALL_IDS)
def test_no_fragile_row_in_any_case(name, codebook):
    """The committed x seed of every row and codebook gives the oracle no fragile row, and the codebooks are what the table says
    they are ("init": a handful of winners, z_q ~ 1e-3; "data": many winners, z_q at the scale of z_e).  A change of torch's
    generator fails here instead of turning the exact-index assertions below into flaky ones."""
    r = fw.reference(name, codebook)
    bad = fw.fragile_rows(r["z_e"], r["idx"], r["sd"][fw.CB])
    assert bad.numel() == 0, f"{bad.numel()} fragile rows on seed {fw.seed_of(name, codebook)}: {bad[:8].tolist()}"
    winners = torch.unique(r["idx"]).numel()
    if codebook == "init":
        assert 4 <= winners <= 23 and float(r["z_q"].abs().max()) < 0.02
    else:
        assert 55 <= winners <= 207 and float(r["z_q"].abs().max()) > 0.5 * float(r["z_e"].abs().max())


def test_the_case_table_is_what_the_plan_accepts():
    """(CPU) the table's route columns restate fwd_plan: which rows fuse the quantizer, which run the encoder's middle layerwise"""
    for name, c in fw.CASES.items():
        pair = c.nl == 2 and 1 <= c.Rh <= 32                                 # conv_res_pair_supported at 8x8, C = 128
        enc_pair_post = pair and c.D in (32, 64, 128)                        # res_pair_post_supported
        dec_front = pair and c.D % 32 == 0 and 32 <= c.D <= 256
        vq_fuse = enc_pair_post and dec_front and c.D == 64 and c.K <= 1024 and -(-c.K // 32) % 4 == 0
        assert c.vq_fused == vq_fuse, name
        assert c.enc_igemm == (1 if enc_pair_post else 3), name
        assert c.enc_res == (1 if c.nl <= 2 else 2), name                    # (nl = 3: a fused pair and a single layer)
        assert c.fwd_res == (1 if vq_fuse else 2 * c.enc_res), name
        assert (name in fw.MIXED) == (dec_front and not enc_pair_post), name
    assert fw.FUSED_VQ == list(fw.CASES)[:4]


# ---- checks 1 to 4 per row and codebook ----------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("name,codebook", ALL, ids=ALL_IDS)
def test_encoder_entry_vs_oracle(name, codebook):
    r = fw.reference(name, codebook)
    z_e = _encoder_entry(_device_model(name, codebook), r["x"])
    _report(f"{name}-{codebook} z_e", z_e.numpy(), r["z_e"].numpy(), 2e-6, 0)


@gpu
@pytest.mark.parametrize("name,codebook", ALL, ids=ALL_IDS)
def test_decoder_entry_on_the_oracles_z_q_vs_oracle(name, codebook):
    r = fw.reference(name, codebook)
    x_hat = _decoder_entry(_device_model(name, codebook), _rows(r["z_q"]))
    _report(f"{name}-{codebook} decoder x_hat", x_hat.cpu().numpy(), r["x_hat"].numpy(), 1e-5, 1e-4)


@gpu
@pytest.mark.parametrize("name,codebook", ALL, ids=ALL_IDS)
def test_forward_vs_oracle_indices_exact(name, codebook):
    r = fw.reference(name, codebook)
    m = _device_model(name, codebook)
    assert m.scheme_hint()[0] == 0                                           # the default two-term fp16 products: the fused kernels
    with torch.no_grad():
        loss, x_hat, ppl, idx = m._forward_c(r["x"].to(dev()), want_idx=True)
    torch.cuda.synchronize()
    got, want = idx.cpu().view(-1), r["idx"].view(-1)
    assert torch.equal(got, want), f"{int((got != want).sum())} of {got.numel()} indices differ from the oracle's"
    _report(f"{name}-{codebook} forward x_hat", x_hat.cpu().numpy(), r["x_hat"].numpy(), 1e-5, 1e-4)
    print(f"widths: {name}-{codebook} loss {loss.item()!r} vs {r['loss']!r}, perplexity {ppl.item()!r} vs {r['ppl']!r}")
    np.testing.assert_allclose(loss.item(), r["loss"], rtol=1e-4)
    np.testing.assert_allclose(ppl.item(), r["ppl"], rtol=1e-5)


@gpu
@pytest.mark.parametrize("name,codebook", ALL, ids=ALL_IDS)
def test_encode_and_decode_entries_equal_the_forward_and_the_decoder(name, codebook):
    """include/vqvae_hip.h: vqvae_encode_f32 gives vqvae_forward_f32's indices; vqvae_decode_f32(idx) is vqvae_decoder_f32 on
    codebook[idx] -- bit for bit, here also where the first decoder kernel gathers rows of 32, 96, 128 and 256 floats."""
    c = fw.CASES[name]
    r = fw.reference(name, codebook)
    m = _device_model(name, codebook)
    xd = r["x"].to(dev())
    with torch.no_grad():
        idx_f = m._forward_c(xd, want_idx=True)[3]
        idx = m.encode(xd)
        x_hat = m.decode_indices(idx, c.B, 8, 8)
        z_q = m.vector_quantization.embedding.weight.detach()[idx.view(-1)].view(c.B, 8, 8, c.D).contiguous()
        x_hat_d = _decoder_entry(m, z_q)
    torch.cuda.synchronize()
    assert idx.dtype == torch.int64 and idx.shape == idx_f.shape
    assert torch.equal(idx, idx_f), f"{int((idx != idx_f).sum())} indices differ from the forward's"
    assert torch.equal(x_hat.view(torch.int32), x_hat_d.view(torch.int32)), \
        f"{int((x_hat.view(torch.int32) != x_hat_d.view(torch.int32)).sum())} x_hat elements differ from the decoder's on the gathered rows"


# ---- check 5: the rows whose quantizer rides in the encoder's last kernel ------------------------------------------------------------

@gpu
@pytest.mark.parametrize("name,codebook", [(n, c) for n, c in ALL if n in fw.FUSED_VQ], ids=[i for (n, _), i in zip(ALL, ALL_IDS) if n in fw.FUSED_VQ])
def test_fused_quantizer_routes_agree_and_match_the_c_oracle_on_their_own_z_e(name, codebook):
    """The three-launch route against the VQVAE_FWD_DEBUG_ZE route (tests/test_forward_midfused_gpu.py) bit for bit with a padded
    hidden tile in the quantizing kernel and in the decoder's head, and the fused quantizer's indices against the C oracle on the
    z_e bits it quantized (test_fused_quantizer_against_the_oracle_on_its_own_z_e_bits)."""
    from oracle import c_oracle
    from vqvae_amd import functional as F
    c = fw.CASES[name]
    r = fw.reference(name, codebook)
    m = _device_model(name, codebook)
    xd = r["x"].to(dev())
    with torch.no_grad():
        a = [t.cpu() for t in m._forward_c(xd, want_idx=True, parts=1, fwd_flags=0)]
        b = m._forward_c(xd, want_idx=True, parts=1, fwd_flags=F.FWD_DEBUG_ZE)
        L, cw, _keep, ws, _st = _entries(m, c.B)
        off = L.vqvae_workspace_ze_offset(cw.dims, c.B, 32, 32)
        assert off > 0
        z_e = ws[off:off + c.B * 64 * 64 * 4].view(torch.float32).view(c.B * 64, 64).cpu().numpy().copy()
        b = [t.cpu() for t in b]
    bits = lambda t: t.contiguous().view(-1).view(torch.int32)
    assert torch.equal(a[3], b[3]), f"{int((a[3] != b[3]).sum())} indices differ between the routes"
    assert torch.equal(bits(a[1]), bits(b[1])), f"{int((bits(a[1]) != bits(b[1])).sum())} x_hat elements differ in their bits"
    assert torch.equal(bits(a[0]), bits(b[0])), f"loss {a[0].item()!r} vs {b[0].item()!r}"
    assert torch.equal(bits(a[2]), bits(b[2])), f"perplexity {a[2].item()!r} vs {b[2].item()!r}"
    want = c_oracle.vq_forward(z_e.reshape(-1, 64, 1, 1), r["sd"][fw.CB].numpy(), fw.BETA)["idx"].reshape(-1)
    got = b[3].view(-1).numpy()
    assert (got == want).all(), f"{int((got != want).sum())} of {got.size} indices differ from the C oracle's on the kernel's own z_e"
    np.testing.assert_allclose(z_e, r["z_e"].permute(0, 2, 3, 1).reshape(-1, 64).numpy(), atol=2e-6, rtol=0)


# ---- check 6: the route is the one the row is named for ------------------------------------------------------------------------------

def _launches(run):
    """-> {hook: launches} of run() alone (the profiler's hooks count per kernel family, vqvae_amd/_lib.py)"""
    from vqvae_amd import _lib
    torch.cuda.synchronize()
    _lib.profile_enable(True)
    try:
        for k in _lib.PROF_IDS:
            _lib.profile_collect(k)
        with torch.no_grad():
            run()
        return {k: _lib.profile_collect(k)[1] for k in _lib.PROF_IDS}
    finally:
        _lib.profile_enable(False)


@gpu
@pytest.mark.parametrize("name,codebook", ALL, ids=ALL_IDS)
def test_the_route_is_the_one_the_row_is_named_for(name, codebook):
    from vqvae_amd import functional as F
    c = fw.CASES[name]
    r = fw.reference(name, codebook)
    m = _device_model(name, codebook)
    xd = r["x"].to(dev())
    with torch.no_grad():
        m._forward_c(xd, want_idx=True, parts=1)                             # (packs the weights, prepares the codebook)
    enc = _launches(lambda: _encoder_entry(m, r["x"]))
    fwd = _launches(lambda: m._forward_c(xd, want_idx=True, parts=1, fwd_flags=0))
    print(f"widths: {name}-{codebook} launches: encoder entry {enc}, forward {fwd}")
    # the encoder entry: enc_front8_h2_kernel alone under 'conv_igemm' where the 3x3 and the 1x1 conv ride in the pair kernel, else
    # those two layerwise launches as well
    assert (enc["conv_igemm"], enc["res_layer"]) == (c.enc_igemm, c.enc_res), enc
    assert enc["vq_main"] == 0 and enc["conv_in"] == 0 and enc["conv_out"] == 0, enc
    # the forward: both fused ends on every row (enc_front: no 'conv_in'; dec_tail: one 'conv_out'), the decoder's 3x3 front conv
    # layerwise only where nl != 2
    assert fwd["conv_in"] == 0 and fwd["conv_out"] == 1, fwd
    assert fwd["conv_igemm"] == c.enc_igemm + (0 if c.nl == 2 else 1), fwd
    assert fwd["res_layer"] == c.fwd_res, fwd
    if c.vq_fused:
        assert fwd["vq_main"] == 0, fwd
        dbg = _launches(lambda: m._forward_c(xd, want_idx=True, parts=1, fwd_flags=F.FWD_DEBUG_ZE))
        assert (dbg["vq_main"], dbg["res_layer"], dbg["conv_igemm"]) == (0, 2, 1), dbg
    else:
        assert fwd["vq_main"] >= 1, fwd


# ---- the padded hidden tile really carries the real channels ---------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("name", ["rh1_k256_d64", "rh20_k1024_d64", "rh31_k100_d64"])
def test_last_real_hidden_channel_is_neither_dropped_nor_duplicated(name):
    """Hidden channel Rh - 1 (its row of the 3x3 conv, its column of the 1x1 conv, both stacks) times 1 + 2^-6 on the device copy and
    in the oracle's state dict: encoder and decoder entries still meet the changed oracle at the tolerances of checks 1 and 2, and
    differ from the unchanged model's (the decoders on the SAME z_q) by more than them -- the tolerances see ONE channel, so a last
    channel that the packing dropped, or copied into the padding, could not pass.  2^-6 is a perturbation far above the tolerances,
    not a tolerance: the oracle itself moves by 2098 / 504 / 390 tolerances in z_e and 90 / 5.5 / 8.0 in x_hat on the three rows, and
    two runs that each sit within one tolerance of their oracle differ by at least that minus two.  The "data" codebook: with the
    constructor's (z_q ~ 1e-3) hidden channel 19 of rh20's decoder stays behind its ReLU and the oracle's x_hat does not move."""
    codebook = "data"
    c = fw.CASES[name]
    r = fw.reference(name, codebook)
    m0 = _device_model(name, codebook)
    z_e0 = _encoder_entry(m0, r["x"])
    sd = fw.state(name, codebook)
    m = fw.model(name)
    m.load_state_dict(sd, strict=True)
    m = m.to(dev())
    _encoder_entry(m, r["x"])                                                # (the packed images of the UNCHANGED weights exist now)
    params = dict(m.named_parameters(remove_duplicate=False))
    with torch.no_grad():                                                    # through .data: neither data_ptr nor _version changes
        fw.scale_last_hidden_channel({k: params[k].data for k in (fw.E5 + "1.weight", fw.E5 + "3.weight", fw.D1 + "1.weight", fw.D1 + "3.weight")}, c.Rh)
    m.invalidate_caches()
    fw.scale_last_hidden_channel(sd, c.Rh)
    ref = fw.oracle(sd, r["x"], c.nl)
    z_e = _encoder_entry(m, r["x"])
    x_hat = _decoder_entry(m, _rows(ref["z_q"])).cpu()
    x_hat0 = _decoder_entry(m0, _rows(ref["z_q"])).cpu()
    _report(f"{name}-{codebook} changed channel z_e", z_e.numpy(), ref["z_e"].numpy(), 2e-6, 0)
    _report(f"{name}-{codebook} changed channel decoder x_hat", x_hat.numpy(), ref["x_hat"].numpy(), 1e-5, 1e-4)
    moved_e = float((z_e - z_e0).abs().max() / 2e-6)
    moved_d = float(((x_hat - x_hat0).abs() / (1e-5 + 1e-4 * x_hat0.abs())).max())
    print(f"widths: {name}-{codebook} one channel times 1 + 2^-6 moves z_e by {moved_e:.1f} and x_hat by {moved_d:.1f} tolerances")
    assert moved_e > 1.0 and moved_d > 1.0


# ---- per-image magnitudes through the padded and the mixed plans ------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("name", ["rh20_k1024_d64", "rh32_k512_d32", "rh32_k512_d256"])
def test_per_image_magnitudes_through_padded_and_mixed_plans(name):
    """test_whole_path_per_image_scales_on_generic_maps' construction (no encoder biases: the encoder is positively homogeneous in x;
    seven images whose magnitudes span ten decades, one all zero) through the fused encoder at a padded hidden tile, at D = 32 and
    on the mixed plan of D = 256, where the per-image maxima are 0xFF-filled and enc_front8_h2_kernel / the residual pair store theirs
    plainly next to the layerwise kernels' atomic maxima.  Every image against the oracle at its own magnitude."""
    from vqvae_amd import _lib, conv
    conv.set_conv_backend("hip")
    c = fw.CASES[name]
    m = fw.model(name)
    with torch.no_grad():
        for p in m.encoder.parameters():
            if p.dim() == 1:
                p.zero_()
        m.pre_quantization_conv.bias.zero_()
    B = 7
    mags = torch.tensor([1.0, 1.0e-5, 3.0e3, 0.0, 2.0e-2, 4.0e4, 7.0]).view(-1, 1, 1, 1)
    x = torch.randn(B, 3, 32, 32, generator=torch.Generator().manual_seed(3)) * mags
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    from oracle import torch_port
    with torch.no_grad():
        z_e_ref = torch_port.encode(sd, x.clone(), c.nl)
    md = m.to(dev())
    L = _lib.load()
    cw, _keep = md._c_weights()
    nws = L.vqvae_workspace_bytes(cw.dims, B, 32, 32)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev())
    xd = x.to(dev()).contiguous()
    z_e = torch.empty(B, 8, 8, c.D, device=dev())
    _lib.check(L.vqvae_encoder_f32(cw, xd.data_ptr(), B, 32, 32, z_e.data_ptr(), ws.data_ptr(), nws, torch.cuda.current_stream().cuda_stream))
    got = z_e.permute(0, 3, 1, 2).cpu().numpy()
    for i in range(B):
        ref = z_e_ref[i].numpy()
        if i != 3:
            _report(f"{name} image {i} (x {float(mags[i]):g})", got[i], ref, 2e-5 * np.abs(ref).max(), 1e-4)
    assert np.all(z_e_ref[3].numpy() == 0.0) and np.all(got[3] == 0.0)
