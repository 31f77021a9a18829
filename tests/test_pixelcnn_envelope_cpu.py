"""CPU side of the GatedPixelCNN envelope tests: the sampler's entry points just outside their documented envelope (fake device
pointers, nothing launched), its buffer sizes against the documented layout, the case tables of tests/pixelcnn_envelope.py against
the planners they are meant to reach, and the ReLU-decision rule of the fp64 restatement (`head_mask`)."""
import ctypes as C

import pytest
import torch

from tests import pixelcnn_envelope as E
from tests import pixelcnn_train_ref as R

NULL, SHAPE, UNSUPPORTED = -1, -2, -3            # VQVAE_ERR_* (include/vqvae_hip.h)


def _sample(L, K=16, dim=8, nl=2, ncls=3, B=2, H=4, W=4):
    a = 256                                      # a 16-byte aligned device pointer that is never dereferenced
    return L.vqvae_pixelcnn_sample_f32(a, 1 << 40, a, a, B, H, W, K, dim, nl, ncls, a, None, a, a, 1 << 40, None)


def _pack(L, K=16, dim=8, nl=2, ncls=3):
    n = 9 * max(nl, 0) + 5
    ptrs = (C.c_void_p * n)(*([256] * n))
    return L.vqvae_pixelcnn_sample_pack_f32(ptrs, n, K, dim, nl, ncls, 256, 1 << 40, None)


def test_sampler_refuses_shapes_just_outside_its_envelope():
    """dim % 4, dim > 256, K < 2, K > 8192, side > 128, H != W -> VQVAE_ERR_UNSUPPORTED; no layers / classes -> VQVAE_ERR_SHAPE;
    the size queries answer 0 for each"""
    from vqvae_amd import _lib
    L = _lib.load()
    for kw in (dict(dim=6), dict(dim=260), dict(K=1), dict(K=8193)):
        assert _sample(L, **kw) == UNSUPPORTED, kw
        assert _pack(L, **kw) == UNSUPPORTED, kw
        args = dict(K=16, dim=8, nl=2, ncls=3)
        args.update(kw)
        assert L.vqvae_pixelcnn_sample_packed_bytes(args["K"], args["dim"], args["nl"], args["ncls"]) == 0, kw
    for dim in (6, 260):
        assert L.vqvae_pixelcnn_sample_workspace_bytes(2, 4, 4, dim, 2) == 0
    assert _sample(L, H=129, W=129) == UNSUPPORTED
    assert L.vqvae_pixelcnn_sample_workspace_bytes(2, 129, 129, 8, 2) == 0
    assert _sample(L, H=4, W=6) == UNSUPPORTED
    assert L.vqvae_pixelcnn_sample_workspace_bytes(2, 4, 6, 8, 2) == 0
    for kw in (dict(nl=0), dict(ncls=0)):
        assert _sample(L, **kw) == SHAPE, kw
        assert _pack(L, **kw) == SHAPE, kw
        args = dict(K=16, dim=8, nl=2, ncls=3)
        args.update(kw)
        assert L.vqvae_pixelcnn_sample_packed_bytes(args["K"], args["dim"], args["nl"], args["ncls"]) == 0, kw
    assert L.vqvae_pixelcnn_sample_workspace_bytes(2, 4, 4, 8, 0) == 0
    assert L.vqvae_pixelcnn_sample_workspace_bytes(0, 4, 4, 8, 2) == 0
    # the corners themselves are inside: sizes are non-zero there
    for K, dim, nl, ncls in ((2, 4, 1, 1), (8192, 256, 1, 1)):
        assert L.vqvae_pixelcnn_sample_packed_bytes(K, dim, nl, ncls) > 0
    assert L.vqvae_pixelcnn_sample_workspace_bytes(1, 1, 1, 4, 1) > 0
    assert L.vqvae_pixelcnn_sample_workspace_bytes(1, 128, 128, 256, 1) > 0
    assert _sample(L, H=0, W=0) == SHAPE
    assert L.vqvae_pixelcnn_sample_f32(None, 1 << 40, 256, 256, 2, 4, 4, 16, 8, 2, 3, 256, None, 256, 256, 1 << 40, None) == NULL


@pytest.mark.parametrize("K,dim,nl,ncls,B,side", [(512, 64, 15, 10, 1024, 8), (3, 4, 1, 1, 8, 8), (8192, 256, 2, 2, 3, 128)])
def test_sampler_buffer_sizes_are_the_documented_layout(K, dim, nl, ncls, B, side):
    """a change of the layout cannot silently shrink the packed image or the workspace"""
    from vqvae_amd import _lib
    L = _lib.load()
    assert L.vqvae_pixelcnn_sample_packed_bytes(K, dim, nl, ncls) == 4 * E.sampler_packed_floats(K, dim, nl, ncls)
    assert L.vqvae_pixelcnn_sample_workspace_bytes(B, side, side, dim, nl) == 4 * E.sampler_workspace_floats(B, side, dim, nl)


def test_sampler_packed_floats_counts_a_real_model():
    """the layout sum against the parameters of a built model: every element but the taps mask 'A' zeroes and the rows of
    layer 0's stacks that are never read"""
    K, dim, nl, ncls = 12, 20, 3, 4
    m = E.build(K, dim, nl, ncls)
    total = sum(p.numel() for p in m.parameters())
    unread = 2 * dim * dim * 7 + 2 * dim * dim * 1           # layer 0: the vertical stack's last row, the horizontal's last column
    assert E.sampler_packed_floats(K, dim, nl, ncls) == total - unread


# ------------------------------------------------------------------------------------------- the tables reach their branches
def _wide_layers(case):
    K, dim, nl, ncls, B, side = E.MODEL_CASES[case]
    return {n for n, ci, co in E.model_convs(dim, K) if E.conv_is_wide(B, side, ci, co)}


def _tile8_layers(case):
    K, dim, nl, ncls, B, side = E.MODEL_CASES[case]
    return {n for n, ci, co in E.model_convs(dim, K) if E.conv_is_tile8(side, ci, co)}


def test_wide_form_thresholds():
    """the batches the tables are built around: the 512-wide head from B = 505, Cout = 128 from B = 2041, Cout = 256 from 1017"""
    assert not E.conv_is_wide(504, 8, 64, 512) and E.conv_is_wide(505, 8, 64, 512)
    assert not E.conv_is_wide(504, 8, 512, 512) and E.conv_is_wide(505, 8, 512, 512)
    assert not E.conv_is_wide(2040, 8, 64, 128) and E.conv_is_wide(2041, 8, 64, 128)
    assert not E.conv_is_wide(1016, 8, 128, 256) and E.conv_is_wide(1017, 8, 128, 256)
    assert not E.conv_is_wide(1 << 20, 8, 64, 64)            # two tiles: never the wide form
    assert not E.conv_is_wide(1 << 20, 9, 64, 128)


def test_model_cases_reach_the_conv_forms_they_name():
    head = {"output_conv.0", "output_conv.2", "d_output_conv.2"}
    assert _wide_layers("k512_d64_l15_c10_b32_s8") == set()
    assert _wide_layers("k512_d64_l15_c10_b1024_s8") == head
    masked = {"vert_stack", "horiz_stack", "vert_to_horiz", "d_vert_to_horiz"}
    assert _wide_layers("k512_d64_l2_c10_b2048_s8") == head | masked
    # dim = 128: Cout = 256 masked convs, two tile columns per image in the wide form; Cout = 128 (horiz_resid, the tap data
    # gradients) stays four-wave below B = 2041
    w = _wide_layers("k256_d128_l2_c10_b1024_s8")
    assert masked <= w and "horiz_resid" not in w and "d_vert_stack" not in w
    # channel counts: dim % 32 != 0 on a 7 x 7 map -> the generic kernel everywhere; dim = 96 -> odd tile counts 3 (horiz_resid,
    # the tap data gradients) go generic, 6 stays tile-8; dim = 160 -> tile count 10 (even, not a multiple of 4)
    assert _tile8_layers("k12_d20_l2_c3_b5_s7") == set()
    t = _tile8_layers("k100_d96_l3_c4_b3_s8")
    assert {"vert_stack", "horiz_stack", "vert_to_horiz", "output_conv.0", "output_conv.2"} <= t
    assert "horiz_resid" not in t and "d_vert_stack" not in t and E.ntile(96) == 3 and E.ntile(192) == 6
    assert E.ntile(100) == 4 and 100 % 32 != 0                                   # ragged last head tile
    assert _tile8_layers("k100_d96_l3_c4_b3_s9") == set()
    assert E.ntile(2 * 160) == 10 and "vert_stack" in _tile8_layers("k1000_d160_l2_c10_b2_s8") and 1000 % 32 != 0
    assert "horiz_resid" not in _tile8_layers("k256_d32_l4_c10_b2_s32") and E.ntile(32) == 1
    for case in ("k256_d64_l15_c10_b4_s28", "k256_d32_l4_c10_b2_s32", "k4_d8_l3_c2_b64_s2", "k8_d4_l1_c1_b1_s1"):
        assert _tile8_layers(case) == set(), case


def test_model_cases_reach_the_weight_gradient_kernels_they_name():
    def plans(case):
        K, dim, nl, ncls, B, side = E.MODEL_CASES[case]
        out = {}
        for name, taps in (("v0", E.T28), ("h0", [(0, kx - 3) for kx in range(4)]), ("v", E.T6), ("h", E.T2)):
            out[name] = E.taps_wgrad_plan(B, side, side, dim, 2 * dim, taps)
        return out

    def form(q):                                             # (kernel, images per split)
        return {"taps_wgrad_map": "map", "taps_wgrad_blk": "blk"}[q.kernel], q.per_split
    p = plans("k512_d64_l15_c10_b1024_s8")
    assert [form(p[k]) for k in ("v0", "h0", "v", "h")] == [("map", 32), ("map", 8), ("map", 8), ("map", 8)]
    p = plans("k512_d64_l15_c10_b32_s8")
    assert all(form(v) == ("map", 1) for v in p.values())
    p = plans("k512_d64_l2_c10_b2048_s8")
    assert [form(p[k]) for k in ("v0", "v")] == [("map", 64), ("map", 16)]
    p = plans("k256_d128_l2_c10_b1024_s8")
    assert form(p["v"]) == ("map", 32) and form(p["v0"]) == ("map", 128)    # 8 tiles: 32 splits; 32 tiles: 8 splits
    p = plans("k100_d96_l3_c4_b3_s8")                        # 96 = one and a half 64-wide tiles
    assert form(p["v"])[0] == "map" and 96 % 64 == 32
    for case in ("k100_d96_l3_c4_b3_s9", "k12_d20_l2_c3_b5_s7", "k8_d4_l1_c1_b1_s1", "k4_d8_l3_c2_b64_s2",
                 "k256_d64_l15_c10_b4_s28", "k256_d32_l4_c10_b2_s32"):
        assert all(form(v)[0] == "blk" for v in plans(case).values()), case
    p = plans("k256_d64_l15_c10_b4_s28")                     # 98 blocks, 12 splits of 9 blocks
    assert p["v"].items == 98 and p["v"].splits > 8


def test_kernel_cases_reach_the_branches_they_name():
    for B, side, Cin, Cout, taps in E.TAPS_FORWARD_CASES:
        assert E.conv_is_wide(B, side, Cin, Cout), (B, Cin, Cout)
    assert E.conv_is_wide(2048, 8, 256, 128)                 # the data gradient of the (128 -> 256) case
    assert not E.conv_is_wide(2048, 8, 128, 64)              # ... while 128 -> 64 has two tiles: four-wave form
    assert 2049 % 8 == 1 and 2041 % 8 == 1                   # a last workgroup with one image of eight
    for B, Cin, Cout in E.CONV1X1_CASES:
        assert E.conv_is_wide(B, 8, Cin, Cout) and not E.conv_is_wide(504, 8, Cin, Cout)
    for B, H, W, Cin, Cout, taps, ips, ns in E.WGRAD_MAP_CASES:
        got = E.taps_wgrad_plan(B, H, W, Cin, Cout, E.TAPS[taps])
        assert got.kernel == "taps_wgrad_map", (B, H, W)
        assert (got.per_split, got.splits) == (ips, ns), (B, H, W, taps)
    got = E.taps_wgrad_plan(257, 7, 5, 32, 64, E.T6)
    assert (got.per_split, got.splits, got.last) == (2, 129, 1)   # the last split holds one image
    got = E.taps_wgrad_plan(1000, 8, 8, 64, 128, E.T28)
    assert (got.per_split, got.splits, got.last) == (32, 32, 8)
    B, H, W, Cin, Cout, taps = E.WGRAD_PATTERN_CASE
    got = E.taps_wgrad_plan(B, H, W, Cin, Cout, E.TAPS[taps])
    assert got.kernel == "taps_wgrad_map" and len(E.TAPS[taps]) == 6 and got.per_split == 8
    for B, H, W, Cin, Cout, taps, nblk, ns in E.WGRAD_BLK_CASES:
        got = E.taps_wgrad_plan(B, H, W, Cin, Cout, E.TAPS[taps])
        assert got.kernel == "taps_wgrad_blk", (B, H, W)
        assert (got.items, got.splits) == (nblk, ns), (B, H, W, got)
    got = E.taps_wgrad_plan(32, 28, 28, 64, 128, E.T6)
    assert got.want > 64 and got.splits <= 64                # the 64-split clamp acts
    assert 7 * 81 % 32 != 0                                   # the last pixel block is partly filled
    assert [E.bias_wide_plan(P, C).want > 512 for P, C in E.BIAS_CASES] == [True, True, True, False]
    bp = [E.bias_wide_plan(P, 128) for P in (65536, 4096)]
    assert [(q.want, q.per_split, q.splits) for q in bp] == [(1024, 128, 512), (64, 64, 64)]
    assert any(C > 256 for _, C in E.BIAS_CASES) and any(C <= 256 and 256 % C for _, C in E.BIAS_CASES)


def test_case_tables_lie_inside_the_documented_envelope():
    for K, dim, nl, ncls, B, side in E.MODEL_CASES.values():
        assert dim % 4 == 0 and K % 4 == 0 and K >= 1 and nl >= 1 and ncls >= 1 and B >= 1 and side >= 1
    for K, dim, nl, ncls, B, side, _ in list(E.SAMPLE_CASES.values()) + [E.SAMPLE_BATCH_CASE]:
        assert dim % 4 == 0 and dim <= 256 and 2 <= K <= 8192 and nl >= 1 and ncls >= 1 and 1 <= side <= 128


# ----------------------------------------------------------------------------------------------------- the ReLU-decision rule
def test_head_mask_makes_fp32_and_fp64_restatements_agree():
    """(512, 64, 2 layers, 10) at B = 64 on 8 x 8 with the fp32 restatement as the implementation: under its ReLU decisions the
    fp64 gradients agree with it within the house tolerance, the hidden activation passes `check_hidden`, and `head_mask=None`
    is the plain ReLU"""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    K, dim, nl, ncls, B, side = 512, 64, 2, 10, 64, 8
    m = E.build(K, dim, nl, ncls)
    state = {k: v.detach().clone() for k, v in m.named_parameters()}
    x, label = E.model_inputs(K, ncls, B, side)
    k32 = {}
    l32, gl32, g32 = R.loss_and_grads(state, x, label, nl, dtype=torch.float32, keep=k32)
    t32 = torch.relu(k32["pre"])
    mask = (t32 > 0)
    k64 = {}
    l64, gl64, g64 = R.loss_and_grads(state, x, label, nl, head_mask=mask, keep=k64)
    n, ratio = E.check_hidden(t32, k64["pre"])
    assert abs(float(l32) - float(l64)) <= 1e-5 * abs(float(l64))
    worst = max([E.within(gl32, gl64, "grad_logits")] + [E.within(g32[k], g64[k], k) for k in g64])
    print(f"B=64: {n} ReLU decisions differ, hidden {ratio:.3g}, worst gradient {worst:.3g} of the tolerance")
    # an all-ones mask is no ReLU at all: the argument is really used
    l_lin, _, _ = R.loss_and_grads(state, x, label, nl, head_mask=torch.ones_like(mask))
    assert abs(float(l_lin) - float(l64)) > 1e-3 * abs(float(l64))
    # the mask of the run's own decisions is the plain ReLU, bit for bit
    k_own = {}
    l_plain, gl_plain, g_plain = R.loss_and_grads(state, x, label, nl, keep=k_own)
    l_own, gl_own, g_own = R.loss_and_grads(state, x, label, nl, head_mask=(k_own["pre"] > 0))
    assert float(l_plain) == float(l_own) and torch.equal(gl_plain, gl_own)
    assert all(torch.equal(g_plain[k], g_own[k]) for k in g_plain)


def test_err_ratio_of_an_all_zero_reference_asks_for_exact_zeros():
    z = torch.zeros(4, 3)
    assert E.err_ratio(z, z) == 0.0
    assert E.err_ratio(z + 1e-30, z) == float("inf")
    assert E.err_ratio(torch.full((2,), float("nan")), torch.ones(2)) == float("inf")
    assert E.err_ratio(torch.tensor([1.0, 2.0]), torch.tensor([1.0, 2.0 + 2.2e-4])) == pytest.approx(1.0, rel=0.02)
    # side 1: layer 0's only in-map taps are the ones mask 'A' zeroes, so the embedding gets exactly no gradient
    K, dim, nl, ncls, B, side = E.MODEL_CASES["k8_d4_l1_c1_b1_s1"]
    m = E.build(K, dim, nl, ncls)
    x, label = E.model_inputs(K, ncls, B, side)
    _, _, g = R.loss_and_grads({k: v.detach().clone() for k, v in m.named_parameters()}, x, label, nl)
    assert float(g["embedding.weight"].abs().max()) == 0.0
    assert float(g["layers.0.vert_stack.weight"][:, :, -1].abs().max()) > 0
    assert float(g["layers.0.horiz_stack.weight"][:, :, :, -1].abs().max()) > 0
