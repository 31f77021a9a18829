"""Case tables and shared helpers of the GatedPixelCNN envelope tests (tests/test_pixelcnn_envelope_{cpu,gpu}.py)  --  TEST
INFRASTRUCTURE ONLY; nothing under vqvae_amd/ imports it.

The tables name the shapes at which the prior's kernels change form: the batch decides between the four-wave and the eight-wave
("wide") tile-8 conv kernel and how many images a weight-gradient split sums; the channel counts decide between the tile-8 and the
generic conv kernels and between the map-resident and the per-tap weight-gradient kernels.  The forward planner mirrors below
restate the host code's arithmetic (csrc/conv.hip conv_forward_impl, csrc/conv_host.h conv_route) in plain Python; the training
reductions are asked of the library itself (vqvae_train_reduction_plan: the plan the entry point launches from).  So the CPU test can
say which case reaches which branch: if a planner is retuned, that test names the case that lost its purpose.

The ReLU-decision rule.  The head's ReLU sits on B H W 512 pre-activations; a few of them lie within rounding of zero, two correct
implementations decide them differently, and one such decision moves a gradient summed over all pixels by more than the house
tolerance.  So the fp64 restatement takes the decisions of the implementation under test (`head_mask`,
tests/pixelcnn_train_ref.py), and `check_hidden` makes sure the mask cannot hide a wrong forward: the implementation's hidden
activation must equal the reference's `pre * mask` at the conv tolerance, and every decision that differs from the reference's own
`pre > 0` must sit at |pre| <= 1e-5 max|pre|."""
import torch

from tests import pixelcnn_train_ref as R

HIDDEN = 512                                   # output_conv's hidden width (models.py:111-115)
NUM_CUS = 256                                  # MI355X, unpartitioned

# ---------------------------------------------------------------------------------------------------------------- case tables
# A. whole model: id -> (K, dim, n_layers, n_classes, B, side)
MODEL_CASES = {
    "k512_d64_l15_c10_b32_s8": (512, 64, 15, 10, 32, 8),          # the reference's default run
    "k512_d64_l15_c10_b1024_s8": (512, 64, 15, 10, 1024, 8),      # the bench batch: wide head, 8 - 32 images per wgrad split
    "k512_d64_l2_c10_b2048_s8": (512, 64, 2, 10, 2048, 8),        # wide form in tap-list mode
    "k256_d128_l2_c10_b1024_s8": (256, 128, 2, 10, 1024, 8),      # Cout = 256: wide masked convs, two tile columns
    "k8_d4_l1_c1_b1_s1": (8, 4, 1, 1, 1, 1),                      # every lower bound at once
    "k4_d8_l3_c2_b64_s2": (4, 8, 3, 2, 64, 2),                    # maps smaller than any tap window
    "k12_d20_l2_c3_b5_s7": (12, 20, 2, 3, 5, 7),                  # dim % 32 != 0, K < 64, odd side
    "k100_d96_l3_c4_b3_s8": (100, 96, 3, 4, 3, 8),                # tile counts 3 / 6, ragged head tile, half wgrad tile
    "k100_d96_l3_c4_b3_s9": (100, 96, 3, 4, 3, 9),                # the same widths one pixel past the 8 x 8 kernels
    "k1000_d160_l2_c10_b2_s8": (1000, 160, 2, 10, 2, 8),          # tile count 10, K not a multiple of 32
    "k64_d256_l2_c2_b2_s8": (64, 256, 2, 2, 2, 8),                # widest dim
    "k256_d64_l15_c10_b4_s28": (256, 64, 15, 10, 4, 28),          # MNIST-sized maps: per-tap wgrad over many blocks
    "k256_d32_l4_c10_b2_s32": (256, 32, 4, 10, 2, 32),            # 32 x 32, dim = 32
}

# C. cached sampler: id -> (K, dim, n_layers, n_classes, B, side, sigma of output_conv.2.bias or None for the usual 0.05)
SAMPLE_CASES = {
    "k2_d8_l2_c2_b8_s8": (2, 8, 2, 2, 8, 8, None),
    "k3_d4_l1_c1_b8_s8": (3, 4, 1, 1, 8, 8, None),
    "k513_d32_l2_c3_b4_s8": (513, 32, 2, 3, 4, 8, 2.0),
    "k8192_d64_l2_c10_b4_s8": (8192, 64, 2, 10, 4, 8, 6.0),
    "k64_d256_l2_c2_b2_s8": (64, 256, 2, 2, 2, 8, None),
    "k16_d20_l3_c4_b2_s16": (16, 20, 3, 4, 2, 16, None),
    "k8_d8_l2_c2_b1_s128": (8, 8, 2, 2, 1, 128, None),
    "k8_d8_l2_c2_b3_s1": (8, 8, 2, 2, 3, 1, None),
}
SAMPLE_BATCH_CASE = (512, 64, 15, 10, 1024, 8, 2.0)               # compared on 32 images; all 1024 against batches of 1 and 37

T6 = [(ky - 1, kx - 1) for ky in range(2) for kx in range(3)]     # a mask-'B' vertical stack
T2 = [(0, kx - 1) for kx in range(2)]                             # a mask-'B' horizontal stack
T28 = [(ky - 3, kx - 3) for ky in range(4) for kx in range(7)]    # layer 0's vertical stack: two slices of 14 taps
TAPS = {"t6": T6, "t2": T2, "t28": T28}

# B. tap-list forward and data gradient: (B, side, Cin, Cout, taps)
TAPS_FORWARD_CASES = [(2048, 8, 64, 128, "t6"), (2048, 8, 64, 128, "t2"), (2048, 8, 64, 128, "t28"), (2041, 8, 64, 128, "t6"),
                      (2049, 8, 64, 128, "t6"), (2048, 8, 128, 256, "t2")]
# plain 1 x 1: (B, Cin, Cout) on 8 x 8
CONV1X1_CASES = [(1024, 64, 512), (1024, 512, 512), (505, 64, 512), (505, 512, 512)]
# map-resident weight gradient: (B, H, W, Cin, Cout, taps, images per split, splits)
WGRAD_MAP_CASES = [(1024, 8, 8, 64, 128, "t6", 8, 128), (1024, 8, 8, 64, 128, "t2", 8, 128), (1024, 8, 8, 64, 128, "t28", 32, 32),
                   (1000, 8, 8, 64, 128, "t6", 8, 125), (1000, 8, 8, 64, 128, "t2", 8, 125), (1000, 8, 8, 64, 128, "t28", 32, 32),
                   (300, 8, 8, 96, 192, "t6", 7, 43), (257, 7, 5, 32, 64, "t6", 2, 129)]
WGRAD_PATTERN_CASE = (1024, 8, 8, 64, 128, "t6")
WGRAD_PATTERNS = ["spike", "zero-middle", "falling"]
# per-tap weight gradient: (B, H, W, Cin, Cout, taps, pixel blocks, splits)
WGRAD_BLK_CASES = [(32, 28, 28, 64, 128, "t6", 784, 61), (7, 9, 9, 20, 40, "t6", 18, 3), (1, 1, 1, 4, 8, "t28", 1, 1)]
# embedding backward: (n, rows, C)
GATHER_CASES = [(65536, 512, 64), (65536, 512, 128), (65536, 512, 40), (65536, 512, 512), (1024, 1, 128), (1024, 10, 128)]
# column sums: (P, C)
BIAS_CASES = [(65536, 128), (65536, 40), (65536, 512), (4096, 8192)]
# gate backward: (B, HW, dim)
GATE_CASES = [(1024, 64, 64), (4, 784, 20), (4, 784, 256)]
# cross-entropy: (B, K, side)
CE_CASES = [(1024, 512, 8), (8, 10, 8), (8, 1000, 8), (8, 8192, 8)]


# ------------------------------------------------------------------------------------------------------------ planner mirrors
def cdiv(a, b):
    return -(-a // b)


def ntile(Cout):
    """32-channel output tiles of the conv kernels"""
    return cdiv(Cout, 32)


def conv_is_tile8(side, Cin, Cout):
    """conv_route: stride-1 convs on 8 x 8 maps with Cin % 32 == 0 and an even tile count run conv_tile8_bf3_kernel; every other
    shape of the prior runs the generic kernel"""
    return side == 8 and Cin % 32 == 0 and ntile(Cout) % 2 == 0


def conv_is_wide(B, side, Cin, Cout, cus=NUM_CUS):
    """conv_forward_impl: the eight-wave form, four output tiles per wave, once it gives every CU a workgroup"""
    nt = ntile(Cout)
    return conv_is_tile8(side, Cin, Cout) and nt % 4 == 0 and cdiv(B, 8) * (nt // 4) >= cus


def model_convs(dim, K):
    """(name, Cin, Cout) of every conv of the forward, and of every data-gradient conv of the backward"""
    fwd = [("vert_stack", dim, 2 * dim), ("horiz_stack", dim, 2 * dim), ("vert_to_horiz", 2 * dim, 2 * dim),
           ("horiz_resid", dim, dim), ("output_conv.0", dim, HIDDEN), ("output_conv.2", HIDDEN, K)]
    return fwd + [("d_" + n, co, ci) for n, ci, co in fwd]


def taps_wgrad_plan(B, H, W, Cin, Cout, taps):
    """what vqvae_conv_taps_wgrad_f32 would launch, from the library: .kernel is 'taps_wgrad_map' (items = images: per_split images
    per split, splits, last) or 'taps_wgrad_blk' (items = 32-pixel blocks; want = the split count before the 64-split clamp)"""
    from vqvae_amd import _lib
    return _lib.train_reduction_plan("conv_taps_wgrad", B, H, W, Cin, Cout, len(taps), *[t[0] for t in taps], *[t[1] for t in taps])


def bias_wide_plan(P, C):
    """what vqvae_bias_grad_wide_f32 would launch: want = blocks before the 512-block clamp, per_split = rows per block, splits"""
    from vqvae_amd import _lib
    return _lib.train_reduction_plan("bias_grad_wide", P, C)


def sampler_packed_floats(K, dim, nl, ncls):
    """the sampler image of include/vqvae_hip.h: embedding; per layer the class embedding, vert_stack (read taps only: 21 of layer
    0's 28, all 6 of the others) + bias, vert_to_horiz + bias, horiz_stack (3 of 4, 2 of 2) + bias, horiz_resid + bias; the head"""
    def layer(first):
        tv, th = (21, 3) if first else (6, 2)
        return (ncls * 2 * dim + 2 * dim * tv * dim + 2 * dim + 2 * dim * 2 * dim + 2 * dim + 2 * dim * th * dim + 2 * dim
                + dim * dim + dim)
    return K * dim + layer(True) + (nl - 1) * layer(False) + HIDDEN * dim + HIDDEN + K * HIDDEN + K


def sampler_workspace_floats(B, side, dim, nl):
    """per image: two rows of V per layer, v2h of the current row per layer, two hv rows, Hs(y, x - 1) of layers 0 .. n - 2"""
    return B * (2 * nl * side * dim + nl * side * 2 * dim + 2 * side * 2 * dim + (nl - 1) * dim)


# -------------------------------------------------------------------------------------------------------------------- helpers
def build(K, dim, nl, ncls, head_bias_sigma=None):
    """the model of the existing tests: torch.manual_seed(0), the reference's initialisation, non-trivial biases; on the CPU"""
    from vqvae_amd.pixelcnn import GatedPixelCNN
    torch.manual_seed(0)
    m = GatedPixelCNN(K, dim, nl, ncls)
    R.perturb_biases(m)
    if head_bias_sigma is not None:
        with torch.no_grad():
            m.output_conv[2].bias.copy_(torch.randn(K, generator=torch.Generator().manual_seed(K)) * head_bias_sigma)
    return m


def model_inputs(K, ncls, B, side, seed=None):
    g = torch.Generator().manual_seed(B * 1000 + side if seed is None else seed)
    return torch.randint(0, K, (B, side, side), generator=g), torch.randint(0, ncls, (B,), generator=g)


def device_hidden(model, x, label):
    """GatedPixelCNN._forward_eval's launches up to the head's hidden activation -> (t = relu(output_conv.0(x_h)) (B, H, W, 512),
    logits (B, K, H, W)).  The caller asserts that these logits are model(x, label)'s bits, so this copy cannot drift."""
    from vqvae_amd import conv_hip
    from vqvae_amd.pixelcnn import _gather_rows
    with torch.no_grad():
        model._check(x)
        B, H, W = x.shape
        t = _gather_rows(x, model.embedding.weight).view(B, H, W, model.dim)
        x_v, x_h = t, t
        for layer in model.layers:
            x_v, x_h = layer.forward_rows(x_v, x_h, label)
        c0, c2 = model.output_conv[0], model.output_conv[2]
        t = conv_hip.conv(conv_hip.CONV_1x1, x_h, c0, c0.weight, c0.bias, model.dim, c0.weight.shape[0], conv_hip.RELU_OUT)
        lg = conv_hip.conv(conv_hip.CONV_1x1, t, c2, c2.weight, c2.bias, c0.weight.shape[0], c2.weight.shape[0], 0)
        return t, conv_hip.rows_to_nchw(lg)


def err_ratio(got, ref, absmax=None):
    """max |got - ref| / (1e-5 max|ref| + 1e-4 |ref|): the house tolerance (R.tolerance) as a ratio, 1 at the limit.  A reference
    that is zero everywhere has no scale: there the result must be exactly zero (ratio 0, else inf)."""
    got = torch.as_tensor(got).detach().cpu().double()
    ref = torch.as_tensor(ref).detach().cpu().double()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    amax = float(ref.abs().max()) if absmax is None else float(absmax)
    if amax == 0.0:
        return 0.0 if bool((got == 0).all()) else float("inf")
    return float(((got - ref).abs() / (1e-5 * amax + 1e-4 * ref.abs())).max())


def within(got, ref, what, absmax=None):
    r = err_ratio(got, ref, absmax)
    assert r <= 1.0, f"{what}: max |err| / tolerance = {r:.3g}"
    return r


def check_hidden(t_nchw, pre):
    """The rule that goes with `head_mask`.  t_nchw: the implementation's hidden activation relu(pre') as (B, 512, H, W); pre: the
    reference's pre-activation computed under the mask t > 0.  -> (number of ReLU decisions that differ from the reference's own,
    |err| / tolerance of t against pre * mask)."""
    t_nchw, pre = t_nchw.detach().cpu().double(), pre.detach().cpu().double()
    mask = t_nchw > 0
    amax = float(pre.abs().max())
    ratio = within(t_nchw, pre * mask, "hidden activation", absmax=amax)
    differ = mask != (pre > 0)
    n = int(differ.sum())
    if n:
        worst = float(pre[differ].abs().max())
        assert worst <= 1e-5 * amax, f"{n} ReLU decisions differ, the farthest at |pre| = {worst:.3g} (max|pre| = {amax:.3g})"
    return n, ratio


def shift(xd, dy, dx):
    """out[b, y, x] = xd[b, y + dy, x + dx], zero outside the map; xd (B, H, W, C)"""
    B, H, W, Cc = xd.shape
    sh = torch.zeros_like(xd)
    ys, ye = max(0, -dy), min(H, H - dy)
    xs, xe = max(0, -dx), min(W, W - dx)
    if ys < ye and xs < xe:
        sh[:, ys:ye, xs:xe] = xd[:, ys + dy:ye + dy, xs + dx:xe + dx]
    return sh


def image_factors(pattern, B, ips):
    """per-image factors (f_gy, f_x) of a weight gradient's operands; image j = b % ips of split b // ips"""
    j = torch.arange(B) % ips
    r = torch.arange(B) // ips
    fa, fb = torch.ones(B, dtype=torch.float64), torch.ones(B, dtype=torch.float64)
    if pattern == "spike":                     # one image 10^6 larger than all others, in the middle of a split
        fa[5 * ips + ips // 2] = 1e6
    elif pattern == "zero-middle":             # an all-zero image in the middle of every third split, of either operand
        fa[(r % 3 == 0) & (j == ips // 2)] = 0.0
        fb[(r % 3 == 1) & (j == ips // 2)] = 0.0
    elif pattern == "falling":                 # the products of a split fall over 12 decades
        fa = 10.0 ** (3.0 - 6.0 * j.double() / (ips - 1))
        fb = fa.clone()
    else:
        raise ValueError(pattern)
    return fa.float(), fb.float()
