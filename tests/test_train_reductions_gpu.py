"""The training step's reductions at the batch it is measured at (B = 4096 in bench.py): every split that depends on the batch size,
driven to many images (rows, pixels) per workgroup, against a plain fp64 restatement of the same sum on the CPU.

  weight gradients   per tap A_tap^T @ Bt_tap in fp64; _close_grad of tests/test_training_gpu.py and the per-slice limit of
                     test_full_model_backward_on_hip_matches_cpu_reference; the scale patterns of the two-term kernel within 2e-5 of
                     each (ca, cb) filter's own maximum (as test_two_term_weight_gradient_across_image_scales states the header's bound)
  bias gradients     fp64 column sums; 1 ulp of the rounded value
  codebook gradient  index_add_ in fp64; 1 ulp of the rounded value + 2^-45 scale (cnt |e_k| + sum |z|) for cancellation
  EMA update         tests/vq_ema_ref.py; the _ulps limits of tests/test_vq_ema_gpu.py

Each case asks the library what it would launch (vqvae_train_reduction_plan: the plan functions the entry points themselves launch
from) and asserts the split it is there to reach, so that a change of the plan cannot quietly turn it back into one image per range.
Every reduction is also required to give the same bits on a second call."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from tests import vq_ema_ref as R
from tests.test_training_gpu import _close_grad
from tests.test_vq_ema_gpu import _layout, _ulps, _update

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BENCH_B = 4096            # bench.py / tools/ema_step_bench.py, config 3


def _cdiv(a, b):
    return -(-a // b)


# ---- the library's own split plans -----------------------------------------------------------------------------------------------

def _plan(what, *dims):
    from vqvae_amd import _lib
    p = _lib.train_reduction_plan(what, *dims)
    assert p is not None, (what, dims)
    return p


def map8_plan(B, k, CA, CB, exact=False):
    """vqvae_conv_wgrad_ex_f32 on 8x8 A maps: splits = image ranges, per_split = images per range of the map-resident kernels"""
    s = 2 if k == 4 else 1
    p = _plan("conv_wgrad", B, 8, 8, CA, 8 * s, 8 * s, CB, k, s, 0 if k == 1 else 1, 0, 0x4 if exact else 0)
    assert p.kernel == ("conv_wgrad_map8_h2" if k >= 3 and not exact else "conv_wgrad_map8"), p
    return p


def img_plan(B, CA, CB):
    """the image-operand branch (4x4 stride 2 on 32x32 NCHW images): workgroups and images per workgroup of conv_wgrad_img_kernel"""
    p = _plan("conv_wgrad", B, 16, 16, CA, 32, 32, CB, 4, 2, 1, 1, 0)
    assert p.kernel == "conv_wgrad_img", p
    return p


def generic_plan(B, HA, WA, CA, CB, k):
    """conv_wgrad_kernel on stride-1 maps of the current device: splits, 32-pixel blocks per split and in the last split"""
    p = _plan("conv_wgrad", B, HA, WA, CA, HA, WA, CB, k, 1, 1 if k == 3 else 0, 0, 0)
    assert p.kernel == "conv_wgrad", p
    return p


def bias_plan(P, C):
    """vqvae_bias_grad_f32: blocks, rows per block and rows of the last block of bias_grad_partial_kernel"""
    return _plan("bias_grad", P, C)


def bwd_units(idx, K, D):
    """a code owns ceil(count / chunk) units of its sorted rows; the chunk is the segmented sum's own"""
    chunk = _plan("segsum", idx.numel(), K, D).aux0
    return (torch.bincount(idx.reshape(-1).cpu(), minlength=K) + chunk - 1) // chunk, chunk


# ---- fp64 restatement of the weight gradient ----------------------------------------------------------------------------------

def _wgrad_ref(a, bt, k, s, pad, bt_nchw=False, chunk=256):
    """dW[ca, cb, ky, kx] = sum over (b, y, x) of a[b, y, x, ca] bt[b, y s + ky - pad, x s + kx - pad, cb]: per tap A_tap^T @ Bt_tap in
    fp64, a chunk of images at a time (a (B, HA, WA, CA) row-major; bt (B, HB, WB, CB), or (B, CB, HB, WB) with bt_nchw)"""
    B, HA, WA, CA = a.shape
    CB = bt.shape[1] if bt_nchw else bt.shape[3]
    out = torch.zeros(CA, CB, k, k, dtype=torch.float64)
    for b0 in range(0, B, chunk):
        ad = a[b0:b0 + chunk].double().reshape(-1, CA)
        bd = bt[b0:b0 + chunk].double()
        if bt_nchw:
            bd = bd.permute(0, 2, 3, 1)
        bd = TF.pad(bd, (0, 0, pad, pad, pad, pad))
        for ky in range(k):
            for kx in range(k):
                tap = bd[:, ky:ky + s * (HA - 1) + 1:s, kx:kx + s * (WA - 1) + 1:s, :]
                out[:, :, ky, kx] += ad.T @ tap.reshape(-1, CB)
    return out


def _per_slice(got, ref):
    """test_full_model_backward_on_hip_matches_cpu_reference's per-slice statement: worst error / limit"""
    err = (got.cpu().double() - ref).abs()
    m0 = ref.abs().amax(dim=(1, 2, 3), keepdim=True)
    m1 = ref.abs().amax(dim=(0, 2, 3), keepdim=True)
    lim = 2e-4 * ref.abs() + 2e-5 * torch.maximum(m0, m1) + 1e-30
    return float((err / lim).max())


def _wgrad(a, bt, k, s, pad, exact, bt_nchw=False):
    from vqvae_amd import autograd_conv as A
    old = A.WGRAD_EXACT_FP32
    A.WGRAD_EXACT_FP32 = exact
    try:
        got = A.conv_wgrad(a, bt, k, s, pad, bt_nchw=bt_nchw)
        again = A.conv_wgrad(a, bt, k, s, pad, bt_nchw=bt_nchw)
    finally:
        A.WGRAD_EXACT_FP32 = old
    assert torch.equal(got, again), "fixed-order sums: the second call must give the same bits"
    return got


# (k, s, CA, CB) of the default model's 8x8-map layers: A = the layer's output gradient or input, Bt = the other one
MAP8_SHAPES = [(3, 1, 128, 128), (4, 2, 128, 64), (3, 1, 64, 128), (1, 1, 64, 128), (3, 1, 32, 128), (1, 1, 128, 32)]


@pytest.mark.parametrize("k,s,CA,CB", MAP8_SHAPES, ids=lambda v: str(v))
def test_map8_weight_gradient_at_the_bench_batch(k, s, CA, CB):
    """conv_wgrad_map8_h2_kernel (fp16x2, k >= 3) and conv_wgrad_map8_kernel (fp32) with 8, 16 or 32 images per range"""
    for exact in (False, True):
        plan = map8_plan(BENCH_B, k, CA, CB, exact)
        assert plan.per_split >= 8 and plan.splits * plan.per_split == BENCH_B, plan
    pad = 0 if k == 1 else 1
    g = torch.Generator().manual_seed(k * 1000 + CA + CB)
    a = torch.randn(BENCH_B, 8, 8, CA, generator=g)
    bt = torch.randn(BENCH_B, 8 * s, 8 * s, CB, generator=g)
    ref = _wgrad_ref(a, bt, k, s, pad)
    ad, bd = a.to(DEV), bt.to(DEV)
    del a, bt
    for exact in (False, True):
        got = _wgrad(ad, bd, k, s, pad, exact)
        what = f"grad_w {'fp32' if exact else 'fp16x2'} ips={plan.per_split}"
        _close_grad(got, ref.float(), what)
        worst = _per_slice(got, ref)
        assert worst <= 1.0, (what, worst)


# ---- magnitudes inside the image ranges of the two-term kernel (conv_wgrad_map8_h2_kernel: k >= 3, the default arithmetic) ------

def _factors(pattern, B, ips, g):
    """per-image factors (fa, fb) of the A and Bt operands; image j of a range is b % ips (ranges are consecutive images)"""
    j = torch.arange(B) % ips
    r = torch.arange(B) // ips
    fa = torch.ones(B, dtype=torch.float64)
    fb = torch.ones(B, dtype=torch.float64)
    if pattern == "small-first":             # the accumulators follow upwards
        fa[j == 0], fb[j == 0] = 1e-6, 1e-6
    elif pattern == "falling":               # each range falls over 52 decades of products: the 2^60 clamp holds the accumulators
        step = 26.0 / (ips - 1)
        fa = 10.0 ** (6.0 - step * j.double())
        fb = fa.clone()
    elif pattern == "spread":                # 10^+-6 per image and operand
        fa = 10.0 ** (torch.rand(B, generator=g, dtype=torch.float64) * 12 - 6)
        fb = 10.0 ** (torch.rand(B, generator=g, dtype=torch.float64) * 12 - 6)
    elif pattern == "zero-tiles":            # all-zero A / Bt tiles, first and in the middle, among images 10^+-3 apart
        fa = 10.0 ** (torch.rand(B, generator=g, dtype=torch.float64) * 6 - 3)
        fb = 10.0 ** (torch.rand(B, generator=g, dtype=torch.float64) * 6 - 3)
        fa[(r % 4 == 0) & (j == 0)] = 0.0
        fb[(r % 4 == 1) & (j == 0)] = 0.0
        fa[(r % 4 == 2) & (j == ips // 2)] = 0.0
        fb[(r % 4 == 3) & (j == ips // 2)] = 0.0
    elif pattern == "zero-among-tiny":       # a zero A tile (its Bt large) between images near 1e-15: the sums before it stay
        fa[:], fb[:] = 1e-15, 1e-15
        mid = j == ips // 2
        fa[mid], fb[mid] = 0.0, 1e6
    elif pattern == "zero-first-tiny":       # a zero A tile first, then A ~ 1e-22, Bt ~ 1: no phantom maximum from the zero tile
        fa[:] = 1e-22
        fa[j == 0] = 0.0
    else:
        raise ValueError(pattern)
    return fa.float(), fb.float()


H2_SHAPES = [(3, 1, 128, 128), (4, 2, 128, 64), (3, 1, 64, 128), (3, 1, 32, 128)]
PATTERNS = ["small-first", "falling", "spread", "zero-tiles", "zero-among-tiny", "zero-first-tiny"]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("k,s,CA,CB", H2_SHAPES, ids=lambda v: str(v))
def test_two_term_weight_gradient_scales_inside_ranges(k, s, CA, CB, pattern):
    # the smallest batch with eight images in every range: ns = ceil(512 / tiles) ranges
    B = 8 * map8_plan(BENCH_B, k, CA, CB).splits
    plan = map8_plan(B, k, CA, CB)
    assert plan.per_split == 8 and plan.splits * 8 == B, plan
    pad = 1
    g = torch.Generator().manual_seed(k * 100 + CA + PATTERNS.index(pattern))
    fa, fb = _factors(pattern, B, plan.per_split, g)
    a = torch.randn(B, 8, 8, CA, generator=g) * fa[:, None, None, None]
    bt = torch.randn(B, 8 * s, 8 * s, CB, generator=g) * fb[:, None, None, None]
    ref = _wgrad_ref(a, bt, k, s, pad)
    got = _wgrad(a.to(DEV), bt.to(DEV), k, s, pad, exact=False)
    assert torch.isfinite(got).all()
    err = (got.cpu().double() - ref).abs().amax(dim=(2, 3))
    lim = 2e-5 * ref.abs().amax(dim=(2, 3)) + 1e-300
    assert bool((err <= lim).all()), (pattern, float((err / lim).max()))


# ---- first / last layer (conv_wgrad_img_kernel) and the per-tap kernel on 56x56 maps --------------------------------------------

@pytest.mark.parametrize("CA,CB", [(64, 3), (32, 1)])
def test_image_operand_weight_gradient_at_the_bench_batch(CA, CB):
    """Conv2d(CB, CA, 4, 2, 1) on 32x32 images (A = grad_y, Bt = x) and ConvTranspose2d(CA, CB, 4, 2, 1) (A = t, Bt = grad_y): the
    same sum, eight images per workgroup at B = 4096"""
    plan = img_plan(BENCH_B, CA, CB)
    assert plan.per_split >= 8 and plan.splits * plan.per_split == BENCH_B, plan
    g = torch.Generator().manual_seed(CA + CB)
    a = torch.randn(BENCH_B, 16, 16, CA, generator=g)
    bt = torch.randn(BENCH_B, CB, 32, 32, generator=g)
    ref = _wgrad_ref(a, bt, 4, 2, 1, bt_nchw=True)
    got = _wgrad(a.to(DEV), bt.to(DEV), 4, 2, 1, exact=False, bt_nchw=True)
    _close_grad(got, ref.float(), "grad_w")
    assert _per_slice(got, ref) <= 1.0


def _generic_batch(k, CA, CB, want):
    """the smallest batch of 56x56 maps whose last split is ragged (0 < last < per_split) or empty (last == 0)"""
    for B in range(4, 64):
        p = generic_plan(B, 56, 56, CA, CB, k)
        if (want == "empty" and p.last == 0) or (want == "ragged" and 0 < p.last < p.per_split):
            return B, p
    raise AssertionError(f"no batch with a {want} last split")


@pytest.mark.parametrize("last", ["ragged", "empty"])
@pytest.mark.parametrize("k,CA,CB", [(3, 128, 128), (1, 128, 32)], ids=lambda v: str(v))
def test_generic_weight_gradient_last_split(k, CA, CB, last):
    """conv_wgrad_kernel on the 56x56 latent maps of config 4 (224x224 images): near its 64-split cap, the last split ragged or empty"""
    B, plan = _generic_batch(k, CA, CB, last)
    assert plan.splits >= 32, plan
    pad = 1 if k == 3 else 0
    g = torch.Generator().manual_seed(B * 10 + k)
    a = torch.randn(B, 56, 56, CA, generator=g)
    bt = torch.randn(B, 56, 56, CB, generator=g)
    ref = _wgrad_ref(a, bt, k, 1, pad)
    got = _wgrad(a.to(DEV), bt.to(DEV), k, 1, pad, exact=False)
    _close_grad(got, ref.float(), f"grad_w B={B} {plan}")
    assert _per_slice(got, ref) <= 1.0


# ---- bias gradient: more than 1 Mi pixels, 512 blocks, a ragged last block ------------------------------------------------------

def _spacing32(ref64):
    r = np.abs(ref64.float().numpy())
    return np.spacing(np.maximum(r, np.float32(np.finfo(np.float32).tiny))).astype(np.float64)


def _fp32_ulps(got, ref64):
    """|got - round32(ref)| in units of the fp32 spacing at round32(ref)"""
    return np.abs(got.cpu().numpy().astype(np.float64) - ref64.float().numpy().astype(np.float64)) / _spacing32(ref64)


@pytest.mark.parametrize("layout,B,H,W,C", [("rowmajor", 16389, 8, 8, 32),      # C % 4 == 0: four channels per thread
                                            ("rowmajor", 16389, 8, 8, 7),       # one channel per thread
                                            ("nchw", 1338, 28, 28, 3)])         # NCHW, blocks across image boundaries
def test_bias_gradient_over_a_million_pixels(layout, B, H, W, C):
    from vqvae_amd import autograd_conv as A
    P = B * H * W
    plan = bias_plan(P, C)
    assert P >= 1 << 20 and plan.splits == 512 and 0 < plan.last < plan.per_split, plan
    g = torch.Generator().manual_seed(C + H)
    shape = (B, C, H, W) if layout == "nchw" else (B, H, W, C)
    x = torch.randn(*shape, generator=g) + 0.25                       # an offset: no column sum near zero
    ref = x.sum(dim=(0, 2, 3) if layout == "nchw" else (0, 1, 2), dtype=torch.float64)
    xd = x.to(DEV)
    got = A.bias_grad(xd, nchw=layout == "nchw")
    assert torch.equal(got, A.bias_grad(xd, nchw=layout == "nchw"))
    assert _fp32_ulps(got, ref).max() <= 1.0, (_fp32_ulps(got, ref).max(), plan)


# ---- VQ codebook gradient and EMA update at N = 262 144 rows --------------------------------------------------------------------

def _vq_case(hist, B, D, K, g):
    """z (B, D, 8, 8) and the rows' codes.  fresh: the forward's own indices on a freshly initialised codebook (z with a shared
    direction, as an untrained encoder's output: a few dozen codes own all rows, the busiest hundreds of units); one-code: every row
    on one code; cluster: 420 codes"""
    from vqvae_amd import functional as F
    cb = (torch.rand(K, D, generator=g) * 2 - 1) / K                  # VectorQuantizer's init (quantizer.py:27)
    z = torch.randn(B, D, 8, 8, generator=g) * 0.05 + 0.2 * torch.randn(1, D, 1, 1, generator=g)
    N = B * 64
    if hist == "fresh":
        idx = F.vq_forward(z.to(DEV), cb.to(DEV), 0.25)[3].reshape(N, 1).cpu()
    elif hist == "one-code":
        idx = torch.full((N, 1), K // 3, dtype=torch.int64)
    else:
        idx = torch.randint(0, 420, (N, 1), generator=g)
    return z, cb, idx


VQ_CASES = [  # histogram, B, D, K -- N = 64 B rows
    ("fresh", 4096, 64, 512),
    ("one-code", 4096, 64, 512),      # 512 units: four interleaved sums, no tail
    ("one-code", 4097, 64, 512),      # 513: a tail of one
    ("one-code", 4105, 64, 512),      # 514: a tail of two
    ("one-code", 4113, 64, 512),      # 515: a tail of three
    ("cluster", 4096, 64, 512),
    ("fresh", 4096, 48, 512),
    ("one-code", 4113, 48, 512),
    ("fresh", 4096, 7, 512),
    ("one-code", 4105, 7, 512),
]


def _check_units(hist, B, units, chunk):
    assert chunk == 512                                              # VQ_CASES' unit counts (512 .. 515 units) are written for it
    if hist == "one-code":
        assert int(units.max()) == _cdiv(B * 64, chunk) and int(units.sum()) == int(units.max()), units.max()
    elif hist == "fresh":
        assert int(units.max()) >= 100, int(units.max())             # hundreds of units on the busiest code
    else:
        assert int((units > 0).sum()) == 420 and int(units.max()) >= 2


@pytest.mark.parametrize("rowmajor", [False, True], ids=["nchw", "rowmajor"])
@pytest.mark.parametrize("hist,B,D,K", VQ_CASES, ids=lambda v: str(v))
def test_codebook_gradient_and_ema_update_at_the_bench_batch(hist, B, D, K, rowmajor):
    from vqvae_amd import training as T
    g = torch.Generator().manual_seed(B + D + len(hist))
    z, cb, idx = _vq_case(hist, B, D, K, g)
    _check_units(hist, B, *bwd_units(idx, K, D))
    N = B * 64
    rows = R.rows_of(z.permute(0, 2, 3, 1), True).double()
    flat = idx.reshape(-1)
    cnt = torch.bincount(flat, minlength=K).double()
    zsum = torch.zeros(K, D, dtype=torch.float64).index_add_(0, flat, rows)
    zabs = torch.zeros(K, D, dtype=torch.float64).index_add_(0, flat, rows.abs())
    zd, cbd, idxd = _layout(z, rowmajor).to(DEV), cb.to(DEV), idx.to(DEV)
    g_loss, beta = torch.tensor(0.7), 0.25

    # dL/dE_k = g_loss 2 beta / (N D) (cnt_k e_k - sum_{i: idx_i = k} z_i)
    ge = T.vq_backward(zd, cbd, idxd, None, g_loss.to(DEV), beta, rowmajor=rowmajor, need_z=False)[1]
    assert torch.equal(ge, T.vq_backward(zd, cbd, idxd, None, g_loss.to(DEV), beta, rowmajor=rowmajor, need_z=False)[1]), \
        "codebook gradient: not bit-reproducible"
    scale = float(g_loss.double()) * 2.0 * beta / (N * D)
    e = cb.double()
    ref = scale * (cnt[:, None] * e - zsum)
    slack = 2.0 ** -45 * scale * (cnt[:, None] * e.abs() + zabs)
    excess = _fp32_ulps(ge, ref) - 1.0 - slack.numpy() / _spacing32(ref)
    assert excess.max() <= 0.0, float(excess.max())
    assert (ge.cpu()[cnt == 0] == 0).all()

    # one EMA update from a cold and from a warm state
    cs0 = torch.rand(K, generator=g) * 2 * (torch.rand(K, generator=g) < 0.5)
    w0 = cb * cs0[:, None] + (torch.rand(K, D, generator=g) - 0.5) * 1e-3
    for cs, w in ((torch.zeros(K), cb.clone()), (cs0, w0)):
        cs_d, w_d, cbn = _update(zd, idxd, cs, w, rowmajor)
        ref = R.ema_update(rows, idx, cs, w, 0.99, 1e-5)
        assert _ulps(cs_d, ref["N"]).max() <= 1
        assert _ulps(w_d, ref["m"]).max() <= 1
        assert _ulps(cbn, ref["e"]).max() <= 2
        again = _update(zd, idxd, cs, w, rowmajor)
        for x, y in zip((cs_d, w_d, cbn), again):
            assert torch.equal(x, y), "EMA update: not bit-reproducible"
