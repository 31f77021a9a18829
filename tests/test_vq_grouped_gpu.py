"""Grouped (product) quantization on the GPU (vqvae_vq_grouped_forward_f32 / _decode_f32 / _backward_f32, functional.vq_grouped_*,
training.vq_grouped_backward, GroupedVectorQuantizer(EMA), VQVAE(codebook_groups=...)).

The yardstick is the one-codebook path on the torch-made contiguous slice of each group -- functional.vq_forward,
training.vq_backward, VectorQuantizerEMA, functional.vq_kmeans: existing entries, pinned to the reference elsewhere -- and every
comparison with it is bit equality: no row left out, no tolerance.  z_q, loss and the slabs are compared, bit for bit too, with the
CPU restatement tests/vq_grouped_ref.py evaluated from those indices (the contract of vqvae_amd/csrc/vq_grouped.hip's header)."""
import copy
import faulthandler
import functools

import numpy as np
import pytest
import torch

from tests import graph_replay as GP
from tests import grid_caps as GC
from tests import vq_grouped_ref as GR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BETA = 0.25

# (K, D, G): d = 32, the fast quantizer; d = 16; d = 16 with D no power of two; d = 2, the element path; d = 1; d = 128, the
# streamed screen
KDG = [(512, 64, 2), (96, 64, 4), (64, 48, 3), (5, 6, 3), (5, 3, 3), (2048, 256, 2)]
# (B, H, W): 192 rows; H W = 32; H W = 15 -- NCHW maps that are no multiple of four pixels: the element path
SHAPES = [(3, 8, 8), (5, 4, 8), (2, 3, 5)]
# (K, D, G, B, H, W) past the element-wise kernels' launch cap (tests/grid_caps.py reads the shape from here)
CAP_SHAPE = (16, 256, 2, 17477, 3, 5)
CAP_SHAPE_ELEMENT = (5, 6, 3, 186414, 3, 5)


def _bits(t):
    a = t.detach().cpu().contiguous().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)
    return a.view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _layout(rows, B, H, W, rowmajor):
    """(N, D) numpy rows -> the device tensor whose rows they are: (B,H,W,D), or (B,D,H,W)"""
    z = torch.from_numpy(np.ascontiguousarray(rows)).view(B, H, W, rows.shape[1])
    return (z if rowmajor else z.permute(0, 3, 1, 2)).contiguous().to(DEV)


def _rows(t, rowmajor):
    """the (N, D) numpy rows of a device tensor in either layout"""
    t = t.detach().cpu()
    t = t if rowmajor else t.permute(0, 2, 3, 1)
    return np.ascontiguousarray(t.contiguous().numpy().reshape(-1, t.shape[-1]))


def _slice(z, g, d, rowmajor):
    """the torch-made contiguous slice of group g"""
    return (z[..., g * d:(g + 1) * d] if rowmajor else z[:, g * d:(g + 1) * d]).contiguous()


def _dev(books):
    return [torch.from_numpy(np.ascontiguousarray(E)).to(DEV) for E in books]


@functools.lru_cache(maxsize=None)
def _case(K, D, G, B, H, W):
    """rows and G codebooks, computed once and left unchanged: half of a group's codes are rows of its slab (rows that equal a code
    exactly), the others such rows moved a little"""
    N, d = B * H * W, D // G
    rng = np.random.default_rng(K + D + G + N)
    rows = rng.standard_normal((N, D)).astype(np.float32)
    sl = GR.slabs(rows, G)
    books = []
    for g in range(G):
        E = sl[g][rng.integers(0, N, K)].copy()
        E[K // 2:] += (0.05 * rng.standard_normal((K - K // 2, d))).astype(np.float32)
        books.append(E)
    return rows, books


def _check_against_the_slices(out, z, dbooks, rows, books, B, H, W, rowmajor, what):
    """idx, hist, loss_group, perplexity: vq_forward's bits on every group's slice; z_q, loss, slabs: the restatement's bits from
    those indices"""
    from vqvae_amd import functional as F
    loss, z_q, ppl, idx, hist, loss_group, slabs = out
    G, d, K = len(dbooks), dbooks[0].shape[1], dbooks[0].shape[0]
    N = B * H * W
    assert idx.shape == (G, N) and idx.dtype == torch.int64 and hist.shape == (G, K) and hist.dtype == torch.int32
    assert ppl.shape == (G,) and loss_group.shape == (G,) and loss.dim() == 0
    for g in range(G):
        l1, _, p1, i1, h1 = F.vq_forward(_slice(z, g, d, rowmajor), dbooks[g], BETA, rowmajor=rowmajor, want_zq=False)
        assert torch.equal(idx[g], i1.view(-1)), f"{what}: indices of group {g}"
        assert torch.equal(hist[g], h1), f"{what}: histogram of group {g}"
        assert _same(loss_group[g], l1), f"{what}: loss of group {g}: {float(loss_group[g])} {float(l1)}"
        assert _same(ppl[g], p1), f"{what}: perplexity of group {g}: {float(ppl[g])} {float(p1)}"
    torch.cuda.synchronize()
    idx_h = idx.cpu().numpy()
    if z_q is not None:
        assert z_q.shape == z.shape
        assert np.array_equal(_bits(_rows(z_q, rowmajor)), _bits(GR.z_q_of(rows, books, idx_h))), f"{what}: z_q"
    assert np.array_equal(_bits(loss).reshape(1), _bits(GR.mean_loss(loss_group.cpu().numpy())).reshape(1)), f"{what}: loss"
    if slabs is not None:
        assert np.array_equal(_bits(slabs), _bits(GR.slab_layout(GR.slabs(rows, G), B, H, W, rowmajor))), f"{what}: slabs"
    # ... and that loss is the reference's formula on the whole rows (fp64, the quantizer's own tolerance)
    c = GR.forward(rows, books, BETA, idx=idx_h)
    np.testing.assert_allclose(float(loss), c.loss, rtol=1e-6, err_msg=what)


# ---- 1. forward ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rowmajor", [False, True])
@pytest.mark.parametrize("B,H,W", SHAPES)
@pytest.mark.parametrize("K,D,G", KDG)
def test_forward_is_the_quantizer_on_every_slice(K, D, G, B, H, W, rowmajor):
    from vqvae_amd import functional as F
    rows, books = _case(K, D, G, B, H, W)
    z, dbooks = _layout(rows, B, H, W, rowmajor), _dev(books)
    out = F.vq_grouped_forward(z, dbooks, BETA, rowmajor=rowmajor, want_slabs=True)
    _check_against_the_slices(out, z, dbooks, rows, books, B, H, W, rowmajor, f"K={K} D={D} G={G} {B}x{H}x{W} rowmajor={rowmajor}")
    again = F.vq_grouped_forward(z, dbooks, BETA, rowmajor=rowmajor, want_slabs=True)
    torch.cuda.synchronize()
    assert all(_same(a, b) for a, b in zip(out, again)), "two runs"


@pytest.mark.parametrize("rowmajor", [False, True])
@pytest.mark.parametrize("K,D,B,H,W", [(512, 64, 3, 8, 8), (96, 32, 5, 4, 8), (64, 48, 2, 3, 5), (5, 3, 2, 3, 5), (2048, 128, 3, 8, 8)])
def test_one_group_has_the_quantizers_bits(K, D, B, H, W, rowmajor):
    from vqvae_amd import functional as F
    rows, books = _case(K, D, 1, B, H, W)
    z, cb = _layout(rows, B, H, W, rowmajor), _dev(books)[0]
    loss, z_q, ppl, idx, hist, loss_group = F.vq_grouped_forward(z, [cb], BETA, rowmajor=rowmajor)
    l1, zq1, p1, i1, h1 = F.vq_forward(z, cb, BETA, rowmajor=rowmajor)
    torch.cuda.synchronize()
    assert torch.equal(idx.view(-1), i1.view(-1)) and torch.equal(hist.view(-1), h1)
    assert _same(z_q, zq1) and _same(loss, l1) and _same(loss_group[0], l1) and _same(ppl[0], p1)


@pytest.mark.parametrize("rowmajor", [False, True])
def test_forward_without_zq_and_on_a_prepared_workspace(rowmajor):
    from vqvae_amd import functional as F
    K, D, G, B, H, W = 96, 64, 4, 3, 8, 8
    rows, books = _case(K, D, G, B, H, W)
    z, dbooks = _layout(rows, B, H, W, rowmajor), _dev(books)
    ws = F.vq_grouped_workspace(B * H * W, K, D, G, DEV)
    first = F.vq_grouped_forward(z, dbooks, BETA, rowmajor=rowmajor, workspace=ws, want_slabs=True)
    again = F.vq_grouped_forward(z, dbooks, BETA, rowmajor=rowmajor, workspace=ws, prepared=True, want_slabs=True)
    _check_against_the_slices(first, z, dbooks, rows, books, B, H, W, rowmajor, "fresh workspace")
    assert all(_same(a, b) for a, b in zip(first, again)), "prepared workspace"
    out = F.vq_grouped_forward(z, dbooks, BETA, rowmajor=rowmajor, workspace=ws, prepared=True, want_zq=False)
    torch.cuda.synchronize()
    assert out[1] is None and len(out) == 6
    assert all(_same(a, b) for a, b in zip(out[:1] + out[2:], first[:1] + first[2:6])), "index-only"


@pytest.mark.parametrize("rowmajor", [False, True])
@pytest.mark.parametrize("K,D,G,B,H,W", [(96, 64, 4, 3, 8, 8), (64, 48, 3, 5, 4, 8), (512, 64, 2, 3, 8, 8)])
def test_both_access_widths_give_the_same_bits(K, D, G, B, H, W, rowmajor):
    """z as a view one float into a larger buffer: no tensor-wide 16-byte alignment, so the split, finish and grad_z kernels go
    element by element where the aligned call moves 16 bytes per access"""
    from vqvae_amd import functional as F, training as T
    rows, books = _case(K, D, G, B, H, W)
    z, dbooks = _layout(rows, B, H, W, rowmajor), _dev(books)
    buf = torch.empty(z.numel() + 4, device=DEV)
    z_off = buf[1:1 + z.numel()].view(z.shape)
    z_off.copy_(z)
    assert z.data_ptr() % 16 == 0 and z_off.data_ptr() % 16 == 4 and z_off.is_contiguous()
    a = F.vq_grouped_forward(z, dbooks, BETA, rowmajor=rowmajor, want_slabs=True)
    b = F.vq_grouped_forward(z_off, dbooks, BETA, rowmajor=rowmajor, want_slabs=True)
    torch.cuda.synchronize()
    assert all(_same(x, y) for x, y in zip(a, b))
    gzq, gl = torch.randn(z.shape, device=DEV), torch.tensor(0.7, device=DEV)
    ga = T.vq_grouped_backward(z, dbooks, a[3], gzq, gl, BETA, rowmajor=rowmajor)
    gb = T.vq_grouped_backward(z_off, dbooks, a[3], gzq, gl, BETA, rowmajor=rowmajor)
    torch.cuda.synchronize()
    assert _same(ga[0], gb[0]) and all(_same(x, y) for x, y in zip(ga[1], gb[1]))


def _past_the_cap(shape, rowmajor):
    """the forward against the slices, then the backward direction past the same cap: grad_z in the header's order, into a buffer
    that starts as NaNs between guards"""
    from vqvae_amd import functional as F, training as T
    K, D, G, B, H, W = shape
    rows, books = _case(K, D, G, B, H, W)
    z, dbooks = _layout(rows, B, H, W, rowmajor), _dev(books)
    out = F.vq_grouped_forward(z, dbooks, BETA, rowmajor=rowmajor, want_slabs=True)
    _check_against_the_slices(out, z, dbooks, rows, books, B, H, W, rowmajor, f"{B * H * W} rows, rowmajor={rowmajor}")
    idx = out[3]
    del out
    gzq = torch.randn(z.shape, generator=torch.Generator().manual_seed(K + G)).to(DEV)
    g = np.float32(0.7)
    with GC.guarded() as guard:
        gz, none = T.vq_grouped_backward(z, dbooks, idx, gzq, torch.tensor(float(g), device=DEV), BETA, rowmajor=rowmajor,
                                         need_codebooks=False)
    guard.check()
    assert none is None
    assert np.array_equal(_bits(_rows(gz, rowmajor)), _bits(GR.grad_z_mirror(rows, books, idx.cpu().numpy(), _rows(gzq, rowmajor), g)))


@pytest.mark.parametrize("rowmajor", [False, True])
def test_grid_stride_past_the_launch_cap(rowmajor):
    """more units than the stream kernels' 65536 workgroups of 256 threads cover in one step, in both access widths (H W = 15: NCHW
    maps go element by element), forward and backward"""
    K, D, G, B, H, W = CAP_SHAPE
    assert B * H * W * D // 4 > 65536 * 256
    _past_the_cap(CAP_SHAPE, rowmajor)


@pytest.mark.parametrize("rowmajor", [False, True])
def test_grid_stride_past_the_launch_cap_element_path(rowmajor):
    """the element path with a last lap that ends inside a workgroup: groups of two channels go element by element in both layouts,
    and 6 channels make an element count that is no multiple of 256 (CAP_SHAPE's 256 channels always give one)"""
    K, D, G, B, H, W = CAP_SHAPE_ELEMENT
    assert B * H * W * D > 65536 * 256 and (B * H * W * D) % 256 != 0 and (D // G) % 4 != 0
    _past_the_cap(CAP_SHAPE_ELEMENT, rowmajor)


def test_decode_past_32_bit_element_counts_16GiB():
    """N D = 2^32 elements, the smallest size at which the launches take the 64-bit element arithmetic (smaller tensors run the same
    bodies on 32-bit integers): a 16 GiB result, compared with torch's gather a block of rows at a time.  NEEDS ABOUT 18 GiB OF
    FREE DEVICE MEMORY: on a smaller or a fuller card this test fails to allocate, and that says nothing about the kernels."""
    from vqvae_amd import functional as F
    K, G, d, B, H, W = 16, 2, 128, 1 << 16, 16, 16
    N, D = B * H * W, G * d
    assert N * D == 1 << 32
    gen = torch.Generator(device=DEV).manual_seed(3)
    books = [torch.randn((K, d), device=DEV, generator=gen) for _ in range(G)]
    idx = torch.randint(0, K, (G, N), device=DEV, generator=gen)
    idx[1, N - 1] = K                                         # the very last segment: NaN, and only there
    got = F.vq_grouped_decode(idx, books, B, H, W, rowmajor=True, validate=False).view(N, D).view(torch.int32)
    step = 1 << 20
    for r0 in range(0, N, step):
        want = torch.cat([books[g][idx[g, r0:r0 + step].clamp(max=K - 1)] for g in range(G)], dim=1).view(torch.int32)
        if r0 + step == N:
            assert bool(got[N - 1, d:].view(torch.float32).isnan().all())
            want[-1, d:] = got[N - 1, d:]
        assert torch.equal(got[r0:r0 + step], want), f"rows from {r0}"


# ---- 2. special values -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rowmajor", [False, True])
@pytest.mark.parametrize("K,D,G,B,H,W", [(96, 64, 4, 3, 8, 8), (5, 6, 3, 2, 3, 5), (512, 64, 2, 5, 4, 8)])
def test_special_values_stay_in_their_group(K, D, G, B, H, W, rowmajor):
    from vqvae_amd import functional as F
    rows, books = _case(K, D, G, B, H, W)
    d, dbooks = D // G, _dev(books)
    base = F.vq_grouped_forward(_layout(rows, B, H, W, rowmajor), dbooks, BETA, rowmajor=rowmajor)
    g1, r1 = G - 1, 7
    for name, vals in (("NaN", [np.nan]), ("+Inf", [np.inf]), ("-Inf", [-np.inf]), ("-0.0", [-0.0] * d)):
        sp = rows.copy()
        sp[r1, g1 * d:g1 * d + len(vals)] = vals
        z = _layout(sp, B, H, W, rowmajor)
        out = F.vq_grouped_forward(z, dbooks, BETA, rowmajor=rowmajor, want_slabs=True)
        torch.cuda.synchronize()
        # the quantizer's own answer on every slice (NaN as the minimum, Inf rows), bit for bit
        for g in range(G):
            l1, _, p1, i1, h1 = F.vq_forward(_slice(z, g, d, rowmajor), dbooks[g], BETA, rowmajor=rowmajor, want_zq=False)
            assert torch.equal(out[3][g], i1.view(-1)) and torch.equal(out[4][g], h1), name
            assert _same(out[5][g], l1) and _same(out[2][g], p1), name
        idx_h = out[3].cpu().numpy()
        got, want = _rows(out[1], rowmajor), GR.z_q_of(sp, books, idx_h)
        assert np.array_equal(np.isnan(got), np.isnan(want)), name
        assert np.array_equal(_bits(got)[~np.isnan(got)], _bits(want)[~np.isnan(want)]), name
        assert np.array_equal(_bits(out[6]), _bits(GR.slab_layout(GR.slabs(sp, G), B, H, W, rowmajor))), f"{name}: the slabs move bits"
        # the other groups of that row and all other rows keep their bits
        keep = np.ones((B * H * W, D), bool)
        keep[r1, g1 * d:(g1 + 1) * d] = False
        assert np.array_equal(_bits(got)[keep], _bits(_rows(base[1], rowmajor))[keep]), name
        ikeep = np.ones((G, B * H * W), bool)
        ikeep[g1, r1] = False
        assert np.array_equal(idx_h[ikeep], base[3].cpu().numpy()[ikeep]), name
        assert all(_same(out[5][g], base[5][g]) and _same(out[2][g], base[2][g]) for g in range(G - 1)), name


# ---- 3. decode ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rowmajor", [False, True])
@pytest.mark.parametrize("K,D,G,B,H,W", [(96, 64, 4, 3, 8, 8), (64, 48, 3, 2, 3, 5), (5, 3, 3, 5, 4, 8), (5, 6, 3, 2, 3, 5)])
def test_decode_is_the_gathered_rows(K, D, G, B, H, W, rowmajor):
    from vqvae_amd import functional as F
    rows, books = _case(K, D, G, B, H, W)
    dbooks, N, d = _dev(books), B * H * W, D // G
    idx = torch.from_numpy(np.random.default_rng(K + N).integers(0, K, (G, N))).to(DEV)
    want = torch.cat([dbooks[g][idx[g]] for g in range(G)], dim=1).cpu().numpy()
    got = F.vq_grouped_decode(idx, dbooks, B, H, W, rowmajor=rowmajor)
    assert got.shape == ((B, H, W, D) if rowmajor else (B, D, H, W))
    assert np.array_equal(_bits(_rows(got, rowmajor)), _bits(want))
    # indices K and -1: NaN in exactly that group's segment (through the C entry: the front end's check is off)
    bad = idx.clone()
    bad[G - 1, 7], bad[0, 11] = K, -1
    with pytest.raises(IndexError):
        F.vq_grouped_decode(bad, dbooks, B, H, W, rowmajor=rowmajor)
    got = _rows(F.vq_grouped_decode(bad, dbooks, B, H, W, rowmajor=rowmajor, validate=False), rowmajor)
    nan = np.zeros((N, D), bool)
    nan[7, (G - 1) * d:], nan[11, :d] = True, True
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


# ---- 4. backward -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rowmajor", [False, True])
@pytest.mark.parametrize("K,D,G,B,H,W", [(96, 64, 4, 3, 8, 8), (64, 48, 3, 2, 3, 5), (5, 6, 3, 5, 4, 8), (5, 3, 3, 2, 3, 5), (512, 64, 2, 5, 4, 8)])
def test_backward_is_the_quantizers_on_every_slice(K, D, G, B, H, W, rowmajor):
    from vqvae_amd import functional as F, training as T
    rows, books = _case(K, D, G, B, H, W)
    z, dbooks, d = _layout(rows, B, H, W, rowmajor), _dev(books), D // G
    idx = F.vq_grouped_forward(z, dbooks, BETA, rowmajor=rowmajor, want_zq=False)[3]
    gzq = torch.randn(z.shape, generator=torch.Generator().manual_seed(K + G)).to(DEV)
    g = np.float32(0.7)
    gl = torch.tensor(float(g), device=DEV)
    gq = torch.tensor(float(np.float32(g / np.float32(G))), device=DEV)       # g / (float)G: one fp32 division
    one_q = torch.tensor(float(np.float32(np.float32(1.0) / np.float32(G))), device=DEV)
    gz, ge = T.vq_grouped_backward(z, dbooks, idx, gzq, gl, BETA, rowmajor=rowmajor)
    gz0, ge0 = T.vq_grouped_backward(z, dbooks, idx, None, None, BETA, rowmajor=rowmajor)          # no upstream z_q gradient, g = 1
    gzc, none = T.vq_grouped_backward(z, dbooks, idx, gzq, gl, BETA, rowmajor=rowmajor, need_codebooks=False, commitment=True)
    gz2, ge2 = T.vq_grouped_backward(z, dbooks, idx, gzq, gl, BETA, rowmajor=rowmajor)
    torch.cuda.synchronize()
    assert none is None and len(ge) == G
    assert _same(gz, gz2) and all(_same(a, b) for a, b in zip(ge, ge2)), "two runs"
    for gi in range(G):
        zs, gs, ig = _slice(z, gi, d, rowmajor), _slice(gzq, gi, d, rowmajor), idx[gi]
        w_gz, w_ge = T.vq_backward(zs, dbooks[gi], ig, gs, gq, BETA, rowmajor=rowmajor)
        assert _same(_slice(gz, gi, d, rowmajor), w_gz), f"grad_z of group {gi}"
        assert _same(ge[gi], w_ge) and float(w_ge.abs().max()) > 0, f"codebook gradient of group {gi}"
        w_gz, w_ge = T.vq_backward(zs, dbooks[gi], ig, None, one_q, BETA, rowmajor=rowmajor)
        assert _same(_slice(gz0, gi, d, rowmajor), w_gz) and _same(ge0[gi], w_ge), f"group {gi} without grad_zq, g = 1"
        w_gz, _ = T.vq_backward(zs, dbooks[gi], ig, gs, gq, BETA, rowmajor=rowmajor, need_codebook=False, commitment=True)
        assert _same(_slice(gzc, gi, d, rowmajor), w_gz), f"commitment-only grad_z of group {gi}"
    # ... and the header's order on the CPU
    assert np.array_equal(_bits(_rows(gz, rowmajor)), _bits(GR.grad_z_mirror(rows, books, idx.cpu().numpy(), _rows(gzq, rowmajor), g)))


def test_autograd_pairing():
    from vqvae_amd import training as T
    from vqvae_amd.modules import GroupedVectorQuantizer
    K, D, G, B, H, W = 96, 64, 4, 3, 8, 8
    rows, books = _case(K, D, G, B, H, W)
    vq = GroupedVectorQuantizer(G, K, D, BETA).to(DEV)
    with torch.no_grad():
        for w, E in zip(vq.codebooks(), _dev(books)):
            w.copy_(E)
    z = _layout(rows, B, H, W, True).requires_grad_(True)
    loss, z_q, ppl, idx, hist = vq.quantize(z, rowmajor=True)
    assert loss.requires_grad and z_q.requires_grad and not ppl.requires_grad and not idx.requires_grad and not hist.requires_grad
    # ... also with the slabs written out, and in the EMA form (what GroupedVectorQuantizerEMA's training forward applies)
    for commitment in (False, True):
        out = T.GroupedStraightThrough.apply(z, BETA, True, commitment, True, None, False, *vq.codebooks())
        assert len(out) == 7 and out[0].requires_grad and out[1].requires_grad
        assert all(not t.requires_grad and t.grad_fn is None for t in out[2:]), [t.requires_grad for t in out]
    gzq = torch.randn(z.shape, device=DEV)
    (loss * 1.5 + (z_q * gzq).sum()).backward()
    gz, ge = T.vq_grouped_backward(z.detach(), [w.detach() for w in vq.codebooks()], idx, gzq, torch.tensor(1.5, device=DEV), BETA,
                                   rowmajor=True)
    assert _same(z.grad, gz) and all(_same(w.grad, g) for w, g in zip(vq.codebooks(), ge))


# ---- 5. the EMA form ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rowmajor", [False, True])
@pytest.mark.parametrize("restart", [None, 0.05])
def test_ema_is_one_ema_quantizer_per_slice(restart, rowmajor):
    from vqvae_amd.modules import GroupedVectorQuantizerEMA, VectorQuantizerEMA
    K, D, G, B, H, W = 96, 64, 4, 3, 8, 8
    d = D // G
    torch.manual_seed(11)
    vq = GroupedVectorQuantizerEMA(G, K, D, BETA, decay=0.9, eps=1e-5, restart_threshold=restart,
                                   generator=torch.Generator(device=DEV).manual_seed(21)).to(DEV).train()
    shared = torch.Generator(device=DEV).manual_seed(21)       # one generator for the G modules: the uniforms in group order
    singles = []
    for g, w in enumerate(vq.codebooks()):
        s = VectorQuantizerEMA(K, d, BETA, decay=0.9, eps=1e-5, restart_threshold=restart, generator=shared).to(DEV).train()
        with torch.no_grad():
            s.embedding.weight.copy_(w)
            s.ema_w.copy_(w)
        singles.append(s)
    assert all(not w.requires_grad for w in vq.codebooks()) and _same(vq.ema_w, torch.stack([s.ema_w for s in singles]))
    rng = np.random.default_rng(5)
    with torch.no_grad():
        for step in range(3):
            z = _layout((0.02 * rng.standard_normal((B * H * W, D))).astype(np.float32), B, H, W, rowmajor)
            loss, z_q, ppl, idx, hist = vq.quantize(z, rowmajor=rowmajor)
            mse = []
            for g, s in enumerate(singles):
                l1, zq1, p1, i1, h1 = s.quantize(_slice(z, g, d, rowmajor), rowmajor=rowmajor)
                mse.append(np.float32(float(l1)) / np.float32(BETA))       # (beta is a power of two: l1 = beta * mse exactly)
                assert torch.equal(idx[g], i1.view(-1)) and torch.equal(hist[g], h1) and _same(ppl[g], p1), f"step {step} group {g}"
                assert _same(_slice(z_q, g, d, rowmajor), zq1), f"step {step} group {g}: z_q"
            torch.cuda.synchronize()
            # the loss: beta times the mean of the groups' mse in the contract's fp32 order
            want = np.float32(GR.mean_loss(np.array(mse, np.float32)) * np.float32(BETA))
            assert np.array_equal(_bits(loss).reshape(1), _bits(want).reshape(1)), f"step {step}: loss {float(loss)} {float(want)}"
            for g, s in enumerate(singles):
                assert _same(vq.ema_cluster_size[g], s.ema_cluster_size), f"step {step} group {g}: ema_cluster_size"
                assert _same(vq.ema_w[g], s.ema_w), f"step {step} group {g}: ema_w"
                assert _same(vq.codebooks()[g], s.embedding.weight), f"step {step} group {g}: codebook"
        if restart is not None:
            assert int((vq.ema_cluster_size < restart).sum()) > 0          # codes were restarted
        # eval mode never updates
        state = [t.clone() for t in (vq.ema_cluster_size, vq.ema_w, *vq.codebooks())]
        vq.eval()
        vq.quantize(z, rowmajor=rowmajor)
        assert all(_same(a, b) for a, b in zip(state, (vq.ema_cluster_size, vq.ema_w, *vq.codebooks())))
    # under autograd in training mode: the commitment-only gradient, and one more update
    vq.train()
    zg = z.clone().requires_grad_(True)
    loss, z_q, ppl, idx, hist = vq.quantize(zg, rowmajor=rowmajor)
    assert loss.requires_grad and z_q.requires_grad, "loss and z_q are differentiable"
    assert not ppl.requires_grad and ppl.grad_fn is None and not idx.requires_grad and not hist.requires_grad, "the rest are not"
    books_before = state[2:]
    loss.backward()
    from vqvae_amd import training as T
    want, _ = T.vq_grouped_backward(z, books_before, idx, None, torch.tensor(1.0, device=DEV), BETA, rowmajor=rowmajor,
                                    need_codebooks=False, commitment=True)
    assert _same(zg.grad, want) and not _same(vq.ema_w, state[1])


# ---- 6. the model ------------------------------------------------------------------------------------------------------------------

def _model(**kw):
    from vqvae_amd import conv
    from vqvae_amd.modules import VQVAE
    conv.set_conv_backend("hip")
    torch.manual_seed(0)
    m = VQVAE(*GP.SMALL, BETA, **kw).to(DEV)
    with torch.no_grad():                                     # codes on the scale of z_e
        for g, w in enumerate(m.vector_quantization.codebooks()):
            w.copy_(torch.randn(w.shape, generator=torch.Generator().manual_seed(g)).to(DEV) * 0.5)
        if "ema_decay" in kw:
            m.vector_quantization.ema_w.copy_(torch.stack([w.detach() for w in m.vector_quantization.codebooks()]))
    return m


@pytest.mark.parametrize("kw", [dict(), dict(ema_decay=0.9)], ids=["plain", "ema"])
def test_model_wire_format(kw):
    from vqvae_amd import conv, functional as F
    m = _model(codebook_groups=2, **kw).train()               # (training mode: encode must not update an EMA codebook)
    vq = m.vector_quantization
    x = torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(1)).to(DEV)
    state = [t.clone() for t in m.state_dict().values()]
    with torch.no_grad():
        code = m.encode(x)
        assert all(_same(a, b) for a, b in zip(state, m.state_dict().values())), "encode() moved the state"
        m.eval()
        z_e = conv.encoder_forward(m.encoder, x, pre_quant=m.pre_quantization_conv)
        loss, z_q, ppl, idx, hist = vq.quantize(z_e, rowmajor=True)
        assert code.shape == (2, 256) and code.dtype == torch.int64 and torch.equal(code, idx)
        el, x_hat, p = m(x)
        got = m.decode_indices(code, 4, 8, 8)
        assert got.shape == (4, 3, 32, 32) and _same(got, x_hat), "decode_indices(encode(x)) is the no-grad x_hat"
        assert p.dim() == 0 and _same(p, ppl.mean()) and _same(el, loss)
        codes = F.vq_grouped_decode(code, [w.detach() for w in vq.codebooks()], 4, 8, 8, rowmajor=True)
        assert _same(got, conv.decoder_forward(m.decoder, codes, rowmajor_in=True))
        assert all(_same(a, b) for a, b in zip(state, m.state_dict().values())), "eval mode moved the state"
        bad = code.clone()
        bad[1, 3] = 64
        with pytest.raises(IndexError):
            m.decode_indices(bad, 4, 8, 8)
        with pytest.raises(ValueError):
            m.decode_indices(code[:1], 4, 8, 8)
        # the quantizer on its own takes NCHW maps and returns the reference's 5-tuple with group 0's one-hot
        out = vq(z_e.permute(0, 3, 1, 2).contiguous())
        assert out[1].shape == (4, 16, 8, 8) and torch.equal(out[4], idx) and out[3].shape == (256, 64)
        assert torch.equal(out[3].argmax(1), idx[0])
        # a codebook written in place re-keys the prepared images; invalidate_caches after a write through .data
        vq.group_embeddings[0].weight.mul_(0.5)
        fresh = F.vq_grouped_forward(z_e, [w.detach() for w in vq.codebooks()], 0.0, rowmajor=True, want_zq=False)[3]
        assert torch.equal(m.encode(x), fresh) and torch.equal(fresh[0], code[0]) and not torch.equal(fresh[1], code[1])
        vq.embedding.weight.data.mul_(-1.0)
        m.invalidate_caches()
        fresh = F.vq_grouped_forward(z_e, [w.detach() for w in vq.codebooks()], 0.0, rowmajor=True, want_zq=False)[3]
        assert torch.equal(m.encode(x), fresh) and not torch.equal(fresh[0], code[0])
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        sd["vector_quantization.embedding.weight"].mul_(-1.0)
        m.load_state_dict(sd)
        assert torch.equal(m.encode(x)[0], code[0])


@pytest.mark.parametrize("kw", [dict(), dict(ema_decay=0.9)], ids=["plain", "ema"])
def test_model_training_step(kw):
    from vqvae_amd import training as T
    m = _model(codebook_groups=2, **kw).train()
    vq = m.vector_quantization
    opt = torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=3e-4, amsgrad=True)
    x = torch.randn(4, 3, 32, 32, generator=torch.Generator().manual_seed(2)).to(DEV)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    seen = {}

    def hook(mod, args, out):
        seen["z_e"], seen["idx"] = args[0].detach().clone(), out[4]
        out[0].register_hook(lambda g: seen.__setitem__("g_loss", g.detach().clone()))
        out[1].register_hook(lambda g: seen.__setitem__("g_zq", g.detach().clone()))

    h = vq.register_forward_hook(hook)
    el, x_hat, p = m(x)
    h.remove()
    assert p.dim() == 0 and seen["z_e"].shape == (4, 8, 8, 16) and seen["idx"].shape == (2, 256)
    stats = T.step_losses(el, x_hat, p, x, 0.06)
    stats[1].backward()
    torch.cuda.synchronize()
    assert torch.isfinite(stats).all()
    for name, prm in m.named_parameters():
        if prm.requires_grad:
            assert prm.grad is not None and torch.isfinite(prm.grad).all(), name
    books = [before["vector_quantization.embedding.weight"], before["vector_quantization.group_embeddings.0.weight"]]
    if kw:
        assert all(w.grad is None for w in vq.codebooks())
        assert all(not _same(w, b) for w, b in zip(vq.codebooks(), books)), "the EMA update moved the codebooks"
        assert not _same(vq.ema_cluster_size, before["vector_quantization.ema_cluster_size"])
    else:
        _, want = T.vq_grouped_backward(seen["z_e"], books, seen["idx"], seen["g_zq"], seen["g_loss"], BETA, rowmajor=True, need_z=False)
        for w, g in zip(vq.codebooks(), want):
            assert _same(w.grad, g) and float(g.abs().max()) > 0
    opt.step()
    torch.cuda.synchronize()
    after = m.state_dict()
    assert not _same(after["encoder.conv_stack.0.weight"], before["encoder.conv_stack.0.weight"])
    assert not _same(after["vector_quantization.embedding.weight"], before["vector_quantization.embedding.weight"])
    assert all(torch.isfinite(v).all() for v in after.values())


@pytest.mark.parametrize("extra", [[], ["--ema_decay", "0.9"]], ids=["plain", "ema"])
def test_train_tool_completes_a_run(tmp_path, extra):
    """tools/train_checkpoint.py --codebook_groups: three updates of a small model, the log lines, the checkpoint and the evaluation
    through the per-layer path (the range guard and the product schemes of the fused whole-path entries do not apply)"""
    from tools import train_checkpoint as tc
    tc.main(["--codebook_groups", "2", "--n_updates", "3", "--batch_size", "8", "--n_train", "64", "--log_interval", "2",
             "--n_hiddens", "32", "--n_residual_hiddens", "8", "--n_residual_layers", "1", "--embedding_dim", "16",
             "--n_embeddings", "64", "--out", str(tmp_path), "--tag", "t"] + extra)
    log = open(tmp_path / "t_log.txt").read()
    assert log.count("Update # ") == 2 and "guard: per-layer path" in log
    assert "# eval[per-layer]" in log and "decode_indices(encode(x)) is x_hat: True" in log
    ck = torch.load(tmp_path / "t.pth", weights_only=False)
    assert ck["hyperparameters"]["codebook_groups"] == 2 and len(ck["results"]["loss_vals"]) == 3
    assert all(np.isfinite(ck["results"]["loss_vals"]))
    assert tuple(ck["model"]["vector_quantization.group_embeddings.0.weight"].shape) == (64, 8)
    assert ("vector_quantization.ema_w" in ck["model"]) == bool(extra)
    assert sorted(np.load(tmp_path / "t_state.npz").files) == sorted(ck["model"])


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


@pytest.mark.parametrize("rowmajor", [False, True])
def test_init_codebook_is_kmeans_slab_by_slab(rowmajor):
    from vqvae_amd import functional as F
    from vqvae_amd.modules import GroupedVectorQuantizer, GroupedVectorQuantizerEMA
    B, H, W, D, K, G, iters = 2, 8, 8, 48, 32, 3, 2
    d = D // G
    rows = np.random.default_rng(9).standard_normal((B * H * W, D)).astype(np.float32)
    z = _layout(rows, B, H, W, rowmajor)
    torch.manual_seed(3)
    for cls in (GroupedVectorQuantizer, GroupedVectorQuantizerEMA):
        vq = cls(G, K, D, BETA).to(DEV).eval()
        vq.quantize(z, rowmajor=rowmajor)                     # a warm module: prepared images of the old codebooks
        out = vq.init_codebook_(z, iters, _gen(5), rowmajor=rowmajor)
        gen = _gen(5)
        for g, w in enumerate(vq.codebooks()):
            want, counts = F.vq_kmeans(_slice(z, g, d, rowmajor), K, iters, generator=gen, rowmajor=rowmajor)
            assert _same(w, want) and torch.equal(out[g][1], counts), f"group {g}"
            if cls is GroupedVectorQuantizerEMA:
                c = counts.to(torch.float32)
                assert _same(vq.ema_cluster_size[g], c) and _same(vq.ema_w[g], c[:, None] * want)
        got = vq.quantize(z, rowmajor=rowmajor)               # the module quantizes against the new codebooks
        ref = F.vq_grouped_forward(z, [w.detach() for w in vq.codebooks()], BETA, rowmajor=rowmajor)
        assert torch.equal(got[3], ref[3]) and _same(got[1], ref[1])


# ---- 7. stream capture -------------------------------------------------------------------------------------------------------------

def test_forward_chain_replays_to_the_eager_bits():
    from vqvae_amd import functional as F
    faulthandler.dump_traceback_later(120, exit=True)        # this test's own time limit: a replay that hangs ends the process
    try:
        K, D, G, B, H, W = 512, 64, 2, 3, 8, 8
        rows, books = _case(K, D, G, B, H, W)
        dbooks = _dev(books)
        static_z = _layout(rows, B, H, W, True)
        ws = F.vq_grouped_workspace(B * H * W, K, D, G, DEV)
        with torch.no_grad():
            cap = GP.Captured(lambda: F.vq_grouped_forward(static_z, dbooks, BETA, rowmajor=True, workspace=ws, want_slabs=True), DEV)
        rng = np.random.default_rng(77)
        # fresh contents: randn, rows next to the first codes, rows next to the last codes (disjoint parts of the histograms)
        sl = GR.slabs(rows, G)
        states = [rng.standard_normal(rows.shape).astype(np.float32)]
        for lo, hi in ((0, K // 4), (K - K // 4, K)):
            states.append(np.concatenate([books[g][rng.integers(lo, hi, len(rows))] + 1e-3 * sl[g] for g in range(G)], axis=1).astype(np.float32))
        for r, st in enumerate(states + states[:1]):
            static_z.copy_(_layout(st, B, H, W, True))
            GP.poison(*cap.out)
            out = cap.replay()
            torch.cuda.synchronize()
            eager = F.vq_grouped_forward(_layout(st, B, H, W, True), dbooks, BETA, rowmajor=True, want_slabs=True)
            torch.cuda.synchronize()
            for name, a, b in zip(("loss", "z_q", "perplexity", "idx", "hist", "loss_group", "slabs"), out, eager):
                assert GP.same_bits(a, b), f"replay {r}: {name} differs in {GP.differing(a, b)} elements"
    finally:
        faulthandler.cancel_dump_traceback_later()


def test_training_forward_with_the_ema_update_replays_to_the_eager_bits():
    from vqvae_amd.modules import GroupedVectorQuantizerEMA
    faulthandler.dump_traceback_later(120, exit=True)
    try:
        K, D, G, B, H, W = 96, 64, 4, 3, 8, 8
        rows, books = _case(K, D, G, B, H, W)
        torch.manual_seed(4)
        vq = GroupedVectorQuantizerEMA(G, K, D, BETA, decay=0.9).to(DEV).train()
        with torch.no_grad():
            for w, E in zip(vq.codebooks(), _dev(books)):
                w.copy_(E)
            vq.ema_w.copy_(torch.stack(_dev(books)))
        twin = copy.deepcopy(vq)
        static_z = _layout(rows, B, H, W, True)
        with torch.no_grad():
            cap = GP.Captured(lambda: vq.quantize(static_z, rowmajor=True), DEV, warmup=GP.N_WARMUP)
            for _ in range(GP.N_WARMUP):                      # the warm-up calls were training forwards: two updates
                twin.quantize(static_z, rowmajor=True)
            rng = np.random.default_rng(78)
            for r in range(4):
                st = (rng.standard_normal(rows.shape) * (0.25 if r % 2 else 1.0)).astype(np.float32)
                static_z.copy_(_layout(st, B, H, W, True))
                GP.poison(*cap.out)
                out = cap.replay()
                torch.cuda.synchronize()
                eager = twin.quantize(_layout(st, B, H, W, True), rowmajor=True)
                torch.cuda.synchronize()
                for name, a, b in zip(("loss", "z_q", "perplexity", "idx", "hist"), out, eager):
                    assert GP.same_bits(a, b), f"replay {r}: {name} differs in {GP.differing(a, b)} elements"
                for (name, a), (_, b) in zip(vq.state_dict().items(), twin.state_dict().items()):
                    assert GP.same_bits(a, b), f"replay {r}: {name} differs in {GP.differing(a, b)} elements"
    finally:
        faulthandler.cancel_dump_traceback_later()


# ---- 8. the envelope ---------------------------------------------------------------------------------------------------------------

def test_envelope_on_the_device():
    """error codes with real device pointers; nothing is launched outside the envelope (the buffers keep their contents)"""
    import ctypes

    from vqvae_amd import _lib
    L = _lib.load()
    z = torch.full((64 * 272,), 3.0, device=DEV)
    out = torch.full((64 * 272,), 5.0, device=DEV)
    big = torch.full((1 << 23,), 7, dtype=torch.uint8, device=DEV)
    cb = torch.full((2, 16384 * 16), 1.0, device=DEV)
    a, o, w = z.data_ptr(), out.data_ptr(), big.data_ptr()
    books = (ctypes.c_void_p * 17)(*([cb[0].data_ptr(), cb[1].data_ptr()] * 8 + [cb[0].data_ptr()]))
    idx, hist, sc = w, w + (1 << 20), w + (2 << 20)
    wsp, nws = w + (3 << 20), 4 << 20
    for D, K, G in ((258, 16, 2), (4, 16385, 2), (4, 16, 0), (4, 16, 17), (6, 16, 4), (64, 16, 3)):
        assert L.vqvae_vq_grouped_workspace_bytes(64, K, D, G) == 0 and L.vqvae_vq_grouped_backward_workspace_bytes(64, K, D, G) == 0
        assert L.vqvae_vq_grouped_forward_f32(a, books, 1, D, 8, 8, K, G, 0.25, 0, o, idx, hist, sc, sc + 64, sc + 128, None, wsp, nws,
                                              None) == _lib.ERR_UNSUPPORTED
        assert L.vqvae_vq_grouped_decode_f32(idx, books, 1, D, 8, 8, K, G, 0, o, None) == _lib.ERR_UNSUPPORTED
        assert L.vqvae_vq_grouped_backward_f32(a, books, idx, None, None, 1, D, 8, 8, K, G, 0.25, 0, o, None, wsp, nws,
                                               None) == _lib.ERR_UNSUPPORTED
    # inside the envelope: alignment and overlap
    D, K, G = 64, 16, 2
    assert L.vqvae_vq_grouped_workspace_bytes(64, K, D, G) <= nws

    def fwd(z=a, zq=o, idx=idx, ws=wsp):
        return L.vqvae_vq_grouped_forward_f32(z, books, 1, D, 8, 8, K, G, 0.25, 0, zq, idx, hist, sc, sc + 64, sc + 128, None, ws, nws, None)
    assert fwd(z=a + 2) == _lib.ERR_UNSUPPORTED and fwd(zq=o + 1) == _lib.ERR_UNSUPPORTED and fwd(idx=idx + 4) == _lib.ERR_UNSUPPORTED
    assert fwd(ws=wsp + 4) == _lib.ERR_UNSUPPORTED
    assert fwd(zq=a) == _lib.ERR_UNSUPPORTED and fwd(zq=a + 128) == _lib.ERR_UNSUPPORTED and fwd(zq=cb[1].data_ptr()) == _lib.ERR_UNSUPPORTED
    assert L.vqvae_vq_grouped_decode_f32(idx, books, 1, D, 8, 8, K, G, 0, cb[0].data_ptr(), None) == _lib.ERR_UNSUPPORTED
    assert L.vqvae_vq_grouped_backward_f32(a, books, idx, None, None, 1, D, 8, 8, K, G, 0.25, 0, a, None, wsp, nws, None) == _lib.ERR_UNSUPPORTED
    assert L.vqvae_vq_grouped_backward_f32(a, books, idx, None, None, 1, D, 8, 8, K, G, 0.25, 0x800, o, books, wsp, nws, None) == _lib.ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((z == 3.0).all()) and bool((out == 5.0).all()) and bool((big == 7).all()) and bool((cb == 1.0).all())
    # ... and the same arguments, aligned and apart, run
    assert fwd() == 0
    torch.cuda.synchronize()
    assert bool((out[:64 * 64] == 3.0 + (1.0 - 3.0)).all())
