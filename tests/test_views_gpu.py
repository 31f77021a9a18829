"""GPU tests: the front end on views.  Every call runs once on fresh dense tensors and again with tensor arguments replaced by
views holding the same values -- each argument in turn, then all together; parameters and in-place state included -- and every
output and every in-place result must have the same bits ("Pointer contract"; profiles/pointer_contract.md).

Three kinds of view:
  displaced   a dense view one element into a larger allocation: data_ptr() % 16 == 4 (8 for int64 / fp64), contiguous
  strided     channels_last for a 4-D map with more than one channel and pixel, else every second column of a buffer twice as
              wide; `expand` for an upstream gradient
  permuted    a buffer laid out with two dimensions exchanged (a (D, K) buffer behind a (K, D) table)

A strided or permuted view reaches its entry as a dense copy.  A displaced view reaches the entry itself wherever the entry is
classed narrow or element in profiles/pointer_contract.md (the front end passes `_lib.dense` the entry's own alignment), so
these tests run the element-wise forms on the device: the quantizer backward's grad_z and rotation kernels, both any-width
quantizer kernels, the k-means seeding, the residual advance / finish / grad_z kernels, conv_in's gather kernel,
vqvae_bias_grad_f32's four-float loads, and every element-class entry on 4-byte (8-byte for int64 / fp64) aligned pointers.
Only the refusing entries get a copy.  None of these forms adds in another order than its wide one -- each thread computes the
same elements from the same values -- so no call is compared under a bound: the requirement is bits throughout.
"""
import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BETA = 0.25


# ------------------------------------------------------------------------------------------------------------------ the views
def displaced(t):
    """the same values one element into a larger allocation"""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == (8 if t.element_size() == 8 else 4)
    return v


def strided(t):
    """the same values behind strides no dense tensor has"""
    wide = [d for d in range(t.dim()) if t.shape[d] > 1]
    if t.dim() == 4 and t.shape[1] > 1 and t.shape[2] * t.shape[3] > 1:
        v = torch.empty_like(t, memory_format=torch.channels_last)
    elif not wide:
        v = torch.empty(2, dtype=t.dtype, device=t.device)[::2].view(t.shape)    # (one element: nothing to stride; a fresh tensor)
    else:
        d = wide[-1]                                                             # every second column of a buffer twice as wide
        shape = list(t.shape)
        shape[d] *= 2
        v = torch.empty(shape, dtype=t.dtype, device=t.device)[(slice(None),) * d + (slice(None, None, 2),)]
    v.copy_(t)
    assert v.shape == t.shape and (not wide or not v.is_contiguous())
    return v


def expanded(t):
    """an upstream gradient as z_q.sum().backward() hands it over: one element, every stride zero"""
    v = t.flatten()[:1].clone().view([1] * t.dim()).expand(t.shape)
    return v


def permuted(t):
    """the same values in a buffer whose last two dimensions (of size > 1) are laid out exchanged"""
    wide = [d for d in range(t.dim()) if t.shape[d] > 1]
    if len(wide) < 2:
        return strided(t)
    a, b = wide[-2], wide[-1]
    v = torch.empty_like(t.transpose(a, b), memory_format=torch.contiguous_format).transpose(a, b)
    v.copy_(t)
    assert v.shape == t.shape and not v.is_contiguous()
    return v


def _none(*_):
    return None


KINDS = {"displaced": displaced, "strided": strided, "permuted": permuted}


def same_bits(a, b, what):
    if a is None or b is None:
        assert a is None and b is None, what
        return
    if isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            same_bits(x, y, f"{what}[{i}]")
        return
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {tuple(a.shape)} {a.dtype} against {tuple(b.shape)} {b.dtype}"
    x, y = a.detach().contiguous().view(-1).view(torch.uint8), b.detach().contiguous().view(-1).view(torch.uint8)
    assert torch.equal(x, y), f"{what}: bits differ"


def check_views(fn, tensors, inplace=(), kinds=KINDS, what=""):
    """fn(**tensors) on fresh dense clones, then with each tensor in turn, and all of them, replaced by a view of each kind.
    Outputs, and the final values of the tensors named in `inplace`, must not differ in a bit."""
    def run(make):
        args = {k: (make[k](v.clone()) if k in make else v.clone()) for k, v in tensors.items()}
        ptrs = {k: args[k].data_ptr() for k in inplace}
        out = fn(**args)
        torch.cuda.synchronize()
        for k in inplace:
            assert args[k].data_ptr() == ptrs[k], f"{what}: {k} changed its storage"
        return out, [args[k].clone() for k in inplace]

    base = run({})
    for kind, make in kinds.items():
        for sel in [(k,) for k in tensors] + [tuple(tensors)]:
            got = run({k: make for k in sel})
            where = f"{what} {kind} {'+'.join(sel)}"
            same_bits(got[0], base[0], where)
            same_bits(got[1], base[1], where + " (in place)")
    return base


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _vq_case(K, D, B, H, W, rowmajor, seed=0):
    """rows near codes and a duplicated code, as tests/test_state_gpu.py builds them"""
    g = _gen(1000 * K + D + seed)
    cb = torch.randn(K, D, device=DEV, generator=g)
    if K > 3:
        cb[K // 2] = cb[1]
    n = B * H * W
    z = cb[torch.randint(0, K, (n,), device=DEV, generator=g)] + 0.1 * torch.randn(n, D, device=DEV, generator=g)
    z = z.view(B, H, W, D)
    return (z if rowmajor else z.permute(0, 3, 1, 2)).contiguous(), cb


# -------------------------------------------------------------------------------------------------------- quantizer forward
VQ_ROUTES = [(512, 64), (96, 64), (1024, 64), (2048, 128), (100, 32), (64, 256), (64, 48), (5, 3)]
VQ_MAPS = [(3, 8, 8), (5, 4, 8), (2, 3, 5)]


@pytest.mark.parametrize("rowmajor", [False, True], ids=["nchw", "rows"])
@pytest.mark.parametrize("B,H,W", VQ_MAPS)
@pytest.mark.parametrize("K,D", VQ_ROUTES)
def test_vq_forward(K, D, B, H, W, rowmajor):
    """every route of vqvae_vq_forward_f32, with and without z_q, on a fresh workspace and on one a dense call prepared"""
    from vqvae_amd import functional as F
    z, cb = _vq_case(K, D, B, H, W, rowmajor)
    for want_zq in (True, False):
        check_views(lambda z_e, codebook: F.vq_forward(z_e, codebook, BETA, rowmajor=rowmajor, want_zq=want_zq),
                    dict(z_e=z, codebook=cb), what=f"K={K} D={D} want_zq={want_zq}")
    ws = F.vq_workspace(K, D, DEV)
    F.vq_forward(z, cb, BETA, rowmajor=rowmajor, workspace=ws)
    check_views(lambda z_e, codebook: F.vq_forward(z_e, codebook, BETA, rowmajor=rowmajor, workspace=ws, prepared=True),
                dict(z_e=z, codebook=cb), what=f"K={K} D={D} prepared")


@pytest.mark.parametrize("rowmajor,kw", [(rm, kw) for kw in (dict(exact_sweep=True), dict(bf16_filter=True)) for rm in (False, True)] +
                         [(True, dict(form=8)), (True, dict(form=16))],          # (the launch forms are forced on row-major rows)
                         ids=lambda v: ("rows" if v else "nchw") if isinstance(v, bool) else "-".join(f"{k}{x}" for k, x in v.items()))
def test_vq_forward_forced_kernels(rowmajor, kw):
    from vqvae_amd import functional as F
    z, cb = _vq_case(512, 64, 3, 8, 8, rowmajor)
    check_views(lambda z_e, codebook: F.vq_forward(z_e, codebook, BETA, rowmajor=rowmajor, **kw), dict(z_e=z, codebook=cb), what=str(kw))


@pytest.mark.parametrize("rowmajor", [False, True], ids=["nchw", "rows"])
@pytest.mark.parametrize("K,D,B,H,W", [(64, 48, 3, 8, 8), (33, 12, 2, 3, 5), (5, 3, 2, 3, 5)])
def test_vq_forward_vector_unit_kernel(K, D, B, H, W, rowmajor):
    """vq_generic_kernel (bf16_filter at a width outside 32 / 64 / 128 / 256): its four-wide form reads the codebook and, on row-major
    rows, z_e 16 bytes at a time, so a displaced view of either takes the element form -- on the device, with the same bits"""
    from vqvae_amd import functional as F
    z, cb = _vq_case(K, D, B, H, W, rowmajor)
    check_views(lambda z_e, codebook: F.vq_forward(z_e, codebook, BETA, rowmajor=rowmajor, bf16_filter=True), dict(z_e=z, codebook=cb),
                what=f"K={K} D={D}")


# ----------------------------------------------------------------------------------------------- quantizer backward and state
STATE_SHAPES = [(96, 64, 3, 8, 8), (5, 3, 2, 3, 5)]


def _state_case(K, D, B, H, W, rowmajor):
    from vqvae_amd import functional as F
    z, cb = _vq_case(K, D, B, H, W, rowmajor, seed=7)
    idx = F.vq_forward(z, cb, BETA, rowmajor=rowmajor, want_zq=False)[3]
    return z, cb, idx


@pytest.mark.parametrize("rowmajor", [False, True], ids=["nchw", "rows"])
@pytest.mark.parametrize("K,D,B,H,W", STATE_SHAPES)
def test_vq_backward(K, D, B, H, W, rowmajor):
    from vqvae_amd import training as T
    z, cb, idx = _state_case(K, D, B, H, W, rowmajor)
    g = _gen(3)
    gzq, gl = torch.randn(z.shape, device=DEV, generator=g), torch.tensor(0.7, device=DEV)
    t = dict(z_e=z, codebook=cb, idx=idx, grad_zq=gzq, grad_loss=gl)
    check_views(lambda **a: T.vq_backward(a["z_e"], a["codebook"], a["idx"], a["grad_zq"], a["grad_loss"], BETA, rowmajor=rowmajor), t,
                what="plain")
    check_views(lambda **a: T.vq_backward(a["z_e"], a["codebook"], a["idx"], a["grad_zq"], a["grad_loss"], BETA, rowmajor=rowmajor,
                                          need_codebook=False, commitment=True), t, what="commitment")
    check_views(lambda **a: T.vq_backward(a["z_e"], a["codebook"], a["idx"], a["grad_zq"], a["grad_loss"], BETA, rowmajor=rowmajor,
                                          rotation=True), t, what="rotation")
    # the gradient z_q.sum().backward() produces: one element expanded over the map
    dense = T.vq_backward(z, cb, idx, torch.ones_like(z), gl, BETA, rowmajor=rowmajor)
    got = T.vq_backward(z, cb, idx, expanded(torch.ones_like(z)), gl, BETA, rowmajor=rowmajor)
    same_bits(got, dense, "expanded grad_zq")


@pytest.mark.parametrize("rowmajor", [False, True], ids=["nchw", "rows"])
@pytest.mark.parametrize("K,D,B,H,W", STATE_SHAPES)
def test_vq_ema_and_kmeans_state(K, D, B, H, W, rowmajor):
    """the entries that write caller state in place: the state keeps its storage and ends with the dense call's bits"""
    from vqvae_amd import functional as F
    z, cb, idx = _state_case(K, D, B, H, W, rowmajor)
    g = _gen(5)
    cs, ew = torch.rand(K, device=DEV, generator=g) * 3, torch.randn(K, D, device=DEV, generator=g)
    u = torch.rand(K, device=DEV, generator=g)
    state = ("ema_cluster_size", "ema_w", "codebook")
    t = dict(z_e=z, idx=idx, ema_cluster_size=cs, ema_w=ew, codebook=cb)
    check_views(lambda **a: _none(F.vq_ema_update(a["z_e"], a["idx"], a["ema_cluster_size"], a["ema_w"], a["codebook"], 0.9,
                                                  rowmajor=rowmajor)), t, inplace=state, what="ema_update")
    check_views(lambda uniforms, **a: _none(F.vq_ema_update(a["z_e"], a["idx"], a["ema_cluster_size"], a["ema_w"], a["codebook"], 0.9,
                                                            threshold=1.0, uniforms=uniforms, rowmajor=rowmajor)),
                dict(t, uniforms=u), inplace=state, what="ema_update restart")
    # statistics and their application
    check_views(lambda z_e, idx, row_uniforms: F.vq_ema_stats(z_e, idx, K, row_uniforms=row_uniforms, rowmajor=rowmajor),
                dict(z_e=z, idx=idx, row_uniforms=u), what="ema_stats")
    C = 2 * D + 1
    check_views(lambda z_e, idx, row_uniforms, out: _none(F.vq_ema_stats(z_e, idx, K, row_uniforms=row_uniforms, rowmajor=rowmajor, out=out)),
                dict(z_e=z, idx=idx, row_uniforms=u, out=torch.zeros(K, C, dtype=torch.float64, device=DEV)), inplace=("out",),
                what="ema_stats out=")
    stats = torch.stack([F.vq_ema_stats(z, idx, K, row_uniforms=u, rowmajor=rowmajor)] * 2)
    check_views(lambda stats, shard_uniforms, **a: _none(F.vq_ema_apply(stats, a["ema_cluster_size"], a["ema_w"], a["codebook"], 0.9,
                                                                        threshold=1.0, shard_uniforms=shard_uniforms)),
                dict(stats=stats, shard_uniforms=u, ema_cluster_size=cs, ema_w=ew, codebook=cb), inplace=state, what="ema_apply")
    # k-means
    check_views(lambda z_e, uniforms: F.vq_kmeans_seed(z_e, K, uniforms, rowmajor=rowmajor), dict(z_e=z, uniforms=u), what="kmeans_seed")
    check_views(lambda z_e, idx, codebook, uniforms: F.vq_kmeans_update(z_e, idx, codebook, uniforms=uniforms, rowmajor=rowmajor),
                dict(z_e=z, idx=idx, codebook=cb, uniforms=u), inplace=("codebook",), what="kmeans_update")


def test_in_place_state_keeps_identity_and_moves_its_version():
    """state behind strides is computed in a dense temporary and copied back (copy_: the version moves); displaced state is 4-byte
    aligned, which is all the element-wise EMA kernels ask, and is written where it lies.  Either way the caller's tensors keep
    their storage and end with the dense call's bits."""
    from vqvae_amd import functional as F
    K, D = 96, 64
    z, cb, idx = _state_case(K, D, 3, 8, 8, True)
    want = [torch.ones(K, device=DEV), torch.zeros(K, D, device=DEV), cb.clone()]
    F.vq_ema_update(z, idx, *want, 0.9, rowmajor=True)
    for make, copied in ((strided, True), (displaced, False)):
        cs, ew, cbv = make(torch.ones(K, device=DEV)), make(torch.zeros(K, D, device=DEV)), make(cb)
        before = [(t.data_ptr(), t._version) for t in (cs, ew, cbv)]
        out = F.vq_ema_update(z, idx, cs, ew, cbv, 0.9, rowmajor=True)
        torch.cuda.synchronize()
        assert out is cbv
        for t, (p, v), w in zip((cs, ew, cbv), before, want):
            assert t.data_ptr() == p and (t._version > v) == copied
            same_bits(t, w, f"{make.__name__} state")


@pytest.mark.parametrize("K,D,B,H,W", STATE_SHAPES)
def test_onehot_decode_l2norm(K, D, B, H, W):
    from vqvae_amd import functional as F
    z, cb, idx = _state_case(K, D, B, H, W, False)
    check_views(lambda idx: F.vq_onehot(idx, K), dict(idx=idx), what="onehot")
    check_views(lambda idx, codebook: F.vq_decode_indices(idx, codebook, B, H, W), dict(idx=idx, codebook=cb), what="decode")
    for rowmajor in (False, True):
        x = z if not rowmajor else z.permute(0, 2, 3, 1).contiguous()
        y, denom = check_views(lambda x: F.l2norm_rows(x, rowmajor=rowmajor), dict(x=x), what="l2norm")[0]
        gy = torch.randn(x.shape, device=DEV, generator=_gen(9))
        check_views(lambda y, denom, grad_y: F.l2norm_rows_backward(y, denom, grad_y, rowmajor=rowmajor),
                    dict(y=y, denom=denom, grad_y=gy), what="l2norm backward")
    check_views(lambda x: F.l2norm_rows(x), dict(x=cb), what="l2norm of a codebook")


@pytest.mark.parametrize("shared", [False, True], ids=["own", "shared"])
@pytest.mark.parametrize("rowmajor", [False, True], ids=["nchw", "rows"])
@pytest.mark.parametrize("K,D,B,H,W", STATE_SHAPES)
def test_vq_residual(K, D, B, H, W, rowmajor, shared):
    from vqvae_amd import functional as F, training as T
    z, cb, _ = _state_case(K, D, B, H, W, rowmajor)
    cb1 = 0.3 * torch.randn(K, D, device=DEV, generator=_gen(11))
    books = dict(b0=cb) if shared else dict(b0=cb, b1=cb1)
    kw = dict(rowmajor=rowmajor, shared=shared)

    def fwd(z_e, **b):
        return F.vq_residual_forward(z_e, list(b.values()), BETA, n_q=2, want_residual=True, **kw)
    base = check_views(fwd, dict(z_e=z, **books), what="residual forward")[0]
    idx = base[3]
    check_views(lambda idx, **b: F.vq_residual_decode(idx, list(b.values()) * (2 if shared else 1), B, H, W, **kw),
                dict(idx=idx, **books), what="residual decode")
    gzq, gl = torch.randn(z.shape, device=DEV, generator=_gen(13)), torch.tensor(0.7, device=DEV)
    check_views(lambda z_e, idx, grad_zq, grad_loss, **b: T.vq_residual_backward(z_e, list(b.values()) * (2 if shared else 1), idx, grad_zq,
                                                                               grad_loss, BETA, **kw),
                dict(z_e=z, idx=idx, grad_zq=gzq, grad_loss=gl, **books), what="residual backward")


# --------------------------------------------------------------------------------------------------------------------- convs
CONV_KINDS = {   # the smallest case of every kind of tests/test_conv_gpu.py's CONV_CASES: kind, ctor, B, Cin, Cout, H, W
    "conv4x4s2": (0, lambda ci, co: nn.Conv2d(ci, co, 4, 2, 1), 2, 32, 64, 12, 20),
    "conv3x3": (1, lambda ci, co: nn.Conv2d(ci, co, 3, 1, 1), 1, 16, 48, 5, 5),
    "conv1x1": (2, lambda ci, co: nn.Conv2d(ci, co, 1, 1), 2, 32, 128, 8, 8),
    "convT3x3": (3, lambda ci, co: nn.ConvTranspose2d(ci, co, 3, 1, 1), 2, 128, 96, 6, 10),
    "convT4x4s2": (4, lambda ci, co: nn.ConvTranspose2d(ci, co, 4, 2, 1), 2, 64, 32, 5, 7),
}


def _module_on(ctor, weight, bias):
    """a fresh module whose parameters ARE the given tensors (views included)"""
    m = ctor().to(DEV)
    m.weight = nn.Parameter(weight)
    if bias is not None:
        m.bias = nn.Parameter(bias)
    assert m.weight.data_ptr() == weight.data_ptr()
    return m


@pytest.mark.parametrize("name", list(CONV_KINDS))
def test_conv_kinds(name):
    from vqvae_amd import conv_hip
    kind, ctor, B, Cin, Cout, H, W = CONV_KINDS[name]
    torch.manual_seed(Cin + Cout)
    ref = ctor(Cin, Cout)
    x = torch.randn(B, H, W, Cin, device=DEV, generator=_gen(1))

    def run(x, weight, bias):
        m = _module_on(lambda: ctor(Cin, Cout), weight, bias)
        return conv_hip.conv(kind, x, m, m.weight, m.bias, Cin, Cout, 2)
    check_views(run, dict(x=x, weight=ref.weight.detach().to(DEV), bias=ref.bias.detach().to(DEV)), what=name)


def test_conv_epilogue_addend_and_mask():
    """the data-gradient form: y = (mask > 0) ? conv + addend : 0, in the kernel's epilogue and in the two-pass form"""
    from vqvae_amd import conv_hip
    for (kind, ctor, B, Cin, Cout, H, W) in (CONV_KINDS["conv1x1"], CONV_KINDS["conv3x3"]):
        torch.manual_seed(3)
        ref = ctor(Cin, Cout)
        g = _gen(17)
        x = torch.randn(B, H, W, Cin, device=DEV, generator=g)
        addend = torch.randn(B, H, W, Cout, device=DEV, generator=g)
        mask = torch.randn(B, H, W, Cout, device=DEV, generator=g)

        def run(x, weight, addend, mask):
            m = _module_on(lambda: ctor(Cin, Cout), weight, None)
            return conv_hip.conv(kind, x, m, m.weight, None, Cin, Cout, 0, addend=addend, mask=mask)
        check_views(run, dict(x=x, weight=ref.weight.detach().to(DEV), addend=addend, mask=mask), what=f"kind {kind}")


def test_conv_in_and_convt_out():
    """vqvae_conv_in_forward_f32 and vqvae_convt_out_forward_f32 behind encoder_forward / decoder_forward, on NCHW images and rows"""
    from vqvae_amd import conv_hip
    from vqvae_amd.modules import Decoder, Encoder
    torch.manual_seed(5)
    enc, dec = Encoder(3, 32, 1, 8).to(DEV).eval(), Decoder(64, 32, 1, 8).to(DEV).eval()
    x = torch.randn(3, 3, 16, 12, device=DEV, generator=_gen(19))
    zq = torch.randn(3, 64, 4, 3, device=DEV, generator=_gen(21))
    with torch.no_grad():
        check_views(lambda x: conv_hip.encoder_forward(enc, x, None), dict(x=x), what="encoder")
        check_views(lambda z_q: conv_hip.decoder_forward(dec, z_q, False), dict(z_q=zq), what="decoder")
        check_views(lambda z_q: conv_hip.decoder_forward(dec, z_q, True), dict(z_q=zq.permute(0, 2, 3, 1).contiguous()), what="decoder rows")
        check_views(lambda x: conv_hip.residual_stack_nchw(x, list(enc.conv_stack[5].stack), True),
                    dict(x=torch.randn(2, 32, 5, 7, device=DEV, generator=_gen(23))), what="residual stack")


@pytest.mark.parametrize("C,Rh,H,W,hidden", [(128, 32, 8, 8, True), (64, 32, 5, 7, False), (96, 48, 6, 6, False)],
                         ids=["fused-hidden-8x8", "fused", "through-ws"])
def test_res_layer(C, Rh, H, W, hidden):
    from vqvae_amd import conv_hip
    from vqvae_amd.modules import ResidualLayer
    torch.manual_seed(C)
    layer = ResidualLayer(C, C, Rh).to(DEV)
    x = torch.randn(3, H, W, C, device=DEV, generator=_gen(C))
    check_views(lambda x: conv_hip.res_layer(x, layer, 3, want_hidden=hidden), dict(x=x), what=f"C={C} Rh={Rh}")


def test_transpose_and_conv_taps():
    from vqvae_amd import conv_hip, pixelcnn
    x = torch.randn(3, 17, 9, device=DEV, generator=_gen(29))
    check_views(lambda x: conv_hip.transpose(x, 3, 17, 9), dict(x=x), what="transpose")
    # a masked 3x3 stack as the prior builds it: five taps, and the data gradient with an addend in its epilogue
    taps = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 0)]
    Cin, Cout = 16, 32
    g = _gen(31)
    xr = torch.randn(2, 6, 6, Cin, device=DEV, generator=g)
    w = torch.randn(Cout, Cin, 1, 5, device=DEV, generator=g)
    b = torch.randn(Cout, device=DEV, generator=g)

    def fwd(x, weight, bias):
        return conv_hip.conv_taps(x, nn.Identity(), weight, bias, taps)
    check_views(fwd, dict(x=xr, weight=w, bias=b), what="conv_taps")
    gy = torch.randn(2, 6, 6, Cout, device=DEV, generator=g)
    addend = torch.randn(2, 6, 6, Cin, device=DEV, generator=g)
    check_views(lambda gy, weight, addend: pixelcnn.taps_dgrad(gy, nn.Identity(), weight, taps, addend=addend),
                dict(gy=gy, weight=w, addend=addend), what="taps_dgrad with an addend")
    check_views(lambda gy, x: pixelcnn.taps_wgrad(gy, x, taps), dict(gy=gy, x=xr), what="taps_wgrad")


# ------------------------------------------------------------------------------------------------------- training reductions
def test_recon_loss_on_a_batch_slice():
    """(5, 3, 17, 9): 459 floats per image, so x_all[1:] is dense and starts 12 bytes past a 16-byte line"""
    from vqvae_amd import training as T
    g = _gen(37)
    x_all, xh_all = torch.randn(6, 3, 17, 9, device=DEV, generator=g), torch.randn(6, 3, 17, 9, device=DEV, generator=g)
    el, pp = torch.tensor(0.3, device=DEV), torch.tensor(41.0, device=DEV)

    def run(x_hat, x, embedding_loss, perplexity):
        xh = x_hat.requires_grad_(True)
        stats = T.step_losses(embedding_loss, xh, perplexity, x, 0.06)
        stats[1].backward()
        return stats, xh.grad
    base = check_views(run, dict(x_hat=xh_all[1:], x=x_all[1:], embedding_loss=el, perplexity=pp), what="step_losses")[0]
    xs, xhs = x_all[1:], xh_all[1:]                                             # the slices themselves
    assert xs.is_contiguous() and xs.data_ptr() % 16 == 12 and xhs.data_ptr() % 16 == 12
    same_bits(run(xhs, xs, el, pp), base, "x_all[1:]")


@pytest.mark.parametrize("C", [32, 3])
def test_bias_grad_both_layouts(C):
    """C = 32 on row-major rows is the four-channels-per-thread form, whose under-aligned variant loads element by element in the
    same order: displaced views reach the kernel as they are"""
    from vqvae_amd import autograd_conv as A, pixelcnn
    g = torch.randn(5, 7, 9, C, device=DEV, generator=_gen(41))
    check_views(lambda g: A.bias_grad(g), dict(g=g), what="rows")
    check_views(lambda g: A.bias_grad(g, nchw=True), dict(g=g.permute(0, 3, 1, 2).contiguous()), what="nchw")
    check_views(lambda g: pixelcnn.bias_grad(g), dict(g=g), what="wide")


def test_conv_wgrad_and_relu_backward():
    from vqvae_amd import autograd_conv as A
    g = _gen(43)
    for (B, H, W, CA, CB, k) in ((3, 8, 8, 64, 64, 3), (2, 5, 7, 12, 20, 3)):          # map-resident 8x8; generic
        a, bt = torch.randn(B, H, W, CA, device=DEV, generator=g), torch.randn(B, H, W, CB, device=DEV, generator=g)
        check_views(lambda a_rows, bt: A.conv_wgrad(a_rows, bt, k, 1, 1), dict(a_rows=a, bt=bt), what=f"wgrad CA={CA}")
    gy, y = torch.randn(3, 5, 7, 9, device=DEV, generator=g), torch.randn(3, 5, 7, 9, device=DEV, generator=g)
    check_views(lambda g, y: A.relu_backward(g, y), dict(g=gy, y=y), what="relu_backward")


# --------------------------------------------------------------------------------------------------------------------- prior
def test_prior_kernels():
    from vqvae_amd import pixelcnn as P
    g = _gen(47)
    K, dim, n = 64, 16, 2 * 6 * 6
    table = torch.randn(K, dim, device=DEV, generator=g)
    idx = torch.randint(0, K, (n,), device=DEV, generator=g)
    check_views(lambda idx, table: P._gather_rows(idx, table), dict(idx=idx, table=table), what="gather_rows")
    check_views(lambda idx, g: P.gather_rows_backward(idx, g, K), dict(idx=idx, g=torch.randn(n, dim, device=DEV, generator=g)),
                what="gather_rows backward")
    t1 = torch.randn(2, 6, 6, 2 * dim, device=DEV, generator=g)
    t2 = torch.randn(2, 6, 6, 2 * dim, device=DEV, generator=g)
    cond = torch.randn(2, 2 * dim, device=DEV, generator=g)
    check_views(lambda t1, t2, cond: P._gate(t1, t2, cond, dim), dict(t1=t1, t2=t2, cond=cond), what="gate")
    go = torch.randn(2, 6, 6, dim, device=DEV, generator=g)

    def gate_bwd(t1, cond, go):
        gcond = torch.empty(2, 2 * dim, device=DEV)
        return P.gate_backward(t1, cond, go, dim, gcond), gcond
    check_views(gate_bwd, dict(t1=t1, cond=cond, go=go), what="gate backward")
    logits = torch.randn(2, K, 6, 6, device=DEV, generator=g)
    x = idx.view(2, 6, 6)

    def ce(logits, x):
        lg = logits.requires_grad_(True)
        loss = P.cross_entropy(lg, x)
        loss.backward()
        return loss, lg.grad
    check_views(ce, dict(logits=logits, x=x), what="cross_entropy")


# ------------------------------------------------------------------------------------------------ whole models on a flat buffer
def flatten_(model, grads=False):
    """Re-point every parameter and buffer of `model` at a view of one flat buffer per dtype -- consecutive views from element 1,
    no padding between them, the layout tests/test_optim_gpu.py's Flat builds -- and, with grads, every .grad at a view of a
    second one.  -> the tensors by name."""
    named = dict(model.named_parameters())
    named.update(dict(model.named_buffers()))
    by_dtype = {}
    for n, t in named.items():
        by_dtype.setdefault(t.dtype, []).append((n, t))
    for dtype, items in by_dtype.items():
        total = sum(t.numel() for _, t in items)
        flat = torch.empty(total + 1, dtype=dtype, device=DEV)
        gflat = torch.zeros(total + 1, dtype=dtype, device=DEV) if grads and dtype == torch.float32 else None
        off = 1
        for n, t in items:
            v = flat[off:off + t.numel()].view(t.shape)
            v.copy_(t.detach())
            t.data = v
            if gflat is not None and isinstance(t, nn.Parameter) and t.requires_grad:
                t.grad = gflat[off:off + t.numel()].view(t.shape)
            off += t.numel()
    if hasattr(model, "invalidate_caches"):
        model.invalidate_caches()
    return named


def _vqvae(variant, big=False):
    from vqvae_amd.modules import VQVAE
    torch.manual_seed(11)
    if big:
        return VQVAE(128, 32, 2, 512, 64, 0.25).to(DEV)
    return VQVAE(32, 8, 1, 64, 64, 0.25, **variant).to(DEV)


VARIANTS = {
    "plain": dict(),
    "ema": dict(ema_decay=0.9, restart_threshold=1.0),
    "residual": dict(n_quantizers=2),
    "grouped": dict(codebook_groups=2),
    "cosine-rotation-factorized": dict(cosine_sim=True, rotation_trick=True, codebook_dim=16),
    "lookup_free": dict(lookup_free=True),
}


def _misaligned(named):
    return [n for n, t in named.items() if t.data_ptr() % 16]


def _model_pair(make):
    from vqvae_amd import conv
    conv.set_conv_backend("hip")
    a, b = make(), make()
    for (n1, t1), (n2, t2) in zip(a.state_dict().items(), b.state_dict().items()):
        assert n1 == n2 and torch.equal(t1, t2)
    for p in a.parameters():                                                   # (both models add their gradients to zeros: a sum
        if p.requires_grad:                                                    # onto +0 turns a -0 into +0, bit 31 of a comparison)
            p.grad = torch.zeros_like(p)
    named = flatten_(b, grads=True)
    bad = _misaligned(named)
    assert sum(n.endswith("bias") for n in bad) >= 3 and any(n.endswith("weight") and named[n].dim() == 4 for n in bad), bad
    for (n1, t1), (n2, t2) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.equal(t1, t2), n1
    return a, b, named


def _compare_models(a, b, x, steps=2):
    from vqvae_amd import training as T
    from vqvae_amd.optim import Adam
    a.eval(), b.eval()
    with torch.no_grad():
        same_bits(list(a(x)), list(b(x)), "eval forward")
        ia, ib = a.encode(x), b.encode(x)
        same_bits(ia, ib, "encode")
        h, w = x.shape[2] // 4, x.shape[3] // 4
        same_bits(a.decode_indices(ia, x.shape[0], h, w), b.decode_indices(ib, x.shape[0], h, w), "decode_indices")
    a.train(), b.train()
    opts = [Adam(m.parameters(), lr=3e-4) for m in (a, b)]
    for step in range(steps):
        for m, opt in ((a, opts[0]), (b, opts[1])):
            torch.manual_seed(100 + step)                                        # (the restart's uniforms: the same for both models)
            opt.zero_grad(set_to_none=False)
            el, xh, pp = m(x)
            T.step_losses(el, xh, pp, x, 0.06)[1].backward()
        torch.cuda.synchronize()
        for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
            same_bits(p.grad, q.grad, f"step {step}: grad of {n}")
        for opt in opts:
            opt.step()
        torch.cuda.synchronize()
        for (n, p), (_, q) in zip(a.state_dict().items(), b.state_dict().items()):
            same_bits(p, q, f"after step {step}: {n}")


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_small_vqvae_on_a_flat_buffer(variant):
    a, b, named = _model_pair(lambda: _vqvae(VARIANTS[variant]))
    if variant != "lookup_free":
        assert any("embedding" in n or "codebook" in n for n in _misaligned(named)), _misaligned(named)
    x = torch.randn(4, 3, 32, 32, device=DEV, generator=_gen(53))
    _compare_models(a, b, x)


def test_default_vqvae_on_a_flat_buffer():
    """VQVAE(128, 32, 2, 512, 64): the fused whole-path kernels and the quantizer inside the encoder's last kernel"""
    a, b, named = _model_pair(lambda: _vqvae(None, big=True))
    assert "vector_quantization.embedding.weight" in _misaligned(named)
    x = torch.randn(5, 3, 32, 32, device=DEV, generator=_gen(59))
    _compare_models(a, b, x)


def test_prior_on_a_flat_buffer():
    """the smallest GatedPixelCNN of tests/test_pixelcnn_train_gpu.py: one training step (every gradient, two optimizer steps) and
    one cached sample with views for label and uniforms"""
    from vqvae_amd import pixelcnn as P
    from vqvae_amd.optim import Adam
    K, dim, nl, ncls, B, H, W = 64, 32, 3, 5, 3, 6, 6

    def make():
        torch.manual_seed(0)
        return P.GatedPixelCNN(K, dim, nl, ncls).to(DEV).train()
    a, b = make(), make()
    for p in a.parameters():
        p.grad = torch.zeros_like(p)
    named = flatten_(b, grads=True)
    assert "embedding.weight" in _misaligned(named) and sum(n.endswith("bias") for n in _misaligned(named)) >= 3
    g = _gen(79)
    x, label = torch.randint(0, K, (B, H, W), device=DEV, generator=g), torch.randint(0, ncls, (B,), device=DEV, generator=g)
    opts = [Adam(m.parameters(), lr=3e-4) for m in (a, b)]
    for step in range(2):
        losses = []
        for m, opt, view in ((a, opts[0], lambda t: t), (b, opts[1], displaced)):
            opt.zero_grad(set_to_none=False)
            loss = P.cross_entropy(m(view(x), view(label)), view(x))
            loss.backward()
            losses.append(loss.detach())
        torch.cuda.synchronize()
        same_bits(losses[0], losses[1], f"step {step}: loss")
        for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
            same_bits(p.grad, q.grad, f"step {step}: grad of {n}")
        for opt in opts:
            opt.step()
        torch.cuda.synchronize()
        for (n, p), (_, q) in zip(a.state_dict().items(), b.state_dict().items()):
            same_bits(p, q, f"after step {step}: {n}")
    a.eval(), b.eval()
    u = torch.rand(B, H, W, device=DEV, generator=g)
    with torch.no_grad():
        want = a.generate_cached(label, (H, W), B, uniforms=u, return_logits=True)
        for kind, make_view in KINDS.items():
            got = b.generate_cached(make_view(label), (H, W), B, uniforms=make_view(u), return_logits=True)
            same_bits(list(got), list(want), f"generate_cached on the flat prior, {kind} label and uniforms")


def test_graphed_forward_on_a_flat_model():
    from vqvae_amd.graph import GraphedForward
    a, b, _ = _model_pair(lambda: _vqvae(None, big=True))
    a.eval(), b.eval()
    x0 = torch.randn(5, 3, 32, 32, device=DEV, generator=_gen(61))
    x1 = torch.randn(5, 3, 32, 32, device=DEV, generator=_gen(67))
    with torch.no_grad():
        g = GraphedForward(b, x0)
        got = [t.clone() for t in g(x1)]
        want = list(a(x1))
    torch.cuda.synchronize()
    same_bits(got, want, "graph replay on the flat model")


def test_inputs_as_users_pass_them():
    from vqvae_amd import conv
    conv.set_conv_backend("hip")
    m = _vqvae(dict()).eval()
    x = torch.randn(4, 3, 32, 32, device=DEV, generator=_gen(71))
    with torch.no_grad():
        want = list(m(x))
        same_bits(list(m(x.to(memory_format=torch.channels_last))), want, "channels_last input")
        # (the model takes images of 4k x 4m pixels, a multiple of 16 bytes each: the batch is a window into a staging buffer)
        x_all = torch.randn(5, 3, 20, 12, device=DEV, generator=_gen(73))
        odd = torch.empty(x_all.numel() + 3, device=DEV)[3:].view(x_all.shape)
        odd.copy_(x_all)
        assert odd[1:].data_ptr() % 16 != 0
        same_bits(list(m(odd[1:])), list(m(x_all[1:].clone())), "a slice of a batch")
    m.train()
    grads = []
    for as_view in (True, False):
        m.zero_grad(set_to_none=True)
        xin = x.clone().requires_grad_(True)
        x_hat = m(xin)[1]
        if as_view:
            x_hat.permute(0, 2, 3, 1)[..., :2].sum().backward()
        else:
            g = torch.zeros_like(x_hat)                                          # the same upstream gradient, dense
            g[:, :2] = 1.0
            x_hat.backward(g)
        grads.append([p.grad.clone() if p.grad is not None else None for p in m.parameters()] + [xin.grad])
    assert any(g is not None for g in grads[0])
    same_bits(grads[0], grads[1], "a sliced, permuted loss against its dense upstream gradient")
