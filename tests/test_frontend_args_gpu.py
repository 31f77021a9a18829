"""GPU tests of the front end's argument handling (vqvae_amd/functional.py, vqvae_amd/training.py), one table for all of it:

  * CALLS      one accepting call per public function, in both layouts: run on views displaced by one element from a 16-byte
               boundary and again on dense, 16-byte-aligned copies of the same values -- every output, and every tensor written in
               place, has the same bits (no helper changed a pointer);
  * REFUSALS   one row per function and refusal -- wrong dtype, wrong rank, every shape mismatch the function checks, "both or
               neither" pairs, nothing wanted -- with the exception TYPE it raises.  Every refusal is raised on the host before a launch;
  * the five decoders: an index of K or of -1 raises IndexError, validate=False returns, and the rows of the valid indices then have
    the validated call's bits.

Shapes: B=2, D=8, H=W=2 (N=8), K=8, G=2, Q=2, levels (3,3), n_e=4 -- the smallest at which every entry still runs its real kernel.
"""
import functools
import types

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B, D, H, W, K, G, Q = 2, 8, 2, 2, 8, 2, 2
N = B * H * W
LEVELS, N_E, BITS = (3, 3), 4, 2
BETA = 0.25


# ---------------------------------------------------------------------------------------------------------------- the inputs
def _displaced(t):
    """the same values one element into a larger allocation: contiguous, 4 (or 8) bytes past a 16-byte boundary"""
    if isinstance(t, (list, tuple)):
        return [_displaced(x) for x in t]
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == t.element_size()
    return v


def _dense(t):
    if isinstance(t, (list, tuple)):
        return [_dense(x) for x in t]
    v = t.clone(memory_format=torch.contiguous_format)
    assert v.data_ptr() % 16 == 0
    return v


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


def _rows(t, rm):
    """the (N, C) rows of a map in either layout"""
    return (t if rm else t.permute(0, 2, 3, 1)).reshape(N, -1)


@functools.lru_cache(maxsize=None)
def _case(rm):
    """every input of the table, made once per layout and never written: the calls get copies"""
    from vqvae_amd import functional as F
    g = torch.Generator(device=DEV).manual_seed(11 + rm)

    def rnd(*shape):
        return torch.randn(*shape, device=DEV, generator=g)

    c = types.SimpleNamespace()
    c.cb = rnd(K, D)
    c.cb[K // 2] = c.cb[1]                                       # a duplicated code
    rows = c.cb[torch.randint(0, K, (N,), device=DEV, generator=g)] + 0.1 * rnd(N, D)
    c.z = (rows.view(B, H, W, D) if rm else rows.view(B, H, W, D).permute(0, 3, 1, 2)).contiguous()
    c.g = rnd(*c.z.shape)                                        # an upstream gradient of z's shape
    c.gl = rnd(1).reshape(())
    c.u = torch.rand(K, device=DEV, generator=g)
    c.idx = F.vq_forward(c.z, c.cb, BETA, rowmajor=rm)[3]
    c.cs, c.ew = torch.rand(K, device=DEV, generator=g) + 0.5, rnd(K, D)
    c.books_q = [c.cb.clone(), 0.3 * rnd(K, D)]
    c.idx_q = F.vq_residual_forward(c.z, c.books_q, BETA, rowmajor=rm)[3]
    c.books_g = [rnd(K, D // G) for _ in range(G)]
    c.idx_g = F.vq_grouped_forward(c.z, c.books_g, BETA, rowmajor=rm)[3]
    c.w_in, c.b_in, c.w_out, c.b_out = rnd(BITS, D), rnd(BITS), rnd(D, BITS), rnd(D)          # (FSQ's and LFQ's d are both 2)
    c.idx_fsq = F.fsq_forward(c.z, c.w_in, c.b_in, c.w_out, c.b_out, LEVELS, rowmajor=rm)[2]
    lfq = F.lfq_forward(c.z, c.w_in, c.b_in, c.w_out, c.b_out, N_E, rowmajor=rm)
    c.idx_lfq, c.avg_lfq = lfq[2], lfq[5]
    c.stats = torch.stack([F.vq_ema_stats(c.z, c.idx, K, row_uniforms=c.u, rowmajor=rm),
                           F.vq_ema_stats(c.g, c.idx, K, row_uniforms=c.u, rowmajor=rm)])         # (2, K, 2 D + 1) float64
    c.y, c.denom = F.l2norm_rows(c.z, rowmajor=rm)
    c.w, c.b = rnd(4, D), rnd(4)
    c.gy = rnd(*F.linear_rows(c.z, c.w, c.b, rowmajor=rm).shape)
    c.hist = torch.tensor([1, 0, 2, 3, 0, 1, 1, 4], dtype=torch.int32, device=DEV)
    _, c.count, c.selected, c.saved = F.vq_orthogonal_forward(c.cb, c.hist, want_saved=True)
    _, c.avg, c.rowstat = F.vq_entropy_forward(c.z, c.cb, inv_temperature=2.0, gamma=1.0, rowmajor=rm)
    c.x, c.x_hat = rnd(B, 3, 8, 8), rnd(B, 3, 8, 8)
    torch.cuda.synchronize()
    return c


# ----------------------------------------------------------------------------------------------------------------- the calls
# name -> f(rm) -> (fn(**tensors, **options), tensors): the accepting call.  A tensor written in place comes back among the outputs.
def _F():
    from vqvae_amd import functional
    return functional


def _T():
    from vqvae_amd import training
    return training


def _vq_forward(rm, c):
    return (lambda z_e, codebook, **o: _F().vq_forward(z_e, codebook, BETA, rowmajor=rm, **o)), dict(z_e=c.z, codebook=c.cb)


def _vq_onehot(rm, c):
    return (lambda idx, **o: _F().vq_onehot(idx, K)), dict(idx=c.idx)


def _vq_decode_indices(rm, c):
    return (lambda idx, codebook, **o: _F().vq_decode_indices(idx, codebook, B, H, W, **o)), dict(idx=c.idx, codebook=c.cb)


def _vq_ema_update(rm, c):
    def fn(z_e, idx, ema_cluster_size, ema_w, codebook, uniforms, threshold=0.9, **o):
        _F().vq_ema_update(z_e, idx, ema_cluster_size, ema_w, codebook, 0.9, threshold=threshold, uniforms=uniforms, rowmajor=rm, **o)
        return ema_cluster_size.clone(), ema_w.clone(), codebook.clone()
    return fn, dict(z_e=c.z, idx=c.idx, ema_cluster_size=c.cs, ema_w=c.ew, codebook=c.cb, uniforms=c.u)


def _vq_ema_stats(rm, c):
    return (lambda z_e, idx, row_uniforms, **o: _F().vq_ema_stats(z_e, idx, K, row_uniforms=row_uniforms, rowmajor=rm, **o)), \
        dict(z_e=c.z, idx=c.idx, row_uniforms=c.u)


def _vq_ema_apply(rm, c):
    def fn(stats, ema_cluster_size, ema_w, codebook, shard_uniforms, threshold=0.9, **o):
        _F().vq_ema_apply(stats, ema_cluster_size, ema_w, codebook, 0.9, threshold=threshold, shard_uniforms=shard_uniforms, **o)
        return ema_cluster_size.clone(), ema_w.clone(), codebook.clone()
    return fn, dict(stats=c.stats, ema_cluster_size=c.cs, ema_w=c.ew, codebook=c.cb, shard_uniforms=c.u)


def _vq_kmeans_seed(rm, c):
    return (lambda z_e, uniforms, **o: _F().vq_kmeans_seed(z_e, K, uniforms, rowmajor=rm)), dict(z_e=c.z, uniforms=c.u)


def _vq_kmeans_update(rm, c):
    def fn(z_e, idx, codebook, uniforms, **o):
        return _F().vq_kmeans_update(z_e, idx, codebook, uniforms=uniforms, rowmajor=rm), codebook.clone()
    return fn, dict(z_e=c.z, idx=c.idx, codebook=c.cb, uniforms=c.u)


def _vq_kmeans(rm, c):
    return (lambda z_e, iters=2, **o: _F().vq_kmeans(z_e, K, iters, generator=torch.Generator(device=DEV).manual_seed(5),
                                                     rowmajor=rm)), dict(z_e=c.z)


def _l2norm_rows(rm, c):
    return (lambda x, **o: _F().l2norm_rows(x, rowmajor=rm)), dict(x=c.z)


def _l2norm_rows_backward(rm, c):
    return (lambda y, denom, grad_y, **o: _F().l2norm_rows_backward(y, denom, grad_y, rowmajor=rm)), \
        dict(y=c.y, denom=c.denom, grad_y=c.g)


def _vq_residual_forward(rm, c):
    return (lambda z_e, codebooks, **o: _F().vq_residual_forward(z_e, codebooks, BETA, rowmajor=rm, want_residual=True, **o)), \
        dict(z_e=c.z, codebooks=c.books_q)


def _vq_residual_decode(rm, c):
    return (lambda idx, codebooks, **o: _F().vq_residual_decode(idx, codebooks, B, H, W, rowmajor=rm, **o)), \
        dict(idx=c.idx_q, codebooks=c.books_q)


def _vq_grouped_forward(rm, c):
    return (lambda z_e, codebooks, **o: _F().vq_grouped_forward(z_e, codebooks, BETA, rowmajor=rm, want_slabs=True, **o)), \
        dict(z_e=c.z, codebooks=c.books_g)


def _vq_grouped_decode(rm, c):
    return (lambda idx, codebooks, **o: _F().vq_grouped_decode(idx, codebooks, B, H, W, rowmajor=rm, **o)), \
        dict(idx=c.idx_g, codebooks=c.books_g)


def _proj(c, n=4):
    return dict(list(dict(w_in=c.w_in, b_in=c.b_in, w_out=c.w_out, b_out=c.b_out).items())[:n])


def _fsq_forward(rm, c):
    return (lambda z_e, w_in, b_in, w_out, b_out, levels=LEVELS, **o: _F().fsq_forward(z_e, w_in, b_in, w_out, b_out, levels, rowmajor=rm)), \
        dict(z_e=c.z, **_proj(c))


def _fsq_decode_indices(rm, c):
    return (lambda idx, w_out, b_out, **o: _F().fsq_decode_indices(idx, w_out, b_out, LEVELS, B, H, W, rowmajor=rm, **o)), \
        dict(idx=c.idx_fsq, w_out=c.w_out, b_out=c.b_out)


def _lfq_forward(rm, c):
    return (lambda z_e, w_in, b_in, w_out, b_out, n_e=N_E, **o: _F().lfq_forward(z_e, w_in, b_in, w_out, b_out, n_e, rowmajor=rm)), \
        dict(z_e=c.z, **_proj(c))


def _lfq_decode_indices(rm, c):
    return (lambda idx, w_out, b_out, **o: _F().lfq_decode_indices(idx, w_out, b_out, N_E, B, H, W, rowmajor=rm, **o)), \
        dict(idx=c.idx_lfq, w_out=c.w_out, b_out=c.b_out)


def _linear_rows(rm, c):
    return (lambda x, w, b, **o: _F().linear_rows(x, w, b, rowmajor=rm)), dict(x=c.z, w=c.w, b=c.b)


def _linear_rows_backward(rm, c):
    return (lambda x, grad_y, w, **o: _F().linear_rows_backward(x, grad_y, w, rowmajor=rm, **o)), dict(x=c.z, grad_y=c.gy, w=c.w)


def _vq_orthogonal_forward(rm, c):
    return (lambda rows, hist, uniforms, max_codes=3, **o: _F().vq_orthogonal_forward(rows, hist, max_codes=max_codes, uniforms=uniforms,
                                                                                      want_saved=True)), \
        dict(rows=c.cb, hist=c.hist, uniforms=c.u)


def _vq_orthogonal_backward(rm, c):
    return (lambda saved, selected, count, grad_loss, **o: _F().vq_orthogonal_backward(saved, selected, count, grad_loss)), \
        dict(saved=c.saved, selected=c.selected, count=c.count, grad_loss=c.gl)


def _vq_entropy_forward(rm, c):
    return (lambda z, codebook, **o: _F().vq_entropy_forward(z, codebook, inv_temperature=2.0, gamma=1.0, rowmajor=rm)), \
        dict(z=c.z, codebook=c.cb)


def _vq_entropy_backward(rm, c):
    return (lambda z, codebook, avg, rowstat, grad_loss, **o: _F().vq_entropy_backward(z, codebook, avg, rowstat, grad_loss,
                                                                                       inv_temperature=2.0, gamma=1.0, rowmajor=rm, **o)), \
        dict(z=c.z, codebook=c.cb, avg=c.avg, rowstat=c.rowstat, grad_loss=c.gl)


def _vq_backward(rm, c):
    return (lambda z_e, codebook, idx, grad_zq, grad_loss, **o: _T().vq_backward(z_e, codebook, idx, grad_zq, grad_loss, BETA,
                                                                                 rowmajor=rm, **o)), \
        dict(z_e=c.z, codebook=c.cb, idx=c.idx, grad_zq=c.g, grad_loss=c.gl)


def _vq_residual_backward(rm, c):
    return (lambda z_e, codebooks, idx, grad_zq, grad_loss, **o: _T().vq_residual_backward(z_e, codebooks, idx, grad_zq, grad_loss, BETA,
                                                                                           rowmajor=rm, **o)), \
        dict(z_e=c.z, codebooks=c.books_q, idx=c.idx_q, grad_zq=c.g, grad_loss=c.gl)


def _vq_grouped_backward(rm, c):
    return (lambda z_e, codebooks, idx, grad_zq, grad_loss, **o: _T().vq_grouped_backward(z_e, codebooks, idx, grad_zq, grad_loss, BETA,
                                                                                          rowmajor=rm, **o)), \
        dict(z_e=c.z, codebooks=c.books_g, idx=c.idx_g, grad_zq=c.g, grad_loss=c.gl)


def _fsq_backward(rm, c):
    return (lambda z_e, grad_zq, w_in, b_in, w_out, levels=LEVELS, **o: _T().fsq_backward(z_e, grad_zq, w_in, b_in, w_out, levels,
                                                                                          rowmajor=rm)), \
        dict(z_e=c.z, grad_zq=c.g, **_proj(c, 3))


def _lfq_backward(rm, c):
    return (lambda z_e, grad_zq, grad_loss, avg, w_in, b_in, w_out, n_e=N_E, **o: _T().lfq_backward(z_e, grad_zq, grad_loss, avg, w_in,
                                                                                                    b_in, w_out, n_e, rowmajor=rm)), \
        dict(z_e=c.z, grad_zq=c.g, grad_loss=c.gl, avg=c.avg_lfq, **_proj(c, 3))


def _step_losses(rm, c):
    return (lambda embedding_loss, x_hat, perplexity, x, **o: _T().step_losses(embedding_loss, x_hat, perplexity, x, 0.5)), \
        dict(embedding_loss=c.gl, x_hat=c.x_hat, perplexity=c.gl.abs(), x=c.x)


NO_LAYOUT = {"vq_onehot", "vq_decode_indices", "vq_ema_apply", "vq_orthogonal_forward", "vq_orthogonal_backward", "step_losses"}
CALLS = {f.__name__[1:]: f for f in (
    _vq_forward, _vq_onehot, _vq_decode_indices, _vq_ema_update, _vq_ema_stats, _vq_ema_apply, _vq_kmeans_seed, _vq_kmeans_update,
    _vq_kmeans, _l2norm_rows, _l2norm_rows_backward, _vq_residual_forward, _vq_residual_decode, _vq_grouped_forward, _vq_grouped_decode,
    _fsq_forward, _fsq_decode_indices, _lfq_forward, _lfq_decode_indices, _linear_rows, _linear_rows_backward, _vq_orthogonal_forward,
    _vq_orthogonal_backward, _vq_entropy_forward, _vq_entropy_backward, _vq_backward, _vq_residual_backward, _vq_grouped_backward,
    _fsq_backward, _lfq_backward, _step_losses)}


def test_the_table_names_every_public_function():
    import inspect
    have = set()
    for mod in (_F(), _T()):
        have |= {n for n, f in vars(mod).items() if inspect.isfunction(f) and f.__module__ == mod.__name__ and not n.startswith("_")
                 and not n.endswith("_workspace")}
    assert have == set(CALLS)


@pytest.mark.parametrize("name,rm", [(n, rm) for n in CALLS for rm in ((False,) if n in NO_LAYOUT else (False, True))],
                         ids=lambda v: v if isinstance(v, str) else ("rows" if v else "nchw"))
def test_accepts_and_takes_no_other_pointer(name, rm):
    fn, tensors = CALLS[name](rm, _case(rm))
    want = fn(**{k: _dense(v) for k, v in tensors.items()})
    got = fn(**{k: _displaced(v) for k, v in tensors.items()})
    torch.cuda.synchronize()
    same_bits(got, want, name)
    flat = []

    def leaves(o):
        if isinstance(o, (list, tuple)):
            for x in o:
                leaves(x)
        elif o is not None:
            flat.append(o)
    leaves(want)
    assert flat and all(t.is_cuda for t in flat)


# ------------------------------------------------------------------------------------------------------------- the refusals
def _dbl(t):
    return t.double()


def _f32(t):
    return t.float()


def _i32(t):
    return t.to(torch.int32)


def _i64(t):
    return t.to(torch.int64)


def _rank3(t):
    return t[0]


def _wider(t):
    """one more column"""
    return torch.cat([t, t[..., :1]], -1)


def _longer(t):
    """one more row"""
    return torch.cat([t, t[:1]], 0)


def _short(t):
    """one element less, flat"""
    return t.flatten()[:-1]


def _none(t):
    return None


def _two(t):
    return torch.ones(2, dtype=t.dtype, device=t.device)


def _first(f):
    return lambda ts: [f(ts[0])] + list(ts[1:])


def _each(f):
    return lambda ts: [f(t) for t in ts]


T_, V_ = TypeError, ValueError
# (function, what is wrong, exception type, {argument: its replacement -- a function of the accepted tensor -- or option: value, or a
# function that makes the value})
REFUSALS = [
    ("vq_forward", "z_e dtype", T_, dict(z_e=_dbl)),
    ("vq_forward", "codebook dtype", T_, dict(codebook=_dbl)),
    ("vq_forward", "z_e rank", V_, dict(z_e=_rank3)),
    ("vq_forward", "codebook width", V_, dict(codebook=_wider)),
    ("vq_onehot", "idx dtype", T_, dict(idx=_i32)),
    ("vq_decode_indices", "idx dtype", T_, dict(idx=_i32)),
    ("vq_decode_indices", "codebook dtype", T_, dict(codebook=_dbl)),
    ("vq_decode_indices", "idx count", V_, dict(idx=_longer)),
    ("vq_ema_update", "z_e dtype", T_, dict(z_e=_dbl)),
    ("vq_ema_update", "idx dtype", T_, dict(idx=_i32)),
    ("vq_ema_update", "ema_cluster_size dtype", T_, dict(ema_cluster_size=_dbl)),
    ("vq_ema_update", "z_e rank", V_, dict(z_e=_rank3)),
    ("vq_ema_update", "codebook width", V_, dict(codebook=_wider)),
    ("vq_ema_update", "ema_w width", V_, dict(ema_w=_wider)),
    ("vq_ema_update", "ema_cluster_size length", V_, dict(ema_cluster_size=_longer)),
    ("vq_ema_update", "idx count", V_, dict(idx=_longer)),
    ("vq_ema_update", "uniforms without threshold", V_, dict(threshold=None)),
    ("vq_ema_update", "threshold without uniforms", V_, dict(uniforms=_none)),
    ("vq_ema_update", "uniforms count", V_, dict(uniforms=_longer)),
    ("vq_ema_update", "uniforms dtype", T_, dict(uniforms=_dbl)),
    ("vq_ema_stats", "z_e dtype", T_, dict(z_e=_dbl)),
    ("vq_ema_stats", "idx dtype", T_, dict(idx=_i32)),
    ("vq_ema_stats", "z_e rank", V_, dict(z_e=_rank3)),
    ("vq_ema_stats", "idx count", V_, dict(idx=_longer)),
    ("vq_ema_stats", "row_uniforms count", V_, dict(row_uniforms=_longer)),
    ("vq_ema_stats", "row_uniforms dtype", T_, dict(row_uniforms=_dbl)),
    ("vq_ema_stats", "out dtype", T_, dict(out=lambda: torch.empty(K, 2 * D + 1, dtype=torch.float32, device=DEV))),
    ("vq_ema_stats", "out shape", V_, dict(out=lambda: torch.empty(K, D + 1, dtype=torch.float64, device=DEV))),
    ("vq_ema_apply", "stats dtype", T_, dict(stats=_f32)),
    ("vq_ema_apply", "empty list of stats", V_, dict(stats=lambda t: [])),
    ("vq_ema_apply", "stats of two shapes", V_, dict(stats=lambda t: [t[0], t[1][:, :-1]])),
    ("vq_ema_apply", "stats rank", V_, dict(stats=_rank3)),
    ("vq_ema_apply", "codebook length", V_, dict(codebook=_longer)),
    ("vq_ema_apply", "stats width", V_, dict(stats=lambda t: t[..., :-1])),
    ("vq_ema_apply", "ema_w width", V_, dict(ema_w=_wider)),
    ("vq_ema_apply", "ema_cluster_size length", V_, dict(ema_cluster_size=_longer)),
    ("vq_ema_apply", "shard_uniforms without threshold", V_, dict(threshold=None)),
    ("vq_ema_apply", "threshold without shard_uniforms", V_, dict(shard_uniforms=_none)),
    ("vq_ema_apply", "shard_uniforms count", V_, dict(shard_uniforms=_longer)),
    ("vq_ema_apply", "restart on statistics without candidates", V_, dict(stats=lambda t: t[..., :D + 1])),
    ("vq_kmeans_seed", "z_e dtype", T_, dict(z_e=_dbl)),
    ("vq_kmeans_seed", "z_e rank", V_, dict(z_e=_rank3)),
    ("vq_kmeans_seed", "uniforms dtype", T_, dict(uniforms=_dbl)),
    ("vq_kmeans_seed", "uniforms count", V_, dict(uniforms=_longer)),
    ("vq_kmeans_update", "z_e dtype", T_, dict(z_e=_dbl)),
    ("vq_kmeans_update", "z_e rank", V_, dict(z_e=_rank3)),
    ("vq_kmeans_update", "idx dtype", T_, dict(idx=_i32)),
    ("vq_kmeans_update", "codebook dtype", T_, dict(codebook=_dbl)),
    ("vq_kmeans_update", "codebook width", V_, dict(codebook=_wider)),
    ("vq_kmeans_update", "idx count", V_, dict(idx=_longer)),
    ("vq_kmeans_update", "uniforms count", V_, dict(uniforms=_longer)),
    ("vq_kmeans", "z_e dtype", T_, dict(z_e=_dbl)),
    ("vq_kmeans", "z_e rank", V_, dict(z_e=_rank3)),
    ("vq_kmeans", "negative iters", V_, dict(iters=-1)),
    ("l2norm_rows", "x dtype", T_, dict(x=_dbl)),
    ("l2norm_rows", "x rank", V_, dict(x=_rank3)),
    ("l2norm_rows_backward", "y dtype", T_, dict(y=_dbl)),
    ("l2norm_rows_backward", "y rank", V_, dict(y=_rank3)),
    ("l2norm_rows_backward", "denom dtype", T_, dict(denom=_dbl)),
    ("l2norm_rows_backward", "grad_y dtype", T_, dict(grad_y=_dbl)),
    ("l2norm_rows_backward", "grad_y shape", V_, dict(grad_y=_wider)),
    ("l2norm_rows_backward", "denom count", V_, dict(denom=_longer)),
    ("vq_residual_forward", "z_e dtype", T_, dict(z_e=_dbl)),
    ("vq_residual_forward", "z_e rank", V_, dict(z_e=_rank3)),
    ("vq_residual_forward", "no codebook", V_, dict(codebooks=lambda ts: [])),
    ("vq_residual_forward", "codebook dtype", T_, dict(codebooks=_first(_dbl))),
    ("vq_residual_forward", "codebooks of two shapes", V_, dict(codebooks=_first(_wider))),
    ("vq_residual_forward", "n_q against the list", V_, dict(n_q=3)),
    ("vq_residual_forward", "codebook width", V_, dict(codebooks=_each(_wider))),
    ("vq_residual_decode", "idx dtype", T_, dict(idx=_i32)),
    ("vq_residual_decode", "idx count", V_, dict(idx=_short)),
    ("vq_residual_decode", "stages against codebooks", V_, dict(idx=lambda t: t[:1])),
    ("vq_residual_decode", "no codebook", V_, dict(codebooks=lambda ts: [])),
    ("vq_grouped_forward", "z_e dtype", T_, dict(z_e=_dbl)),
    ("vq_grouped_forward", "z_e rank", V_, dict(z_e=_rank3)),
    ("vq_grouped_forward", "seventeen codebooks", V_, dict(codebooks=lambda ts: [ts[0]] * 17)),
    ("vq_grouped_forward", "codebooks of two shapes", V_, dict(codebooks=_first(_wider))),
    ("vq_grouped_forward", "groups against channels", V_, dict(codebooks=lambda ts: ts[:1])),
    ("vq_grouped_forward", "codebook dtype", T_, dict(codebooks=_first(_dbl))),
    ("vq_grouped_decode", "idx dtype", T_, dict(idx=_i32)),
    ("vq_grouped_decode", "idx count", V_, dict(idx=lambda t: t[:1])),
    ("fsq_forward", "z_e dtype", T_, dict(z_e=_dbl)),
    ("fsq_forward", "z_e rank", V_, dict(z_e=_rank3)),
    ("fsq_forward", "a level of one value", V_, dict(levels=(1, 3))),
    ("fsq_forward", "w_in shape", V_, dict(w_in=_wider)),
    ("fsq_forward", "b_out dtype", T_, dict(b_out=_dbl)),
    ("fsq_decode_indices", "idx dtype", T_, dict(idx=_i32)),
    ("fsq_decode_indices", "w_out dtype", T_, dict(w_out=_dbl)),
    ("fsq_decode_indices", "w_out rank", V_, dict(w_out=_rank3)),
    ("fsq_decode_indices", "b_out shape", V_, dict(b_out=_longer)),
    ("fsq_decode_indices", "idx count", V_, dict(idx=_longer)),
    ("lfq_forward", "z_e dtype", T_, dict(z_e=_dbl)),
    ("lfq_forward", "z_e rank", V_, dict(z_e=_rank3)),
    ("lfq_forward", "n_e no power of two", V_, dict(n_e=3)),
    ("lfq_forward", "w_in shape", V_, dict(w_in=_wider)),
    ("lfq_decode_indices", "idx dtype", T_, dict(idx=_i32)),
    ("lfq_decode_indices", "w_out dtype", T_, dict(w_out=_dbl)),
    ("lfq_decode_indices", "w_out rank", V_, dict(w_out=_rank3)),
    ("lfq_decode_indices", "b_out shape", V_, dict(b_out=_longer)),
    ("lfq_decode_indices", "idx count", V_, dict(idx=_longer)),
    ("linear_rows", "x dtype", T_, dict(x=_dbl)),
    ("linear_rows", "x rank", V_, dict(x=_rank3)),
    ("linear_rows", "w width", V_, dict(w=_wider)),
    ("linear_rows", "w rank", V_, dict(w=_rank3)),
    ("linear_rows", "b length", V_, dict(b=_longer)),
    ("linear_rows", "b dtype", T_, dict(b=_dbl)),
    ("linear_rows_backward", "x rank", V_, dict(x=_rank3)),
    ("linear_rows_backward", "grad_y dtype", T_, dict(grad_y=_dbl)),
    ("linear_rows_backward", "grad_y shape", V_, dict(grad_y=_wider)),
    ("linear_rows_backward", "nothing wanted", V_, dict(want=(False, False, False))),
    ("vq_orthogonal_forward", "rows dtype", T_, dict(rows=_dbl)),
    ("vq_orthogonal_forward", "rows rank", V_, dict(rows=_rank3)),
    ("vq_orthogonal_forward", "hist dtype", T_, dict(hist=_i64)),
    ("vq_orthogonal_forward", "hist length", V_, dict(hist=_longer)),
    ("vq_orthogonal_forward", "max_codes without uniforms", V_, dict(uniforms=_none)),
    ("vq_orthogonal_forward", "uniforms length", V_, dict(uniforms=_longer)),
    ("vq_orthogonal_backward", "saved dtype", T_, dict(saved=_f32)),
    ("vq_orthogonal_backward", "selected dtype", T_, dict(selected=_i64)),
    ("vq_orthogonal_backward", "count dtype", T_, dict(count=_i64)),
    ("vq_orthogonal_backward", "saved rank", V_, dict(saved=_rank3)),
    ("vq_orthogonal_backward", "selected length", V_, dict(selected=_longer)),
    ("vq_orthogonal_backward", "grad_loss of two elements", V_, dict(grad_loss=_two)),
    ("vq_orthogonal_backward", "grad_loss dtype", T_, dict(grad_loss=_dbl)),
    ("vq_entropy_forward", "z dtype", T_, dict(z=_dbl)),
    ("vq_entropy_forward", "codebook dtype", T_, dict(codebook=_dbl)),
    ("vq_entropy_forward", "z rank", V_, dict(z=_rank3)),
    ("vq_entropy_forward", "codebook width", V_, dict(codebook=_wider)),
    ("vq_entropy_backward", "avg dtype", T_, dict(avg=_f32)),
    ("vq_entropy_backward", "rowstat dtype", T_, dict(rowstat=_f32)),
    ("vq_entropy_backward", "avg length", V_, dict(avg=_longer)),
    ("vq_entropy_backward", "rowstat length", V_, dict(rowstat=_longer)),
    ("vq_entropy_backward", "nothing wanted", V_, dict(want=(False, False))),
    ("vq_entropy_backward", "grad_loss of two elements", V_, dict(grad_loss=_two)),
    ("vq_backward", "commitment with a codebook gradient", V_, dict(commitment=True)),
    ("vq_backward", "rotation without grad_z", V_, dict(rotation=True, need_z=False)),
    ("vq_backward", "z_e dtype", T_, dict(z_e=_dbl)),
    ("vq_backward", "codebook dtype", T_, dict(codebook=_dbl)),
    ("vq_backward", "idx dtype", T_, dict(idx=_i32)),
    ("vq_backward", "grad_zq dtype", T_, dict(grad_zq=_dbl)),
    ("vq_backward", "grad_loss dtype", T_, dict(grad_loss=_dbl)),
    ("vq_backward", "z_e rank", V_, dict(z_e=_rank3)),
    ("vq_backward", "codebook width", V_, dict(codebook=_wider)),
    ("vq_backward", "idx count", V_, dict(idx=_longer)),
    ("vq_backward", "grad_zq shape", V_, dict(grad_zq=_wider)),
    ("vq_residual_backward", "z_e dtype", T_, dict(z_e=_dbl)),
    ("vq_residual_backward", "idx dtype", T_, dict(idx=_i32)),
    ("vq_residual_backward", "codebook dtype", T_, dict(codebooks=_first(_dbl))),
    ("vq_residual_backward", "z_e rank", V_, dict(z_e=_rank3)),
    ("vq_residual_backward", "codebook width", V_, dict(codebooks=_each(_wider))),
    ("vq_residual_backward", "idx count", V_, dict(idx=_short)),
    ("vq_residual_backward", "stages against codebooks", V_, dict(idx=lambda t: t[:1])),
    ("vq_residual_backward", "grad_zq shape", V_, dict(grad_zq=_wider)),
    ("vq_residual_backward", "grad_zq dtype", T_, dict(grad_zq=_dbl)),
    ("vq_grouped_backward", "commitment with codebook gradients", V_, dict(commitment=True)),
    ("vq_grouped_backward", "z_e dtype", T_, dict(z_e=_dbl)),
    ("vq_grouped_backward", "idx dtype", T_, dict(idx=_i32)),
    ("vq_grouped_backward", "z_e rank", V_, dict(z_e=_rank3)),
    ("vq_grouped_backward", "groups against channels", V_, dict(codebooks=lambda ts: ts[:1])),
    ("vq_grouped_backward", "idx count", V_, dict(idx=lambda t: t[:1])),
    ("vq_grouped_backward", "grad_zq shape", V_, dict(grad_zq=_wider)),
    ("vq_grouped_backward", "grad_loss dtype", T_, dict(grad_loss=_dbl)),
    ("fsq_backward", "z_e dtype", T_, dict(z_e=_dbl)),
    ("fsq_backward", "grad_zq dtype", T_, dict(grad_zq=_dbl)),
    ("fsq_backward", "z_e rank", V_, dict(z_e=_rank3, grad_zq=_rank3)),
    ("fsq_backward", "grad_zq shape", V_, dict(grad_zq=_wider)),
    ("fsq_backward", "w_in shape", V_, dict(w_in=_wider)),
    ("fsq_backward", "a level of one value", V_, dict(levels=(1, 3))),
    ("lfq_backward", "z_e dtype", T_, dict(z_e=_dbl)),
    ("lfq_backward", "grad_zq dtype", T_, dict(grad_zq=_dbl)),
    ("lfq_backward", "z_e rank", V_, dict(z_e=_rank3, grad_zq=_rank3)),
    ("lfq_backward", "grad_zq shape", V_, dict(grad_zq=_wider)),
    ("lfq_backward", "avg dtype", T_, dict(avg=_f32)),
    ("lfq_backward", "avg length", V_, dict(avg=_longer)),
    ("lfq_backward", "grad_loss dtype", T_, dict(grad_loss=_dbl)),
    ("lfq_backward", "n_e no power of two", V_, dict(n_e=3)),
    ("step_losses", "x_hat dtype", T_, dict(x_hat=_dbl)),
    ("step_losses", "x shape", V_, dict(x=_wider)),
]


def test_every_function_has_refusal_rows():
    assert {r[0] for r in REFUSALS} == set(CALLS)


@pytest.mark.parametrize("name,what,exc,change", REFUSALS, ids=[f"{r[0]}-{r[1].replace(' ', '_')}" for r in REFUSALS])
def test_refuses(name, what, exc, change):
    """(row-major maps: the layout plays no part in a refusal)"""
    fn, tensors = CALLS[name](True, _case(True))
    args = {k: _dense(v) for k, v in tensors.items()}
    for k, v in change.items():
        args[k] = v(args[k]) if k in tensors else v() if callable(v) else v
    with pytest.raises(exc):
        fn(**args)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------ the decoders
DECODERS = {"vq_decode_indices": ("idx", K), "vq_residual_decode": ("idx_q", K), "vq_grouped_decode": ("idx_g", K),
            "fsq_decode_indices": ("idx_fsq", 9), "lfq_decode_indices": ("idx_lfq", N_E)}


@pytest.mark.parametrize("name,rm", [(n, rm) for n in DECODERS for rm in ((False,) if n in NO_LAYOUT else (False, True))],
                         ids=lambda v: v if isinstance(v, str) else ("rows" if v else "nchw"))
def test_decoder_index_range(name, rm):
    fn, tensors = CALLS[name](rm, _case(rm))
    n_codes = DECODERS[name][1]
    args = {k: _dense(v) for k, v in tensors.items()}
    want = fn(**args)
    same_bits(fn(**args, validate=False), want, f"{name} validate=False")
    for bad in (n_codes, -1):
        idx = args["idx"].clone()
        idx.view(-1, N)[0, 3] = bad                              # (row 3, the first stage / group where there are several)
        with pytest.raises(IndexError):
            fn(**{**args, "idx": idx})
        got = fn(**{**args, "idx": idx}, validate=False)         # returns; the kernel reads nothing out of range
        torch.cuda.synchronize()
        keep = [n for n in range(N) if n != 3]
        same_bits(_rows(got, rm)[keep], _rows(want, rm)[keep], f"{name} rows of the valid indices, bad index {bad}")
