"""CPU tests of the front end's argument handling (vqvae_amd/functional.py, vqvae_amd/training.py; the helpers are in
vqvae_amd/_lib.py, "front-end helpers"):

  * every public tensor-taking function refuses a CPU tensor in its first tensor argument with VqvaeHipError, before any other check;
  * every public `*_workspace` function raises VqvaeHipError just outside its envelope -- the message carries the refused value -- and
    allocates nothing; inside the envelope it allocates exactly what the size entry says (the size entries are host-only);
  * `_lib.ws_args` and `_lib.ptr` on CPU tensors.
"""
import inspect

import pytest
import torch

from vqvae_amd import _lib
from vqvae_amd import functional as F
from vqvae_amd import training as T
from vqvae_amd._lib import VqvaeHipError

B, D, H, W, K, G, Q = 2, 8, 2, 2, 8, 2, 2
N = B * H * W
LEVELS, N_E, BITS = (3, 3), 4, 2


def _f(*shape):
    return torch.zeros(shape, dtype=torch.float32)


def _i(*shape):
    return torch.zeros(shape, dtype=torch.int64)


def _proj(d):
    return _f(d, D), _f(d), _f(D, d), _f(D)


Z, CB, IDX = _f(B, D, H, W), _f(K, D), _i(N, 1)
BOOKS_Q, BOOKS_G = [_f(K, D) for _ in range(Q)], [_f(K, D // G) for _ in range(G)]

# name -> a call whose every tensor is on the CPU (the first tensor argument is the one the first check names)
CPU_CALLS = {
    "functional.vq_forward": lambda: F.vq_forward(Z, CB, 0.25),
    "functional.vq_onehot": lambda: F.vq_onehot(IDX, K),
    "functional.vq_decode_indices": lambda: F.vq_decode_indices(IDX, CB, B, H, W),
    "functional.vq_ema_update": lambda: F.vq_ema_update(Z, IDX, _f(K), _f(K, D), CB, 0.99),
    "functional.vq_ema_stats": lambda: F.vq_ema_stats(Z, IDX, K),
    "functional.vq_ema_apply": lambda: F.vq_ema_apply(torch.zeros(1, K, D + 1, dtype=torch.float64), _f(K), _f(K, D), CB, 0.99),
    "functional.vq_kmeans_seed": lambda: F.vq_kmeans_seed(Z, K, _f(K)),
    "functional.vq_kmeans_update": lambda: F.vq_kmeans_update(Z, IDX, CB),
    "functional.vq_kmeans": lambda: F.vq_kmeans(Z, K, 1),
    "functional.l2norm_rows": lambda: F.l2norm_rows(Z),
    "functional.l2norm_rows_backward": lambda: F.l2norm_rows_backward(Z, _f(N), Z),
    "functional.vq_residual_forward": lambda: F.vq_residual_forward(Z, BOOKS_Q, 0.25),
    "functional.vq_residual_decode": lambda: F.vq_residual_decode(_i(Q, N), BOOKS_Q, B, H, W),
    "functional.vq_grouped_forward": lambda: F.vq_grouped_forward(Z, BOOKS_G, 0.25),
    "functional.vq_grouped_decode": lambda: F.vq_grouped_decode(_i(G, N), BOOKS_G, B, H, W),
    "functional.fsq_forward": lambda: F.fsq_forward(Z, *_proj(len(LEVELS)), LEVELS),
    "functional.fsq_decode_indices": lambda: F.fsq_decode_indices(IDX, *_proj(len(LEVELS))[2:], LEVELS, B, H, W),
    "functional.lfq_forward": lambda: F.lfq_forward(Z, *_proj(BITS), N_E),
    "functional.lfq_decode_indices": lambda: F.lfq_decode_indices(IDX, *_proj(BITS)[2:], N_E, B, H, W),
    "functional.linear_rows": lambda: F.linear_rows(Z, _f(4, D), _f(4)),
    "functional.linear_rows_backward": lambda: F.linear_rows_backward(Z, _f(B, 4, H, W), _f(4, D)),
    "functional.vq_orthogonal_forward": lambda: F.vq_orthogonal_forward(CB),
    "functional.vq_orthogonal_backward": lambda: F.vq_orthogonal_backward(torch.zeros(K, D, dtype=torch.float64),
                                                                          torch.zeros(K, dtype=torch.int32),
                                                                          torch.zeros((), dtype=torch.int32)),
    "functional.vq_entropy_forward": lambda: F.vq_entropy_forward(Z, CB, inv_temperature=1.0, gamma=1.0),
    "functional.vq_entropy_backward": lambda: F.vq_entropy_backward(Z, CB, torch.zeros(K, dtype=torch.float64),
                                                                    torch.zeros(N, 2, dtype=torch.float64), inv_temperature=1.0,
                                                                    gamma=1.0),
    "training.vq_backward": lambda: T.vq_backward(Z, CB, IDX, Z, None, 0.25),
    "training.vq_residual_backward": lambda: T.vq_residual_backward(Z, BOOKS_Q, _i(Q, N), Z, None, 0.25),
    "training.vq_grouped_backward": lambda: T.vq_grouped_backward(Z, BOOKS_G, _i(G, N), Z, None, 0.25),
    "training.fsq_backward": lambda: T.fsq_backward(Z, Z, *_proj(len(LEVELS))[:3], LEVELS),
    "training.lfq_backward": lambda: T.lfq_backward(Z, Z, None, None, *_proj(BITS)[:3], N_E),
    "training.step_losses": lambda: T.step_losses(_f(), _f(B, 3, 8, 8), _f(), _f(B, 3, 8, 8), 1.0),
}

# name -> (the size entry's arguments from the function's dimensions, accepted dimensions, [(position of the dimension pushed out of the
# envelope, its value)]); `device` follows the dimensions
WORKSPACES = {
    "vq_workspace": (lambda d: ("vqvae_vq_workspace_bytes", (0, *d)), (K, D), [(0, 16385), (1, 257)]),
    "vq_ema_workspace": (lambda d: ("vqvae_vq_ema_workspace_bytes", d), (N, K, D), [(1, 16385), (2, 257)]),
    "vq_ema_stats_workspace": (lambda d: ("vqvae_vq_ema_stats_workspace_bytes", d), (N, K, D), [(0, 0), (1, 16385), (2, 257)]),
    "vq_ema_apply_workspace": (lambda d: ("vqvae_vq_ema_apply_workspace_bytes", d), (3, K, D), [(0, 0), (0, 1025), (1, 16385), (2, 257)]),
    "vq_kmeans_workspace": (lambda d: ("vqvae_vq_kmeans_workspace_bytes", d), (N, K, D), [(0, 0), (1, 16385), (2, 257)]),
    "vq_residual_workspace": (lambda d: ("vqvae_vq_residual_workspace_bytes", (*d, 0)), (N, K, D, Q), [(1, 16385), (2, 257), (3, 17)]),
    "vq_grouped_workspace": (lambda d: ("vqvae_vq_grouped_workspace_bytes", d), (N, K, D, G), [(1, 16385), (2, 257), (3, 17)]),
    "fsq_backward_workspace": (lambda d: ("vqvae_fsq_backward_workspace_bytes", d), (N, D, len(LEVELS)), [(0, 0), (1, 257)]),
    "lfq_workspace": (lambda d: ("vqvae_lfq_workspace_bytes", d), (N, D, BITS), [(0, 0), (1, 257), (2, 17)]),
    "linear_rows_backward_workspace": (lambda d: ("vqvae_linear_rows_backward_workspace_bytes", d), (N, D, 4),
                                       [(0, 0), (1, 257), (2, 257)]),
    "vq_orthogonal_workspace": (lambda d: ("vqvae_vq_orthogonal_workspace_bytes", d), (K, D), [(0, 16385), (1, 257)]),
    "vq_entropy_workspace": (lambda d: ("vqvae_vq_entropy_workspace_bytes", d), (N, K, D), [(0, 0), (1, 16385), (2, 257)]),
}


def _public(mod):
    return {n for n, f in vars(mod).items() if inspect.isfunction(f) and f.__module__ == mod.__name__ and not n.startswith("_")}


def test_tables_name_every_public_function():
    have = {f"functional.{n}" for n in _public(F)} | {f"training.{n}" for n in _public(T)}
    assert have == set(CPU_CALLS) | {f"functional.{n}" for n in WORKSPACES}


@pytest.mark.parametrize("name", sorted(CPU_CALLS))
def test_cpu_tensor_is_refused_first(name):
    with pytest.raises(VqvaeHipError):
        CPU_CALLS[name]()


@pytest.mark.parametrize("name", sorted(WORKSPACES))
def test_workspace_outside_its_envelope(name, monkeypatch):
    entry, dims, outside = WORKSPACES[name]
    fn = getattr(F, name)
    ws = fn(*dims, "cpu")
    entry, args = entry(dims)
    assert ws.dtype == torch.uint8 and ws.dim() == 1 and ws.numel() > 0 and ws.numel() == getattr(_lib.load(), entry)(*args)

    def no_allocation(*a, **k):
        raise AssertionError("a refused workspace must not allocate")
    monkeypatch.setattr(torch, "empty", no_allocation)
    for pos, bad in outside:
        args = list(dims)
        args[pos] = bad
        with pytest.raises(VqvaeHipError) as e:
            fn(*args, "cpu")
        assert str(bad) in str(e.value), f"{name}: the message does not carry the refused value {bad}: {e.value}"


def test_residual_workspace_shared_flag_reaches_the_entry():
    L = _lib.load()
    for shared in (False, True):
        assert F.vq_residual_workspace(N, K, D, Q, "cpu", shared=shared).numel() == \
            L.vqvae_vq_residual_workspace_bytes(N, K, D, Q, 1 if shared else 0)


def test_ptr_and_ws_args_helpers():
    assert _lib.ptr(None) is None
    t = torch.zeros(5, dtype=torch.float32)
    assert _lib.ptr(t) == t.data_ptr()
    assert _lib.ws_args(None) == (None, 0)
    ws = torch.zeros(24, dtype=torch.uint8)
    assert _lib.ws_args(ws) == (ws.data_ptr(), 24)
    for dtype, size in ((torch.float32, 4), (torch.float64, 8), (torch.int16, 2)):       # bytes, not elements
        w = torch.zeros(6, dtype=dtype)
        assert _lib.ws_args(w) == (w.data_ptr(), 6 * size)
