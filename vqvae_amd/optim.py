"""Adam / AMSGrad / AdamW on the HIP kernels of csrc/optim.hip: every tensor of the optimizer in one elementwise launch.

    opt = vqvae_amd.optim.Adam(model.parameters(), lr=3e-4, amsgrad=True)        # main.py:59
    loss.backward(); opt.step()                                                   # main.py:78-80

A step is two launches (a one-workgroup kernel that advances the device step counters and forms the bias corrections, then the update
kernel), four with `max_grad_norm` (the global gradient norm first).  Nothing synchronises and nothing is read back to the host.
The per-element operation order is written down in csrc/optim.hip's header comment and is the same in every run, on every
partition of the data into tensors.

`Adam` subclasses torch.optim.Optimizer: param_groups, add_param_group, zero_grad, lr schedulers and state_dict / load_state_dict
are torch's, and the per-parameter state uses torch's keys (`step`, `exp_avg`, `exp_avg_sq`, `max_exp_avg_sq`), so a state dict moves
both ways between this class and torch.optim.Adam.  `step` is one fp32 scalar on the device per parameter (the layout of torch's
capturable / fused Adam); a state loaded from torch's default Adam, whose counters are host tensors, is moved there at the next step.

There is no CPU path and no fallback: CPU, non-fp32 or non-contiguous parameters or gradients, sparse gradients and the options
`maximize`, `foreach`, `fused`, `capturable`, `differentiable` raise before anything is launched.

Stream capture (torch.cuda.graph): a captured step keeps the hyper-parameters of capture time (they travel as launch arguments), and
the gradients must be static tensors -- `zero_grad(set_to_none=False)` or `step(zero_grad=True)` -- with at least one eager step on
them before the capture, so that the cached plan already names them; a step that would have to rebuild its plan while capturing raises.

`lr` and `eps` must be positive: the constructor refuses 0, and a scheduler that takes a group's lr to exactly 0
(CosineAnnealingLR with eta_min=0, LinearLR with end_factor=0) makes the next `step()` raise -- give it a small positive floor.

With `max_grad_norm` the clipped gradient g * clip_coef enters the update, but the `.grad` tensors in memory stay unscaled
(torch.nn.utils.clip_grad_norm_ scales them in place); `last_grad_norm` is the total norm as a device tensor -- a view of a
buffer that belongs to the plan and is overwritten by the next step (clone it to keep a value); nothing is allocated in a step, so
a clipping step captures like a plain one, as a chain of four kernels.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _lib
from ._lib import VqvaeHipError

ZERO_GRAD = 0x1            # VQVAE_ADAM_ZERO_GRAD
DECOUPLED_WD = 0x1         # VQVAE_ADAM_DECOUPLED_WD
MAX_GROUPS = 16            # VQVAE_ADAM_MAX_GROUPS

_REFUSED = ("maximize", "foreach", "fused", "capturable", "differentiable")


class _Plan:
    __slots__ = ("key", "params", "dev", "nbytes", "n_tensors", "n_chunks", "updated", "ws", "norm", "states")


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *,
                 decoupled_weight_decay=False, max_grad_norm=None, **refused):
        for k, v in refused.items():
            if k not in _REFUSED:
                raise TypeError(f"Adam() got an unexpected keyword argument {k!r}")
            if v:
                raise ValueError(f"{k}={v!r}: the HIP optimizer has one implementation and does not take this option")
        if isinstance(lr, torch.Tensor):
            raise ValueError("lr must be a Python number: hyper-parameters travel as launch arguments")
        if not 0.0 < lr:                                     # (torch takes 0; vqvae_adam_step_f32 takes neither lr nor eps of 0)
            raise ValueError(f"Invalid learning rate: {lr} (must be > 0)")
        if not 0.0 < eps:
            raise ValueError(f"Invalid epsilon value: {eps} (must be > 0)")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if max_grad_norm is not None and not (max_grad_norm > 0 and math.isfinite(max_grad_norm)):
            raise ValueError(f"Invalid max_grad_norm: {max_grad_norm}")
        self.max_grad_norm = max_grad_norm
        self.last_grad_norm = None
        self._plan = None
        # torch.optim.Adam's group keys, so that a state dict of this class loads into it as it is
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=False, foreach=None,
                        capturable=False, differentiable=False, fused=None, decoupled_weight_decay=decoupled_weight_decay)
        super().__init__(params, defaults)

    def __setstate__(self, state):
        super().__setstate__(state)
        self.__dict__.setdefault("max_grad_norm", None)
        self.__dict__.setdefault("last_grad_norm", None)
        self._plan = None
        for g in self.param_groups:
            g.setdefault("amsgrad", False)
            g.setdefault("decoupled_weight_decay", False)

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        for p in self.param_groups[-1]["params"]:
            if p.requires_grad:                              # (frozen tensors never enter the plan)
                _check_tensor("parameter", p)
        self._plan = None

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._plan = None

    # ---------------------------------------------------------------------------------------------------------------- the plan
    def _state_of(self, p, amsgrad):
        st = self.state[p]
        if "exp_avg" not in st:
            st["step"] = torch.zeros((), dtype=torch.float32, device=p.device)
            st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
            st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        if amsgrad and "max_exp_avg_sq" not in st:
            st["max_exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
        s = st["step"]
        if not (isinstance(s, torch.Tensor) and s.device == p.device and s.dtype == torch.float32 and s.numel() == 1):
            st["step"] = torch.tensor(float(s), dtype=torch.float32, device=p.device)      # torch's default Adam counts on the host
        for k in ("exp_avg", "exp_avg_sq") + (("max_exp_avg_sq",) if amsgrad else ()):
            _check_tensor(k, st[k], like=p)
        return st

    def _build(self, entries, key):
        """entries: [(param, grad or None, group index, amsgrad)] of every parameter that requires grad, in group order"""
        if torch.cuda.is_current_stream_capturing():
            raise VqvaeHipError("the optimizer's plan changed under stream capture (a parameter or gradient moved): capture needs static "
                                "gradient tensors and one eager step on them first")
        L = _lib.load()
        n = len(entries)
        dev = entries[0][0].device
        cols = [[] for _ in range(6)]
        states = []
        for p, g, gi, ams in entries:
            _check_tensor("parameter", p)
            if p.device != dev:
                raise ValueError("all parameters of one optimizer must be on one device")
            if g is not None:
                _check_tensor("gradient", g, like=p)
            st = self._state_of(p, ams)
            # (the dict and the tensors the plan points at: kept alive, and compared by identity every step)
            states.append((st, st["step"], st["exp_avg"], st["exp_avg_sq"], st["max_exp_avg_sq"] if ams else None))
            for c, t in zip(cols, (p, g, st["exp_avg"], st["exp_avg_sq"], st["max_exp_avg_sq"] if ams else None, st["step"])):
                # (an empty tensor has no address: its counter's stands in, never dereferenced, so that the table still says
                # whether the tensor has a gradient -- its counter advances as torch's does)
                c.append(None if t is None else t.data_ptr() if t.numel() else st["step"].data_ptr())
        numel = (C.c_int64 * n)(*[e[0].numel() for e in entries])
        arrs = [(C.c_void_p * n)(*c) for c in cols]
        group = (C.c_int * n)(*[e[2] for e in entries])
        nbytes = L.vqvae_adam_plan_bytes(n, numel)
        if nbytes == 0:
            raise VqvaeHipError("vqvae_adam_plan_bytes refused the parameter set")
        host = torch.empty(nbytes, dtype=torch.uint8)
        n_chunks = C.c_int64()
        _lib.check(L.vqvae_adam_plan_write(n, numel, *arrs, group, len(self.param_groups), host.data_ptr(), nbytes, C.byref(n_chunks)))
        pl = _Plan()
        pl.key, pl.nbytes, pl.n_tensors, pl.n_chunks = key, nbytes, n, n_chunks.value
        pl.params = [e[0] for e in entries]
        pl.states = states
        pl.updated = [e[0] for e in entries if e[1] is not None]
        pl.dev = host.to(dev)
        pl.ws = pl.norm = None
        if self.max_grad_norm is not None:
            pl.ws = torch.empty(L.vqvae_grad_norm_workspace_bytes(pl.n_chunks), dtype=torch.uint8, device=dev)
            pl.norm = torch.zeros(2, dtype=torch.float32, device=dev)                     # [total_norm, clip_coef]
        return pl

    # ---------------------------------------------------------------------------------------------------------------- the step
    @torch.no_grad()
    def step(self, closure=None, *, zero_grad=False):
        """One update of every parameter that has a gradient (parameters whose .grad is None keep their value, state and counter).
        zero_grad=True also zeroes, in the same pass, the gradients it consumed; the update's bits do not depend on it."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if len(self.param_groups) > MAX_GROUPS:
            raise VqvaeHipError(f"at most {MAX_GROUPS} parameter groups")
        entries, key, hyper = [], [], (_lib.VqvaeAdamGroup * len(self.param_groups))()
        any_grad = False
        for gi, group in enumerate(self.param_groups):
            for k in _REFUSED:
                if group.get(k):
                    raise ValueError(f"{k}={group[k]!r}: the HIP optimizer has one implementation and does not take this option")
            if isinstance(group["lr"], torch.Tensor):
                raise ValueError("lr must be a Python number: hyper-parameters travel as launch arguments")
            h = hyper[gi]
            h.lr, (h.beta1, h.beta2), h.eps, h.weight_decay = group["lr"], group["betas"], group["eps"], group["weight_decay"]
            h.flags = DECOUPLED_WD if group.get("decoupled_weight_decay") else 0
            ams = bool(group["amsgrad"])
            for p in group["params"]:
                if not p.requires_grad:
                    continue
                g = p.grad
                if g is not None:
                    if g.is_sparse:
                        raise ValueError("sparse gradients are not supported")
                    any_grad = True
                entries.append((p, g, gi, ams))
                key.append((p.data_ptr(), g.data_ptr() if g is not None else 0, gi, ams))
        if not any_grad:
            return loss
        pl = self._plan
        if pl is None or pl.key != key or (pl.norm is None) != (self.max_grad_norm is None) or not self._states_unchanged(pl):
            pl = self._plan = self._build(entries, key)
        L = _lib.load()
        stream = _lib.stream_ptr(pl.dev)
        clip = None
        if self.max_grad_norm is not None:
            out = pl.norm
            _lib.check(L.vqvae_grad_norm_f32(pl.dev.data_ptr(), pl.nbytes, pl.n_tensors, pl.n_chunks, float(self.max_grad_norm),
                                             out.data_ptr(), out.data_ptr() + 4, *_lib.ws_args(pl.ws), stream))
            self.last_grad_norm = out[0]
            clip = out.data_ptr() + 4
        _lib.check(L.vqvae_adam_step_f32(pl.dev.data_ptr(), pl.nbytes, pl.n_tensors, pl.n_chunks, hyper, len(self.param_groups),
                                         ZERO_GRAD if zero_grad else 0, clip, stream))
        # the packed-weight and codebook caches of this package are keyed on (data_ptr, _version): a raw-pointer write must bump it
        torch.autograd.graph.increment_version(pl.updated)
        return loss

    def _states_unchanged(self, pl):
        state = self.state
        for p, (st, step, m, v, vmax) in zip(pl.params, pl.states):
            if state.get(p) is not st or st.get("step") is not step or st.get("exp_avg") is not m or st.get("exp_avg_sq") is not v \
                    or (vmax is not None and st.get("max_exp_avg_sq") is not vmax):
                return False
        return True


def _check_tensor(what, t, like=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise VqvaeHipError(f"{what} must be on the GPU: the HIP optimizer has no CPU fallback")
    if t.dtype != torch.float32:
        raise VqvaeHipError(f"{what} must be float32, not {t.dtype}")
    if t.layout != torch.strided or not t.is_contiguous():
        raise VqvaeHipError(f"{what} must be dense and contiguous")
    if like is not None and (t.shape != like.shape or t.device != like.device):
        raise VqvaeHipError(f"{what} does not match its parameter's shape or device")
