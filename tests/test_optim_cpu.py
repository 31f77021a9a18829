"""CPU tests of the HIP optimizer (vqvae_amd/optim.py, csrc/optim.hip): the fp64 restatement the GPU tests compare with is itself
checked against torch's CPU Adam; the new C entries' argument errors and the plan's host logic need no GPU; the class refuses CPU
tensors."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import adam_ref as R

CONFIGS = [dict(amsgrad=False), dict(amsgrad=True), dict(amsgrad=True, wd=1e-2), dict(amsgrad=False, wd=1e-2, decoupled=True)]


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()))
def test_restatement_matches_torch_cpu_adam(cfg):
    _torch_cpu_against_restatement(cfg, 2048, enforce=cfg.get("wd", 0.0) == 0)


def test_torch_fp32_step_at_70001_elements_is_printed_not_asserted():
    """The GPU tests' largest tensor.  Among this many elements m' = m + (1 - b1)(g - m) nearly cancels in a few, and torch's fp32
    step leaves the single-step bound on p there (several times the bound; the figure is printed, and depends on the seeds): the
    bound and fp32 arithmetic do not go together at this size, which is why the HIP kernel evaluates in fp64.  Asserted: the
    trajectory, and that the restatement's m and v bounds still hold for torch (they are absolute, not relative to the step)."""
    worst = _torch_cpu_against_restatement(dict(amsgrad=False), 70001, enforce=False)
    assert worst["m"] <= 1.0 and worst["v"] <= 1.0


def _torch_cpu_against_restatement(cfg, n, enforce):
    """50 steps of the input family: torch's fp32 single-tensor Adam, restarted from its own fp32 state at every step, stays within
    the single-step bounds of the fp64 restatement -- so the restatement states torch's arithmetic, and the bounds leave the
    reference itself room.  Also the whole trajectory: torch's fp32 result lies within a few 1e-7 of the fp64 one.
    With weight decay only the trajectory is asserted and the per-step figures are printed.  Coupled: torch forms g + wd * p in
    fp32, whose error of 2^-24 |wd p| per rounding is not bounded by any multiple of |g'| where the two nearly cancel (measured on
    this family: 1.5 x the bound on m, 7 x on v).  Decoupled: fp32(1 - lr wd), the product with p and the final subtraction are three
    roundings of 2^-24 |p| against the bound's 2^-23 |p'| (measured: 1.008 x the bound on p).  The same happens to the bound on p
    without any decay once there are enough elements for m' = m + (1 - b1)(g - m) to nearly cancel in one of them (g ~ -9 m): the
    errors of m' scale with max(|m|, |g|), the bound with |p' - p|; 2 048 elements stay inside, 70 001 do not (the next test).  That is
    why the HIP kernel evaluates the step in fp64 and rounds each result once; it is held to the bounds at every size and with either
    decay: tests/test_optim_gpu.py."""
    steps = 50
    p0, grads = R.family_params(n, 11), R.family_grads(n, steps, 12)
    kw = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, **cfg)
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([p], lr=kw["lr"], betas=(0.9, 0.999), eps=kw["eps"], weight_decay=cfg.get("wd", 0.0),
                           amsgrad=cfg["amsgrad"], foreach=False, decoupled_weight_decay=cfg.get("decoupled", False))
    m = v = np.zeros(n, np.float32)
    vmax = np.zeros(n, np.float32) if cfg["amsgrad"] else None
    cur = p0
    worst = {}
    for t, g in enumerate(grads, 1):
        ref = R.step(cur, g, m, v, vmax, t, **kw)
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        st = opt.state[p]
        got = {"p": p.detach().numpy().copy(), "m": st["exp_avg"].numpy().copy(), "v": st["exp_avg_sq"].numpy().copy()}
        if cfg["amsgrad"]:
            got["vmax"] = st["max_exp_avg_sq"].numpy().copy()
        w = R.check_step(got, ref, cur, m, cfg["amsgrad"], where=f"torch cpu n={n} t={t}", enforce=enforce)
        worst = {k: max(worst.get(k, 0.0), r) for k, r in w.items()}
        cur, m, v, vmax = got["p"], got["m"], got["v"], got.get("vmax")
    print("torch cpu worst error / bound over the trajectory:", worst)
    p64 = R.trajectory(p0, grads, **kw)
    bound, terr, pmax = R.trajectory_bound(p64, cur)
    print(f"torch cpu trajectory error vs fp64: {terr:.3e} at max|p| {pmax:.3f}")
    assert terr < 1e-6
    return worst


def test_grad_norm_reference_and_clip_coef():
    g = [np.array([3.0, 0.0], np.float32), np.array([4.0], np.float32)]
    assert R.grad_norm(g) == 5.0
    assert R.clip_coef(5.0, 10.0) == 1.0 and abs(R.clip_coef(5.0, 1.0) - 1.0 / (5.0 + 1e-6)) < 1e-15


# ------------------------------------------------------------------------------------------------------- C entries, host side only
A = 4096          # a fake, 16-byte aligned "device pointer" (never dereferenced)


def _lib():
    from vqvae_amd import _lib
    return _lib, _lib.load()


def _groups(_lib, *rows):
    g = (_lib.VqvaeAdamGroup * len(rows))()
    for i, (lr, b1, b2, eps, wd) in enumerate(rows):
        g[i].lr, g[i].beta1, g[i].beta2, g[i].eps, g[i].weight_decay = lr, b1, b2, eps, wd
    return g


def _plan(L, numels, grads=None, groups=None, n_groups=1):
    n = len(numels)
    numel = (C.c_int64 * n)(*numels)
    ptr = lambda base, skip=None: (C.c_void_p * n)(*[None if skip and skip[i] else base + 64 * i for i in range(n)])
    nbytes = L.vqvae_adam_plan_bytes(n, numel)
    blob = np.zeros(nbytes, np.uint8)
    nch = C.c_int64(-1)
    rc = L.vqvae_adam_plan_write(n, numel, ptr(A), ptr(2 * A, [g is None for g in grads] if grads else None), ptr(3 * A), ptr(4 * A),
                                 None, ptr(5 * A), (C.c_int * n)(*(groups or [0] * n)), n_groups, blob.ctypes.data, nbytes, C.byref(nch))
    return rc, blob, nch.value, nbytes


def test_step_and_norm_argument_errors_without_gpu():
    """every refusal is a negative code, returned before any HIP call"""
    _l, L = _lib()
    ok = _groups(_l, (1e-3, 0.9, 0.999, 1e-8, 0.0))
    big = 1 << 20
    step = L.vqvae_adam_step_f32
    assert step(None, big, 1, 1, ok, 1, 0, None, None) == -1                       # NULL plan
    assert step(A, big, 1, 1, None, 1, 0, None, None) == -1                        # NULL groups
    assert step(A, big, 0, 1, ok, 1, 0, None, None) == -2                          # n_tensors <= 0
    assert step(A, big, -3, 1, ok, 1, 0, None, None) == -2
    assert step(A, big, 1, -1, ok, 1, 0, None, None) == -2
    assert step(A, big, 1, 1, ok, 0, 0, None, None) == -2                          # no group
    assert step(A, big, 1, 1, ok, 17, 0, None, None) == -3                         # more groups than launch arguments carry
    assert step(A + 4, big, 1, 1, ok, 1, 0, None, None) == -3                      # misaligned plan
    assert step(A, big, 1, 1, ok, 1, 0x2, None, None) == -3                        # unknown flag
    assert step(A, 64 + 64 + 8 + 79, 1, 1, ok, 1, 0, None, None) == -4             # plan size too small: header, 1 tensor, 1 chunk, scratch
    for bad in (0.0, -1e-3, float("inf"), float("nan")):
        assert step(A, big, 1, 1, _groups(_l, (bad, 0.9, 0.999, 1e-8, 0.0)), 1, 0, None, None) == -3       # lr
        assert step(A, big, 1, 1, _groups(_l, (1e-3, 0.9, 0.999, bad, 0.0)), 1, 0, None, None) == -3       # eps
    for bad in (1.0, -0.1, 1.5, float("nan")):
        assert step(A, big, 1, 1, _groups(_l, (1e-3, bad, 0.999, 1e-8, 0.0)), 1, 0, None, None) == -3      # beta1 outside [0, 1)
        assert step(A, big, 1, 1, _groups(_l, (1e-3, 0.9, bad, 1e-8, 0.0)), 1, 0, None, None) == -3        # beta2
    assert step(A, big, 1, 1, _groups(_l, (1e-3, 0.9, 0.999, 1e-8, -1.0)), 1, 0, None, None) == -3         # weight decay
    # a bad second group is found too
    assert step(A, big, 1, 1, _groups(_l, (1e-3, 0.9, 0.999, 1e-8, 0.0), (0.0, 0.9, 0.999, 1e-8, 0.0)), 2, 0, None, None) == -3
    norm = L.vqvae_grad_norm_f32
    assert L.vqvae_grad_norm_workspace_bytes(3) >= 24 and L.vqvae_grad_norm_workspace_bytes(-1) == 0
    assert norm(None, big, 1, 1, 1.0, A, A, A, big, None) == -1
    assert norm(A, big, 1, 1, 1.0, None, A, A, big, None) == -1
    assert norm(A, big, 0, 1, 1.0, A, A, A, big, None) == -2
    assert norm(A, 100, 1, 1, 1.0, A, A, A, big, None) == -4
    assert norm(A, big, 1, 3, 1.0, A, A, A, 16, None) == -4                        # workspace too small
    assert norm(A, big, 1, 3, 1.0, A, A, None, 0, None) == -4
    assert norm(A, big, 1, 1, 0.0, A, A, A, big, None) == -3                       # max_norm <= 0 with a clip output
    assert norm(A, big, 1, 1, float("nan"), A, A, A, big, None) == -3


def test_plan_host_logic():
    """vqvae_adam_plan_bytes / _plan_write: chunk counts around the chunk size, no chunk for an empty or a skipped tensor, chunk
    order = tensor order, and the refusals"""
    _l, L = _lib()
    ch = L.vqvae_adam_chunk_elems()
    assert ch == 4096
    numels = [0, 1, ch - 1, ch, ch + 1, 3 * ch]
    want = [0, 1, 1, 1, 2, 3]
    rc, blob, nch, nbytes = _plan(L, numels)
    assert rc == 0 and nch == sum(want)
    hd = blob[:64].view(np.int64)
    assert hd[1] == len(numels) and hd[2] == nch and hd[3] == ch and hd[4] == 64 and hd[7] == nbytes
    assert hd[5] == 64 + 64 * len(numels) and hd[6] >= hd[5] + 8 * nch and hd[6] % 16 == 0 and hd[7] == hd[6] + 80 * len(numels)
    tens = blob[64:64 + 64 * len(numels)].view(np.int64).reshape(-1, 8)
    assert tens[:, 6].tolist() == numels
    assert tens[:, 0].tolist() == [A + 64 * i for i in range(len(numels))] and (tens[:, 4] == 0).all()      # no max_exp_avg_sq
    chunks = blob[hd[5]:hd[5] + 8 * nch].view(np.int32).reshape(-1, 2)
    assert chunks.tolist() == [[i, k] for i, w in enumerate(want) for k in range(w)]
    for n, w in zip(numels, want):                        # each size alone
        if w:
            assert _plan(L, [n])[2] == w
    assert _plan(L, [0])[:3:2] == (0, 0)                  # only an empty tensor: a valid plan without chunks
    # a tensor without a gradient: in the table (NULL grad), in no chunk
    rc, blob, nch, _ = _plan(L, [ch + 1, 5, 7], grads=[1, None, 1])
    hd = blob[:64].view(np.int64)
    assert rc == 0 and nch == 3 and blob[64:64 + 192].view(np.int64).reshape(-1, 8)[1, 1] == 0
    assert blob[hd[5]:hd[5] + 24].view(np.int32).reshape(-1, 2).tolist() == [[0, 0], [0, 1], [2, 0]]
    # two groups
    rc, blob, _, _ = _plan(L, [5, 7], groups=[1, 0], n_groups=2)
    assert rc == 0 and blob[64:64 + 128].view(np.int32).reshape(-1, 16)[:, 14].tolist() == [1, 0]
    assert _plan(L, [5, 7], groups=[2, 0], n_groups=2)[0] == -2          # group index out of range
    # refusals
    one = (C.c_int64 * 1)(8)
    assert L.vqvae_adam_plan_bytes(0, one) == 0 and L.vqvae_adam_plan_bytes(1, None) == 0
    assert L.vqvae_adam_plan_bytes(1, (C.c_int64 * 1)(-1)) == 0
    p = (C.c_void_p * 1)(A)
    odd = (C.c_void_p * 1)(A + 2)
    g0 = (C.c_int * 1)(0)
    buf = np.zeros(1024, np.uint8)
    nch = C.c_int64()
    w = L.vqvae_adam_plan_write
    assert w(1, one, p, p, p, p, None, p, g0, 1, None, 1024, C.byref(nch)) == -1
    assert w(1, one, (C.c_void_p * 1)(None), p, p, p, None, p, g0, 1, buf.ctypes.data, 1024, C.byref(nch)) == -1
    assert w(0, one, p, p, p, p, None, p, g0, 1, buf.ctypes.data, 1024, C.byref(nch)) == -2
    assert w(1, one, p, odd, p, p, None, p, g0, 1, buf.ctypes.data, 1024, C.byref(nch)) == -3          # not an fp32 address
    assert w(1, one, p, p, p, p, None, p, g0, 17, buf.ctypes.data, 1024, C.byref(nch)) == -3
    assert w(1, one, p, p, p, p, None, p, g0, 1, buf.ctypes.data, 64, C.byref(nch)) == -4


def test_class_refuses_cpu_tensors_and_foreign_options():
    from vqvae_amd import optim
    from vqvae_amd._lib import VqvaeHipError
    w = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(VqvaeHipError, match="GPU"):
        optim.Adam([w])
    for k in ("maximize", "foreach", "fused", "capturable", "differentiable"):
        with pytest.raises(ValueError, match=k):
            optim.Adam([w], **{k: True})
    with pytest.raises(TypeError):
        optim.Adam([w], nesterov=True)
    for kw in (dict(lr=-1.0), dict(lr=0.0), dict(eps=-1.0), dict(eps=0.0), dict(betas=(1.0, 0.9)), dict(betas=(0.9, -0.1)), dict(weight_decay=-1.0),
               dict(max_grad_norm=0.0), dict(lr=torch.tensor(1e-3))):
        with pytest.raises(ValueError):
            optim.Adam([w], **kw)
    frozen = torch.nn.Parameter(torch.zeros(4), requires_grad=False)      # never enters the plan: nothing to refuse, nothing to do
    opt = optim.Adam([frozen])
    assert opt.step() is None and opt.state_dict()["state"] == {}
    assert issubclass(optim.Adam, torch.optim.Optimizer)
    assert set(torch.optim.Adam([w]).param_groups[0]) <= set(opt.param_groups[0])      # torch's group keys: state dicts move both ways
