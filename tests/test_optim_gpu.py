"""GPU tests of the HIP optimizer (vqvae_amd/optim.py, csrc/optim.hip) against the fp64 restatement tests/adam_ref.py.

The bounds count roundings (adam_ref.check_step, adam_ref.trajectory_bound); none is tuned to the kernel.  Shapes are the smallest at
which the kernel can go wrong: sizes around the 4-element vector, the 64-lane wave, the 256-lane workgroup and the 4096-element chunk,
each as its own (16-byte aligned) allocation and as a 4-byte aligned view into a flat buffer."""
import copy

import numpy as np
import pytest
import torch

from tests import adam_ref as R

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 5, 63, 64, 65, 255, 257, 1023, 4097, 70001]
HYPER = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)
SENTINEL = 123.25


def dev():
    return torch.device("cuda:0")


def make_opt(params, cfg, **kw):
    from vqvae_amd import optim
    return optim.Adam(params, lr=cfg.get("lr", HYPER["lr"]), betas=(HYPER["b1"], HYPER["b2"]), eps=HYPER["eps"],
                      weight_decay=cfg.get("wd", 0.0), amsgrad=cfg.get("amsgrad", False),
                      decoupled_weight_decay=cfg.get("decoupled", False), **kw)


def ref_kw(cfg, **over):
    return {**HYPER, **{k: v for k, v in cfg.items() if k in ("wd", "decoupled", "amsgrad", "lr")}, **over}


class Flat:
    """p, g, m, v, vmax of several tensors laid out per `layout`: 'own' = one allocation per tensor and array (16-byte aligned);
    'flat' = consecutive views from element 1 of one flat buffer per array (4-byte aligned, tensors meeting inside a 16-byte line),
    with sentinels in front and behind"""

    def __init__(self, sizes, layout, seed, amsgrad, t0=0, gscale=1.0):
        rng = np.random.default_rng(seed)
        self.sizes, self.layout, self.amsgrad, self.t0 = sizes, layout, amsgrad, t0
        self.host = []
        for i, n in enumerate(sizes):
            p = R.family_params(n, seed * 1000 + i)
            g = gscale * 10.0 ** rng.uniform(-6, 2) * rng.standard_normal(n)             # the family's scales (adam_ref.family_grads)
            g = np.where(np.abs(g) < 1e-12, np.where(g < 0, -1e-12, 1e-12), g).astype(np.float32)
            if t0:
                m, v, vmax = R.preset_state(n, seed * 1000 + 500 + i, amsgrad)
            else:
                m, v, vmax = np.zeros(n, np.float32), np.zeros(n, np.float32), (np.zeros(n, np.float32) if amsgrad else None)
            self.host.append(dict(p=p, g=g, m=m, v=v, vmax=vmax))
        names = ["p", "g", "m", "v"] + (["vmax"] if amsgrad else [])
        self.views = {k: [] for k in names}
        self.bufs = {}
        if layout == "flat":
            total = 1 + sum(sizes) + 7
            for k in names:
                buf = torch.full((total,), SENTINEL, dtype=torch.float32, device=dev())
                off = 1
                for h in self.host:
                    n = h["p"].shape[0]
                    buf[off:off + n] = torch.from_numpy(h[k])
                    self.views[k].append(buf[off:off + n])
                    off += n
                self.bufs[k] = buf
        else:
            for k in names:
                self.views[k] = [torch.from_numpy(h[k]).to(dev()) for h in self.host]
        self.params = [torch.nn.Parameter(t) for t in self.views["p"]]
        for p, g in zip(self.params, self.views["g"]):
            p.grad = g

    def attach_state(self, opt):
        for i, p in enumerate(self.params):
            st = {"step": torch.tensor(float(self.t0), device=dev()), "exp_avg": self.views["m"][i], "exp_avg_sq": self.views["v"][i]}
            if self.amsgrad:
                st["max_exp_avg_sq"] = self.views["vmax"][i]
            opt.state[p] = st

    def read(self, i):
        out = {"p": self.params[i].detach().cpu().numpy(), "m": self.views["m"][i].cpu().numpy(), "v": self.views["v"][i].cpu().numpy()}
        if self.amsgrad:
            out["vmax"] = self.views["vmax"][i].cpu().numpy()
        return out

    def check_sentinels(self):
        for k, buf in self.bufs.items():
            b = buf.cpu().numpy()
            n = sum(self.sizes)
            assert b[0] == SENTINEL and (b[1 + n:] == SENTINEL).all(), f"{k}: written outside the views"

    def check_against_ref(self, cfg, where, skip=(), **over):
        for i, h in enumerate(self.host):
            if i in skip or h["p"].shape[0] == 0:
                continue
            ref = R.step(h["p"], h["g"], h["m"], h["v"], h["vmax"], self.t0 + 1, **ref_kw(cfg, **over))
            R.check_step(self.read(i), ref, h["p"], h["m"], self.amsgrad, where=f"{where} numel={h['p'].shape[0]}")


# ------------------------------------------------------------------------------------------------------------------ 1. single step
@pytest.mark.parametrize("t0", [0, 999], ids=["t1", "t1000"])
@pytest.mark.parametrize("wd", [dict(), dict(wd=1e-2), dict(wd=1e-2, decoupled=True)], ids=["wd0", "coupled", "decoupled"])
@pytest.mark.parametrize("amsgrad", [False, True], ids=["adam", "amsgrad"])
@pytest.mark.parametrize("layout", ["own", "flat"])
def test_single_step_against_restatement(layout, amsgrad, wd, t0):
    cfg = dict(amsgrad=amsgrad, **wd)
    f = Flat(SIZES, layout, 7, amsgrad, t0=t0)
    opt = make_opt(f.params, cfg)
    f.attach_state(opt)
    g_before = [g.clone() for g in f.views["g"]]
    opt.step()
    torch.cuda.synchronize()
    f.check_against_ref(cfg, f"{layout} t={t0 + 1}")
    f.check_sentinels()
    for p, g, g0 in zip(f.params, f.views["g"], g_before):
        assert opt.state[p]["step"].item() == t0 + 1
        assert torch.equal(g, g0)                                        # zero_grad=False leaves the gradients alone
    if layout == "flat":                                                   # the views really are only 4-byte aligned
        assert any(p.data_ptr() % 16 for p in f.params)
    else:
        assert all(p.data_ptr() % 16 == 0 for p in f.params)


# ------------------------------------------------------------------------------------------------------------------- 2. trajectory
TRAJ_CONFIGS = {"adam": dict(amsgrad=False), "amsgrad": dict(amsgrad=True), "amsgrad-coupled": dict(amsgrad=True, wd=1e-2),
                "adamw": dict(amsgrad=False, wd=1e-2, decoupled=True)}
TRAJ_N, TRAJ_STEPS = 4097, 50
_traj_cache = {}


def traj_refs(name):
    """(p0, recorded gradients, fp64 final p, torch CPU fp32 final p) of a configuration: computed once, never modified"""
    if name not in _traj_cache:
        p0, grads = R.family_params(TRAJ_N, 21), R.family_grads(TRAJ_N, TRAJ_STEPS, 22)
        kw = ref_kw(TRAJ_CONFIGS[name])
        out = (p0, grads, R.trajectory(p0, grads, **kw), R.torch_cpu_trajectory(p0, grads, **kw))
        for a in out:
            a.setflags(write=False)
        _traj_cache[name] = out
    return _traj_cache[name]


def check_trajectory(p_final, name, where):
    _, _, p64, p_torch = traj_refs(name)
    bound, torch_err, pmax = R.trajectory_bound(p64, p_torch)
    err = float(np.abs(p_final.astype(np.float64) - p64).max())
    print(f"{where} [{name}]: error vs fp64 {err:.3e}; torch cpu fp32 {torch_err:.3e}; bound {bound:.3e}; max|p| {pmax:.3f}")
    assert err <= bound, f"{where} [{name}]: {err:.3e} > {bound:.3e} (torch's own error {torch_err:.3e})"


@pytest.mark.parametrize("name", list(TRAJ_CONFIGS))
def test_trajectory_of_50_steps(name):
    p0, grads, _, _ = traj_refs(name)
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()).to(dev()))
    opt = make_opt([p], TRAJ_CONFIGS[name])
    gd = torch.from_numpy(grads.copy()).to(dev())
    p.grad = torch.empty_like(p)
    for s in range(TRAJ_STEPS):
        p.grad.copy_(gd[s])
        opt.step()
    assert opt.state[p]["step"].item() == TRAJ_STEPS
    check_trajectory(p.detach().cpu().numpy(), name, "HIP")


# -------------------------------------------------------------------------------------------------- 3. tensor count and skipping
def test_300_tensors_two_groups_empty_and_skipped():
    rng = np.random.default_rng(3)
    sizes = [int(s) for s in rng.integers(1, 300, 300)]
    sizes[5], sizes[17], sizes[140], sizes[299] = 4096, 8193, 0, 5000
    cfg = dict(amsgrad=True)
    f = Flat(sizes, "own", 3, True)
    lrs = [1e-3, 2.5e-4]
    opt = make_opt([{"params": f.params[:120], "lr": lrs[0]}, {"params": f.params[120:], "lr": lrs[1]}], cfg)
    f.attach_state(opt)
    opt.step()                                                             # every tensor has a gradient: all counters 1
    torch.cuda.synchronize()
    for i in range(300):
        if sizes[i]:
            h = f.host[i]
            ref = R.step(h["p"], h["g"], h["m"], h["v"], h["vmax"], 1, **ref_kw(cfg, lr=lrs[i >= 120]))
            if i % 37 == 0 or sizes[i] > 300:
                R.check_step(f.read(i), ref, h["p"], h["m"], True, where=f"tensor {i} step 1")
        assert opt.state[f.params[i]]["step"].item() == 1
    # second step: two tensors without a gradient
    skipped = (9, 200)
    for i in range(300):
        got = f.read(i)
        f.host[i].update(p=got["p"].copy(), m=got["m"].copy(), v=got["v"].copy(), vmax=got["vmax"].copy())
    f.t0 = 1
    for i in skipped:
        f.params[i].grad = None
    versions = [p._version for p in f.params]
    opt.step()
    torch.cuda.synchronize()
    for i in skipped:
        got, h = f.read(i), f.host[i]
        for k in ("p", "m", "v", "vmax"):
            assert np.array_equal(got[k].view(np.uint32), h[k].view(np.uint32)), (i, k)
        assert opt.state[f.params[i]]["step"].item() == 1 and f.params[i]._version == versions[i]
    for i in range(300):
        if i in skipped:
            continue
        assert opt.state[f.params[i]]["step"].item() == 2 and f.params[i]._version > versions[i]
        if sizes[i]:
            h = f.host[i]
            ref = R.step(h["p"], h["g"], h["m"], h["v"], h["vmax"], 2, **ref_kw(cfg, lr=lrs[i >= 120]))
            R.check_step(f.read(i), ref, h["p"], h["m"], True, where=f"tensor {i} step 2")


# ------------------------------------------------------------------------------------------------- 4. partition independence
def _partition_run(cuts, data, cfg, zero_grad=False, steps=2):
    """the flat data updated as the tensors [cuts[i], cuts[i + 1]) -> flat p, m, v, vmax after `steps` steps (uint32 views)"""
    N = data["p"].shape[0]
    bufs = {k: torch.from_numpy(data[k].copy()).to(dev()) for k in ("p", "m", "v", "vmax")}
    gbuf = torch.empty(N, dtype=torch.float32, device=dev())
    params = [torch.nn.Parameter(bufs["p"][a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    opt = make_opt(params, cfg)
    for p, a, b in zip(params, cuts[:-1], cuts[1:]):
        p.grad = gbuf[a:b]
        opt.state[p] = {"step": torch.tensor(0.0, device=dev()), "exp_avg": bufs["m"][a:b], "exp_avg_sq": bufs["v"][a:b],
                        "max_exp_avg_sq": bufs["vmax"][a:b]}
    for s in range(steps):
        gbuf.copy_(torch.from_numpy(data["g"][s]))
        opt.step(zero_grad=zero_grad)
        if zero_grad:
            assert not gbuf.any()
    torch.cuda.synchronize()
    return {k: bufs[k].cpu().numpy().view(np.uint32) for k in bufs}


def _partition_data(N=20003):
    z = np.zeros(N, np.float32)
    return dict(p=R.family_params(N, 41), g=R.family_grads(N, 2, 42) * np.float32(1e-2), m=z, v=z, vmax=z)


def test_partition_independence_and_run_to_run_bits():
    data = _partition_data()
    N = data["p"].shape[0]
    rng = np.random.default_rng(4)
    parts = {"1": [0, N], "7": [0, 1, 6, 70, 4167, 4168, 12361, N],
             "300": [0] + sorted(int(c) for c in rng.choice(np.arange(1, N), 299, replace=False)) + [N]}
    cfg = dict(amsgrad=True, wd=1e-2)
    res = {k: _partition_run(c, data, cfg) for k, c in parts.items()}
    for k, c in parts.items():
        again = _partition_run(c, data, cfg)
        for a in res[k]:
            assert np.array_equal(res[k][a], again[a]), f"{k} tensors: {a} differs between two runs"
            assert np.array_equal(res[k][a], res["1"][a]), f"{a}: {k} tensors and 1 tensor give different bits"
    assert not np.array_equal(res["1"]["p"], data["p"].view(np.uint32))


# ----------------------------------------------------------------------------------------------------------- 5. fused zeroing
def test_fused_zero_grad_same_update_bits():
    data = _partition_data()
    N = data["p"].shape[0]
    cuts = [0, 3, 4099, 4100, 12361, N]
    cfg = dict(amsgrad=True, wd=1e-2)
    plain, zeroed = _partition_run(cuts, data, cfg), _partition_run(cuts, data, cfg, zero_grad=True)     # (asserts the grads are zero)
    for a in plain:
        assert np.array_equal(plain[a], zeroed[a]), a
    f = Flat(SIZES, "own", 9, False)                                    # aligned allocations: the 16-byte path's zeroing
    opt = make_opt(f.params, dict())
    f.attach_state(opt)
    opt.step(zero_grad=True)
    assert all(not g.any() for g in f.views["g"])
    f.check_against_ref(dict(), "zero_grad own")


# ------------------------------------------------------------------------------------------------- 6. cache freshness on a model
def _model_cases():
    def vqvae():
        from vqvae_amd import conv
        from vqvae_amd.modules import VQVAE
        conv.set_conv_backend("hip")
        torch.manual_seed(11)
        m = VQVAE(64, 16, 1, 64, 32, 0.25)
        x = torch.randn(6, 3, 16, 16).to(dev())

        def loss(mod):
            el, xh, _ = mod(x)
            return torch.mean((xh - x) ** 2) / 0.06 + el
        return m, (lambda: VQVAE(64, 16, 1, 64, 32, 0.25)), loss, (lambda mod: mod(x)[1])

    def prior():
        from tests import pixelcnn_envelope as E
        from vqvae_amd.pixelcnn import GatedPixelCNN, cross_entropy
        K, dim, nl, ncls, B, side = E.MODEL_CASES["k12_d20_l2_c3_b5_s7"]
        m = E.build(K, dim, nl, ncls)
        x, label = (t.to(dev()) for t in E.model_inputs(K, ncls, B, side))
        return m, (lambda: GatedPixelCNN(K, dim, nl, ncls)), (lambda mod: cross_entropy(mod(x, label), x)), (lambda mod: mod(x, label))
    return {"vqvae": vqvae, "prior": prior}


@pytest.mark.parametrize("which", ["vqvae", "prior"])
def test_model_step_bumps_versions_and_caches_stay_fresh(which):
    """the packed-weight and codebook caches are keyed on (data_ptr, _version): after a raw-pointer update the stepped model must
    compute with the NEW weights"""
    base, fresh, loss_of, eval_of = _model_cases()[which]()
    m = base.to(dev())
    mt = copy.deepcopy(m)
    m.eval()
    with torch.no_grad():
        out_pre = eval_of(m).clone()                                     # fills the caches with the old weights
    m.train()
    mt.train()
    cfg = dict(amsgrad=True, lr=3e-4)                                    # main.py:59
    opt = make_opt(m.parameters(), cfg)
    opt_t = torch.optim.Adam(mt.parameters(), lr=3e-4, amsgrad=True)
    loss_of(m).backward()
    loss_of(mt).backward()
    named = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
    before = {n: (p._version, p.detach().clone(), p.grad.clone() if p.grad is not None else None) for n, p in named}
    for (n, p), (_, q) in zip(named, [(n, q) for n, q in mt.named_parameters() if q.requires_grad]):
        assert (p.grad is None) == (q.grad is None) and (p.grad is None or torch.equal(p.grad, q.grad)), n    # bit-reproducible backward
    opt.step()
    opt_t.step()
    torch.cuda.synchronize()
    assert any(g is not None for _, _, g in before.values())
    for n, p in named:
        v0, p0, g = before[n]
        if g is None:
            assert p._version == v0 and torch.equal(p, p0), n
            continue
        assert p._version > v0, f"{n}: _version did not advance"
        h = dict(p=p0.cpu().numpy().ravel(), g=g.cpu().numpy().ravel())
        z = np.zeros_like(h["p"])
        ref = R.step(h["p"], h["g"], z, z, z, 1, **ref_kw(cfg))
        st = opt.state[p]
        got = {"p": p.detach().cpu().numpy().ravel(), "m": st["exp_avg"].cpu().numpy().ravel(), "v": st["exp_avg_sq"].cpu().numpy().ravel(),
               "vmax": st["max_exp_avg_sq"].cpu().numpy().ravel()}
        R.check_step(got, ref, h["p"], z, True, where=f"{which} {n}")
        # torch's Adam on the same device from the same bits: the single-step bound on p between the two, and torch's own distance
        # from the fp64 step beside it
        q = dict(mt.named_parameters())[n].detach().cpu().numpy().ravel().astype(np.float64)
        bound = R.EPS23 * np.abs(ref["p"]) + R.EPS21 * np.abs(ref["p"] - h["p"])
        ratio = float((np.abs(got["p"].astype(np.float64) - q) / bound).max())
        ratio_t = float((np.abs(q - ref["p"]) / bound).max())
        print(f"{which} {n}: |HIP - torch device Adam| / bound = {ratio:.3f}; |torch device Adam - fp64| / bound = {ratio_t:.3f}")
        assert ratio <= 1.0, f"{n}: HIP against torch's device Adam {ratio:.3f} x the single-step bound (torch against fp64: {ratio_t:.3f})"
    m.eval()
    with torch.no_grad():
        out_post = eval_of(m).clone()
        m2 = fresh().to(dev())
        m2.load_state_dict(m.state_dict())
        m2.eval()
        out_fresh = eval_of(m2)
    assert torch.equal(out_post, out_fresh), "the stepped model computes with stale cached weights"
    assert not torch.equal(out_post, out_pre)


# ---------------------------------------------------------------------------------------------------- 7. state dict both ways
@pytest.mark.parametrize("direction", ["hip_to_torch", "torch_to_hip"])
def test_state_dict_moves_both_ways(direction):
    name = "amsgrad"
    p0, grads, _, _ = traj_refs(name)
    gd = torch.from_numpy(grads.copy()).to(dev())

    def fresh(kind):
        p = torch.nn.Parameter(torch.from_numpy(p0.copy()).to(dev()))
        p.grad = torch.empty_like(p)
        o = make_opt([p], TRAJ_CONFIGS[name]) if kind == "hip" else \
            torch.optim.Adam([p], lr=HYPER["lr"], betas=(HYPER["b1"], HYPER["b2"]), eps=HYPER["eps"], amsgrad=True)
        return p, o

    first, second = ("hip", "torch") if direction == "hip_to_torch" else ("torch", "hip")
    pa, oa = fresh(first)
    for s in range(3):
        pa.grad.copy_(gd[s])
        oa.step()
    pb, ob = fresh(second)
    with torch.no_grad():
        pb.copy_(pa)
    ob.load_state_dict(copy.deepcopy(oa.state_dict()))
    assert set(ob.state[pb]) == {"step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"} and float(ob.state[pb]["step"]) == 3
    assert torch.equal(ob.state[pb]["exp_avg"], oa.state[pa]["exp_avg"])
    for s in range(3, TRAJ_STEPS):
        pb.grad.copy_(gd[s])
        ob.step()
    assert float(ob.state[pb]["step"]) == TRAJ_STEPS
    check_trajectory(pb.detach().cpu().numpy(), name, direction)


# ------------------------------------------------------------------------------------------------------------ 8. stream capture
@pytest.mark.parametrize("clip", [False, True], ids=["plain", "clipping"])
def test_captured_step_equals_eager_steps(tmp_path, clip):
    cfg = dict(amsgrad=True, wd=1e-2)
    sizes = [5, 257, 4097, 9000]
    kw = dict(max_grad_norm=0.5) if clip else {}

    def setup():
        f = Flat(sizes, "own", 13, True, t0=0)
        opt = make_opt(f.params, cfg, **kw)
        f.attach_state(opt)
        return f, opt

    fe, oe = setup()
    for _ in range(3):
        oe.step()
    fg, og = setup()
    init = {k: [t.clone() for t in fg.views[k]] for k in ("p", "m", "v", "vmax")}
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        og.step()                                                         # one eager step: the plan names the static tensors
        for k in init:                                                    # back to the start, in place
            for t, t0 in zip(fg.views[k], init[k]):
                t.detach().copy_(t0)
        for p in fg.params:
            og.state[p]["step"].zero_()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)                             # (keeps the captured graph itself, for the dump below)
    with torch.cuda.graph(g, stream=s):
        og.step(zero_grad=False)
    g.instantiate()
    dot = tmp_path / "step.dot"
    g.debug_dump(str(dot))
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    for i in range(len(sizes)):
        a, b = fe.read(i), fg.read(i)
        for k in a:
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (i, k)
        assert og.state[fg.params[i]]["step"].item() == 3 and oe.state[fe.params[i]]["step"].item() == 3
    if clip:
        assert torch.equal(og.last_grad_norm, oe.last_grad_norm) and float(og.last_grad_norm) > 0.5      # (so the clip was active)
    # the captured step is one chain (two kernel nodes and one edge; four and three when clipping): the dump names the step's
    # kernels, and no node has two successors or two predecessors
    assert dot.exists(), "CUDAGraph.debug_dump wrote no dot file: the captured graph's shape cannot be checked"
    text = dot.read_text()
    edges = [ln for ln in text.splitlines() if "->" in ln]
    names = ["adam_prologue_kernel", "adam_update_kernel"] + (["grad_sq_partial_kernel", "grad_norm_final_kernel"] if clip else [])
    print(f"captured graph: {len(edges)} edges; " + ", ".join(f"{n} x {text.count(n)}" for n in names))
    for n in names:
        assert n in text, f"{n} is not in the dumped graph"
    assert len(edges) >= len(names) - 1, "fewer edges than a chain of the step's kernels has"
    tails = [ln.split("->")[0].strip() for ln in edges]
    heads = [ln.split("->")[1].split("[")[0].strip().rstrip(";") for ln in edges]
    assert len(set(tails)) == len(tails) and len(set(heads)) == len(heads), "a node with two successors or two predecessors"


# ------------------------------------------------------------------------------------------------------------------ 9. clipping
@pytest.mark.parametrize("factor", [0.25, 4.0], ids=["clips", "above-norm"])
def test_global_norm_clipping(factor):
    cfg = dict(amsgrad=True)
    f = Flat(SIZES, "flat", 17, True, t0=999)
    norm64 = R.grad_norm([h["g"] for h in f.host])
    max_norm = float(np.float32(norm64 * factor))
    norms = []
    for rep in range(2):
        fr = Flat(SIZES, "flat", 17, True, t0=999)
        opt = make_opt(fr.params, cfg, max_grad_norm=max_norm)
        fr.attach_state(opt)
        g_before = [g.clone() for g in fr.views["g"]]
        opt.step()
        assert isinstance(opt.last_grad_norm, torch.Tensor) and opt.last_grad_norm.is_cuda
        norms.append(opt.last_grad_norm.cpu().numpy().copy())
        for g, g0 in zip(fr.views["g"], g_before):
            assert torch.equal(g, g0)                                     # the gradients in memory stay unscaled
    rel = abs(float(norms[0]) - norm64) / norm64
    print(f"total_norm {float(norms[0]):.9g} vs fp64 {norm64:.9g}: relative error {rel:.3e} (bound {R.EPS23:.3e})")
    assert rel <= R.EPS23
    assert norms[0].view(np.uint32) == norms[1].view(np.uint32)
    coef = R.clip_coef(norm64, max_norm)
    assert (coef < 1.0) == (factor < 1.0)
    for i, h in enumerate(fr.host):
        ref = R.step(h["p"], h["g"], h["m"], h["v"], h["vmax"], 1000, clip=coef, **ref_kw(cfg))
        got = fr.read(i)
        u = np.abs(ref["p"] - h["p"].astype(np.float64))
        ratio = float((np.abs(got["p"].astype(np.float64) - ref["p"]) / (R.EPS23 * np.abs(ref["p"]) + R.EPS21 * u)).max())
        print(f"clipped step numel={h['p'].shape[0]}: p error / bound {ratio:.3f}")
        assert ratio <= 1.0
    fr.check_sentinels()


# ----------------------------------------------------------------------------------------------------------------- 10. scheduler
def test_lr_scheduler_changes_the_next_step():
    cfg = dict(amsgrad=True)
    f = Flat([257, 4097], "own", 19, True)
    opt = make_opt(f.params, cfg)
    f.attach_state(opt)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    opt.step()
    sched.step()
    assert opt.param_groups[0]["lr"] == HYPER["lr"] * 0.5
    for i in range(2):
        got = f.read(i)
        f.host[i].update(p=got["p"].copy(), m=got["m"].copy(), v=got["v"].copy(), vmax=got["vmax"].copy())
    f.t0 = 1
    opt.step()
    f.check_against_ref(cfg, "after StepLR", lr=HYPER["lr"] * 0.5)
    with pytest.raises(AssertionError):                                   # and the old lr would not have passed
        f.check_against_ref(cfg, "after StepLR, old lr", lr=HYPER["lr"])


# ---------------------------------------------------------------------------------------------------------------- 11. non-finite
@pytest.mark.parametrize("amsgrad", [False, True], ids=["adam", "amsgrad"])
def test_non_finite_gradients_propagate_as_in_torch(amsgrad):
    cfg = dict(amsgrad=amsgrad)
    f = Flat([4097], "own", 23, amsgrad, t0=999)
    h = f.host[0]
    h["g"][10], h["g"][2000] = np.inf, np.nan
    f.views["g"][0].copy_(torch.from_numpy(h["g"]))
    opt = make_opt(f.params, cfg)
    f.attach_state(opt)
    opt.step()
    got = f.read(0)
    # torch's CPU Adam from the same state
    p = torch.nn.Parameter(torch.from_numpy(h["p"].copy()))
    p.grad = torch.from_numpy(h["g"].copy())
    ot = torch.optim.Adam([p], lr=HYPER["lr"], betas=(HYPER["b1"], HYPER["b2"]), eps=HYPER["eps"], amsgrad=amsgrad, foreach=False)
    ot.state[p] = {"step": torch.tensor(999.0), "exp_avg": torch.from_numpy(h["m"].copy()), "exp_avg_sq": torch.from_numpy(h["v"].copy())}
    if amsgrad:
        ot.state[p]["max_exp_avg_sq"] = torch.from_numpy(h["vmax"].copy())
    ot.step()
    theirs = {"p": p.detach().numpy(), "m": ot.state[p]["exp_avg"].numpy(), "v": ot.state[p]["exp_avg_sq"].numpy()}
    for k in ("p", "m", "v"):
        assert np.array_equal(np.isfinite(got[k]), np.isfinite(theirs[k])), k
        assert np.array_equal(np.isnan(got[k]), np.isnan(theirs[k])), k
        assert not np.isfinite(got[k][[10, 2000]]).any() and np.isfinite(np.delete(got[k], [10, 2000])).all(), k
    keep = np.ones(4097, bool)
    keep[[10, 2000]] = False
    ref = R.step(h["p"][keep], h["g"][keep], h["m"][keep], h["v"][keep], h["vmax"][keep] if amsgrad else None, 1000, **ref_kw(cfg))
    R.check_step({k: a[keep] for k, a in got.items()}, ref, h["p"][keep], h["m"][keep], amsgrad, where="finite elements")
