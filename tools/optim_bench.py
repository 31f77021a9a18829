#!/usr/bin/env python3
"""The optimizer step alone: torch.optim.Adam (default = foreach), torch.optim.Adam(fused=True) and vqvae_amd.optim.Adam
(csrc/optim.hip) on the parameter sets of the two models -- the VQ-VAE of main.py's defaults (23 tensors) and
GatedPixelCNN(512, 64, 15, 10) (140 tensors) -- with amsgrad on and off, on static random gradients.

    python tools/optim_bench.py [--steps 200] [--repeats 5] [--sets vqvae,prior] [--json OUT]
        one process = one round: the three implementations alternate --repeats times; ms per step (host + device, synchronised
        once after --steps steps) as the median over the repeats.  Run several processes for the spread between rounds.
    python tools/optim_bench.py --launch-counts [--sets prior] [--out DIR]
        kernel launches per step of each implementation, from a `rocprofv3 --kernel-trace --stats` run of its own per
        implementation (the program after `--`): the kernel sequence of the last steps is periodic; its period is the count.
    python tools/optim_bench.py --profile IMPL --set SET --amsgrad 0|1 --steps N          (what --launch-counts runs)
"""
import argparse
import glob
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

IMPLS = ["torch", "torch_fused", "hip"]
WARMUP = 5


def parameter_set(which, dev):
    import torch
    torch.manual_seed(0)
    if which == "vqvae":
        from vqvae_amd.modules import VQVAE
        m = VQVAE(128, 32, 2, 512, 64, 0.25)
    else:
        from vqvae_amd.pixelcnn import GatedPixelCNN
        m = GatedPixelCNN(512, 64, 15, 10)
    params = [p for p in m.to(dev).parameters() if p.requires_grad]
    g = torch.Generator(device=dev).manual_seed(1)
    for p in params:
        p.grad = torch.randn(p.shape, device=dev, generator=g) * 1e-2
    return m, params


def make(impl, params, amsgrad):
    import torch
    if impl == "hip":
        from vqvae_amd import optim
        return optim.Adam(params, lr=3e-4, amsgrad=amsgrad)
    return torch.optim.Adam(params, lr=3e-4, amsgrad=amsgrad, fused=True if impl == "torch_fused" else None)


def timed(opt, n):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        opt.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def bench(a):
    import torch
    dev = torch.device("cuda:0")
    out = []
    for which in a.sets.split(","):
        for amsgrad in (False, True):
            opts = {}
            for impl in IMPLS:
                model, params = parameter_set(which, dev)
                opts[impl] = (model, make(impl, params, amsgrad))
                for _ in range(WARMUP):
                    opts[impl][1].step()
            ms = {impl: [] for impl in IMPLS}
            for _ in range(a.repeats):
                for impl in IMPLS:
                    ms[impl].append(timed(opts[impl][1], a.steps))
            n_t, n_e = len(params), sum(p.numel() for p in params)
            r = {"set": which, "tensors": n_t, "elements": n_e, "amsgrad": amsgrad, "steps": a.steps,
                 **{f"{impl}_ms": statistics.median(v) for impl, v in ms.items()}, **{f"{impl}_ms_all": v for impl, v in ms.items()}}
            out.append(r)
            print(f"{which:6s} {n_t:4d} tensors {n_e:9d} elements amsgrad={int(amsgrad)}: " +
                  "   ".join(f"{impl} {r[impl + '_ms']:.4f} ms" for impl in IMPLS), flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(out, open(a.json, "w"), indent=1)


def profile(a):
    import torch
    _, params = parameter_set(a.set, torch.device("cuda:0"))
    opt = make(a.profile, params, bool(a.amsgrad))
    for _ in range(WARMUP + a.steps):
        opt.step()
    torch.cuda.synchronize()


def period_of(names, steps):
    """launches per step: the smallest k whose last k names, repeated, are the last k * steps names"""
    for k in range(1, len(names) // steps + 1):
        tail = names[-k:]
        if names[-k * steps:] == tail * steps:
            return k, tail
    return None, []


def launch_counts(a):
    import sqlite3
    steps = 12
    for which in a.sets.split(","):
        for amsgrad in (0, 1):
            for impl in IMPLS:
                d = os.path.join(a.out, f"{which}_{impl}_{amsgrad}")
                cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                       "--profile", impl, "--set", which, "--amsgrad", str(amsgrad), "--steps", str(steps)]
                subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=180)
                dbs = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)
                if not dbs:
                    raise SystemExit(f"no results database under {d}")
                db = sqlite3.connect(dbs[0])
                cols = [r[1] for r in db.execute("pragma table_info(kernels)")]
                order = "start" if "start" in cols else "rowid"
                names = [r[0] for r in db.execute(f"select name from kernels order by {order}")]
                k, tail = period_of(names, steps)
                kinds = {}
                for n in tail:
                    kinds[n.split("(")[0][:70]] = kinds.get(n.split("(")[0][:70], 0) + 1
                print(f"{which:6s} amsgrad={amsgrad} {impl:12s}: {k} launches per step   " +
                      "; ".join(f"{c} x {n}" for n, c in sorted(kinds.items(), key=lambda kv: -kv[1])), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sets", default="vqvae,prior")
    ap.add_argument("--json", default=None)
    ap.add_argument("--launch-counts", action="store_true")
    ap.add_argument("--out", default="build/optim_prof")
    ap.add_argument("--profile", choices=IMPLS, default=None)
    ap.add_argument("--set", default="prior")
    ap.add_argument("--amsgrad", type=int, default=0)
    a = ap.parse_args()
    if a.profile:
        profile(a)
    elif a.launch_counts:
        launch_counts(a)
    else:
        bench(a)


if __name__ == "__main__":
    main()
