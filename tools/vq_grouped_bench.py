#!/usr/bin/env python3
"""Grouped (product) quantization: the one entry (functional.vq_grouped_forward / training.vq_grouped_backward =
vqvae_vq_grouped_forward_f32 / _backward_f32) against the composition a user would write without it -- every group's slice made
contiguous, functional.vq_forward and training.vq_backward per group, torch.cat of the results -- at N = 262 144 rows (B = 4096,
8 x 8 maps), D = 64, K = 512, G = 2, 4, 8, in both layouts.

    python tools/vq_grouped_bench.py [--rounds 3] [--steps 400] [--repeats 3] [--out profiles/vq_grouped.txt] [--no-step] [--no-trace]
        every round is a FRESH process (--worker) in which, per (layout, G), five things alternate --repeats times: the new forward,
        the new forward + backward, the composition's forward, the composition's forward + backward, and torch's copy_ of z (the
        memory yardstick: N D 4 bytes read and written).  A sample is the mean ms per call over --steps calls (host clock around
        work that ends in a device synchronise); reported: the median over all samples of all rounds and the spread (min .. max) of
        the rounds' medians.  Then, in one more fresh process (--step-worker), the training step of tools/train_bench.py
        (B = 4096, HIP convs, forward + loss + backward) on the default model and on VQVAE(..., codebook_groups=4), alternated.
        Then one `rocprofv3 --kernel-trace --stats` run of its own (--trace-worker after `--`): time per launch of the split, finish
        and grad_z kernels per case and the bytes per second that is.  Last, the resources of the new kernels as the compiler reports them (hipcc -Rpass-analysis=kernel-resource-usage).
    python tools/vq_grouped_bench.py --worker --json OUT | --step-worker --json OUT | --trace-worker       (what the driver starts)
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, H, W, K, D = 4096, 8, 8, 512, 64
N = B * H * W
GS = (2, 4, 8)
BETA = 0.25
WARMUP = 3
IMPLS = ("new fwd", "new fwd+bwd", "composed fwd", "composed fwd+bwd", "copy_")


def inputs(rowmajor, G):
    import torch
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(G + 10 * int(rowmajor))
    z = torch.randn((B, H, W, D) if rowmajor else (B, D, H, W), device=dev, generator=g)
    books = [torch.randn((K, D // G), device=dev, generator=g) for _ in range(G)]
    gzq = torch.randn(z.shape, device=dev, generator=g)
    return z, books, gzq, torch.tensor(0.7, device=dev)


def _slice(t, g, d, rowmajor):
    return (t[..., g * d:(g + 1) * d] if rowmajor else t[:, g * d:(g + 1) * d]).contiguous()


def composed(F, T, z, books, gzq, gl, vws, rowmajor, backward):
    """what a user writes today: contiguous slices, the one-codebook calls per group, cat"""
    import torch
    G, d = len(books), books[0].shape[1]
    dim = 3 if rowmajor else 1
    zs = [_slice(z, g, d, rowmajor) for g in range(G)]
    outs = [F.vq_forward(zs[g], books[g], BETA, rowmajor=rowmajor, workspace=vws, prepared=False) for g in range(G)]
    z_q = torch.cat([o[1] for o in outs], dim=dim)
    loss = sum(o[0] for o in outs) / G
    idx = [o[3] for o in outs]
    if not backward:
        return loss, z_q, idx
    gq = gl / G
    gr = [T.vq_backward(zs[g], books[g], idx[g], _slice(gzq, g, d, rowmajor), gq, BETA, rowmajor=rowmajor) for g in range(G)]
    return loss, z_q, idx, torch.cat([r[0] for r in gr], dim=dim), [r[1] for r in gr]


def new(F, T, z, books, gzq, gl, ws, rowmajor, backward):
    out = F.vq_grouped_forward(z, books, BETA, rowmajor=rowmajor, workspace=ws, prepared=False)
    if not backward:
        return out
    return out + T.vq_grouped_backward(z, books, out[3], gzq, gl, BETA, rowmajor=rowmajor)


def timed(fn, steps):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def worker(a):
    import torch
    from vqvae_amd import functional as F, training as T
    out = []
    for rowmajor in (True, False):
        for G in GS:
            z, books, gzq, gl = inputs(rowmajor, G)
            ws = F.vq_grouped_workspace(N, K, D, G, z.device)
            vws = F.vq_workspace(K, D // G, z.device)
            dst = torch.empty_like(z)
            fns = {"new fwd": lambda: new(F, T, z, books, gzq, gl, ws, rowmajor, False),
                   "new fwd+bwd": lambda: new(F, T, z, books, gzq, gl, ws, rowmajor, True),
                   "composed fwd": lambda: composed(F, T, z, books, gzq, gl, vws, rowmajor, False),
                   "composed fwd+bwd": lambda: composed(F, T, z, books, gzq, gl, vws, rowmajor, True),
                   "copy_": lambda: dst.copy_(z)}
            a_, b_ = fns["new fwd+bwd"](), fns["composed fwd+bwd"]()
            torch.cuda.synchronize()
            # (the composition's loss and upstream gradient go through torch's own division: only what must agree bit for bit is compared)
            same = bool(torch.equal(a_[1], b_[1]) and all(torch.equal(a_[3][g], b_[2][g].view(-1)) for g in range(G)))
            close = bool(torch.allclose(a_[6], b_[3], rtol=1e-5, atol=1e-9) and
                         all(torch.allclose(x, y, rtol=1e-5, atol=1e-9) for x, y in zip(a_[7], b_[4])))
            for _ in range(WARMUP):
                for f in fns.values():
                    f()
            ms = {k: [] for k in fns}
            for _ in range(a.repeats):
                for k, f in fns.items():
                    ms[k].append(timed(f, a.steps))
            out.append({"rowmajor": rowmajor, "G": G, "same_bits": same, "grads_close": close, **ms})
            print(f"{'rows' if rowmajor else 'NCHW'} G={G}: " + ", ".join(f"{k} {statistics.median(v):.4f}" for k, v in ms.items()) +
                  f" ms; same z_q and indices: {same}, gradients agree: {close}", flush=True)
    json.dump(out, open(a.json, "w"))


def step_worker(a):
    """tools/train_bench.py's step (forward + loss + backward, HIP convs, no optimizer) on the default model and on
    codebook_groups=4, alternated in one process"""
    import torch
    from vqvae_amd import conv, training as T
    from vqvae_amd.modules import VQVAE
    dev = torch.device("cuda:0")
    conv.set_conv_backend("hip")
    torch.manual_seed(0)
    models = {"default": VQVAE(128, 32, 2, 512, 64, 0.25).to(dev).train(),
              "codebook_groups=4": VQVAE(128, 32, 2, 512, 64, 0.25, codebook_groups=4).to(dev).train()}
    x = torch.randn(B, 3, 32, 32, device=dev)

    def step(m):
        m.zero_grad(set_to_none=True)
        el, xh, pp = m(x)
        T.step_losses(el, xh, pp, x, 0.06)[1].backward()
    for m in models.values():
        for _ in range(WARMUP):
            step(m)
    ms = {k: [] for k in models}
    for _ in range(a.repeats):
        for k, m in models.items():
            ms[k].append(timed(lambda: step(m), 100))
    json.dump(ms, open(a.json, "w"))


TRACE_CALLS = 13                      # per (layout, G) in the trace worker; the first WARMUP of them are left out of the means


def trace_worker(a):
    """what the kernel trace watches: per (layout, G) TRACE_CALLS forwards, then, after all of them, TRACE_CALLS backwards each"""
    import torch
    from vqvae_amd import functional as F, training as T
    cases = []
    for rowmajor in (True, False):
        for G in GS:
            z, books, gzq, gl = inputs(rowmajor, G)
            ws = F.vq_grouped_workspace(N, K, D, G, z.device)
            for _ in range(TRACE_CALLS):
                out = F.vq_grouped_forward(z, books, BETA, rowmajor=rowmajor, workspace=ws, prepared=False)
            cases.append((z, books, gzq, gl, out[3], rowmajor))
    torch.cuda.synchronize()
    for z, books, gzq, gl, idx, rowmajor in cases:
        for _ in range(TRACE_CALLS):
            T.vq_grouped_backward(z, books, idx, gzq, gl, BETA, rowmajor=rowmajor)
    torch.cuda.synchronize()


def trace_report(d, say):
    """mean time per launch of the new stream kernels per (layout, G), and the bytes per second that is (the bytes the kernel has to
    move, from the shapes); the quantizer's kernels beside them"""
    import glob
    import sqlite3
    dbs = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)
    if not dbs:
        say(f"(no results database under {d}: the kernel trace was not taken; kernel times are NOT MEASURED)")
        return
    db = sqlite3.connect(dbs[0])
    tables = [r[0] for r in db.execute("select name from sqlite_master where type in ('table', 'view')")]
    table = "kernels" if "kernels" in tables else next((t for t in tables if t.startswith("kernels")), None)
    if table is None:
        say("(the results database has no kernels table: kernel times are NOT MEASURED)")
        return
    cols = [r[1] for r in db.execute(f"pragma table_info({table})")]
    order = "start" if "start" in cols else "rowid"
    launches = [(n, dur) for n, dur in db.execute(f"select name, duration from {table} order by {order}")]
    per = {}
    for n, dur in launches:
        per.setdefault(n, []).append(dur)
    say("kernel trace (rocprofv3 --kernel-trace --stats, a run of its own; us per launch: mean, min .. max; launches):")
    for n, v in sorted(per.items(), key=lambda kv: -sum(kv[1]))[:12]:
        say(f"  {statistics.mean(v) / 1e3:9.2f}  {min(v) / 1e3:8.2f} .. {max(v) / 1e3:8.2f}  {len(v):6d}  {n[:110]}")
    map_bytes = N * D * 4
    ncases = 2 * len(GS)
    say("the new stream kernels per case (us per launch after warm-up; TB/s over the bytes the kernel must move):")
    for key, what, moved in (("grp_split_kernel<4,", "split: z read, slabs written", lambda G: 2 * map_bytes),
                             ("grp_finish_kernel<4,", "finish: z read, z_q written, G N indices", lambda G: 2 * map_bytes + G * N * 8),
                             ("grp_gradz_kernel<4,", "grad_z: z and grad_zq read, grad_z written, G N indices", lambda G: 3 * map_bytes + G * N * 8)):
        v = [dur for n, dur in launches if key in n][:ncases * TRACE_CALLS]       # (the split's later launches are the backward's, one group each)
        if len(v) < ncases * TRACE_CALLS:
            say(f"  (too few launches of {key} in the trace: NOT MEASURED)")
            continue
        cells = []
        for i, (layout, G) in enumerate((l, G) for l in ("rows", "NCHW") for G in GS):
            us = statistics.mean(v[i * TRACE_CALLS + WARMUP:(i + 1) * TRACE_CALLS]) / 1e3
            cells.append(f"{layout} G={G}: {us:.2f} us, {moved(G) / us / 1e6:.2f} TB/s")
        say(f"  {key} ({what}): " + "; ".join(cells))


def kernel_resources(say, tmp):
    from vqvae_amd import build
    src = os.path.join(build.CSRC, "vq_grouped.hip")
    try:
        r = subprocess.run([build.hipcc(), *build.flags_for(src), "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(tmp, "vq_grouped_resources.o")],
                           capture_output=True, text=True, timeout=600)
    except (RuntimeError, OSError, subprocess.TimeoutExpired) as e:
        say(f"(kernel resources not recorded: {e})")
        return
    say("kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): VGPRs, SGPRs, scratch bytes / lane, LDS bytes / block, waves / SIMD")
    cur = {}
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|LDS Size \[bytes/block\]|Occupancy \[waves/SIMD\]): (\S+)", line)
        if not m:
            continue
        cur[m.group(1)] = m.group(2)
        if m.group(1).startswith("LDS"):
            name = subprocess.run(["c++filt", cur["Function Name"]], capture_output=True, text=True).stdout.strip() or cur["Function Name"]
            say(f"  {name.split('(')[0][:60]:60s} {cur.get('VGPRs'):>4s} {cur.get('TotalSGPRs'):>4s} {cur.get('ScratchSize [bytes/lane]'):>4s} "
                f"{cur.get('LDS Size [bytes/block]'):>4s} {cur.get('Occupancy [waves/SIMD]'):>3s}")
            cur = {}


def driver(a):
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    os.makedirs(a.tmp, exist_ok=True)
    rounds = []
    for i in range(a.rounds):
        path = os.path.join(a.tmp, f"round{i}.json")
        subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--json", path, "--steps", str(a.steps),
                        "--repeats", str(a.repeats)], check=True, timeout=600, stdout=subprocess.DEVNULL)
        rounds.append(json.load(open(path)))
    say(f"# tools/vq_grouped_bench.py: N = {N} rows (B = {B}, {H} x {W}), K = {K}, D = {D}, beta = {BETA}; {a.rounds} fresh processes x "
        f"{a.repeats} alternating samples of {a.steps} calls; ms per call, host clock around a device synchronise")
    say("# new = vqvae_vq_grouped_forward_f32 (+ _backward_f32: grad_z and G codebook gradients); composed = per group slice.contiguous(), "
        "vq_forward (+ vq_backward), then torch.cat; copy_ = torch's copy of z (N D 4 bytes read + written)")
    say("# median over all samples (the rounds' medians min .. max)")
    say("layout  G   " + "".join(f"{k:>30s}" for k in IMPLS) + "   composed/new fwd  fwd+bwd  same bits  grads agree")
    for j, first in enumerate(rounds[0]):
        cell = {}
        for impl in IMPLS:
            per_round = [statistics.median(r[j][impl]) for r in rounds]
            every = [v for r in rounds for v in r[j][impl]]
            cell[impl] = (statistics.median(every), min(per_round), max(per_round))
        say(f"{'rows' if first['rowmajor'] else 'NCHW'}   {first['G']:2d}   " +
            "".join(f"{cell[k][0]:10.4f} ({cell[k][1]:.4f} .. {cell[k][2]:.4f})" for k in IMPLS) +
            f"   {cell['composed fwd'][0] / cell['new fwd'][0]:16.2f} {cell['composed fwd+bwd'][0] / cell['new fwd+bwd'][0]:8.2f}"
            f"  {all(r[j]['same_bits'] for r in rounds)!s:>9s}  {all(r[j]['grads_close'] for r in rounds)!s:>11s}")
    if not a.no_step:
        path = os.path.join(a.tmp, "step.json")
        subprocess.run([sys.executable, os.path.abspath(__file__), "--step-worker", "--json", path, "--repeats", str(a.repeats)],
                       check=True, timeout=900, stdout=subprocess.DEVNULL)
        ms = json.load(open(path))
        say(f"training step (tools/train_bench.py's: B = {B}, HIP convs, forward + loss + backward, 100 steps a sample, alternated in one process):")
        for k, v in ms.items():
            say(f"  {k:20s} {statistics.median(v):8.2f} ms (min {min(v):.2f} .. max {max(v):.2f})")
    if not a.no_trace:
        d = os.path.join(a.tmp, "trace")
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                            "--trace-worker"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        if r.returncode != 0:
            say(f"(the kernel-trace run ended with status {r.returncode})")
        trace_report(d, say)
    kernel_resources(say, a.tmp)
    say("not measured: what the option does to the perplexity or the dead codes of a trained checkpoint")
    open(a.out, "w").write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=400)       # (0.3 to 2 ms a call: a sample is a tenth of a second at the least)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default="profiles/vq_grouped.txt")
    ap.add_argument("--tmp", default="build/vq_grouped_bench")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-worker", action="store_true")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--step-worker", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.worker:
        worker(a)
    elif a.step_worker:
        step_worker(a)
    elif a.trace_worker:
        trace_worker(a)
    else:
        driver(a)


if __name__ == "__main__":
    main()
