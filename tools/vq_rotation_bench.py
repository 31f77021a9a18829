#!/usr/bin/env python3
"""The rotation-trick z gradient (training.vq_backward(rotation=True) = vqvae_vq_backward_f32 | VQVAE_VQ_BWD_ROTATION) against the
straight-through gradient of the same entry in the same process, at N = 262 144 rows (B = 4096, 8 x 8 maps), K = 512, D = 64, in
both layouts, need_codebook=False.  Both kernels move the same bytes (z, grad_zq and the indices in, grad_z out, code rows through
L2), so the ratio is what the second pass over the row and the fp64 arithmetic cost.

    python tools/vq_rotation_bench.py [--rounds 5] [--steps 50] [--repeats 5] [--out profiles/vq_rotation.txt]
        every round is a FRESH process (--worker) in which the two forms alternate --repeats times per layout; a sample is the mean
        ms per call over --steps calls (host clock around work that ends in a device synchronise).  Reported: the median over all
        samples of all rounds, the spread (min .. max) of the rounds' medians, the ratio, and bytes per second over the call time.
        Then one `rocprofv3 --kernel-trace --stats` run of its own (--trace-worker after `--`): time per kernel and the bytes per
        second over the kernel time.  Last, the compiler's own report of the kernels' registers, LDS and scratch (no GPU needed).
    python tools/vq_rotation_bench.py --worker --json OUT | --trace-worker           (what the driver starts)
"""
import argparse
import glob
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
BETA = 0.25
WARMUP = 3
MOVED = 3 * N * D * 4 + N * 8          # z and grad_zq read, grad_z written, the indices; code rows (K D 4 bytes) come through L2


def inputs(rowmajor):
    import torch
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(10 + int(rowmajor))
    shape = (B, H, W, D) if rowmajor else (B, D, H, W)
    z = torch.randn(shape, device=dev, generator=g)
    gz = torch.randn(shape, device=dev, generator=g)
    cb = torch.randn((K, D), device=dev, generator=g)
    idx = torch.randint(0, K, (N,), device=dev, generator=g)
    gl = torch.tensor(1.0, device=dev)
    return z, cb, idx, gz, gl


def timed(fn, steps):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def forms(rowmajor):
    from vqvae_amd import training as T
    z, cb, idx, gz, gl = inputs(rowmajor)
    rot = lambda: T.vq_backward(z, cb, idx, gz, gl, BETA, rowmajor=rowmajor, need_codebook=False, rotation=True)     # noqa: E731
    st = lambda: T.vq_backward(z, cb, idx, gz, gl, BETA, rowmajor=rowmajor, need_codebook=False)                      # noqa: E731
    return rot, st


def worker(a):
    import torch
    out = []
    for rowmajor in (True, False):
        rot, st = forms(rowmajor)
        r = rot()[0]
        torch.cuda.synchronize()
        finite = bool(torch.isfinite(r).all())
        for _ in range(WARMUP):
            rot(), st()
        ms = {"rotation": [], "straight": []}
        for _ in range(a.repeats):
            ms["rotation"].append(timed(rot, a.steps))
            ms["straight"].append(timed(st, a.steps))
        out.append({"rowmajor": rowmajor, "finite": finite, **ms})
        print(f"{'rows' if rowmajor else 'NCHW'}: rotation {statistics.median(ms['rotation']):.4f} ms, straight-through "
              f"{statistics.median(ms['straight']):.4f} ms", flush=True)
    if a.json:
        json.dump(out, open(a.json, "w"))


def trace_worker(a):
    import torch
    for rowmajor in (True, False):
        rot, st = forms(rowmajor)
        for _ in range(WARMUP + 10):
            rot(), st()
    torch.cuda.synchronize()


def trace_report(d, say):
    import sqlite3
    dbs = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)
    if not dbs:
        say(f"(no results database under {d}: the kernel trace was not taken)")
        return
    db = sqlite3.connect(dbs[0])
    cols = [r[1] for r in db.execute("pragma table_info(kernels)")]
    order = "start" if "start" in cols else "rowid"
    launches = [(n, dur) for n, dur in db.execute(f"select name, duration from kernels order by {order}")]
    say("kernel trace (a run of its own; the trace worker runs row-major first, then NCHW: a kernel's first half of launches is "
        "row-major; us per launch: mean, min .. max):")
    for key, layouts in (("vq_rotation_gradz_kernel", ("rows", "NCHW")), ("vqb_gradz_kernel", ("rows", "NCHW"))):
        v = [dur for n, dur in launches if key in n]
        if not v:
            say(f"  (no launch of {key} in the trace)")
            continue
        n_l = len(layouts)
        for i, layout in enumerate(layouts):
            part = v[i * len(v) // n_l:(i + 1) * len(v) // n_l][WARMUP:]
            m = statistics.mean(part) / 1e3
            say(f"  {key:26s} {layout}: {m:8.2f}  {min(part) / 1e3:8.2f} .. {max(part) / 1e3:8.2f}  ({len(part)} launches)  "
                f"{MOVED / m / 1e6:.2f} TB/s of the {MOVED / 1e6:.0f} MB the algorithm moves")


def resource_report(say):
    from vqvae_amd import build
    src = os.path.join(build.CSRC, "vq_rotation.hip")
    r = subprocess.run([build.hipcc(), *build.flags_for(src), "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull],
                       capture_output=True, text=True)
    say("compiler report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): kernel<D up to which a row stays in registers (0: "
        "re-read), floats per access>")
    name, row = None, {}
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            t = re.search(r"(vq_rotation_\w+?_kernel)ILi(\d+)E(?:Li(\d+)E)?", m.group(2))
            name = f"{t.group(1)}<{t.group(2)}{', ' + t.group(3) if t.group(3) else ''}>" if t else m.group(2)
            row = {}
        else:
            row[m.group(1)] = m.group(2)
            if m.group(1).startswith("LDS"):
                say(f"  {name}: VGPRs {row.get('VGPRs')}, AGPRs {row.get('AGPRs')}, scratch {row.get('ScratchSize [bytes/lane]')} B/lane, "
                    f"LDS {row.get('LDS Size [bytes/block]')} B, occupancy {row.get('Occupancy [waves/SIMD]')} waves/SIMD")


def driver(a):
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    tmp = a.tmp
    os.makedirs(tmp, exist_ok=True)
    rounds = []
    for i in range(a.rounds):
        path = os.path.join(tmp, f"round{i}.json")
        subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--json", path, "--steps", str(a.steps),
                        "--repeats", str(a.repeats)], check=True, timeout=300, stdout=subprocess.DEVNULL)
        rounds.append(json.load(open(path)))
    say(f"# tools/vq_rotation_bench.py: N = {N} rows (B = {B}, {H} x {W}), K = {K}, D = {D}; vq_backward(need_codebook=False); {a.rounds} "
        f"fresh processes x {a.repeats} alternating samples of {a.steps} calls; ms per call, host clock around a device synchronise")
    say(f"# rotation = VQVAE_VQ_BWD_ROTATION (vq_rotation_gradz_kernel); straight = the same entry without the flag (vqb_gradz_kernel); "
        f"both move {MOVED / 1e6:.0f} MB")
    say("layout  rotation ms (rounds' medians min .. max)   straight ms (min .. max)     rotation / straight   rotation TB/s   straight TB/s")
    for j, first in enumerate(rounds[0]):
        cell = {}
        for impl in ("rotation", "straight"):
            per_round = [statistics.median(r[j][impl]) for r in rounds]
            every = [v for r in rounds for v in r[j][impl]]
            cell[impl] = (statistics.median(every), min(per_round), max(per_round))
        ro, st = cell["rotation"], cell["straight"]
        say(f"{'rows' if first['rowmajor'] else 'NCHW'}    {ro[0]:8.4f} ({ro[1]:.4f} .. {ro[2]:.4f})              {st[0]:8.4f} ({st[1]:.4f} .. {st[2]:.4f})"
            f"          {ro[0] / st[0]:6.2f}              {MOVED / ro[0] / 1e9:6.2f}          {MOVED / st[0] / 1e9:6.2f}")
    if not a.no_trace:
        d = os.path.join(tmp, "trace")
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                            "--trace-worker"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300)
        if r.returncode != 0:
            say(f"(the kernel-trace run ended with status {r.returncode})")
        else:
            trace_report(d, say)
    resource_report(say)
    open(a.out, "w").write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="profiles/vq_rotation.txt")
    ap.add_argument("--tmp", default="build/vq_rotation_bench")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--trace-worker", action="store_true")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.worker:
        worker(a)
    elif a.trace_worker:
        trace_worker(a)
    else:
        driver(a)


if __name__ == "__main__":
    main()
