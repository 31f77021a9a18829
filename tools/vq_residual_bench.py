#!/usr/bin/env python3
"""Residual quantization: the one entry (functional.vq_residual_forward = vqvae_vq_residual_forward_f32) against the same result
composed from the public calls that existed before it -- per stage functional.vq_forward(want_zq=False), then torch ops for the
gather E_q[idx_q], the residual r - e, the running sum and z + (S - z) -- at N = 262 144 rows (B = 4096, 8 x 8 maps), K = 512,
D = 64, Q = 1, 2, 4, 8, in both layouts.

    python tools/vq_residual_bench.py [--rounds 5] [--steps 50] [--repeats 5] [--out profiles/vq_residual.txt]
        every round is a FRESH process (--worker) in which the two implementations alternate --repeats times per (layout, Q); a
        sample is the mean ms per call over --steps calls (host clock around work that ends in a device synchronise).  Reported:
        the median over all samples of all rounds and the spread (min .. max) of the rounds' medians.  Then one
        `rocprofv3 --kernel-trace --stats` run of its own (--trace-worker after `--`): mean time per kernel, the advance
        kernel's bytes per second (N D 4 read + N D 4 written + N 8 of indices) per layout, and the per-stage overhead.  Beside it
        a plain device copy of the same N D 4 bytes: a torch clone, which is how tools/copy_calib.py copies, but timed here by the
        workers' host clock at this size -- not that tool's own 1 GiB figure.
    python tools/vq_residual_bench.py --worker --json OUT | --trace-worker           (what the driver starts)
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

B, H, W, K, D = 4096, 8, 8, 512, 64
N = B * H * W
QS = (1, 2, 4, 8)
BETA = 0.25
WARMUP = 3


def inputs(rowmajor, Q):
    import torch
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(Q + 10 * int(rowmajor))
    z = torch.randn((B, H, W, D) if rowmajor else (B, D, H, W), device=dev, generator=g)
    # stage q's codes on the scale of what stage q sees
    books = [torch.randn((K, D), device=dev, generator=g) * 0.7 ** q for q in range(Q)]
    return z, books


def composed(F, z, books, vws, rowmajor):
    """the result from the parent's public calls: index-only quantizer per stage + torch for everything else"""
    r, S, loss, idx_all = z, None, None, []
    for E in books:
        l, _, _, idx, _ = F.vq_forward(r, E, BETA, rowmajor=rowmajor, workspace=vws, prepared=False, want_zq=False)
        e = E[idx.view(-1)].view(B, H, W, D)
        e = e if rowmajor else e.permute(0, 3, 1, 2)
        r = r - e
        S = e if S is None else S + e
        loss = l if loss is None else loss + l
        idx_all.append(idx)
    return loss, z + (S - z), idx_all


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
    from vqvae_amd import functional as F
    out = []
    for rowmajor in (True, False):
        for Q in QS:
            z, books = inputs(rowmajor, Q)
            ws = F.vq_residual_workspace(N, K, D, Q, z.device)
            vws = F.vq_workspace(K, D, z.device)
            new = lambda: F.vq_residual_forward(z, books, BETA, rowmajor=rowmajor, workspace=ws, prepared=False)     # noqa: E731
            old = lambda: composed(F, z, books, vws, rowmajor)                                                       # noqa: E731
            a_, b_ = new(), old()
            torch.cuda.synchronize()
            same = bool(torch.equal(a_[1], b_[1]) and all(torch.equal(a_[3][q], b_[2][q].view(-1)) for q in range(Q)))
            for _ in range(WARMUP):
                new(), old()
            ms = {"new": [], "composed": []}
            for _ in range(a.repeats):
                ms["new"].append(timed(new, a.steps))
                ms["composed"].append(timed(old, a.steps))
            out.append({"rowmajor": rowmajor, "Q": Q, "same_bits": same, **ms})
            print(f"{'rows' if rowmajor else 'NCHW'} Q={Q}: new {statistics.median(ms['new']):.4f} ms, composed "
                  f"{statistics.median(ms['composed']):.4f} ms, same z_q and indices: {same}", flush=True)
    # a plain device copy of the same N D 4 bytes (a torch clone, as tools/copy_calib.py copies), on the same clock
    z, _ = inputs(True, 1)
    for _ in range(WARMUP):
        z.clone()
    copy = [timed(z.clone, 4 * a.steps) for _ in range(a.repeats)]
    out.append({"copy_ms": copy})
    print(f"device copy of {N * D * 4 / 2 ** 20:.0f} MiB: {statistics.median(copy) * 1e3:.2f} us", flush=True)
    if a.json:
        json.dump(out, open(a.json, "w"))


def trace_worker(a):
    import torch
    from vqvae_amd import functional as F
    for rowmajor in (True, False):
        for Q in QS:
            z, books = inputs(rowmajor, Q)
            ws = F.vq_residual_workspace(N, K, D, Q, z.device)
            for _ in range(WARMUP + 10):
                F.vq_residual_forward(z, books, BETA, rowmajor=rowmajor, workspace=ws, prepared=False)
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
    per = {}
    for n, dur in launches:
        per.setdefault(n, []).append(dur)
    say("kernel trace (a run of its own; us per launch: mean, min .. max; launches):")
    for n, v in sorted(per.items(), key=lambda kv: -sum(kv[1]))[:14]:
        say(f"  {statistics.mean(v) / 1e3:9.2f}  {min(v) / 1e3:8.2f} .. {max(v) / 1e3:8.2f}  {len(v):6d}  {n[:110]}")

    def by_layout(key):
        """the launches of the kernel whose (demangled) name holds `key`, in time order: the trace worker runs every row-major
        case first, then the same cases on NCHW maps, so the first half is row-major"""
        v = [dur for n, dur in launches if key in n]
        if not v:
            say(f"(no launch of {key} in the trace: its figures are missing below)")
            return None, None
        return statistics.mean(v[:len(v) // 2]) / 1e3, statistics.mean(v[len(v) // 2:]) / 1e3

    moved = 2 * N * D * 4 + N * 8
    adv = by_layout("rvq_advance_kernel<4>")
    fin = by_layout("rvq_finish_kernel<4>")
    trk = by_layout("vq_track_kernel_d64")
    for i, layout in enumerate(("rows", "NCHW")):
        if adv[i]:
            say(f"{layout}: advance kernel {adv[i]:.2f} us for {moved / 2 ** 20:.1f} MiB (r_q read, r_q+1 written, indices) = "
                f"{moved / adv[i] / 1e6:.2f} TB/s")
        if adv[i] and fin[i] and trk[i]:
            say(f"{layout}: per stage beyond the quantizer's own launches ({trk[i]:.2f} us tracker kernel): one advance kernel, "
                f"{adv[i]:.2f} us; per call one finish kernel, {fin[i]:.2f} us on average over Q = 1 .. 8")


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
                        "--repeats", str(a.repeats)], check=True, timeout=600, stdout=subprocess.DEVNULL)
        rounds.append(json.load(open(path)))
    say(f"# tools/vq_residual_bench.py: N = {N} rows (B = {B}, {H} x {W}), K = {K}, D = {D}, beta = {BETA}; {a.rounds} fresh processes x "
        f"{a.repeats} alternating samples of {a.steps} calls; ms per call, host clock around a device synchronise")
    say("# new = vqvae_vq_residual_forward_f32 (z_q, indices, histograms, losses); composed = vq_forward(want_zq=False) per stage + "
        "torch gather / subtract / add")
    say("layout  Q   new ms (rounds' medians min .. max)   composed ms (min .. max)     composed / new   same bits")
    copy_us = statistics.median(v for r in rounds for v in r[-1]["copy_ms"]) * 1e3
    for j, first in enumerate(rounds[0][:-1]):
        cell = {}
        for impl in ("new", "composed"):
            per_round = [statistics.median(r[j][impl]) for r in rounds]
            every = [v for r in rounds for v in r[j][impl]]
            cell[impl] = (statistics.median(every), min(per_round), max(per_round))
        same = all(r[j]["same_bits"] for r in rounds)
        say(f"{'rows' if first['rowmajor'] else 'NCHW'}   {first['Q']:2d}   {cell['new'][0]:8.4f} ({cell['new'][1]:.4f} .. {cell['new'][2]:.4f})"
            f"        {cell['composed'][0]:8.4f} ({cell['composed'][1]:.4f} .. {cell['composed'][2]:.4f})"
            f"       {cell['composed'][0] / cell['new'][0]:6.2f}        {same}")
    say(f"device copy of N D 4 = {N * D * 4 / 2 ** 20:.0f} MiB (torch clone, per call in a stream of calls): {copy_us:.2f} us = "
        f"{2 * N * D * 4 / copy_us / 1e6:.2f} TB/s read + write")
    if not a.no_trace:
        d = os.path.join(tmp, "trace")
        r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                            "--trace-worker"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        if r.returncode != 0:
            say(f"(the kernel-trace run ended with status {r.returncode})")
        trace_report(d, say)
    open(a.out, "w").write("\n".join(lines) + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="profiles/vq_residual.txt")
    ap.add_argument("--tmp", default="build/vq_residual_bench")
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
