#!/usr/bin/env python3
"""Time of the k-means initialisation of the codebook (csrc/vq_kmeans.hip): k-means++ seeding and one Lloyd round (assignment by
the quantizer + mean update) on N rows, K = 512, D = 64 -- against the same algorithm written with torch ops on the same GPU
(fp64 squared distances, cumsum + searchsorted for the D^2 sampling; fp32 distance matrix + argmin and an fp64 index_add for the
Lloyd round).  Row-major rows, as the model hands them over.

    python tools/kmeans_init_bench.py [--rows 262144 32768] [--K 512] [--D 64] [--procs 3] [--limit 240]

Every measurement runs in a fresh child process under its own time limit (--limit seconds); the parent prints each child's JSON
line and, per row count, the median over the processes.  Times are device events around work that ends in a synchronise, after one
untimed pass of everything.  bytes_per_round is what one seeding round must move (the rows once, fp32, and the fp64 weights read
and written); GB/s follows from the measured per-round time."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_seed(z, K, u):
    """k-means++ with torch ops, no host sync: fp64 distances, inclusive cumsum, first row whose prefix exceeds u_k T"""
    import torch
    N = z.shape[0]
    z64 = z.double()
    rows = torch.empty(K, dtype=torch.int64, device=z.device)
    rows[0:1] = torch.floor(u[0:1].double() * N).long().clamp_(0, N - 1)
    w = None
    for k in range(1, K):
        d = ((z64 - z64.index_select(0, rows[k - 1:k])) ** 2).sum(1)
        w = d if w is None else torch.minimum(w, d)
        c = torch.cumsum(w, 0)
        rows[k:k + 1] = torch.searchsorted(c, u[k:k + 1].double() * c[-1:], right=True).clamp_(max=N - 1)
    return z.index_select(0, rows), rows


def torch_lloyd(z, cb):
    """one Lloyd round with torch ops: the reference's distance matrix and argmin, fp64 sums per code, empty codes keep their bits"""
    import torch
    K = cb.shape[0]
    d = (z ** 2).sum(1, keepdim=True) + (cb ** 2).sum(1) - 2 * z @ cb.t()
    idx = d.argmin(1)
    counts = torch.bincount(idx, minlength=K)
    s = torch.zeros(K, z.shape[1], dtype=torch.float64, device=z.device).index_add_(0, idx, z.double())
    new = torch.where((counts > 0)[:, None], (s / counts.clamp(min=1)[:, None].double()).float(), cb)
    return new, counts


def child(N, K, D):
    import torch
    from vqvae_amd import functional as F
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(N)
    z = torch.randn(N // 64, 8, 8, D, device=dev, generator=g) * 0.5
    rows2d = z.view(N, D)
    u = torch.rand(K, device=dev, generator=g)
    ws, vws = F.vq_kmeans_workspace(N, K, D, dev), F.vq_workspace(K, D, dev)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b), out

    def hip_lloyd(cb):
        idx = F.vq_forward(z, cb, 0.0, rowmajor=True, workspace=vws, want_zq=False)[3]
        return F.vq_kmeans_update(z, idx, cb, rowmajor=True, workspace=ws)

    res = {"rows": N, "K": K, "D": D, "device": torch.cuda.get_device_name(dev)}
    for timed_pass in (False, True):                               # one untimed pass of everything, then the timed one
        t_seed, (cb, rows) = timed(lambda: F.vq_kmeans_seed(z, K, u, rowmajor=True, workspace=ws))
        t_lloyd, _ = timed(lambda: hip_lloyd(cb.clone()))
        t_tseed, (tcb, trows) = timed(lambda: torch_seed(rows2d, K, u))
        t_tlloyd, _ = timed(lambda: torch_lloyd(rows2d, tcb))
        if timed_pass:
            bytes_round = N * D * 4 + 2 * N * 8
            per_round = t_seed / (K - 1)
            res.update(hip_seed_ms=t_seed, hip_seed_round_us=per_round * 1e3, hip_lloyd_ms=t_lloyd, torch_seed_ms=t_tseed,
                       torch_seed_round_us=t_tseed / (K - 1) * 1e3, torch_lloyd_ms=t_tlloyd, bytes_per_round=bytes_round,
                       hip_seed_gbps=bytes_round / (per_round * 1e-3) / 1e9, launches_per_round=2,
                       rows_agreeing_with_torch=int((rows == trows).sum()))
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}), flush=True)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--rows", type=int, nargs="+", default=[262144, 32768])
    p.add_argument("--K", type=int, default=512)
    p.add_argument("--D", type=int, default=64)
    p.add_argument("--procs", type=int, default=3)
    p.add_argument("--limit", type=float, default=240.0)
    p.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    args = p.parse_args()
    if args.child:
        child(args.child, args.K, args.D)
        return
    for N in args.rows:
        if N % 64:
            raise SystemExit("--rows must be multiples of 64 (8x8 maps)")
        runs = []
        for _ in range(args.procs):
            # a fresh process per measurement, ended at its own time limit; a failure ends the benchmark (nothing more is started)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(N), "--K", str(args.K), "--D", str(args.D)],
                                 capture_output=True, text=True, timeout=args.limit, cwd=ROOT)
            if out.returncode != 0:
                sys.stderr.write(out.stdout + out.stderr)
                raise SystemExit(f"child for {N} rows ended with status {out.returncode}")
            line = out.stdout.strip().splitlines()[-1]
            print(line, flush=True)
            runs.append(json.loads(line))
        keys = [k for k, v in runs[0].items() if isinstance(v, float)]
        print(json.dumps({"rows": N, "K": args.K, "D": args.D, "median_of": len(runs),
                          **{k: round(statistics.median(r[k] for r in runs), 4) for k in keys}}), flush=True)


if __name__ == "__main__":
    main()
