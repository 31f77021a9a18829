#!/usr/bin/env python3
"""The split EMA codebook update (csrc/vq_ema_merge.hip) at N = 262 144 rows (B = 4096, 8 x 8 maps), D = 64, K = 512, in both
layouts: functional.vq_ema_stats + functional.vq_ema_apply at R = 1 beside functional.vq_ema_update (the same result, bit for bit),
the apply alone at R = 8 and R = 64, and the training step of tools/train_bench.py with ema_decay against ema_decay plus
ema_accumulate=2.

    python tools/vq_ema_merge_bench.py [--repeats 7] [--steps 30] [--out profiles/vq_ema_merge.txt]
        one process; the forms of a group alternate --repeats times, a sample is the mean ms per call over --steps calls (host clock
        around work that ends in a device synchronise).  Reported: the median of the samples and their spread (min .. max) and the
        ratio split / one-shot; for the apply alone the bytes per second over the R K C 8 bytes of statistics it reads.  The
        training steps run as child processes, alternating, --train-repeats times each (tools/train_bench.py 4096 hip 20).  Last,
        the compiler's own report of the kernels' registers, LDS and scratch (no GPU needed)."""
import argparse
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
DECAY, EPS = 0.99, 1e-5
WARMUP = 3


def timed(fn, steps):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def alternate(forms, repeats, steps):
    """forms: {name: callable}; -> {name: [ms per call, one per repeat]} with the forms alternating inside every repeat"""
    for _ in range(WARMUP):
        for fn in forms.values():
            fn()
    ms = {k: [] for k in forms}
    for _ in range(repeats):
        for k, fn in forms.items():
            ms[k].append(timed(fn, steps))
    return ms


def groups(rowmajor):
    """-> [(title, {form: callable}, bytes the first form reads or None)] for one layout"""
    import torch
    from vqvae_amd import functional as F
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(20 + int(rowmajor))
    z = torch.randn((B, H, W, D) if rowmajor else (B, D, H, W), device=dev, generator=g)
    idx = torch.randint(0, K, (N,), device=dev, generator=g)
    cs, w, cb = torch.rand(K, device=dev, generator=g) * 500, torch.randn(K, D, device=dev, generator=g), torch.empty(K, D, device=dev)
    ws_u, ws_s = F.vq_ema_workspace(N, K, D, dev), F.vq_ema_stats_workspace(N, K, D, dev)
    st = torch.empty(1, K, D + 1, dtype=torch.float64, device=dev)
    ws_a = {R: F.vq_ema_apply_workspace(R, K, D, dev) for R in (1, 8, 64)}
    many = {R: torch.randn(R, K, D + 1, dtype=torch.float64, device=dev, generator=g).abs_() for R in (8, 64)}

    def one_shot():
        F.vq_ema_update(z, idx, cs, w, cb, DECAY, EPS, rowmajor=rowmajor, workspace=ws_u)

    def split():
        F.vq_ema_stats(z, idx, K, rowmajor=rowmajor, workspace=ws_s, out=st[0])
        F.vq_ema_apply(st, cs, w, cb, DECAY, EPS, workspace=ws_a[1])

    out = [("update at R = 1", {"stats + apply": split, "vq_ema_update": one_shot}, None)]
    if rowmajor:                                                     # the apply never sees z: timed once
        out.append(("apply alone", {f"R = {R}": (lambda R=R: F.vq_ema_apply(many[R], cs, w, cb, DECAY, EPS, workspace=ws_a[R]))
                                    for R in (8, 64)}, None))
    return out


def train_steps(say, repeats):
    """tools/train_bench.py 4096 hip 20 with ema_decay, and with ema_accumulate=2 on top: child processes, alternating"""
    ms = {"ema": [], "ema_accumulate": []}
    for _ in range(repeats):
        for word in ms:
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_bench.py"), "4096", "hip", "20", "-", word],
                               capture_output=True, text=True, timeout=600)
            m = re.search(r":\s+([0-9.]+) ms per forward\+backward", r.stdout)
            if r.returncode != 0 or not m:
                raise RuntimeError(f"train_bench.py {word} failed:\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
            ms[word].append(float(m.group(1)))
    med = {k: statistics.median(v) for k, v in ms.items()}
    say(f"training step, tools/train_bench.py 4096 hip 20 (ms per forward + backward, {repeats} processes each, alternating): "
        f"ema_decay=0.99 {med['ema']:.2f} ({min(ms['ema']):.2f} .. {max(ms['ema']):.2f})   + ema_accumulate=2 "
        f"{med['ema_accumulate']:.2f} ({min(ms['ema_accumulate']):.2f} .. {max(ms['ema_accumulate']):.2f})   "
        f"accumulate / plain {med['ema_accumulate'] / med['ema']:.3f}")


def resource_report(say):
    from vqvae_amd import build
    src = os.path.join(build.CSRC, "vq_ema_merge.hip")
    r = subprocess.run([build.hipcc(), *build.flags_for(src), "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull],
                       capture_output=True, text=True)
    say("compiler report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):")
    name, row = None, {}
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            t = re.search(r"(ema_\w+?_kernel)", m.group(2))
            name, row = (t.group(1) if t else m.group(2)), {}
        else:
            row[m.group(1)] = m.group(2)
            if m.group(1).startswith("LDS"):
                say(f"  {name}: VGPRs {row.get('VGPRs')}, AGPRs {row.get('AGPRs')}, scratch {row.get('ScratchSize [bytes/lane]')} B/lane, "
                    f"LDS {row.get('LDS Size [bytes/block]')} B, occupancy {row.get('Occupancy [waves/SIMD]')} waves/SIMD")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--train-repeats", type=int, default=3)
    ap.add_argument("--out", default="profiles/vq_ema_merge.txt")
    ap.add_argument("--no-gpu", action="store_true", help="the compiler report only")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/vq_ema_merge_bench.py: N = {N} rows (B = {B}, {H} x {W}), D = {D}, K = {K}; one process, the forms of a group alternate; "
        f"{a.repeats} samples of {a.steps} calls; ms per call, host clock around a device synchronise: median (min .. max)")
    say("# stats + apply = functional.vq_ema_stats then functional.vq_ema_apply on its one record (csrc/vq_ema_merge.hip); "
        "vq_ema_update = the one-shot update (csrc/train.hip), the same bits; apply alone = functional.vq_ema_apply on R records")
    if not a.no_gpu:
        for rowmajor in (True, False):
            layout = "rows" if rowmajor else "NCHW"
            for title, forms, _ in groups(rowmajor):
                ms = alternate(forms, a.repeats, a.steps)
                med = {k: statistics.median(v) for k, v in ms.items()}
                cells = "   ".join(f"{k} {med[k]:.4f} ({min(v):.4f} .. {max(v):.4f})" for k, v in ms.items())
                tail = ""
                if "vq_ema_update" in med:
                    tail = f"   split / one-shot {med['stats + apply'] / med['vq_ema_update']:.3f}"
                else:
                    tail = "   " + "   ".join(f"{k}: {int(k.split()[-1]) * K * (D + 1) * 8 / med[k] / 1e6:.1f} GB/s of "
                                               f"{int(k.split()[-1]) * K * (D + 1) * 8 / 1e6:.2f} MB read" for k in med)
                say(f"{layout if 'vq_ema_update' in med else 'any layout'}  {title}: {cells}{tail}")
        train_steps(say, a.train_repeats)
    else:
        say("(--no-gpu: nothing timed)")
    resource_report(say)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
