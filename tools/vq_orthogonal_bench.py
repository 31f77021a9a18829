#!/usr/bin/env python3
"""The orthogonal regularization loss of a codebook (csrc/vq_orthogonal.hip) at (K, D) = (512, 64), (8192, 128) and (16384, 256), beside
the composition a user would write from torch ops on the same GPU.

    python tools/vq_orthogonal_bench.py [--repeats 5] [--out profiles/vq_orthogonal.txt] [--train]
        one process; per shape the forms of a group alternate --repeats times, a sample is the mean ms per call over a number of calls
        that fits the shape (host clock around work that ends in a device synchronise).  Reported: the median of the samples and
        their spread (min .. max), the ratio to the torch composition, and the peak of torch's allocator above what was allocated
        before the call.
          forward              functional.l2norm_rows + vq_orthogonal_forward with `saved`    torch: F.normalize, mm, pow(2).sum() in
                                                                                              fp32 under no_grad
          forward + backward   training.L2NormRows + OrthogonalLoss under autograd, the       torch: autograd of that composition
                               gradient of the un-normalised codebook
          active, fwd + bwd    the same with a histogram in which every second code is 0      torch: the rows picked by a boolean
                                                                                              mask of the histogram (a host sync)
        --train: also tools/train_bench.py 4096 hip 20 with and without `- orth`, alternated, each in a process of its own.
        Last, the compiler's own report of the kernels' registers, LDS and scratch (no GPU needed).
"""
import argparse
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from vq_cosine_bench import alternate          # noqa: E402  (the cosine section's method: alternating forms, host clock + synchronise)

SHAPES = [(512, 64, 50), (8192, 128, 5), (16384, 256, 2)]          # K, D, calls per sample


def groups(K, D):
    import torch
    import torch.nn.functional as TF
    from vqvae_amd import functional as F, training as T
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(K + D)
    W = torch.randn(K, D, device=dev, generator=g).requires_grad_(True)
    hist = (torch.arange(K, device=dev) % 2).to(torch.int32)
    ws = F.vq_orthogonal_workspace(K, D, dev)

    def hip_fwd():
        with torch.no_grad():
            return F.vq_orthogonal_forward(F.l2norm_rows(W)[0], want_saved=True, workspace=ws)

    def torch_loss(n):
        m = n.shape[0]
        return (n @ n.t()).pow(2).sum() / (m * m) - 1.0 / m

    def torch_fwd():
        with torch.no_grad():
            return torch_loss(TF.normalize(W, dim=1))

    def hip_train(h):
        return torch.autograd.grad(T.OrthogonalLoss.apply(T.L2NormRows.apply(W), h, None, None, ws), W)

    def torch_train(h):
        n = TF.normalize(W, dim=1)
        if h is not None:
            n = n[h > 0]
        return torch.autograd.grad(torch_loss(n), W)

    return [("forward", {"hip": hip_fwd, "torch": torch_fwd}),
            ("forward + backward", {"hip": lambda: hip_train(None), "torch": lambda: torch_train(None)}),
            ("active, fwd + bwd", {"hip": lambda: hip_train(hist), "torch": lambda: torch_train(hist)})]


def peak_mib(fn):
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return peak / 2 ** 20


def resource_report(say):
    from vqvae_amd import build
    src = os.path.join(build.CSRC, "vq_orthogonal.hip")
    r = subprocess.run([build.hipcc(), *build.flags_for(src), "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull],
                       capture_output=True, text=True)
    say("compiler report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): orth_main_kernel<width class, with V>")
    name, row = None, {}
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            t = re.search(r"(orth_\w+?_kernel)(?:I((?:L[ib]\d+E)+))?", m.group(2))
            name = m.group(2)
            if t:
                name = t.group(1) + (("<" + ", ".join(re.findall(r"L[ib](\d+)E", t.group(2))) + ">") if t.group(2) else "")
            row = {}
        else:
            row[m.group(1)] = m.group(2)
            if m.group(1).startswith("LDS"):
                say(f"  {name}: VGPRs {row.get('VGPRs')}, AGPRs {row.get('AGPRs')}, scratch {row.get('ScratchSize [bytes/lane]')} B/lane, "
                    f"LDS {row.get('LDS Size [bytes/block]')} B, occupancy {row.get('Occupancy [waves/SIMD]')} waves/SIMD")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default="profiles/vq_orthogonal.txt")
    ap.add_argument("--train", action="store_true", help="also tools/train_bench.py 4096 hip 20 with and without the option")
    ap.add_argument("--no-gpu", action="store_true", help="the compiler report only")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")

    say(f"# tools/vq_orthogonal_bench.py: one process, the forms of a group alternate; {a.repeats} samples of the stated number of calls; "
        "ms per call, host clock around a device synchronise: median (min .. max); peak = torch's allocator above the state before one call")
    say("# hip = csrc/vq_orthogonal.hip behind csrc/vq_cosine.hip's row normalisation (functional.l2norm_rows + vq_orthogonal_forward "
        "with saved; training.L2NormRows + OrthogonalLoss under autograd); torch = F.normalize, mm, pow(2).sum() in fp32 and its autograd, "
        "the active rows picked by a boolean mask")
    say("# fp64 rate = K^2 D (one fma, one multiply, one add) over the hip forward's time, the normalisation and the launches included: "
        "a whole-call figure, not a kernel's share of peak")
    if not a.no_gpu:
        for K, D, steps in SHAPES:
            for title, forms in groups(K, D):
                ms = alternate(forms, a.repeats, steps)
                med = {k: statistics.median(v) for k, v in ms.items()}
                peaks = {k: peak_mib(fn) for k, fn in forms.items()}
                cells = "   ".join(f"{k} {med[k]:.4f} ({min(v):.4f} .. {max(v):.4f}) peak {peaks[k]:.1f} MiB" for k, v in ms.items())
                rate = f"   fp64 rate {3.0 * K * K * D / med['hip'] / 1e9:.2f} Top/s" if title == "forward" else ""
                say(f"K = {K:5d} D = {D:3d}  {steps:2d} calls  {title}: {cells}   hip / torch {med['hip'] / med['torch']:.2f}{rate}")
        if a.train:
            for extra in ([], ["-", "orth"], [], ["-", "orth"]):
                out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_bench.py"), "4096", "hip", "20", *extra],
                                     capture_output=True, text=True, timeout=600)
                for line in (out.stdout.strip().splitlines() or [f"train_bench.py failed: {out.stderr[-300:]}"]):
                    say("train_bench.py 4096 hip 20" + (" - orth" if extra else "") + ":  " + line)
                if out.returncode != 0:                # a fault, an abort or a time limit: nothing more is started on this GPU
                    say(f"train_bench.py exited with {out.returncode}: stopping here")
                    write()
                    sys.exit(out.returncode or 1)
    else:
        say("(--no-gpu: nothing timed)")
    resource_report(say)
    write()


if __name__ == "__main__":
    main()
