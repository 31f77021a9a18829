#!/usr/bin/env python3
"""The cosine-similarity codebook's kernels (csrc/vq_cosine.hip) at N = 262 144 rows (B = 4096, 8 x 8 maps), D = 64, K = 512, in both
layouts: functional.l2norm_rows, functional.l2norm_rows_backward, and the cosine quantizer's forward and forward + backward, each
beside (a) the same result composed from torch.nn.functional.normalize (and its autograd) around the existing HIP quantizer and
(b) the quantizer with the option off.

    python tools/vq_cosine_bench.py [--repeats 7] [--steps 30] [--out profiles/vq_cosine.txt]
        one process; per layout the forms of a group alternate --repeats times, a sample is the mean ms per call over --steps calls
        (host clock around work that ends in a device synchronise).  Reported: the median of the samples and their spread
        (min .. max), the ratio to the torch composition, and for the normalisation alone the bytes per second over the call time
        against the bytes the algorithm moves (forward: x read, y and denom written = 2 N D 4 + 4 N; backward: y, grad_y and denom
        read, grad_x written = 3 N D 4 + 4 N) and against a bare copy of the same tensor (torch's copy_ of N D floats, 2 N D 4
        bytes, timed the same way in the same process; bench.py --full's VQ_COPY_ROOF holds its own figure for this row count).
        Last, the compiler's own report of the kernels' registers, LDS and scratch (no GPU needed).
"""
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
BETA = 0.25
WARMUP = 3
FWD_BYTES = 2 * N * D * 4 + 4 * N
BWD_BYTES = 3 * N * D * 4 + 4 * N
COPY_BYTES = 2 * N * D * 4


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
    """-> [(title, {form: callable}, bytes the first form's algorithm moves or None)] for one layout"""
    import torch
    import torch.nn.functional as TF
    from vqvae_amd import functional as F, training as T
    from vqvae_amd.modules import VectorQuantizer
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(10 + int(rowmajor))
    shape = (B, H, W, D) if rowmajor else (B, D, H, W)
    dim = 3 if rowmajor else 1
    x = torch.randn(shape, device=dev, generator=g)
    gy = torch.randn(shape, device=dev, generator=g)
    y, den = F.l2norm_rows(x, rowmajor=rowmajor)
    xt = x.clone().requires_grad_(True)
    yt = TF.normalize(xt, dim=dim, eps=1e-12)
    dst = torch.empty_like(x)
    on = VectorQuantizer(K, D, BETA, cosine_sim=True).to(dev)
    off = VectorQuantizer(K, D, BETA).to(dev)
    with torch.no_grad():
        on.embedding.weight.copy_(0.3 * torch.randn(K, D, device=dev, generator=g))
        off.embedding.weight.copy_(on.embedding.weight)
    ws = F.vq_workspace(K, D, dev)

    def composed_fwd():
        with torch.no_grad():
            return F.vq_forward(TF.normalize(x, dim=dim, eps=1e-12), TF.normalize(on.embedding.weight, dim=1, eps=1e-12), BETA,
                                rowmajor=rowmajor, workspace=ws)

    def module_fwd(m):
        with torch.no_grad():
            return m.quantize(x, rowmajor=rowmajor)

    def module_step(m):
        z = x.detach().requires_grad_(True)
        m.embedding.weight.grad = None
        loss, z_q, *_ = m.quantize(z, rowmajor=rowmajor)
        ((z_q * gy).sum() + loss).backward()

    def composed_step():
        z = x.detach().requires_grad_(True)
        w = on.embedding.weight
        w.grad = None
        loss, z_q, *_ = T.VQStraightThrough.apply(TF.normalize(z, dim=dim, eps=1e-12), TF.normalize(w, dim=1, eps=1e-12), BETA,
                                                  rowmajor, ws, False)
        ((z_q * gy).sum() + loss).backward()

    return [
        ("l2norm_rows", {"hip": lambda: F.l2norm_rows(x, rowmajor=rowmajor),
                         "torch": lambda: TF.normalize(x, dim=dim, eps=1e-12),
                         "copy": lambda: dst.copy_(x)}, FWD_BYTES),
        ("l2norm_rows_backward", {"hip": lambda: F.l2norm_rows_backward(y, den, gy, rowmajor=rowmajor),
                                  "torch": lambda: torch.autograd.grad(yt, xt, gy, retain_graph=True)}, BWD_BYTES),
        ("cosine quantizer, forward", {"hip": lambda: module_fwd(on), "torch": composed_fwd, "option off": lambda: module_fwd(off)}, None),
        ("cosine quantizer, forward + backward", {"hip": lambda: module_step(on), "torch": composed_step,
                                                  "option off": lambda: module_step(off)}, None),
    ]


def resource_report(say):
    from vqvae_amd import build
    src = os.path.join(build.CSRC, "vq_cosine.hip")
    r = subprocess.run([build.hipcc(), *build.flags_for(src), "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull],
                       capture_output=True, text=True)
    say("compiler report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): vq_l2norm_nchw_kernel<backward, D up to which a row "
        "stays in registers (0: re-read), pixels per lane>, vq_l2norm_rows_kernel<backward, floats per global access>")
    name, row = None, {}
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            t = re.search(r"(vq_l2norm_\w+?_kernel)ILb([01])E(?:Li(\d+)E)?(?:Li(\d+)E)?", m.group(2))
            name = m.group(2)
            if t:
                name = f"{t.group(1)}<{'true' if t.group(2) == '1' else 'false'}" + "".join(f", {v}" for v in t.groups()[2:] if v) + ">"
            row = {}
        else:
            row[m.group(1)] = m.group(2)
            if m.group(1).startswith("LDS"):
                say(f"  {name}: VGPRs {row.get('VGPRs')}, AGPRs {row.get('AGPRs')}, scratch {row.get('ScratchSize [bytes/lane]')} B/lane, "
                    f"LDS {row.get('LDS Size [bytes/block]')} B, occupancy {row.get('Occupancy [waves/SIMD]')} waves/SIMD")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", default="profiles/vq_cosine.txt")
    ap.add_argument("--no-gpu", action="store_true", help="the compiler report only")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/vq_cosine_bench.py: N = {N} rows (B = {B}, {H} x {W}), D = {D}, K = {K}; one process, the forms of a group alternate; "
        f"{a.repeats} samples of {a.steps} calls; ms per call, host clock around a device synchronise: median (min .. max)")
    say("# hip = csrc/vq_cosine.hip (functional.l2norm_rows / l2norm_rows_backward; VectorQuantizer(cosine_sim=True).quantize); torch = "
        "the same result from torch.nn.functional.normalize (and its autograd) around the existing HIP quantizer; option off = the "
        "quantizer without the normalisation; copy = torch's copy_ of the same N D floats")
    if not a.no_gpu:
        for rowmajor in (True, False):
            layout = "rows" if rowmajor else "NCHW"
            for title, forms, moved in groups(rowmajor):
                ms = alternate(forms, a.repeats, a.steps)
                med = {k: statistics.median(v) for k, v in ms.items()}
                cells = "   ".join(f"{k} {med[k]:.4f} ({min(v):.4f} .. {max(v):.4f})" for k, v in ms.items())
                tail = f"   hip / torch {med['hip'] / med['torch']:.2f}"
                if "option off" in med:
                    tail += f"   hip / option off {med['hip'] / med['option off']:.2f}"
                if moved:
                    tail += f"   hip {moved / med['hip'] / 1e9:.2f} TB/s of the {moved / 1e6:.0f} MB the algorithm moves"
                if "copy" in med:
                    tail += f"   copy {COPY_BYTES / med['copy'] / 1e9:.2f} TB/s of its {COPY_BYTES / 1e6:.0f} MB"
                say(f"{layout}  {title}: {cells}{tail}")
    else:
        say("(--no-gpu: nothing timed)")
    resource_report(say)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
