#!/usr/bin/env python3
"""The per-row linear map (csrc/vq_linear.hip) and the factorized quantizer built on it at N = 262 144 rows (B = 4096, 8 x 8 maps),
D = 64, d in {8, 32}, in both layouts, each beside the composition a user would write from torch ops on the same GPU and beside torch's
copy_ of z.

    python tools/linear_rows_bench.py [--repeats 7] [--steps 30] [--out profiles/linear_rows.txt] [--train]
        one process; per layout and d the forms of a group alternate --repeats times, a sample is the mean ms per call over --steps
        calls (host clock around work that ends in a device synchronise).  Reported: the median of the samples and their spread
        (min .. max), the ratio to the torch composition and to the copy.
          in / out forward     functional.linear_rows D -> d / d -> D         torch: F.linear in fp32 on rows (a permute around it for
                                                                               NCHW maps)
          in / out backward    functional.linear_rows_backward, all three     torch: autograd of that F.linear
          quantizer forward    FactorizedVectorQuantizer.quantize, no grad    torch: F.linear, VectorQuantizer.quantize, F.linear
          quantizer fwd+bwd    the same under autograd, backward from z_q     torch: the same with torch autograd for the two linears
                               and the loss                                   and training.VQStraightThrough in between
        --train: also tools/train_bench.py 4096 hip 20 with and without `- factorized`, each in a process of its own.
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

B, H, W, D, K = 4096, 8, 8, 64, 512
N = B * H * W
DS = [8, 32]
COPY_BYTES = 2 * N * D * 4


def groups(rowmajor, d):
    import torch
    import torch.nn.functional as TF
    from vqvae_amd import functional as F, training as T
    from vqvae_amd.modules import FactorizedVectorQuantizer, VectorQuantizer
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(30 + int(rowmajor) + d)
    shape = lambda c: (B, H, W, c) if rowmajor else (B, c, H, W)
    z, gz = torch.randn(shape(D), device=dev, generator=g), torch.randn(shape(D), device=dev, generator=g)
    y, gy = torch.randn(shape(d), device=dev, generator=g), torch.randn(shape(d), device=dev, generator=g)
    torch.manual_seed(d)
    q = FactorizedVectorQuantizer(K, D, d, 0.25).to(dev)
    with torch.no_grad():
        q.embedding.weight.normal_()
    w_in, b_in, w_out, b_out = [p.detach() for p in (q.project_in.weight, q.project_in.bias, q.project_out.weight, q.project_out.bias)]
    dst = torch.empty_like(z)

    def rows(t):                                   # F.linear works on (..., C): channels last
        return t if rowmajor else t.permute(0, 2, 3, 1)

    def back(t):
        return t if rowmajor else t.permute(0, 3, 1, 2).contiguous()

    def torch_fwd(x, w, b):
        with torch.no_grad():
            return back(TF.linear(rows(x), w, b))

    def torch_bwd(x, gyy, w, b):
        xt, wt, bt = x.detach().requires_grad_(True), w.detach().requires_grad_(True), b.detach().requires_grad_(True)
        return torch.autograd.grad(back(TF.linear(rows(xt), wt, bt)), [xt, wt, bt], gyy)

    def torch_quant():
        with torch.no_grad():
            yy = back(TF.linear(rows(z), w_in, b_in))
            loss, zq, ppl, idx, hist = VectorQuantizer.quantize(q, yy, rowmajor=rowmajor)        # (the inner quantizer as the module runs it)
            return loss, back(TF.linear(rows(zq), w_out, b_out)), ppl, idx, hist

    def quant_train(hip):
        params = list(q.parameters())
        zt = z.detach().requires_grad_(True)
        if hip:
            loss, zq = q.quantize(zt, rowmajor=rowmajor)[:2]
        else:
            yy = back(TF.linear(rows(zt), q.project_in.weight, q.project_in.bias))
            loss, zq_low = VectorQuantizer.quantize(q, yy, rowmajor=rowmajor)[:2]                  # (training.VQStraightThrough)
            zq = back(TF.linear(rows(zq_low), q.project_out.weight, q.project_out.bias))
        return torch.autograd.grad([zq, loss], [zt, *params], [gz, torch.ones_like(loss)])

    def hip_quant():
        with torch.no_grad():
            return q.quantize(z, rowmajor=rowmajor)

    copy = lambda: dst.copy_(z)
    return [
        (f"in  ({D} -> {d}) forward", {"hip": lambda: F.linear_rows(z, w_in, b_in, rowmajor=rowmajor), "torch": lambda: torch_fwd(z, w_in, b_in), "copy": copy}),
        (f"out ({d} -> {D}) forward", {"hip": lambda: F.linear_rows(y, w_out, b_out, rowmajor=rowmajor), "torch": lambda: torch_fwd(y, w_out, b_out), "copy": copy}),
        (f"in  ({D} -> {d}) backward", {"hip": lambda: F.linear_rows_backward(z, gy, w_in, rowmajor=rowmajor), "torch": lambda: torch_bwd(z, gy, w_in, b_in), "copy": copy}),
        (f"out ({d} -> {D}) backward", {"hip": lambda: F.linear_rows_backward(y, gz, w_out, rowmajor=rowmajor), "torch": lambda: torch_bwd(y, gz, w_out, b_out), "copy": copy}),
        ("quantizer forward", {"hip": hip_quant, "torch": torch_quant, "copy": copy}),
        ("quantizer fwd+bwd", {"hip": lambda: quant_train(True), "torch": lambda: quant_train(False), "copy": copy}),
    ]


def resource_report(say):
    from vqvae_amd import build
    src = os.path.join(build.CSRC, "vq_linear.hip")
    r = subprocess.run([build.hipcc(), *build.flags_for(src), "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull],
                       capture_output=True, text=True)
    say("compiler report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): lin_nchw_kernel<sums per row, pixels per lane, fp64 weights in LDS>, "
        "lin_rows_kernel<sums per row, floats per global access, fp64 weights in LDS>, lin_params_kernel<row-major, floats per global access>")
    name, row = None, {}
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            t = re.search(r"(lin_\w+?_kernel)(?:I((?:L[ib]\d+E)+))?", m.group(2))
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
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", default="profiles/linear_rows.txt")
    ap.add_argument("--train", action="store_true", help="also tools/train_bench.py 4096 hip 20 with and without the option")
    ap.add_argument("--no-gpu", action="store_true", help="the compiler report only")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/linear_rows_bench.py: N = {N} rows (B = {B}, {H} x {W}), D = {D}, K = {K}; one process, the forms of a group alternate; "
        f"{a.repeats} samples of {a.steps} calls; ms per call, host clock around a device synchronise: median (min .. max)")
    say("# hip = csrc/vq_linear.hip (functional.linear_rows; functional.linear_rows_backward with grad_x, grad_w and grad_b; "
        "FactorizedVectorQuantizer.quantize without and under autograd); torch = F.linear in fp32 on rows (a permute around it for NCHW "
        "maps), its autograd, and the same quantizer kernels between two such linears; copy = torch's copy_ of the N D floats of z")
    if not a.no_gpu:
        for d in DS:
            for rowmajor in (True, False):
                layout = "rows" if rowmajor else "NCHW"
                for title, forms in groups(rowmajor, d):
                    ms = alternate(forms, a.repeats, a.steps)
                    med = {k: statistics.median(v) for k, v in ms.items()}
                    cells = "   ".join(f"{k} {med[k]:.4f} ({min(v):.4f} .. {max(v):.4f})" for k, v in ms.items())
                    say(f"d = {d:2d}  {layout}  {title}: {cells}   hip / torch {med['hip'] / med['torch']:.2f}   hip / copy "
                        f"{med['hip'] / med['copy']:.2f}   copy {COPY_BYTES / med['copy'] / 1e9:.2f} TB/s of its {COPY_BYTES / 1e6:.0f} MB")
        if a.train:
            for extra in ([], ["-", "factorized"]):
                out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_bench.py"), "4096", "hip", "20", *extra],
                                     capture_output=True, text=True, timeout=600)
                for line in (out.stdout.strip().splitlines() or [f"train_bench.py failed: {out.stderr[-300:]}"]):
                    say("train_bench.py 4096 hip 20" + (" - factorized" if extra else "") + ":  " + line)
                if out.returncode != 0:                # a fault, an abort or a time limit: nothing more is started on this GPU
                    say(f"train_bench.py exited with {out.returncode}: stopping here")
                    open(a.out, "w").write("\n".join(lines) + "\n")
                    sys.exit(out.returncode or 1)
    else:
        say("(--no-gpu: nothing timed)")
    resource_report(say)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
