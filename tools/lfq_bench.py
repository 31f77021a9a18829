#!/usr/bin/env python3
"""The lookup-free-quantization kernels (csrc/vq_lfq.hip) at N = 262 144 rows (B = 4096, 8 x 8 maps), D = 64, d = 10 (K = 1024) and
d = 12 (K = 4096), in both layouts: functional.lfq_forward with the losses and training.lfq_backward with every gradient, each beside
the same result composed from torch ops on the same GPU (F.linear, sign, the (N, K) softmax entropy loss in fp32, and its autograd)
and beside torch's copy_ of z.

    python tools/lfq_bench.py [--repeats 5] [--steps 10] [--out profiles/lfq.txt] [--train]
        one process; per layout and d the forms of a group alternate --repeats times, a sample is the mean ms per call over --steps
        calls (host clock around work that ends in a device synchronise).  Reported: the median of the samples and their spread
        (min .. max), the ratio to the torch composition and to the copy, the losses of both forms, and the peak device memory one call
        of each form allocates.  A composition that cannot allocate its (N, K) tensors is recorded as such.
        --train: also tools/train_bench.py 4096 hip 20 with and without the option, each in a process of its own.
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

B, H, W, D = 4096, 8, 8, 64
N = B * H * W
BITS = [10, 12]
BETA, WE, GAMMA, INV_T = 0.25, 0.1, 1.0, 100.0
COPY_BYTES = 2 * N * D * 4


def groups(rowmajor, d):
    import torch
    import torch.nn.functional as TF
    from vqvae_amd import functional as F, training as T
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(30 + int(rowmajor))
    K = 1 << d
    shape = (B, H, W, D) if rowmajor else (B, D, H, W)
    z = torch.randn(shape, device=dev, generator=g)
    gq = torch.randn(shape, device=dev, generator=g)
    w_in = torch.randn(d, D, device=dev, generator=g) * (0.02 / D ** 0.5)          # |s y| of a few units: nothing saturates
    b_in = 0.002 * torch.randn(d, device=dev, generator=g)
    w_out = torch.randn(D, d, device=dev, generator=g) / d ** 0.5
    b_out = 0.1 * torch.randn(D, device=dev, generator=g)
    gl = torch.ones((), device=dev)
    ws = F.lfq_workspace(N, D, d, dev)
    kw = dict(beta=BETA, entropy_weight=WE, diversity_gamma=GAMMA, inv_temperature=INV_T, rowmajor=rowmajor, workspace=ws)
    avg = F.lfq_forward(z, w_in, b_in, w_out, b_out, K, **kw)[5]
    dst = torch.empty_like(z)
    codes = (((torch.arange(K, device=dev)[:, None] >> torch.arange(d, device=dev)[None, :]) & 1) * 2 - 1).float()

    def rows(t):                                   # the composition works on (..., D): channels last
        return t if rowmajor else t.permute(0, 2, 3, 1)

    def back(t):
        return t if rowmajor else t.permute(0, 3, 1, 2).contiguous()

    params = [p.clone().requires_grad_(True) for p in (w_in, b_in, w_out, b_out)]

    def compose(zr, wi, bi, wo, bo):               # what a user would write (vector-quantize-pytorch's LFQ without its clamp)
        y = TF.linear(zr, wi, bi)
        c = torch.where(y > 0, 1.0, -1.0)
        zq = TF.linear(y + (c - y).detach(), wo, bo)
        commit = ((y - c) ** 2).mean()
        logp = torch.log_softmax(2.0 * INV_T * (y.reshape(-1, d) @ codes.T), dim=1)
        prob = logp.exp()
        per_sample = -(prob * logp).sum(1).mean()
        a = prob.mean(0)
        codebook = -(a * torch.log(a.clamp_min(1e-38))).sum()
        return zq, BETA * commit + WE * (per_sample - GAMMA * codebook)

    def torch_fwd():
        with torch.no_grad():
            zq, loss = compose(rows(z), w_in, b_in, w_out, b_out)
            return back(zq), loss

    def torch_bwd():
        zt = z.detach().requires_grad_(True)
        zq, loss = compose(rows(zt), *params)
        return torch.autograd.grad([back(zq), loss], [zt, *params], [gq, gl])

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = fn()
        torch.cuda.synchronize()
        del out
        return (torch.cuda.max_memory_allocated() - base) / 2 ** 20

    hip_fwd = lambda: F.lfq_forward(z, w_in, b_in, w_out, b_out, K, **kw)
    hip_bwd = lambda: T.lfq_backward(z, gq, gl, avg, w_in, b_in, w_out, K, **kw)
    info = {"hip loss": float(hip_fwd()[4][0]), "workspace MiB": ws.numel() / 2 ** 20,
            "hip forward peak MiB": peak(hip_fwd), "hip backward peak MiB": peak(hip_bwd)}
    fwd = {"hip": hip_fwd, "copy": lambda: dst.copy_(z)}
    bwd = {"hip": hip_bwd, "copy": lambda: dst.copy_(z)}
    try:
        info["torch loss"] = float(torch_fwd()[1])
        info["torch forward peak MiB"] = peak(torch_fwd)
        info["torch backward peak MiB"] = peak(torch_bwd)
        fwd["torch"], bwd["torch"] = torch_fwd, torch_bwd
    except torch.OutOfMemoryError as e:
        info["torch"] = f"the composition could not allocate its (N, K) tensors: {str(e)[:120]}"
        torch.cuda.empty_cache()
    return [("forward with losses", fwd), ("backward, all gradients", bwd)], info


def resource_report(say):
    from vqvae_amd import build
    src = os.path.join(build.CSRC, "vq_lfq.hip")
    r = subprocess.run([build.hipcc(), *build.flags_for(src), "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull],
                       capture_output=True, text=True)
    say("compiler report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): proj_fwd_nchw_kernel<Lfq, decode, weight floats>, "
        "proj_fwd_rows_kernel<Lfq, decode, floats per global access, weight floats>, proj_bwd_nchw_kernel<Lfq, parameter gradients, "
        "weight floats>, proj_bwd_rows_kernel<Lfq, parameter gradients, floats per global access, weight floats> (vq_proj_kernels.h), "
        "lfq_entgrad_kernel<doubles of log avg in LDS>")
    name, row = None, {}
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            t = re.search(r"((?:lfq|proj)_\w+?_kernel)(?:I(?:NS_\d(Lfq)E)?(?:Lb([01])E)?((?:Li\d+E)*))?", m.group(2))
            name = m.group(2)
            if t:
                args = ([t.group(2)] if t.group(2) else []) + ([("true" if t.group(3) == "1" else "false")] if t.group(3) is not None else []) + \
                    re.findall(r"Li(\d+)E", t.group(4) or "")
                name = t.group(1) + (f"<{', '.join(args)}>" if args else "")
            row = {}
        else:
            row[m.group(1)] = m.group(2)
            if m.group(1).startswith("LDS"):
                say(f"  {name}: VGPRs {row.get('VGPRs')}, AGPRs {row.get('AGPRs')}, scratch {row.get('ScratchSize [bytes/lane]')} B/lane, "
                    f"LDS {row.get('LDS Size [bytes/block]')} B, occupancy {row.get('Occupancy [waves/SIMD]')} waves/SIMD")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default="profiles/lfq.txt")
    ap.add_argument("--train", action="store_true", help="also tools/train_bench.py 4096 hip 20 with and without the option")
    ap.add_argument("--no-gpu", action="store_true", help="the compiler report only")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/lfq_bench.py: N = {N} rows (B = {B}, {H} x {W}), D = {D}; one process, the forms of a group alternate; "
        f"{a.repeats} samples of {a.steps} calls; ms per call, host clock around a device synchronise: median (min .. max)")
    say("# hip = csrc/vq_lfq.hip (functional.lfq_forward with z_q, idx, hist, perplexity, the four losses and avg; training.lfq_backward "
        "with grad_z and the four parameter gradients, from grad_zq and grad_loss); torch = the same results from F.linear, where, the "
        "(N, K) log_softmax entropy loss and F.linear in fp32 (and their autograd) on the same GPU; copy = torch's copy_ of the same N D floats")
    say(f"# beta {BETA}, entropy_weight {WE}, diversity_gamma {GAMMA}, inv_temperature {INV_T}; y of scale 0.02 (|s y| of a few units)")
    if not a.no_gpu:
        for d in BITS:
            for rowmajor in (True, False):
                layout = "rows" if rowmajor else "NCHW"
                gs, info = groups(rowmajor, d)
                say(f"d {d} (K = {1 << d})  {layout}  " + "   ".join(f"{k}: {v:.6g}" if isinstance(v, float) else f"{k}: {v}" for k, v in info.items()))
                for title, forms in gs:
                    ms = alternate(forms, a.repeats, a.steps)
                    med = {k: statistics.median(v) for k, v in ms.items()}
                    cells = "   ".join(f"{k} {med[k]:.4f} ({min(v):.4f} .. {max(v):.4f})" for k, v in ms.items())
                    ratio = f"hip / torch {med['hip'] / med['torch']:.3f}   " if "torch" in med else ""
                    say(f"d {d} (K = {1 << d})  {layout}  {title}: {cells}   {ratio}hip / copy {med['hip'] / med['copy']:.2f}   "
                        f"copy {COPY_BYTES / med['copy'] / 1e9:.2f} TB/s of its {COPY_BYTES / 1e6:.0f} MB")
        if a.train:
            for extra in ([], ["-", "lfq"]):
                out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_bench.py"), "4096", "hip", "20", *extra],
                                     capture_output=True, text=True, timeout=600)
                for line in (out.stdout.strip().splitlines() or [f"train_bench.py failed: {out.stderr[-300:]}"]):
                    say("train_bench.py 4096 hip 20" + (" - lfq" if extra else "") + ":  " + line)
    else:
        say("(--no-gpu: nothing timed)")
    resource_report(say)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
