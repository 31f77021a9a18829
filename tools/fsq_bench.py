#!/usr/bin/env python3
"""The finite-scalar-quantization kernels (csrc/vq_fsq.hip) at N = 262 144 rows (B = 4096, 8 x 8 maps), D = 64, levels (8, 5, 5, 5)
and (8, 8, 8, 5, 5, 5), in both layouts: functional.fsq_forward, training.fsq_backward and functional.fsq_decode_indices, each beside
the same result composed from torch ops on the same GPU (F.linear, tanh, round, F.linear in fp32, and its autograd) and beside torch's
copy_ of the same tensor.

    python tools/fsq_bench.py [--repeats 7] [--steps 30] [--out profiles/fsq.txt] [--train]
        one process; per layout and level list the forms of a group alternate --repeats times, a sample is the mean ms per call over
        --steps calls (host clock around work that ends in a device synchronise).  Reported: the median of the samples and their
        spread (min .. max), the ratio to the torch composition, the bytes per second over the call time against the bytes the
        algorithm moves (forward: z read, z_q and idx written = 2 N D 4 + 8 N; backward: z and grad_zq read, grad_z written = 3 N D 4,
        plus the partials; decode: idx read, z_q written = N D 4 + 8 N) and against a bare copy (2 N D 4 bytes).
        --train: also tools/train_bench.py 4096 hip 20 with and without the option, each in a process of its own.
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from vq_cosine_bench import alternate          # noqa: E402  (the cosine section's method: alternating forms, host clock + synchronise)

B, H, W, D = 4096, 8, 8, 64
N = B * H * W
LEVELS = [(8, 5, 5, 5), (8, 8, 8, 5, 5, 5)]
COPY_BYTES = 2 * N * D * 4


def moved_bytes(d):
    partials = (N // 256) * (2 * D * d + D + d) * 8
    return {"forward": 2 * N * D * 4 + 8 * N, "backward": 3 * N * D * 4 + 2 * partials, "decode": N * D * 4 + 8 * N}


def groups(rowmajor, levels):
    import torch
    import torch.nn.functional as TF
    from tests import vq_fsq_ref as R
    from vqvae_amd import functional as F, training as T
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(20 + int(rowmajor))
    d = len(levels)
    shape = (B, H, W, D) if rowmajor else (B, D, H, W)
    z = torch.randn(shape, device=dev, generator=g)
    gq = torch.randn(shape, device=dev, generator=g)
    w_in = torch.randn(d, D, device=dev, generator=g) * (1.5 / D ** 0.5)
    b_in = 0.1 * torch.randn(d, device=dev, generator=g)
    w_out = torch.randn(D, d, device=dev, generator=g) / d ** 0.5
    b_out = 0.1 * torch.randn(D, device=dev, generator=g)
    idx = F.fsq_forward(z, w_in, b_in, w_out, b_out, levels, rowmajor=rowmajor)[2]
    dst = torch.empty_like(z)
    k = R.Consts(levels)
    lv = torch.tensor(k.levels, device=dev)
    basis = torch.tensor(k.basis, device=dev)
    hw = torch.tensor(k.hw, device=dev)

    def rows(t):                                   # the composition works on (..., D): channels last
        return t if rowmajor else t.permute(0, 2, 3, 1)

    def back(t):
        return t if rowmajor else t.permute(0, 3, 1, 2).contiguous()

    params = [p.clone().requires_grad_(True) for p in (w_in, b_in, w_out, b_out)]
    half_l, offset, shift = [torch.tensor(v, dtype=torch.float32, device=dev) for v in (k.half_l, k.offset, k.shift)]
    hwf = hw.float()

    def compose(zr, wi, bi, wo, bo):               # tests/vq_fsq_ref.py's torch_composition with its constants made once
        b = torch.tanh(TF.linear(zr, wi, bi) + shift) * half_l - offset
        q = b + (torch.round(b) - b).detach()
        return TF.linear(q / hwf, wo, bo)

    def torch_fwd():
        with torch.no_grad():
            return back(compose(rows(z), w_in, b_in, w_out, b_out))

    def torch_bwd():
        zt = z.detach().requires_grad_(True)
        zq = back(compose(rows(zt), *params))
        return torch.autograd.grad(zq, [zt, *params], gq)

    def torch_dec():
        q = (idx.view(-1, 1) // basis[None, :]) % lv[None, :] - hw[None, :]
        return back(TF.linear(q.float() / hw.float()[None, :], w_out, b_out).view(B, H, W, D))

    return [
        ("forward", {"hip": lambda: F.fsq_forward(z, w_in, b_in, w_out, b_out, levels, rowmajor=rowmajor), "torch": torch_fwd,
                     "copy": lambda: dst.copy_(z)}),
        ("backward", {"hip": lambda: T.fsq_backward(z, gq, w_in, b_in, w_out, levels, rowmajor=rowmajor), "torch": torch_bwd,
                      "copy": lambda: dst.copy_(z)}),
        ("decode", {"hip": lambda: F.fsq_decode_indices(idx, w_out, b_out, levels, B, H, W, rowmajor=rowmajor, validate=False),
                    "torch": torch_dec, "copy": lambda: dst.copy_(z)}),
    ]


def resource_report(say):
    from vqvae_amd import build
    src = os.path.join(build.CSRC, "vq_fsq.hip")
    r = subprocess.run([build.hipcc(), *build.flags_for(src), "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull],
                       capture_output=True, text=True)
    say("compiler report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): proj_fwd_nchw_kernel<Fsq, decode, weight floats>, "
        "proj_fwd_rows_kernel<Fsq, decode, floats per global access, weight floats>, proj_bwd_nchw_kernel<Fsq, parameter gradients, "
        "weight floats>, proj_bwd_rows_kernel<Fsq, parameter gradients, floats per global access, weight floats> (vq_proj_kernels.h)")
    name, row = None, {}
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            t = re.search(r"(proj_\w+?_kernel)INS_\d(Fsq)E(?:Lb([01])E((?:Li\d+E)*))?", m.group(2))
            name = m.group(2)
            if t and t.group(3) is not None:
                name = f"{t.group(1)}<{t.group(2)}, {'true' if t.group(3) == '1' else 'false'}" + "".join(f", {v}" for v in re.findall(r"Li(\d+)E", t.group(4))) + ">"
            elif t:
                name = f"{t.group(1)}<{t.group(2)}>"
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
    ap.add_argument("--out", default="profiles/fsq.txt")
    ap.add_argument("--train", action="store_true", help="also tools/train_bench.py 4096 hip 20 with and without the option")
    ap.add_argument("--no-gpu", action="store_true", help="the compiler report only")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# tools/fsq_bench.py: N = {N} rows (B = {B}, {H} x {W}), D = {D}; one process, the forms of a group alternate; "
        f"{a.repeats} samples of {a.steps} calls; ms per call, host clock around a device synchronise: median (min .. max)")
    say("# hip = csrc/vq_fsq.hip (functional.fsq_forward with z_q, idx, hist and perplexity; training.fsq_backward with grad_z and the "
        "four parameter gradients; functional.fsq_decode_indices); torch = the same results from F.linear, tanh, round and F.linear "
        "in fp32 (and their autograd; the decode from integer ops and F.linear) on the same GPU; copy = torch's copy_ of the same N D floats")
    if not a.no_gpu:
        for levels in LEVELS:
            moved = moved_bytes(len(levels))
            for rowmajor in (True, False):
                layout = "rows" if rowmajor else "NCHW"
                for title, forms in groups(rowmajor, levels):
                    ms = alternate(forms, a.repeats, a.steps)
                    med = {k: statistics.median(v) for k, v in ms.items()}
                    cells = "   ".join(f"{k} {med[k]:.4f} ({min(v):.4f} .. {max(v):.4f})" for k, v in ms.items())
                    say(f"levels {levels}  {layout}  {title}: {cells}   hip / torch {med['hip'] / med['torch']:.2f}   hip / copy "
                        f"{med['hip'] / med['copy']:.2f}   hip {moved[title] / med['hip'] / 1e9:.2f} TB/s of the {moved[title] / 1e6:.0f} MB the "
                        f"algorithm moves   copy {COPY_BYTES / med['copy'] / 1e9:.2f} TB/s of its {COPY_BYTES / 1e6:.0f} MB")
        if a.train:
            for extra in ([], ["-", "fsq"]):
                out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_bench.py"), "4096", "hip", "20", *extra],
                                     capture_output=True, text=True, timeout=600)
                for line in (out.stdout.strip().splitlines() or [f"train_bench.py failed: {out.stderr[-300:]}"]):
                    say("train_bench.py 4096 hip 20" + (" - fsq" if extra else "") + ":  " + line)
    else:
        say("(--no-gpu: nothing timed)")
    resource_report(say)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
