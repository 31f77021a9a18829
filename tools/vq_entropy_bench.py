#!/usr/bin/env python3
"""The code-entropy loss of a learned codebook (csrc/vq_entropy.hip) at 262 144 rows, D = 64, K = 512 and K = 4096, in both layouts,
beside the composition a user would write from torch ops on the same GPU.

    python tools/vq_entropy_bench.py [--repeats 5] [--rows 262144] [--out profiles/vq_entropy.txt] [--train]
        one process; per shape the forms of a group alternate --repeats times, a sample is the mean ms per call over a number of calls
        that fits the shape (host clock around work that ends in a device synchronise).  Reported: the median of the samples and
        their spread (min .. max), the ratio to the torch composition, and the peak of torch's allocator above what was allocated
        before the call.
          forward              functional.vq_entropy_forward with rowstat                torch: zz + ee - 2 z E^T, log_softmax and the two
                                                                                         entropies in fp32 under no_grad
          forward + backward   training.CodeEntropyLoss under autograd, the gradients    torch: autograd of that composition
                               of z and of the codebook
          copy                 torch's copy_ of z: the memory yardstick
        --train: also tools/train_bench.py 4096 hip 20 with and without `- entropy`, alternated, each in a process of its own.
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
from vq_orthogonal_bench import peak_mib       # noqa: E402

S, GAMMA = 100.0, 1.0


def groups(N, K, D, rowmajor):
    import torch
    from vqvae_amd import functional as F, training as T
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(K + D)
    B, HW = N // 1024, 32
    E = (0.05 / D ** 0.5 * torch.randn(K, D, device=dev, generator=g)).requires_grad_(True)
    rows = 0.05 / D ** 0.5 * torch.randn(B, HW, HW, D, device=dev, generator=g)
    z = (rows if rowmajor else rows.permute(0, 3, 1, 2).contiguous()).requires_grad_(True)
    other = torch.empty_like(z)
    ws = F.vq_entropy_workspace(N, K, D, dev)

    def hip_fwd():
        with torch.no_grad():
            return F.vq_entropy_forward(z, E, inv_temperature=S, gamma=GAMMA, rowmajor=rowmajor, workspace=ws)

    def torch_term():
        r = (z if rowmajor else z.permute(0, 2, 3, 1)).reshape(-1, D)
        d = (r * r).sum(1, keepdim=True) + (E * E).sum(1)[None, :] - 2.0 * r @ E.t()
        logp = torch.log_softmax(-S * d, dim=1)
        p = logp.exp()
        P = -(p * logp).sum(1).mean()
        avg = p.mean(0)
        return P - GAMMA * -(avg * torch.log(avg)).sum()

    def torch_fwd():
        with torch.no_grad():
            return torch_term()

    def hip_train():
        return torch.autograd.grad(T.CodeEntropyLoss.apply(z, E, S, GAMMA, rowmajor, ws), (z, E))

    def torch_train():
        return torch.autograd.grad(torch_term(), (z, E))

    def copy():
        with torch.no_grad():
            return other.copy_(z)

    return [("forward", {"hip": hip_fwd, "torch": torch_fwd, "copy": copy}),
            ("forward + backward", {"hip": hip_train, "torch": torch_train})]


def resource_report(say):
    from vqvae_amd import build
    src = os.path.join(build.CSRC, "vq_entropy.hip")
    r = subprocess.run([build.hipcc(), *build.flags_for(src), "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.devnull],
                       capture_output=True, text=True)
    say("compiler report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): ent_row_bwd_kernel<width class, with grad_z>, "
        "ent_grad_e_kernel<width class>")
    name, row = None, {}
    for line in r.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|VGPRs|AGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            t = re.search(r"(ent_\w+?_kernel)(?:I((?:L[ib]\d+E)+))?", m.group(2))
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
    ap.add_argument("--rows", type=int, default=262144, help="a multiple of 1024: maps of 32 x 32")
    ap.add_argument("--out", default="profiles/vq_entropy.txt")
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

    say(f"# tools/vq_entropy_bench.py: one process, the forms of a group alternate; {a.repeats} samples of the stated number of calls; "
        "ms per call, host clock around a device synchronise: median (min .. max); peak = torch's allocator above the state before one call")
    say("# hip = csrc/vq_entropy.hip (functional.vq_entropy_forward with rowstat; training.CodeEntropyLoss under autograd, both "
        "gradients); torch = zz + ee - 2 z E^T, log_softmax, the two entropies in fp32 and their autograd; copy = torch's copy_ of z")
    say(f"# {a.rows} rows, D = 64, inv_temperature = {S}, gamma = {GAMMA}")
    if not a.no_gpu:
        for K, steps in ((512, 5), (4096, 2)):
            for rowmajor in (True, False):
                for title, forms in groups(a.rows, K, 64, rowmajor):
                    ms = alternate(forms, a.repeats, steps)
                    med = {k: statistics.median(v) for k, v in ms.items()}
                    peaks = {k: peak_mib(fn) for k, fn in forms.items()}
                    cells = "   ".join(f"{k} {med[k]:.3f} ({min(v):.3f} .. {max(v):.3f}) peak {peaks[k]:.1f} MiB" for k, v in ms.items())
                    say(f"K = {K:4d} {'rows' if rowmajor else 'NCHW'}  {steps} calls  {title}: {cells}   hip / torch {med['hip'] / med['torch']:.2f}")
                write()
        if a.train:
            for extra in ([], ["-", "entropy"], [], ["-", "entropy"]):
                out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_bench.py"), "4096", "hip", "20", *extra],
                                     capture_output=True, text=True, timeout=600)
                for line in (out.stdout.strip().splitlines() or [f"train_bench.py failed: {out.stderr[-300:]}"]):
                    say("train_bench.py 4096 hip 20" + (" - entropy" if extra else "") + ":  " + line)
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
