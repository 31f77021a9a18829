#!/usr/bin/env python3
"""Training-step time with the three quantizers: VectorQuantizer (the reference's codebook gradient), VectorQuantizerEMA, and
VectorQuantizerEMA with dead-code restart.  The step is main.py:74-78 on the HIP path without the optimizer: forward, fused losses,
backward -- and, for the EMA quantizers, the codebook update inside the forward.  Default model (h 128, K 512, D 64), 32x32 images.

    python tools/ema_step_bench.py [--batches 32 4096] [--steps 50] [--warmup 10]

Prints one JSON line per (quantizer, batch) and a final summary line: median / mean ms per step (CUDA events around each step)."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from vqvae_amd import conv, training as T
from vqvae_amd.modules import VQVAE

QUANTIZERS = {"vq": {}, "ema": {"ema_decay": 0.99}, "ema_restart": {"ema_decay": 0.99, "restart_threshold": 1.0}}


def time_step(kw, B, steps, warmup, dev):
    torch.manual_seed(0)
    model = VQVAE(128, 32, 2, 512, 64, 0.25, **kw).to(dev).train()
    x = torch.randn(B, 3, 32, 32, device=dev)

    def step():
        model.zero_grad(set_to_none=False)
        el, xh, pp = model(x)
        st = T.step_losses(el, xh, pp, x, 0.06)
        st[1].backward()

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        step()
        b.record()
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    return {"median_ms": statistics.median(ms), "mean_ms": statistics.fmean(ms), "min_ms": min(ms)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--batches", type=int, nargs="+", default=[32, 4096])
    p.add_argument("--steps", type=int, default=50)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--quantizers", nargs="+", default=list(QUANTIZERS), choices=list(QUANTIZERS))
    args = p.parse_args()
    dev = torch.device("cuda:0")
    conv.set_conv_backend("hip")
    summary = {}
    for B in args.batches:
        for q in args.quantizers:
            r = time_step(QUANTIZERS[q], B, args.steps, args.warmup, dev)
            summary[f"{q}@B{B}"] = round(r["median_ms"], 4)
            print(json.dumps({"quantizer": q, "batch": B, **{k: round(v, 4) for k, v in r.items()}}), flush=True)
    print(json.dumps({"step_median_ms": summary, "device": torch.cuda.get_device_name(dev)}), flush=True)


if __name__ == "__main__":
    main()
