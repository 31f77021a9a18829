#!/usr/bin/env python3
"""Sampling from the GatedPixelCNN prior (pixelcnn/models.py:129-142): GatedPixelCNN.generate (one full forward per position, eager
and replayed from a hipGraph) against GatedPixelCNN.generate_cached (csrc/pixelcnn_sample.hip), device-synchronised wall time per
call after warm-up, the median of --repeats.

    python tools/pixelcnn_sample_bench.py [--json OUT]                # 8x8, K 512, dim 64, 15 layers at B 64 / 100 / 1024 (both),
                                                                      # generate_cached alone on 28x28 (K 256) and 64x64 (K 512)
    python tools/pixelcnn_sample_bench.py --profile B,side,K          # generate_cached only, 3 calls: for rocprofv3 --kernel-trace --stats
    python tools/pixelcnn_sample_bench.py --top_k 50 --top_p 0.9      # the generate_cached column with sampling controls:
                                                                      # --temperature T, --top_k k, --top_p p, --given_rows r (the top
                                                                      # r rows of every map are given codes, the rest is drawn)
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

DIM, NL, NCLS = 64, 15, 10


def model(K):
    from vqvae_amd.pixelcnn import GatedPixelCNN
    torch.manual_seed(0)
    return GatedPixelCNN(K, DIM, NL, NCLS).eval().cuda()


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), ts


def sampler_kw(a, B, side, K):
    """generate_cached's sampling controls from the command line; --given_rows fixes the top rows of every map to random codes"""
    kw = {}
    if a.temperature != 1.0:
        kw["temperature"] = a.temperature
    if a.top_k:
        kw["top_k"] = a.top_k
    if a.top_p < 1.0:
        kw["top_p"] = a.top_p
    if a.given_rows > 0:
        given = torch.randint(0, K, (B, side, side), generator=torch.Generator().manual_seed(B + side)).cuda()
        given[:, min(a.given_rows, side):] = -1
        kw["given"] = given
    if a.return_logits:
        kw["return_logits"] = True
    return kw


def macs_per_image(K, side):
    """multiply-adds the recurrence needs per image: per pixel the vertical stacks and vert_to_horiz of every layer, the
    horizontal stacks, horiz_resid and the head"""
    d = DIM
    vert = (21 + 6 * (NL - 1)) * d * 2 * d + NL * 4 * d * d
    horiz = (3 + 2 * (NL - 1)) * d * 2 * d + NL * d * d
    head = d * 512 + 512 * K
    return side * side * (vert + horiz + head)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--profile", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--top_k", type=int, default=0)
    ap.add_argument("--top_p", type=float, default=1.0)
    ap.add_argument("--given_rows", type=int, default=0)
    ap.add_argument("--return_logits", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: a CPU timing says nothing about the MI355X"
    if a.profile:
        B, side, K = (int(v) for v in a.profile.split(","))
        m = model(K)
        lab = torch.zeros(B, dtype=torch.int64, device="cuda")
        kw = sampler_kw(a, B, side, K)
        for _ in range(3):
            m.generate_cached(lab, (side, side), B, **kw)
        torch.cuda.synchronize()
        return
    rows = []

    def row(kind, B, side, K, fn, repeats):
        ms, ts = timed(fn, a.warmup if repeats > 1 else 1, repeats)
        r = {"method": kind, "B": B, "side": side, "K": K, "ms": round(ms, 3), "all_ms": [round(t, 3) for t in ts],
             "maps_per_s": round(B / ms * 1e3, 1)}
        if kind == "generate_cached":
            r["gmac_per_s"] = round(B * macs_per_image(K, side) / ms / 1e6, 1)
        rows.append(r)
        print(json.dumps(r), flush=True)

    m512 = model(512)
    for B in (64, 100, 1024):
        lab = torch.arange(B, device="cuda") % NCLS
        kw = sampler_kw(a, B, 8, 512)
        row("generate_cached", B, 8, 512, lambda: m512.generate_cached(lab, (8, 8), B, **kw), a.repeats)
        reps = a.repeats if B < 1024 else 2
        row("generate_graph", B, 8, 512, lambda: m512.generate(lab, (8, 8), B, use_graph=True), reps)
        row("generate_eager", B, 8, 512, lambda: m512.generate(lab, (8, 8), B), reps)
    m256 = model(256)
    for B in (1, 64):
        lab = torch.arange(B, device="cuda") % NCLS
        kw = sampler_kw(a, B, 28, 256)
        row("generate_cached", B, 28, 256, lambda: m256.generate_cached(lab, (28, 28), B, **kw), 3)
    for B in (1, 64):
        lab = torch.arange(B, device="cuda") % NCLS
        kw = sampler_kw(a, B, 64, 512)
        row("generate_cached", B, 64, 512, lambda: m512.generate_cached(lab, (64, 64), B, **kw), 1)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(rows, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
