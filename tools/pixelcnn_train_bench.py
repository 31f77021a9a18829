#!/usr/bin/env python3
"""GatedPixelCNN(512, 64, 15, 10) training step on 8 x 8 maps (pixelcnn/gated_pixelcnn.py:78-99: forward, cross-entropy, backward,
Adam) on the HIP kernels, next to the same module's ops issued through torch autograd (MIOpen / rocBLAS) on the same GPU, the two
alternated; then the HIP step captured into a hipGraph and replayed (its gradients checked against the eager step's bits).

    python tools/pixelcnn_train_bench.py [--batches 32,1024] [--steps 20] [--repeats 3] [--json OUT] [--adam torch|hip]
        --adam hip: the HIP step's optimizer is vqvae_amd.optim.Adam (csrc/optim.hip), eager and captured; torch (the default):
        torch.optim.Adam, capturable=True inside the graph
    python tools/pixelcnn_train_bench.py --profile-steps N --batches 1024      # HIP steps only, for a rocprofv3 --kernel-trace --stats run
    python tools/pixelcnn_train_bench.py --report-stats run_results.db --batches 1024 --profile-steps N
        -> the per-kernel split per step, and the taps weight-gradient kernel's share of the fp32 MFMA peak (FLOPs from the shapes)
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F

K, DIM, NL, NCLS, HW = 512, 64, 15, 10, 8
FP32_MFMA_PEAK_TF = 157.3          # MI355X, v_mfma_f32_32x32x2_f32 (MI355X_MICROARCH.md)


def taps_wgrad_flops_per_step(B):
    """2 B H W Cout Cin ntaps over every masked conv: layer 0 (4 x 7 vertical, 1 x 4 horizontal), 14 mask-'B' layers (2 x 3, 1 x 2)"""
    taps = (28 + 4) + (NL - 1) * (6 + 2)
    return 2.0 * B * HW * HW * (2 * DIM) * DIM * taps


def torch_forward(m, x, label):                                   # pixelcnn/models.py:64-84, 118-127 with torch ops
    with torch.no_grad():
        m.layers[0].vert_stack.weight[:, :, -1].zero_()
        m.layers[0].horiz_stack.weight[:, :, :, -1].zero_()
    t = m.embedding(x.view(-1)).view(x.size() + (-1,)).permute(0, 3, 1, 2)
    xv, xh = t, t
    for L in m.layers:
        h = L.class_cond_embedding(label)
        hv = L.vert_stack(xv)[:, :, :xv.size(-1), :]
        a, b = (hv + h[:, :, None, None]).chunk(2, dim=1)
        ov = torch.tanh(a) * torch.sigmoid(b)
        hh = L.horiz_stack(xh)[:, :, :, :xh.size(-2)]
        a, b = (L.vert_to_horiz(hv) + hh + h[:, :, None, None]).chunk(2, dim=1)
        o = L.horiz_resid(torch.tanh(a) * torch.sigmoid(b))
        xv, xh = ov, (o + xh if L.residual else o)
    return m.output_conv(xh)


def hip_step(m, opt, x, label):
    from vqvae_amd.pixelcnn import cross_entropy
    loss = cross_entropy(m(x, label), x)
    opt.zero_grad(set_to_none=False)
    loss.backward()
    opt.step()
    return loss


def torch_step(m, opt, x, label):
    logits = torch_forward(m, x, label).permute(0, 2, 3, 1).contiguous()
    loss = F.cross_entropy(logits.view(-1, K), x.view(-1))
    opt.zero_grad(set_to_none=False)
    loss.backward()
    opt.step()
    return loss


def timed(f, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def make_adam(params, which, capturable=False):
    if which == "hip":
        from vqvae_amd import optim as hip_optim
        return hip_optim.Adam(params, lr=3e-4)                 # (captures as it is: its counters live on the device)
    return torch.optim.Adam(params, lr=3e-4, capturable=True) if capturable else torch.optim.Adam(params, lr=3e-4)


def graph_step(m, x, label, steps, adam="torch"):
    """capture forward + loss + backward + Adam (torch's: capturable) into one graph; replay; check the replayed gradients against
    an eager backward at the same parameters"""
    from vqvae_amd.pixelcnn import cross_entropy
    opt = make_adam(m.parameters(), adam, capturable=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            hip_step(m, opt, x, label)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    opt.zero_grad(set_to_none=False)
    with torch.cuda.graph(g, stream=s):
        static_loss = hip_step(m, opt, x, label)
    params = list(m.parameters())
    p0 = [p.detach().clone() for p in params]
    g.replay()
    torch.cuda.synchronize()
    g_graph = [p.grad.detach().clone() for p in params]
    with torch.no_grad():                       # back to the parameters the replay started from (bumps the versions: re-pack)
        for p, q in zip(params, p0):
            p.copy_(q)
    loss = cross_entropy(m(x, label), x)
    g_eager = torch.autograd.grad(loss, params)
    same = all(torch.equal(a, b) for a, b in zip(g_graph, g_eager))
    ms = timed(g.replay, steps)
    return ms, same, float(static_loss)


def report(db_path, B, steps, top=16):
    """per-kernel split of a `rocprofv3 --kernel-trace` run of --profile-steps (its results database), and the taps
    weight-gradient kernel's rate against the fp32 MFMA peak, its FLOPs counted from the shapes"""
    import sqlite3
    db = sqlite3.connect(db_path)
    per = {}
    for name, dur, calls in db.execute("select name, sum(duration), count(*) from kernels group by name"):
        per[name] = (dur / 1e6 / steps, calls / steps)
    total = sum(v[0] for v in per.values())
    print(f"B={B}: kernel time {total:.3f} ms per step, {sum(v[1] for v in per.values()):.0f} launches per step")
    for name, (ms, calls) in sorted(per.items(), key=lambda kv: -kv[1][0])[:top]:
        print(f"  {ms:8.3f} ms  {100 * ms / total:5.1f} %  {calls:6.1f} calls  {name[:100]}")
    ms = sum(v[0] for n, v in per.items() if "taps_wgrad_map_kernel" in n or "taps_wgrad_blk_kernel" in n)
    tf = taps_wgrad_flops_per_step(B) / (ms * 1e-3) / 1e12
    print(f"  taps weight gradient: {ms:.3f} ms per step, {taps_wgrad_flops_per_step(B) / 1e9:.1f} GFLOP -> {tf:.1f} TF/s = "
          f"{100 * tf / FP32_MFMA_PEAK_TF:.1f} % of the fp32 MFMA peak ({FP32_MFMA_PEAK_TF} TF/s)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="32,1024")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--profile-steps", type=int, default=0)
    ap.add_argument("--report-stats", default=None)
    ap.add_argument("--json", default=None)
    ap.add_argument("--adam", choices=["torch", "hip"], default="torch")
    a = ap.parse_args()
    batches = [int(b) for b in a.batches.split(",")]

    if a.report_stats:
        report(a.report_stats, batches[0], a.profile_steps)
        return

    from vqvae_amd.pixelcnn import GatedPixelCNN
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    base = GatedPixelCNN(K, DIM, NL, NCLS)
    if a.profile_steps:
        m = copy.deepcopy(base).to(dev).train()
        opt = make_adam(m.parameters(), a.adam)
        x = torch.randint(0, K, (batches[0], HW, HW), device=dev)
        label = torch.randint(0, NCLS, (batches[0],), device=dev)
        for _ in range(a.profile_steps):
            hip_step(m, opt, x, label)
        torch.cuda.synchronize()
        print(f"profiled {a.profile_steps} HIP steps at B={batches[0]}")
        return

    out = {"workload": "GatedPixelCNN(512, 64, 15, 10) train step, 8x8", "results": []}
    for B in batches:
        g = torch.Generator().manual_seed(B)
        x = torch.randint(0, K, (B, HW, HW), generator=g).to(dev)
        label = torch.randint(0, NCLS, (B,), generator=g).to(dev)
        mh, mt = copy.deepcopy(base).to(dev).train(), copy.deepcopy(base).to(dev).train()
        oh, ot = make_adam(mh.parameters(), a.adam), torch.optim.Adam(mt.parameters(), lr=3e-4)
        for _ in range(a.warmup):
            hip_step(mh, oh, x, label)
            torch_step(mt, ot, x, label)
        th, tt = [], []
        for _ in range(a.repeats):
            th.append(timed(lambda: hip_step(mh, oh, x, label), a.steps))
            tt.append(timed(lambda: torch_step(mt, ot, x, label), a.steps))
        tg, same, _ = graph_step(copy.deepcopy(base).to(dev).train(), x, label, a.steps, a.adam)
        r = {"B": B, "adam": a.adam, "hip_ms": statistics.median(th), "torch_ms": statistics.median(tt), "hip_graph_ms": tg,
             "graph_grads_equal_eager": same, "hip_ms_all": th, "torch_ms_all": tt}
        out["results"].append(r)
        print(f"train step B={B:5d} adam={a.adam}: HIP {r['hip_ms']:8.2f} ms   torch autograd {r['torch_ms']:8.2f} ms   "
              f"HIP hipGraph {tg:8.2f} ms   (graph grads == eager: {same})", flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(out, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
