#!/usr/bin/env python3
"""Train a real checkpoint with the HIP training path  --  the loop of main.py:67-98 (Adam amsgrad lr 3e-4, model.train(),
recon / x_train_var + embedding loss, a random batch per update) on structured synthetic 32x32x3 images (tests/synthdata.py;
no dataset can be fetched here).  Every forward and backward runs on libvqvae_hip.so (vqvae_amd/autograd_conv.py,
training.VQStraightThrough, training.step_losses); the optimizer is torch's, as in the reference, unless --hip_adam asks for
vqvae_amd.optim.Adam (csrc/optim.hip: a written-down operation order, so the run no longer depends on which Adam torch picks).

    python tools/train_checkpoint.py [--n_updates 5000] [--batch_size 32] [--out gpurun_out/trained]
                                     [--ema_decay 0.99 [--restart_threshold 1]]     (the EMA codebook; off by default)
                                     [--hip_adam]                                   (off by default: the committed checkpoints are torch's)
                                     [--kmeans_init [BATCHES]]                      (off by default: k-means start of the codebook)
                                     [--n_quantizers Q [--shared_codebook]]         (off by default: residual quantization, Q stages)
                                     [--rotation_trick]                             (off by default: the rotation-trick gradient)
                                     [--cosine_sim]                                 (off by default: the cosine-similarity codebook)
                                     [--fsq_levels 8,5,5,5 --n_embeddings 1000]     (off by default: finite scalar quantization)
                                     [--codebook_dim 8]                             (off by default: factorized codes)
                                     [--orthogonal_reg_weight W [--orthogonal_reg_active_codes_only] [--orthogonal_reg_max_codes M]]
                                                                                    (off by default: orthogonal regularization of the codebook)
                                     [--entropy_weight W [--entropy_diversity_gamma G --entropy_inv_temperature S]]
                                                                                    (off by default: the code-entropy loss of the codebook)
                                     [--lookup_free --n_embeddings 1024 [--lfq_entropy_weight 0.1 --lfq_diversity_gamma 1 --lfq_inv_temperature 100]]
                                                                                    (off by default: lookup-free quantization)
                                     [--codebook_groups G]                          (off by default: grouped quantization, G codebooks)

Writes <out>/<tag>.pth in the reference's checkpoint layout (utils.py:109-113: {'model', 'results', 'hyperparameters'}),
<out>/<tag>_log.txt (the reference's log line every --log_interval updates + the range guard's per-layer spreads along the way;
committed as profiles/r06_train_*_log.txt) and <out>/<tag>_state.npz (the 23 state_dict tensors, fp32: what tests/golden/ keeps as
trained_main_defaults_state.npz [defaults] and trained_b128x20k_state.npz [--batch_size 128 --n_updates 20000]).
"""
from __future__ import annotations

import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from tests import synthdata
from vqvae_amd import conv, training as T
from vqvae_amd.modules import GroupedVectorQuantizer, LookupFreeQuantizer, VQVAE


def parse(argv=None):
    """-> (args, the keyword options of VQVAE that were given: every opt-in option is absent from both unless named)"""
    p = argparse.ArgumentParser()
    p.add_argument("--batch_size", type=int, default=32)           # main.py:17-27's defaults
    p.add_argument("--n_updates", type=int, default=5000)
    p.add_argument("--n_hiddens", type=int, default=128)
    p.add_argument("--n_residual_hiddens", type=int, default=32)
    p.add_argument("--n_residual_layers", type=int, default=2)
    p.add_argument("--embedding_dim", type=int, default=64)
    p.add_argument("--n_embeddings", type=int, default=512)
    p.add_argument("--beta", type=float, default=.25)
    p.add_argument("--learning_rate", type=float, default=3e-4)
    p.add_argument("--log_interval", type=int, default=250)
    p.add_argument("--n_train", type=int, default=50000)            # CIFAR-10's training set size
    p.add_argument("--data_seed", type=int, default=2026)
    p.add_argument("--out", default="gpurun_out/trained")
    p.add_argument("--tag", default="vqvae_trained")
    # opt-in EMA codebook (VectorQuantizerEMA); absent from the namespace unless given, so a default run writes what it always did
    p.add_argument("--ema_decay", type=float, default=argparse.SUPPRESS)
    p.add_argument("--restart_threshold", type=float, default=argparse.SUPPRESS)
    p.add_argument("--hip_adam", action="store_true", default=argparse.SUPPRESS)        # (absent unless given, like the EMA options)
    # opt-in k-means start of the codebook (VQVAE.init_codebook_) on the first BATCHES batches, before update 0
    p.add_argument("--kmeans_init", type=int, nargs="?", const=1, default=argparse.SUPPRESS, metavar="BATCHES")
    p.add_argument("--kmeans_iters", type=int, default=argparse.SUPPRESS)
    # opt-in residual quantization (ResidualVectorQuantizer); absent unless given, like the EMA options
    p.add_argument("--n_quantizers", type=int, default=argparse.SUPPRESS)
    p.add_argument("--shared_codebook", action="store_true", default=argparse.SUPPRESS)
    # opt-in rotation-trick gradient through the quantizer (rotation_trick=True); absent unless given, like the EMA options
    p.add_argument("--rotation_trick", action="store_true", default=argparse.SUPPRESS)
    # opt-in cosine-similarity codebook (cosine_sim=True: l2-normalised rows and codes); absent unless given, like the EMA options
    p.add_argument("--cosine_sim", action="store_true", default=argparse.SUPPRESS)
    # opt-in finite scalar quantization (fsq_levels=(8, 5, 5, 5): no codebook; --n_embeddings must be the levels' product); absent unless given
    p.add_argument("--fsq_levels", type=lambda v: tuple(int(l) for l in v.split(",")), default=argparse.SUPPRESS, metavar="L0,L1,..")
    # opt-in grouped (product) quantization (codebook_groups=G: G codebooks of embedding_dim / G channels); absent unless given
    p.add_argument("--codebook_groups", type=int, default=argparse.SUPPRESS, metavar="G")
    # opt-in lookup-free quantization (lookup_free=True: the codebook is {-1, +1}^log2(n_embeddings); --beta weighs its commitment term);
    # absent unless given
    p.add_argument("--lookup_free", action="store_true", default=argparse.SUPPRESS)
    p.add_argument("--lfq_entropy_weight", type=float, default=argparse.SUPPRESS)
    p.add_argument("--lfq_diversity_gamma", type=float, default=argparse.SUPPRESS)
    p.add_argument("--lfq_inv_temperature", type=float, default=argparse.SUPPRESS)
    # opt-in factorized codes (codebook_dim=d: the codebook is searched in d channels between two projections); absent unless given
    p.add_argument("--codebook_dim", type=int, default=argparse.SUPPRESS, metavar="d")
    # opt-in orthogonal regularization loss of the codebook (orthogonal_reg_weight=W; csrc/vq_orthogonal.hip); absent unless given
    p.add_argument("--orthogonal_reg_weight", type=float, default=argparse.SUPPRESS, metavar="W")
    p.add_argument("--orthogonal_reg_active_codes_only", action="store_true", default=argparse.SUPPRESS)
    p.add_argument("--orthogonal_reg_max_codes", type=int, default=argparse.SUPPRESS, metavar="M")
    # opt-in code-entropy loss of the learned codebook (entropy_weight=W; csrc/vq_entropy.hip); absent unless given
    p.add_argument("--entropy_weight", type=float, default=argparse.SUPPRESS, metavar="W")
    p.add_argument("--entropy_diversity_gamma", type=float, default=argparse.SUPPRESS, metavar="G")
    p.add_argument("--entropy_inv_temperature", type=float, default=argparse.SUPPRESS, metavar="S")
    # opt-in merged EMA statistics (ema_accumulate=A: the codebook moves once per A forwards; ema_sync: merged across the process
    # group's ranks; csrc/vq_ema_merge.hip); absent unless given
    p.add_argument("--ema_accumulate", type=int, default=argparse.SUPPRESS, metavar="A")
    p.add_argument("--ema_sync", action="store_true", default=argparse.SUPPRESS)
    args = p.parse_args(argv)
    ema_kw = {}
    for name in ("ema_accumulate", "ema_sync"):
        if hasattr(args, name):
            ema_kw[name] = getattr(args, name)
    for name in ("entropy_weight", "entropy_diversity_gamma", "entropy_inv_temperature"):
        if hasattr(args, name):
            ema_kw[name] = getattr(args, name)
    for name in ("orthogonal_reg_weight", "orthogonal_reg_active_codes_only", "orthogonal_reg_max_codes"):
        if hasattr(args, name):
            ema_kw[name] = getattr(args, name)
    if hasattr(args, "lookup_free"):
        ema_kw["lookup_free"] = True
    for name in ("lfq_entropy_weight", "lfq_diversity_gamma", "lfq_inv_temperature"):
        if hasattr(args, name):
            ema_kw[name] = getattr(args, name)
    if hasattr(args, "codebook_dim"):
        ema_kw["codebook_dim"] = args.codebook_dim
    if hasattr(args, "codebook_groups"):
        ema_kw["codebook_groups"] = args.codebook_groups
    if hasattr(args, "fsq_levels"):
        ema_kw["fsq_levels"] = args.fsq_levels
    if hasattr(args, "cosine_sim"):
        ema_kw["cosine_sim"] = True
    if hasattr(args, "rotation_trick"):
        ema_kw["rotation_trick"] = True
    if hasattr(args, "n_quantizers"):
        ema_kw["n_quantizers"] = args.n_quantizers
    if hasattr(args, "shared_codebook"):
        ema_kw["shared_codebook"] = True
    if hasattr(args, "ema_decay"):
        ema_kw["ema_decay"] = args.ema_decay
    if hasattr(args, "restart_threshold"):
        ema_kw["restart_threshold"] = args.restart_threshold
    return args, ema_kw


def main(argv=None):
    args, ema_kw = parse(argv)
    dev = torch.device("cuda:0")
    conv.set_conv_backend("hip")
    os.makedirs(args.out, exist_ok=True)
    log = open(os.path.join(args.out, f"{args.tag}_log.txt"), "w")

    def say(*a):
        s = " ".join(str(v) for v in a)
        print(s, flush=True)
        log.write(s + "\n")
        log.flush()

    t0 = time.time()
    x01 = synthdata.images01(args.n_train, args.data_seed)
    x_train_var = synthdata.train_var(x01)                          # utils.py:86
    data = ((x01 - 0.5) / 0.5).to(dev)                              # utils.py:15-16
    say(f"# data: {args.n_train} structured synthetic images (tests/synthdata.py seed {args.data_seed}), x_train_var={x_train_var:.6f}, "
        f"{time.time() - t0:.1f} s")
    say(f"# hyperparameters: {vars(args)}")

    torch.manual_seed(0)
    model = VQVAE(args.n_hiddens, args.n_residual_hiddens, args.n_residual_layers, args.n_embeddings, args.embedding_dim,
                  args.beta, **ema_kw).to(dev)
    if getattr(args, "hip_adam", False):
        from vqvae_amd import optim as hip_optim
        opt = hip_optim.Adam(model.parameters(), lr=args.learning_rate, amsgrad=True)
    else:
        opt = torch.optim.Adam(model.parameters(), lr=args.learning_rate, amsgrad=True)   # main.py:59
    model.train()
    # grouped models run layer by layer: the range guard and the product schemes belong to the fused whole-path entries they do not use
    # (and so do lookup-free models)
    whole_path = not isinstance(model.vector_quantization, (GroupedVectorQuantizer, LookupFreeQuantizer))
    results = {"n_updates": 0, "recon_errors": [], "loss_vals": [], "perplexities": []}
    if getattr(args, "kmeans_init", 0) > 0:
        # the batches the loop below is about to draw (the same generator seed; the loop's own generator starts afresh)
        gi = torch.Generator().manual_seed(1)
        sel = torch.cat([torch.randint(0, args.n_train, (args.batch_size,), generator=gi) for _ in range(args.kmeans_init)])
        init = model.init_codebook_(data[sel.to(dev)].contiguous(), iters=getattr(args, "kmeans_iters", 10),
                                    generator=torch.Generator(device=dev).manual_seed(2))
        counts = init[0][1] if isinstance(init, list) else init[1]              # (residual stages: stage 0's counts)
        say(f"# k-means init on {sel.numel()} images ({args.kmeans_init} batches): codes with rows {int((counts > 0).sum())} / "
            f"{args.n_embeddings}, largest cluster {int(counts.max())} rows")
    g = torch.Generator().manual_seed(1)
    stats_dev = []
    t0 = time.time()
    for i in range(args.n_updates):
        sel = torch.randint(0, args.n_train, (args.batch_size,), generator=g).to(dev)     # a shuffled loader's first batch
        x = data[sel].contiguous()
        opt.zero_grad()
        embedding_loss, x_hat, perplexity = model(x)
        stats = T.step_losses(embedding_loss, x_hat, perplexity, x, x_train_var)          # [recon_loss, loss, perplexity]
        stats[1].backward()                                                               # main.py:78
        opt.step()
        stats_dev.append(stats.detach())
        if i % args.log_interval == 0 or i == args.n_updates - 1:
            block = torch.stack(stats_dev).cpu().numpy()
            stats_dev = []
            results["recon_errors"] += block[:, 0].tolist()
            results["loss_vals"] += block[:, 1].tolist()
            results["perplexities"] += block[:, 2].tolist()
            results["n_updates"] = i
            guard = "per-layer path"
            if whole_path:
                model.eval()
                with torch.no_grad():
                    rec, spreads = model.scheme_hint()
                model.train()
                guard = f"flags={rec:#x} max spread {max(spreads):.2f} binades"
            say(f"Update # {i} Recon Error: {block[:, 0].mean():.5f} Loss {block[:, 1].mean():.5f} Perplexity: {block[:, 2].mean():.3f}"
                f"   | guard: {guard}   [{time.time() - t0:.1f} s]")
    torch.cuda.synchronize()
    say(f"# {args.n_updates} updates in {time.time() - t0:.1f} s")

    model.eval()
    if whole_path:
        rec, spreads = model.scheme_hint()
        say(f"# final guard: flags={rec:#x}; per-layer input-channel spreads (binades): {[round(s, 2) for s in spreads]}")
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    torch.save({"model": sd, "results": results, "hyperparameters": vars(args)}, os.path.join(args.out, f"{args.tag}.pth"))
    np.savez_compressed(os.path.join(args.out, f"{args.tag}_state.npz"), **{k: v.numpy() for k, v in sd.items()})

    # a first look at the checkpoint through the product path: validation images, all three product schemes
    from vqvae_amd import functional as F_hip
    xv = synthdata.normalised(4096, args.data_seed + 1).to(dev)
    if not whole_path:
        # the per-layer path: the eval forward, and the index wire format back through the decoder (the same x_hat, bit for bit)
        with torch.no_grad():
            loss, x_hat, ppl = model(xv)
            idx = model.encode(xv)
            same = torch.equal(model.decode_indices(idx, xv.shape[0], xv.shape[2] // 4, xv.shape[3] // 4), x_hat)
        say(f"# eval[per-layer]: embedding_loss={loss.item():.6g} mean perplexity={ppl.item():.4f} distinct codes per group="
            f"{[g.unique().numel() for g in (idx if isinstance(model.vector_quantization, GroupedVectorQuantizer) else [idx])]} recon mse/var={((x_hat - xv) ** 2).mean().item() / x_train_var:.5f} "
            f"decode_indices(encode(x)) is x_hat: {same}")
        log.close()
        return
    with torch.no_grad():
        out = {}
        for name, fl in (("guard", None), ("fp16x2", 0), ("bf16x3", F_hip.FWD_CONV_BF16_SPLIT), ("fp32", F_hip.FWD_CONV_EXACT_FP32)):
            loss, x_hat, ppl, idx = model._forward_c(xv, want_idx=True, fwd_flags=fl)
            out[name] = (loss.item(), ppl.item(), idx.cpu(), x_hat.cpu())
            say(f"# eval[{name}]: embedding_loss={loss.item():.6g} perplexity={ppl.item():.4f} distinct codes={idx.unique().numel()} "
                f"recon mse/var={((x_hat - xv) ** 2).mean().item() / x_train_var:.5f}")
        for name in ("fp16x2", "bf16x3"):
            say(f"# index flips {name} vs fp32 scheme: {(out[name][2] != out['fp32'][2]).sum().item()} / {out['fp32'][2].numel()}; "
                f"max|x_hat diff| {(out[name][3] - out['fp32'][3]).abs().max().item():.3g}")
    log.close()


if __name__ == "__main__":
    main()
