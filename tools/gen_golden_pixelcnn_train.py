#!/usr/bin/env python3
"""Training goldens of the GatedPixelCNN prior: run the REAL reference module (pixelcnn/models.py, imported unmodified from the
reference tree given as the first argument; CPU, fp32) on the seeded cases of tests/golden/pixelcnn_cases.npz (same seed, same
inputs, same bias perturbation as oracle/gen_golden_pixelcnn.py) and record tests/golden/pixelcnn_train_cases.npz:

  <case>/loss          nn.CrossEntropyLoss of gated_pixelcnn.py:91-96 on the case's inputs
  <case>/grad_logits   its gradient w.r.t. the (B, K, H, W) logits
  <case>/grad/<param>  parameter gradients (every one of k64_dim32_l3; a subset of k512_dim64_l15, tests/pixelcnn_train_ref.py)
                       tensors of more than 1024 elements as 1024 seeded positions (tests/pixelcnn_train_ref.py::store) -- plus
                       512 mask-'A' taps of each of layers.0's stacks and four absent codes' embedding rows -- and the whole
                       tensor's maximum magnitude
  <case>/traj_loss     the losses of 3 steps of the reference's train() body (gated_pixelcnn.py:78-99: Adam, lr 3e-4)
  k64_dim32_l3/final/<param>   the parameters after those 3 steps

    python tools/gen_golden_pixelcnn_train.py /path/to/reference
"""
import os
import sys

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.pixelcnn_train_ref import (CASES, grad_keys, inputs, mask_a_positions, perturb_biases, store,  # noqa: E402
                                      train_batches)

LR = 3e-4


def build(GatedPixelCNN, name):
    K, dim, nl, ncls, B, H, W = CASES[name]
    torch.manual_seed(0)
    m = GatedPixelCNN(K, dim, nl, ncls)
    perturb_biases(m)
    return m


def main(ref_root):
    sys.path.insert(0, ref_root)
    sys.dont_write_bytecode = True
    from pixelcnn.models import GatedPixelCNN
    torch.set_num_threads(1)
    out = {}
    for name, (K, dim, nl, ncls, B, H, W) in CASES.items():
        m = build(GatedPixelCNN, name)
        x, label = inputs(name)
        logits = m(x, label)
        logits.retain_grad()
        loss = nn.CrossEntropyLoss()(logits.permute(0, 2, 3, 1).contiguous().view(-1, K), x.view(-1))
        loss.backward()
        out[f"{name}/loss"] = np.float32(loss.item())
        store(out, f"{name}/grad_logits", logits.grad.numpy())
        grads = {n_: p.grad for n_, p in m.named_parameters()}
        absent = np.setdiff1d(np.arange(K), x.numpy().ravel())[:4]
        for k in grad_keys(name, grads):
            must = None
            if k == "layers.0.vert_stack.weight" or k == "layers.0.horiz_stack.weight":
                pos = mask_a_positions(grads[k].shape, k.endswith("vert_stack.weight"))
                must = pos[np.random.default_rng(len(k)).choice(pos.size, min(512, pos.size), replace=False)]
            elif k == "embedding.weight":
                must = (absent[:, None] * dim + np.arange(dim)[None, :]).ravel()
            store(out, f"{name}/grad/{k}", grads[k].numpy(), must)

        # the reference's train() body, verbatim in its model / criterion / optimizer calls
        m = build(GatedPixelCNN, name)
        criterion = nn.CrossEntropyLoss()
        opt = torch.optim.Adam(m.parameters(), lr=LR)
        traj = []
        for xb, lb in train_batches(name):
            logits = m(xb, lb)
            logits = logits.permute(0, 2, 3, 1).contiguous()
            loss = criterion(logits.view(-1, K), xb.view(-1))
            opt.zero_grad()
            loss.backward()
            opt.step()
            traj.append(loss.item())
        out[f"{name}/traj_loss"] = np.array(traj, dtype=np.float64)
        if name == "k64_dim32_l3":
            for n_, p in m.named_parameters():
                store(out, f"{name}/final/{n_}", p.detach().numpy())
    path = os.path.join(ROOT, "tests", "golden", "pixelcnn_train_cases.npz")
    np.savez_compressed(path, **out)
    print("wrote", len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("VQVAE_REFERENCE", "/root/reference"))
