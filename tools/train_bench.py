#!/usr/bin/env python3
"""Training-step time (forward + loss + backward, no optimizer) of main.py:74-78: convs on the HIP kernels vs
torch's conv autograd (MIOpen), the quantizer on the HIP forward/backward either way.
    train_bench.py [B] [backends] [steps] [adam|hipadam|-] [rotation] [cosine] [fsq] [groups] [lfq] [factorized] [orth] [entropy] [ema] [ema_accumulate]
                                                     ema: VQVAE(..., ema_decay=0.99), the EMA codebook (one update per forward);
                                                     ema_accumulate: + ema_accumulate=2, the codebook moves once per two forwards from
                                                     their merged statistics (csrc/vq_ema_merge.hip); absent: the model as it always was
                                                     entropy: VQVAE(..., entropy_weight=0.1), the code-entropy loss of the codebook joins the training
                                                     loss (csrc/vq_entropy.hip); absent: the model as it always was
                                                     orth: VQVAE(..., orthogonal_reg_weight=10.0), the orthogonal regularization loss of
                                                     the codebook joins the training loss (csrc/vq_orthogonal.hip); absent: the model as it always was
                                                     factorized: VQVAE(..., codebook_dim=8), the codebook searched in 8 channels between
                                                     two projections (csrc/vq_linear.hip); absent: the model as it always was
                                                     lfq: VQVAE(128, 32, 2, 1024, 64, 0.25, lookup_free=True), lookup-free quantization
                                                     with its entropy loss (csrc/vq_lfq.hip); absent: the model as it always was
                                                     groups: VQVAE(..., codebook_groups=4), grouped (product) quantization: four
                                                     codebooks of 16 channels (csrc/vq_grouped.hip); absent: the model as it always was
                                                     fsq: VQVAE(128, 32, 2, 1000, 64, 0.25, fsq_levels=(8, 5, 5, 5)), finite scalar
                                                     quantization in place of the codebook (csrc/vq_fsq.hip); absent: the model as it always was
                                                     cosine: VQVAE(..., cosine_sim=True), l2-normalised rows and codes in front of
                                                     the quantizer (csrc/vq_cosine.hip); absent: the model as it always was
                                                     rotation: VQVAE(..., rotation_trick=True), the rotation-trick gradient through
                                                     the quantizer (csrc/vq_rotation.hip); absent: the model as it always was
                                                     adam: + main.py:59,80 (optim.Adam(amsgrad=True).step(); every
                                                     layer's weights are packed again each step); hipadam: the same step on
                                                     vqvae_amd.optim.Adam (csrc/optim.hip)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from vqvae_amd import conv, training as T, _lib
from vqvae_amd.modules import VQVAE

dev = torch.device("cuda:0")
B = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
torch.manual_seed(0)
rotation = "rotation" in sys.argv[4:]
cosine = "cosine" in sys.argv[4:]
fsq = "fsq" in sys.argv[4:]
groups = "groups" in sys.argv[4:]
lfq = "lfq" in sys.argv[4:]
factorized = "factorized" in sys.argv[4:]
orth = "orth" in sys.argv[4:]
entropy = "entropy" in sys.argv[4:]
ema_acc = "ema_accumulate" in sys.argv[4:]
ema = ema_acc or "ema" in sys.argv[4:]
opts = {**({"rotation_trick": True} if rotation else {}), **({"cosine_sim": True} if cosine else {}),
        **({"fsq_levels": (8, 5, 5, 5)} if fsq else {}), **({"codebook_groups": 4} if groups else {}),
        **({"lookup_free": True} if lfq else {}), **({"codebook_dim": 8} if factorized else {}),
        **({"orthogonal_reg_weight": 10.0} if orth else {}), **({"entropy_weight": 0.1} if entropy else {}),
        **({"ema_decay": 0.99} if ema else {}), **({"ema_accumulate": 2} if ema_acc else {})}
model = VQVAE(128, 32, 2, 1000 if fsq else (1024 if lfq else 512), 64, 0.25, **opts).to(dev).train()
x = torch.randn(B, 3, 32, 32, device=dev)
backends = sys.argv[2].split(",") if len(sys.argv) > 2 else ["hip", "torch"]
nsteps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
which_adam = sys.argv[4] if len(sys.argv) > 4 and sys.argv[4] in ("adam", "hipadam") else None
with_adam = which_adam is not None
if which_adam == "hipadam":
    from vqvae_amd import optim as hip_optim
    opt = hip_optim.Adam(model.parameters(), lr=3e-4, amsgrad=True)
else:
    opt = torch.optim.Adam(model.parameters(), lr=3e-4, amsgrad=True) if with_adam else None
for backend in backends:
    conv.set_conv_backend(backend)

    def step():
        model.zero_grad(set_to_none=True)
        el, xh, pp = model(x)
        stats = T.step_losses(el, xh, pp, x, 0.06)
        stats[1].backward()
        if opt is not None:
            opt.step()
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    n = nsteps
    t0 = time.perf_counter()
    for _ in range(n):
        step()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / n
    print(f"backend={backend:5s} B={B}{' +' + which_adam if with_adam else ''}{' rotation_trick' if rotation else ''}{' cosine_sim' if cosine else ''}{' fsq_levels=(8,5,5,5)' if fsq else ''}{' codebook_groups=4' if groups else ''}{' lookup_free' if lfq else ''}{' codebook_dim=8' if factorized else ''}{' orthogonal_reg_weight=10' if orth else ''}{' entropy_weight=0.1' if entropy else ''}{' ema_decay=0.99' if ema else ''}{' ema_accumulate=2' if ema_acc else ''}: {dt * 1e3:8.2f} ms per forward+backward   {B / dt / 1e3:8.1f} k img/s", flush=True)
conv.set_conv_backend("hip")
