#!/usr/bin/env python3
"""Bit goldens of the default 32x32 forward for tests/test_forward_ends_gpu.py -> tests/golden/forward_ends.npz (needs a GPU).

VQVAE(128, 32, 2, K, 64, 0.25), torch.manual_seed(0) right before the model, on seeded N(0, 1) images: x_hat, embedding_loss,
perplexity and the indices of `_forward_c(x, want_idx=True, parts=1, fwd_flags=0)` (the three-launch route: enc_front8, the fused
middle kernel, dec_tail8) as the library that `vqvae_amd._lib` loads computes them.  The file records what a KNOWN-GOOD library
gave, so that a change to the end kernels which must not move a bit can be held against it: generate it with the library of the
commit BEFORE such a change (VQVAE_HIP_LIB_OVERRIDE=<that library>), never with the tree under test.

    VQVAE_HIP_LIB_OVERRIDE=<parent's libvqvae_hip.so> python tools/gen_golden_forward_ends.py [OUT.npz]

Cases: B in {1, 4, 5, 9} x K in {256, 512} (idle waves, one full workgroup, a partial last workgroup), and at B = 5, K = 512 the
biases of the first two and the last two layers set to zeros and to +-[8, 12] (the tables the end kernels stage on chip).
Each case also stores the sha256 of its input image bytes and of the model's parameters: a test that fails on those has a
different torch generator in front of it, not a different kernel."""
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "tests", "golden", "forward_ends.npz")

END_BIASES = ("encoder.conv_stack.0.bias", "encoder.conv_stack.2.bias",
              "decoder.inverse_conv_stack.2.bias", "decoder.inverse_conv_stack.4.bias")

# (name, B, K, bias mode)
CASES = [(f"B{B}_K{K}", B, K, None) for K in (256, 512) for B in (1, 4, 5, 9)] + \
        [("B5_K512_zero_biases", 5, 512, "zero"), ("B5_K512_large_biases", 5, 512, "large")]


def make_model(K, bias_mode, device):
    from vqvae_amd import conv
    from vqvae_amd.modules import VQVAE
    conv.set_conv_backend("hip")
    torch.manual_seed(0)
    m = VQVAE(128, 32, 2, K, 64, 0.25).eval()
    if bias_mode is not None:
        g = torch.Generator().manual_seed(77)
        params = dict(m.named_parameters())
        with torch.no_grad():
            for name in END_BIASES:
                b = params[name]
                if bias_mode == "zero":
                    b.zero_()
                else:                                   # |b| in [8, 12], random signs
                    mag = 8.0 + 4.0 * torch.rand(b.shape, generator=g)
                    sign = torch.where(torch.rand(b.shape, generator=g) < 0.5, -1.0, 1.0)
                    b.copy_(mag * sign)
    return m.to(device)


def make_input(B, K):
    return torch.randn(B, 3, 32, 32, generator=torch.Generator().manual_seed(1000 + 16 * B + K // 256))


def fingerprint(m, x):
    h = hashlib.sha256()
    h.update(x.numpy().tobytes())
    for name, p in sorted(m.state_dict().items()):
        h.update(name.encode())
        h.update(p.detach().cpu().numpy().tobytes())
    return h.hexdigest()


def run_case(name, B, K, bias_mode, device):
    """-> dict of host arrays: x_hat (uint32 bits), loss / perplexity (uint32 bits), idx (int16), inputs (sha256 hex)"""
    m = make_model(K, bias_mode, device)
    x = make_input(B, K)
    with torch.no_grad():
        loss, x_hat, ppl, idx = m._forward_c(x.to(device), want_idx=True, parts=1, fwd_flags=0)
    torch.cuda.synchronize()
    return {"x_hat": x_hat.cpu().numpy().view(np.uint32), "loss": loss.cpu().numpy().reshape(1).view(np.uint32),
            "perplexity": ppl.cpu().numpy().reshape(1).view(np.uint32), "idx": idx.cpu().numpy().reshape(-1).astype(np.int16),
            "inputs": np.array(fingerprint(m, x))}


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    assert torch.cuda.is_available(), "the goldens are what the GPU kernels compute: this needs a GPU"
    device = torch.device("cuda:0")
    arrays = {}
    for name, B, K, bias_mode in CASES:
        r = run_case(name, B, K, bias_mode, device)
        assert np.isfinite(r["x_hat"].view(np.float32)).all(), name
        for k, v in r.items():
            arrays[f"{name}/{k}"] = v
    from vqvae_amd import _lib, build
    arrays["library_fingerprint"] = np.array(build.library_fingerprint(_lib.LIB_PATH) or "")      # of the sources it was built from
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez(out, **arrays)
    print(f"{out}: {os.path.getsize(out)} bytes, {len(CASES)} cases, library {_lib.LIB_PATH}")


if __name__ == "__main__":
    main()
