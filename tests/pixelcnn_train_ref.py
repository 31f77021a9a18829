"""CPU torch-autograd restatement of the reference GatedPixelCNN (pixelcnn/models.py:20-127) and its training criterion, written
from the model's definition with torch.nn.functional over a plain dict of parameters -- any dtype (the GPU tests run it in fp64 as
the yardstick for shapes larger than the goldens hold).  tests/test_pixelcnn_train_cpu.py pins it to the reference's recorded
gradients (tests/golden/pixelcnn_train_cases.npz).

Mask 'A' (models.py:60-62): the reference zeroes the last row of the vertical stack and the last column of the horizontal stack
through `.data` before each forward, so autograd still differentiates with respect to those (zero) entries; here the weights are
zeroed in place before the forward and stay leaves, which gives the same gradient."""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

CASES = {"k512_dim64_l15": (512, 64, 15, 10, 4, 8, 8), "k64_dim32_l3": (64, 32, 3, 5, 3, 6, 6)}


def inputs(name):
    """the seeded (x, label) of tests/golden/pixelcnn_cases.npz (oracle/gen_golden_pixelcnn.py)"""
    K, dim, nl, ncls, B, H, W = CASES[name]
    g = torch.Generator().manual_seed(77 + len(name))
    x = torch.randint(0, K, (B, H, W), generator=g)
    label = torch.randint(0, ncls, (B,), generator=g)
    return x, label


def train_batches(name, steps=3):
    """the batches of the recorded 3-step training trajectory"""
    K, dim, nl, ncls, B, H, W = CASES[name]
    out = []
    for i in range(steps):
        g = torch.Generator().manual_seed(1000 + 17 * i + len(name))
        out.append((torch.randint(0, K, (B, H, W), generator=g), torch.randint(0, ncls, (B,), generator=g)))
    return out


def perturb_biases(model):
    """oracle/gen_golden_pixelcnn.py: non-trivial biases (the reference initialises them to 0)"""
    with torch.no_grad():
        for n_, p in model.named_parameters():
            if n_.endswith("bias"):
                p.copy_(torch.randn(p.shape, generator=torch.Generator().manual_seed(len(n_))) * 0.05)


def make_causal(params):
    with torch.no_grad():
        params["layers.0.vert_stack.weight"][:, :, -1].zero_()
        params["layers.0.horiz_stack.weight"][:, :, :, -1].zero_()


def _gate(t):
    a, g = t.chunk(2, dim=1)
    return torch.tanh(a) * torch.sigmoid(g)


def forward(p, x, label, n_layers, head_mask=None, keep=None):
    """logits (B, K, H, W) of GatedPixelCNN.forward; p: name -> tensor (the state_dict's names).
    head_mask ((B, 512, H, W) of 0 / 1): the head's ReLU becomes `pre * head_mask`, i.e. the ReLU decisions are given instead of
    taken from this run's own pre-activations (tests/pixelcnn_envelope.py: a pre-activation within rounding of zero may fall on
    either side in two correct implementations, and one such decision moves a gradient summed over many pixels by more than the
    tolerance).  keep: a dict that receives the head's pre-activation under "pre" (detached)."""
    B, H, W = x.shape
    t = F.embedding(x.reshape(-1), p["embedding.weight"]).view(B, H, W, -1).permute(0, 3, 1, 2)
    x_v = x_h = t
    for i in range(n_layers):
        q = f"layers.{i}."
        k = 7 if i == 0 else 3
        h = F.embedding(label, p[q + "class_cond_embedding.weight"])[:, :, None, None]
        h_vert = F.conv2d(x_v, p[q + "vert_stack.weight"], p[q + "vert_stack.bias"], 1, (k // 2, k // 2))[:, :, :x_v.size(-1), :]
        out_v = _gate(h_vert + h)
        h_horiz = F.conv2d(x_h, p[q + "horiz_stack.weight"], p[q + "horiz_stack.bias"], 1, (0, k // 2))[:, :, :, :x_h.size(-2)]
        v2h = F.conv2d(h_vert, p[q + "vert_to_horiz.weight"], p[q + "vert_to_horiz.bias"])
        out = _gate(v2h + h_horiz + h)
        out_h = F.conv2d(out, p[q + "horiz_resid.weight"], p[q + "horiz_resid.bias"])
        x_v, x_h = out_v, (out_h + x_h if i > 0 else out_h)
    pre = F.conv2d(x_h, p["output_conv.0.weight"], p["output_conv.0.bias"])
    if keep is not None:
        keep["pre"] = pre.detach()
    t = F.relu(pre) if head_mask is None else pre * head_mask.to(pre.dtype)
    return F.conv2d(t, p["output_conv.2.weight"], p["output_conv.2.bias"])


def loss_and_grads(state, x, label, n_layers, dtype=torch.float64, head_mask=None, keep=None):
    """-> (loss, grad_logits (B,K,H,W), {name: grad}) of the reference criterion (gated_pixelcnn.py:91-96), on the CPU.
    head_mask, keep: as in `forward`; keep also receives the logits under "logits"."""
    p = {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in state.items()}
    make_causal(p)
    x, label = x.cpu(), label.cpu()
    logits = forward(p, x, label, n_layers, head_mask, keep)
    logits.retain_grad()
    if keep is not None:
        keep["logits"] = logits.detach()
    K = logits.shape[1]
    loss = F.cross_entropy(logits.permute(0, 2, 3, 1).contiguous().view(-1, K), x.view(-1))
    loss.backward()
    return loss.detach(), logits.grad.detach(), {k: v.grad.detach() for k, v in p.items()}


def grad_keys(name, keys):
    """the parameter gradients the golden file stores: all of the small case; a subset of the large one"""
    if name == "k64_dim32_l3":
        return list(keys)
    keep = ("embedding.", "layers.0.", "layers.1.", "layers.14.", "output_conv.")
    return [k for k in keys if k.startswith(keep) or "class_cond_embedding" in k]


def tolerance(ref, absmax=None):
    """the house tolerance of tests/test_training_gpu.py: atol 1e-5 * max|g| + rtol 1e-4 (max|g| over the whole tensor)"""
    ref = np.asarray(ref, dtype=np.float64)
    return 1e-5 * (float(np.abs(ref).max()) if absmax is None else absmax) + 1e-4 * np.abs(ref)


# The golden file keeps tensors of up to SAMPLE elements whole; of larger ones, the values at SAMPLE seeded flat positions (plus
# positions a test needs, e.g. the mask-'A' taps) and the maximum magnitude of the whole tensor, which sets the tolerance's atol.
SAMPLE = 1024


def store(out, path, arr, must=None):
    """write tensor `arr` to the golden dict `out` under `path`: whole, or sampled (path/idx, path/val); always path/absmax"""
    a = np.ascontiguousarray(np.asarray(arr, dtype=np.float32))
    out[path + "/absmax"] = np.float64(np.abs(a).max())
    if a.size <= SAMPLE and must is None:
        out[path] = a
        return
    rng = np.random.default_rng(zlib.crc32(path.encode()))
    idx = rng.choice(a.size, min(SAMPLE, a.size), replace=False)
    if must is not None:
        idx = np.union1d(idx, np.asarray(must, dtype=np.int64))
    idx = np.unique(idx).astype(np.int32)
    out[path + "/idx"] = idx
    out[path + "/val"] = a.ravel()[idx]


def stored(golden, path):
    """-> (flat positions or None for a whole tensor, values, max |.| of the whole tensor)"""
    absmax = float(golden[path + "/absmax"])
    if path in golden.files:
        return None, np.asarray(golden[path]), absmax
    return np.asarray(golden[path + "/idx"]), np.asarray(golden[path + "/val"]), absmax


def stored_names(golden, prefix):
    """names of the tensors stored under `prefix` (e.g. 'k64_dim32_l3/grad/')"""
    return sorted(k[len(prefix):-len("/absmax")] for k in golden.files if k.startswith(prefix) and k.endswith("/absmax"))


def at_stored(golden, path, got):
    """(got at the stored positions, stored values, absmax), got as a full tensor"""
    idx, ref, absmax = stored(golden, path)
    got = np.asarray(got, dtype=np.float64)
    return (got.reshape(ref.shape) if idx is None else got.ravel()[idx]), ref.astype(np.float64), absmax


def mask_a_positions(shape, vertical):
    """flat positions of the taps mask 'A' zeroes: the vertical stack's last row, the horizontal stack's last column"""
    m = np.zeros(shape, dtype=bool)
    if vertical:
        m[:, :, -1] = True
    else:
        m[:, :, :, -1] = True
    return np.flatnonzero(m)
