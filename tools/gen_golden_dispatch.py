#!/usr/bin/env python3
"""Kernel-selection goldens: record the host-side query answers of the library that vqvae_amd._lib loads (no GPU needed; launch
forms assume 256 CUs, as they do without a device) into tests/golden/dispatch_table.json:

  vq          vq_kernel_name and vq_sweeps over K x D x flags
  vq_forms    vq_launch_form and vq_kernel_instance over rows x K x D x HW x flags, only where a launch form exists
              ([flat index, waves, unit rows, pooled %, index into "instances"]; every other grid point answers None)
  vq_ws       vqvae_vq_workspace_bytes over K x D
  conv        vqvae_conv_term_products over kinds x map sizes x channel pairs x flags
  model_ws    vqvae_workspace_bytes and vqvae_workspace_ze_offset for a few VqvaeDims and batch shapes
  train_ws    every training *_workspace_bytes query over channels x k, taps x channels, rows x keys x channels (one table each),
              asked in a child process that sees no GPU: the radix sort's scratch inside three of them is rocPRIM's and follows the
              device's architecture
  train_plans vqvae_train_reduction_plan over the same shapes x batch: indices into "train_plan_values", the distinct answers
              (None where the entry point refuses the shape)

Every table is a flat list in the row-major order of its grid's axes.  tests/test_capi.py::test_dispatch_table_unchanged asserts
every entry.  Regenerate only when a selection changes on purpose:

    python tools/gen_golden_dispatch.py
"""
import itertools
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from vqvae_amd import _lib  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "dispatch_table.json")

GRID = {
    "K": [480, 481, 512, 513, 600, 1024, 1025, 1056, 16384, 16385],
    "D": [1, 3, 48, 63, 64, 65, 128, 200, 256, 257],
    "HW": [49, 64, 96, 784],
    "rows": [1, 4096, 8 * 256 * 32, 32 * 256 * 32, 256 * 256 * 32],
    # row-major / NCHW, alone and with every other bit: prepared, exact sweep, bf16 filter, the removed 0x10 / 0x20, unfused,
    # the forced launch forms (0x300: twelve waves)
    "vq_flags": [base | extra for base in (0x0, 0x1)
                 for extra in (0x0, 0x2, 0x4, 0x8, 0x4 | 0x8, 0x10, 0x20, 0x40, 0x100, 0x200, 0x300, 0x400)],
    "conv_kind": list(range(8)),
    "conv_map": [[4, 4], [7, 7], [8, 8], [8, 16], [15, 15], [16, 16], [28, 28], [32, 32], [56, 56], [64, 64]],
    "conv_ch": [[3, 64], [32, 32], [48, 32], [64, 3], [64, 48], [64, 128], [128, 64], [128, 128]],
    "conv_flags": [0x0, 0x1, 0x2, 0x3, 0x4, 0x8, 0xC, 0x100, 0x102, 0x104, 0x108],
    # VqvaeDims fields: h_dim, res_h_dim, n_res_layers, n_embeddings, embedding_dim, in_ch (beta 0.25)
    "model_dims": [[128, 32, 2, 512, 64, 3], [128, 32, 2, 1024, 64, 3], [128, 32, 2, 2048, 128, 3], [64, 32, 1, 512, 48, 3],
                   [256, 64, 2, 512, 64, 1]],
    "model_shape": [[1, 32, 32], [4096, 32, 32], [2, 64, 64], [3, 28, 28], [4, 30, 32], [8, 224, 224]],
    # training reductions
    "train_ch": [3, 32, 48, 64, 96, 100, 128, 256, 512],
    "train_k": [1, 2, 3, 4],
    "train_ntaps": [1, 2, 6, 8, 9, 21, 28, 32],
    "train_N": [1, 4096, 262144],
    "train_keys": [10, 512],
    "train_B": [1, 37, 257, 1024, 4096],
    # weight-gradient geometries: A map side, Bt is an NCHW image, flags.  stride 2 for k = 4, else 1; pad 0 for k = 1, else 1; the
    # Bt map is stride times the A map
    "train_wgrad_geom": [[8, 0, 0x0], [16, 1, 0x0]],
    "train_taps_side": 8,      # tap lists: the first ntaps of a 5 x 7 window above and around the pixel, row by row
}


def taps_of(ntaps):
    """(dy list, dx list) of the grid's tap lists; 28 taps are layer 0's vertical stack"""
    win = [(ky - 3, kx - 3) for ky in range(5) for kx in range(7)][:ntaps]
    return [t[0] for t in win], [t[1] for t in win]


def train_ws(L, g=GRID):
    """the workspace-size tables of the training entry points (L: the loaded library)"""
    ch, N = g["train_ch"], g["train_N"]
    rows = list(itertools.product(N, g["train_keys"], ch))
    return {
        "conv_wgrad": [L.vqvae_conv_wgrad_workspace_bytes(ca, cb, k) for ca, cb, k in itertools.product(ch, ch, g["train_k"])],
        "conv_taps_wgrad": [L.vqvae_conv_taps_wgrad_workspace_bytes(t, ci, co) for t, ci, co in itertools.product(g["train_ntaps"], ch, ch)],
        "bias_grad": [L.vqvae_bias_grad_workspace_bytes(c) for c in ch],
        "bias_grad_wide": [L.vqvae_bias_grad_wide_workspace_bytes(c) for c in ch],
        "vq_backward": [L.vqvae_vq_backward_workspace_bytes(n, K, D) for n, K, D in rows],
        "vq_ema": [L.vqvae_vq_ema_workspace_bytes(n, K, D) for n, K, D in rows],
        "gather_rows_backward": [L.vqvae_gather_rows_backward_workspace_bytes(n, C, r) for n, r, C in rows],
        "cross_entropy": [L.vqvae_cross_entropy_workspace_bytes(n) for n in N],
        "recon_loss": [L.vqvae_recon_loss_workspace_bytes()],
    }


def train_ws_without_device(g=GRID):
    """train_ws as a machine without a GPU answers it (this file as a child process with every device hidden)"""
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", ROCR_VISIBLE_DEVICES="-1")
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--train-ws", json.dumps(g)], env=env, check=True,
                         capture_output=True, text=True).stdout
    return json.loads(out.strip().splitlines()[-1])


def train_plan_queries(g=GRID):
    """(reduction, dims) of every vqvae_train_reduction_plan query of the goldens, in table order"""
    ch, Bs = g["train_ch"], g["train_B"]
    for (side, nchw, flags), ca, cb, k, B in itertools.product(g["train_wgrad_geom"], ch, ch, g["train_k"], Bs):
        s = 2 if k == 4 else 1
        yield "conv_wgrad", (B, side, side, ca, side * s, side * s, cb, k, s, 0 if k == 1 else 1, nchw, flags)
    side = g["train_taps_side"]
    for t, ci, co, B in itertools.product(g["train_ntaps"], ch, ch, Bs):
        dy, dx = taps_of(t)
        yield "conv_taps_wgrad", (B, side, side, ci, co, t, *dy, *dx)
    for what, c, B in itertools.product(("bias_grad", "bias_grad_wide"), ch, Bs):
        yield what, (B * 64, c)
    for n, K, D in itertools.product(g["train_N"], g["train_keys"], ch):
        yield "segsum", (n, K, D)


def table():
    L = _lib.load()
    g = GRID
    names, instances = [], []

    def idx_of(lst, s):
        if s not in lst:
            lst.append(s)
        return lst.index(s)

    vq = []
    for K, D, f in itertools.product(g["K"], g["D"], g["vq_flags"]):
        vq.append([idx_of(names, _lib.vq_kernel_name(K, D, f)), _lib.vq_sweeps(K, D, f)])
    forms = []
    for i, (n, K, D, HW, f) in enumerate(itertools.product(g["rows"], g["K"], g["D"], g["HW"], g["vq_flags"])):
        form = _lib.vq_launch_form(n, K, D, HW, f)
        if form is not None:
            forms.append([i, *form, idx_of(instances, _lib.vq_kernel_instance(n, K, D, HW, f))])
    vq_ws = [L.vqvae_vq_workspace_bytes(1000, K, D) for K, D in itertools.product(g["K"], g["D"])]
    conv = [L.vqvae_conv_term_products(k, hw[0], hw[1], ch[0], ch[1], f)
            for k, hw, ch, f in itertools.product(g["conv_kind"], g["conv_map"], g["conv_ch"], g["conv_flags"])]
    model_ws = []
    for dm, (B, H, W) in itertools.product(g["model_dims"], g["model_shape"]):
        d = _lib.VqvaeDims(*dm, 0.25)
        model_ws.append([L.vqvae_workspace_bytes(d, B, H, W), L.vqvae_workspace_ze_offset(d, B, H, W)])
    plan_values, plans = [], []
    for what, dims in train_plan_queries(g):
        p = _lib.train_reduction_plan(what, *dims)
        plans.append(idx_of(plan_values, None if p is None else list(p)))
    return {"grid": g, "names": names, "instances": instances, "vq": vq, "vq_forms": forms, "vq_ws": vq_ws, "conv": conv,
            "model_ws": model_ws, "train_ws": train_ws_without_device(g), "train_plan_values": plan_values, "train_plans": plans}


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--train-ws":
        print(json.dumps(train_ws(_lib.load(), json.loads(sys.argv[2]))))
        return
    t = table()
    with open(OUT, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in t.items()) + "\n}\n")
    print(f"{OUT}: {os.path.getsize(OUT)} bytes, {len(t['vq'])} quantizer queries, {len(t['vq_forms'])} launch forms, "
          f"{len(t['conv'])} conv queries")


if __name__ == "__main__":
    main()
