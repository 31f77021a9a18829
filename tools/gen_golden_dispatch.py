#!/usr/bin/env python3
"""Kernel-selection goldens: record the host-side query answers of the library that vqvae_amd._lib loads (no GPU needed; launch
forms assume 256 CUs, as they do without a device) into tests/golden/dispatch_table.json:

  vq          vq_kernel_name and vq_sweeps over K x D x flags
  vq_forms    vq_launch_form and vq_kernel_instance over rows x K x D x HW x flags, only where a launch form exists
              ([flat index, waves, unit rows, pooled %, index into "instances"]; every other grid point answers None)
  vq_ws       vqvae_vq_workspace_bytes over K x D
  conv        vqvae_conv_term_products over kinds x map sizes x channel pairs x flags
  model_ws    vqvae_workspace_bytes and vqvae_workspace_ze_offset for a few VqvaeDims and batch shapes

Every table is a flat list in the row-major order of its grid's axes.  tests/test_capi.py::test_dispatch_table_unchanged asserts
every entry.  Regenerate only when a selection changes on purpose:

    python tools/gen_golden_dispatch.py
"""
import itertools
import json
import os
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
}


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
    return {"grid": g, "names": names, "instances": instances, "vq": vq, "vq_forms": forms, "vq_ws": vq_ws, "conv": conv,
            "model_ws": model_ws}


def main():
    t = table()
    with open(OUT, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in t.items()) + "\n}\n")
    print(f"{OUT}: {os.path.getsize(OUT)} bytes, {len(t['vq'])} quantizer queries, {len(t['vq_forms'])} launch forms, "
          f"{len(t['conv'])} conv queries")


if __name__ == "__main__":
    main()
