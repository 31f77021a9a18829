"""CPU tests of the pointer contract ("Pointer contract"; profiles/pointer_contract.md is the audit behind the table):

  * every pointer parameter of every `VQVAE_API int` entry of include/vqvae_hip.h has a row below;
  * every row of class "refuses" is shown to refuse: the entry, called with valid arguments except for that one pointer displaced
    by 4 bytes, returns VQVAE_ERR_UNSUPPORTED before any HIP call -- no device is present here;
  * `_lib.dense` / `_lib.written`, the front end's one helper, on CPU tensors.

Classes of a row (what the widest access of any reachable kernel on that pointer is, and what the entry does about it):
  narrow    16-byte accesses where the pointer allows them; an element-wise path with the same result where it does not
  refuses   16-byte accesses; VQVAE_ERR_UNSUPPORTED for a pointer that is not 16-byte aligned, before anything is launched
  element   accesses of one element only (4 bytes; 8 for int64 / fp64)
  host      read or written by the host during the call
"""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED = -3
N, R, E, H = "narrow", "refuses", "element", "host"

# entry -> {pointer parameter: class}
TABLE = {
    # vq_exact.hip.  z_e / codebook / z_q: the fixed widths D = 32 / 64 / 128 / 256 refuse; other widths run vq_generic.hip's kernels,
    # which pick their element-wise forms by these pointers.  The refusal is what is tested (D = 64).
    "vqvae_vq_forward_f32": dict(z_e=R, codebook=R, z_q=R, idx=E, hist=E, loss=E, perplexity=E, workspace=R),
    "vqvae_vq_onehot_f32": dict(idx=E, onehot=E),
    "vqvae_vq_decode_indices_f32": dict(idx=E, codebook=E, z_q=E),
    "vqvae_vq_launch_form": dict(waves=H, unit_rows=H, pool_pct=H),
    # train.hip
    "vqvae_vq_backward_f32": dict(z_e=N, codebook=N, idx=E, grad_zq=N, grad_loss=E, grad_z=N, grad_codebook=E, workspace=E),
    "vqvae_vq_ema_update_f32": dict(z_e=E, idx=E, uniforms=E, ema_cluster_size=E, ema_w=E, codebook=E, workspace=E),
    "vqvae_recon_loss_f32": dict(x_hat=R, x=R, embedding_loss=E, perplexity=E, out3=E, workspace=E),
    "vqvae_recon_loss_backward_f32": dict(x_hat=E, x=E, grad_loss=E, grad_x_hat=E),
    # backward.hip
    "vqvae_conv_wgrad_f32": dict(a=R, bt=R, grad_w=E, workspace=E),
    "vqvae_conv_wgrad_ex_f32": dict(a=R, bt=R, grad_w=E, workspace=E),
    "vqvae_bias_grad_f32": dict(grad_y=N, grad_b=E, workspace=E),
    "vqvae_relu_backward_f32": dict(grad_out=R, y=R, grad_in=R),
    # vq_ema_merge.hip, vq_kmeans.hip, vq_cosine.hip
    "vqvae_vq_ema_stats_f32": dict(z_e=E, idx=E, row_uniforms=E, stats=E, workspace=E),
    "vqvae_vq_ema_apply_f32": dict(stats=E, shard_uniforms=E, ema_cluster_size=E, ema_w=E, codebook=E, workspace=E),
    "vqvae_vq_kmeans_seed_f32": dict(z_e=N, uniforms=E, codebook=E, rows=E, workspace=E),
    "vqvae_vq_kmeans_update_f32": dict(z_e=E, idx=E, uniforms=E, codebook=E, counts=E, workspace=E),
    "vqvae_l2norm_forward_f32": dict(x=N, y=N, denom=N),
    "vqvae_l2norm_backward_f32": dict(y=N, denom=N, grad_y=N, grad_x=N),
    # vq_residual.hip: the stages run vqvae_vq_forward_f32 on z_e and on each codebook (refused up front at the fixed widths, as
    # there); the advance / finish / grad_z kernels pick their width by z_e, z_q, residual_out, grad_zq, grad_z and the codebooks
    "vqvae_vq_residual_forward_f32": dict(z_e=R, codebooks=H, z_q=N, idx=E, hist=E, loss_stage=E, perplexity_stage=E, loss=E,
                                          residual_out=N, workspace=R),
    "vqvae_vq_residual_decode_f32": dict(idx=E, codebooks=H, z_q=N),
    "vqvae_vq_residual_backward_f32": dict(z_e=N, codebooks=H, idx=E, grad_zq=N, grad_loss=E, grad_z=N, grad_codebooks=H, workspace=N),
    # vq_linear.hip (x / grad_y / y / grad_x by pointer; the weights go to LDS element by element)
    "vqvae_linear_rows_forward_f32": dict(x=N, w=E, b=E, y=N),
    "vqvae_linear_rows_backward_f32": dict(x=N, grad_y=N, w=E, grad_x=N, grad_w=E, grad_b=E, workspace=E),
    # pixelcnn.hip, pixelcnn_backward.hip
    "vqvae_gather_rows_f32": dict(idx=E, table=R, out=R),
    "vqvae_im2col_rows_f32": dict(x=R, dy=H, dx=H, out=R),
    "vqvae_gated_activation_f32": dict(t1=E, t2=E, cond=E, out=E),
    "vqvae_add_f32": dict(a=R, b=R, out=R),
    "vqvae_conv_taps_wgrad_f32": dict(grad_y=R, x=R, dy=H, dx=H, grad_w=E, workspace=E),
    "vqvae_gated_activation_backward_f32": dict(t1=E, t2=E, cond=E, grad_out=E, grad_pre=E, grad_cond_in=E, grad_cond=E),
    "vqvae_gather_rows_backward_f32": dict(idx=E, grad_out=E, grad_table=E, workspace=E),
    "vqvae_cross_entropy_f32": dict(logits=E, targets=E, loss=E, workspace=E),
    "vqvae_cross_entropy_backward_f32": dict(logits=E, targets=E, grad_loss=E, grad_logits=E),
    "vqvae_bias_grad_wide_f32": dict(grad_y=E, grad_b=E, workspace=E),
    # conv.hip / conv_res.hip / conv_ends.hip: activations, epilogue operands and packed images 16 bytes at a time; a bias one float
    # at a time (bias[n] per lane); the raw weight of a pack entry one float at a time
    "vqvae_conv_pack_f32": dict(w=E, packed=R),
    "vqvae_conv_forward_f32": dict(x=R, packed=R, bias=E, y=R),
    "vqvae_conv_forward_ep_f32": dict(x=R, packed=R, bias=E, addend=R, mask=R, y=R),
    "vqvae_conv_taps_pack_f32": dict(w=E, dy=H, dx=H, packed=R),
    "vqvae_conv_taps_forward_f32": dict(x=R, packed=R, bias=E, dy=H, dx=H, y=R),
    "vqvae_conv_taps_forward_ep_f32": dict(x=R, packed=R, bias=E, dy=H, dx=H, addend=R, mask=R, y=R),
    "vqvae_conv_taps_pack_dgrad_f32": dict(w=E, dy=H, dx=H, packed=R),
    "vqvae_res_layer_forward_f32": dict(x=R, packed_w1=R, packed_w2=R, y=R),
    "vqvae_res_layer_forward_ws_f32": dict(x=R, packed_w1=R, packed_w2=R, y=R, scratch=R),
    "vqvae_res_layer_forward_hidden_f32": dict(x=R, packed_w1=R, packed_w2=R, y=R, hidden=R),
    # the first and the last layer: conv_in's row-band kernel (16-byte loads and stores) only for aligned x_nchw / y, else the gather
    # kernel; convt_out reads x with 16-byte buffer loads and picks its store width by y_nchw
    "vqvae_conv_in_pack_f32": dict(w=E, packed=R),
    "vqvae_conv_in_forward_f32": dict(x_nchw=N, packed=R, bias=E, y=N),
    # (the mask lives in the row-band kernel only: with one, the entry refuses what conv_in alone would give to the gather kernel)
    "vqvae_conv_in_forward_ep_f32": dict(x_nchw=R, packed=R, bias=E, mask=R, y=R),
    "vqvae_convt_out_pack_f32": dict(w=E, packed=R),
    "vqvae_convt_out_forward_f32": dict(x=R, packed=R, bias=E, y_nchw=N),
    "vqvae_transpose_f32": dict(x=E, y=E),
    # model.hip: the whole-path entries test every image, map and workspace up front (the kernels of some route move 16 bytes per access
    # on each); w is a host struct whose device pointers vqvae_weights_pack_f32 made
    "vqvae_resstack_f32": dict(packed_w1=R, packed_w2=R, x=R, y=R, tmp=R),
    "vqvae_encoder_f32": dict(w=H, x=R, z_e=R, workspace=R),
    "vqvae_encoder_ex_f32": dict(w=H, x=R, z_e=R, workspace=R),
    "vqvae_decoder_f32": dict(w=H, z_q=R, x_hat=R, workspace=R),
    "vqvae_decoder_ex_f32": dict(w=H, z_q=R, x_hat=R, workspace=R),
    "vqvae_forward_f32": dict(w=H, x=R, x_hat=R, loss=E, perplexity=E, idx=E, workspace=R, vq_workspace=R),
    "vqvae_encode_f32": dict(w=H, x=R, idx=E, workspace=R, vq_workspace=R),
    "vqvae_decode_f32": dict(w=H, idx=E, x_hat=R, workspace=R),
    "vqvae_forward_begin_f32": dict(w=H, workspace=R, vq_workspace=R),
    "vqvae_forward_part_f32": dict(w=H, x=R, x_hat=R, idx=E, workspace=R, vq_workspace=R),
    "vqvae_forward_end_f32": dict(w=H, loss=E, perplexity=E, workspace=R),
    "vqvae_forward_abort_f32": dict(workspace=H),                                  # (a key of the host's table of open steps)
    # vq_grouped.hip: `grp_vec4` / `grp_vec4_books` pick every launch's width from the maps it touches; the groups' quantizers read
    # slabs in the workspace and the codebooks (refused up front at the fixed slab widths)
    "vqvae_vq_grouped_forward_f32": dict(z_e=N, codebooks=H, z_q=N, idx=E, hist=E, loss_group=E, perplexity_group=E, loss=E, slabs_out=N,
                                         workspace=R),
    "vqvae_vq_grouped_decode_f32": dict(idx=E, codebooks=H, z_q=N),
    "vqvae_vq_grouped_backward_f32": dict(z_e=N, codebooks=H, idx=E, grad_zq=N, grad_loss=E, grad_z=N, grad_codebooks=H, workspace=N),
    # vq_fsq.hip / vq_lfq.hip (vq_proj_kernels.h: `proj_wide` over the maps; the projections go to LDS one float at a time), vq_entropy.*
    "vqvae_fsq_forward_f32": dict(z_e=N, w_in=E, b_in=E, w_out=E, b_out=E, levels=H, z_q=N, idx=E, hist=E, perplexity=E),
    "vqvae_fsq_decode_indices_f32": dict(idx=E, w_out=E, b_out=E, levels=H, z_q=N),
    "vqvae_fsq_backward_f32": dict(z_e=N, grad_zq=N, w_in=E, b_in=E, w_out=E, levels=H, grad_z=N, grad_w_in=E, grad_b_in=E, grad_w_out=E,
                                   grad_b_out=E, workspace=E),
    "vqvae_lfq_forward_f32": dict(z_e=N, w_in=E, b_in=E, w_out=E, b_out=E, z_q=N, idx=E, hist=E, perplexity=E, losses=E, avg=E, workspace=E),
    "vqvae_lfq_decode_indices_f32": dict(idx=E, w_out=E, b_out=E, z_q=N),
    "vqvae_lfq_backward_f32": dict(z_e=N, grad_zq=N, grad_loss=E, avg=E, w_in=E, b_in=E, w_out=E, grad_z=N, grad_w_in=E, grad_b_in=E,
                                   grad_w_out=E, grad_b_out=E, workspace=E),
    "vqvae_vq_entropy_forward_f32": dict(z_e=E, codebook=E, losses=E, avg=E, rowstat=E, workspace=E),
    "vqvae_vq_entropy_backward_f32": dict(z_e=E, codebook=E, avg=E, rowstat=E, grad_loss=E, grad_z=E, grad_codebook=E, workspace=E),
    # optim.hip: the plan is a host blob (then its device copy, read 16 bytes at a time); the tensors it names take 16-byte accesses
    # only where all of a tensor's pointers allow them (optim.hip:134,190), and must be 4-byte aligned (vqvae_adam_plan_write)
    "vqvae_adam_plan_write": dict(numel_host=H, param=H, grad=H, exp_avg=H, exp_avg_sq=H, max_exp_avg_sq=H, step=H, group=H, plan_host=H,
                                  n_chunks_out=H),
    "vqvae_adam_step_f32": dict(plan_dev=R, groups_host=H, clip_coef=E),
    "vqvae_grad_norm_f32": dict(plan_dev=R, total_norm_out=E, clip_coef_out=E, workspace=E),
    # vq_orthogonal.*: the row tiles are staged 16 bytes per lane only for D % 4 == 0 and 16-byte aligned rows (vq_orthogonal.h:84);
    # everything else one element (the fp64 record as 8-byte words)
    "vqvae_vq_orthogonal_forward_f32": dict(rows=N, hist=E, uniforms=E, loss=E, count=E, selected=E, saved=E, workspace=E),
    "vqvae_vq_orthogonal_backward_f32": dict(saved=E, selected=E, count=E, grad_loss=E, grad_rows=E),
    # pixelcnn_sample.hip: `ld4` on the packed image and on the per-image state in the workspace; labels, uniforms, given codes,
    # samples, logits and status one element at a time.  The pack kernel copies every parameter one float at a time.
    "vqvae_pixelcnn_sample_pack_f32": dict(params=H, packed=R),
    "vqvae_pixelcnn_sample_f32": dict(packed=R, label=E, uniforms=E, samples=E, logits=E, status=E, workspace=R),
    "vqvae_pixelcnn_sample_ex_f32": dict(packed=R, label=E, uniforms=E, given=E, samples=E, logits=E, status=E, workspace=R),
    # model.hip: the raw weights go through the per-layer pack entries (one float at a time); the blob every image is carved from is
    # tested up front.  The range check reads the weights one float at a time and writes eleven floats.
    "vqvae_weights_pack_f32": dict(dims=H, raw=H, packed=R, out=H),
    "vqvae_weights_range_check_f32": dict(dims=H, raw=H, spread_log2_host=H, recommended_flags=H, scratch_device=E),
    # capi.hip / vq_generic.hip test hooks
    "vqvae_calibration_mfma_f16": dict(scratch=E),
    "vqvae_debug_row_sqnorm_f32": dict(x=E, out=E),
    # host-only entries
    "vqvae_profile_collect": dict(total_ms=H, launches=H),
    "vqvae_train_reduction_plan": dict(dims=H, out=H),
}



# The device pointers inside the two host structs, by field: what vqvae_weights_pack_f32 (raw) and every whole-path entry that takes a
# VqvaeWeights test before their first launch.  A raw weight is read one float at a time by the pack kernels; a bias is handed on and
# read as bias[n]; the codebook is handed on to kernels that read it 16 bytes at a time (vq_exact.hip:51, vq_unit.h:283,353,400, the
# gathering decoder kernel); the packed fields are operand images.
STRUCT_TABLE = {
    "VqvaeRawWeights": dict(enc0_w=E, enc0_b=E, enc2_w=E, enc2_b=E, enc4_w=E, enc4_b=E, enc_res_w1=E, enc_res_w2=E, pre_w=E, pre_b=E,
                            codebook=R, dec0_w=E, dec0_b=E, dec_res_w1=E, dec_res_w2=E, dec2_w=E, dec2_b=E, dec4_w=E, dec4_b=E),
    "VqvaeWeights": dict(enc0=R, enc0_b=E, enc2=R, enc2_b=E, enc4=R, enc4_b=E, enc_res_w1=R, enc_res_w2=R, pre=R, pre_b=E, codebook=R,
                         dec0=R, dec0_b=E, dec_res_w1=R, dec_res_w2=R, dec2=R, dec2_b=E, dec4=R, dec4_b=E),
}
WEIGHTS_ENTRIES = ["vqvae_encoder_f32", "vqvae_encoder_ex_f32", "vqvae_decoder_f32", "vqvae_decoder_ex_f32", "vqvae_forward_f32",
                   "vqvae_encode_f32", "vqvae_decode_f32", "vqvae_forward_begin_f32", "vqvae_forward_part_f32"]


def declared_entries():
    """{entry: [(type, name) of every pointer parameter]} of the `VQVAE_API int` entries, parsed as tests/test_capi.py parses"""
    hdr = open(os.path.join(ROOT, "include/vqvae_hip.h")).read()
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    out = {}
    for m in re.finditer(r"VQVAE_API\s+int\s+(vqvae_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", code, flags=re.S):
        ptrs = []
        for a in m.group(2).split(","):
            a = " ".join(a.split())
            if "*" in a:
                ptrs.append((a[:a.rindex("*") + 1].strip(), a[a.rindex("*") + 1:].strip()))
        out[m.group(1)] = ptrs
    return out


def test_every_pointer_parameter_has_a_row():
    decl = {e: p for e, p in declared_entries().items() if p}
    assert len(decl) > 80 and sum(len(p) for p in decl.values()) > 400          # the parse found the header
    assert set(decl) == set(TABLE), sorted(set(decl) ^ set(TABLE))
    for entry, rows in TABLE.items():
        assert [n for _, n in decl[entry]] == list(rows), f"{entry}: the table's rows are not the header's pointer parameters"
        assert all(c in (N, R, E, H) for c in rows.values()), entry


# ---- refusing rows: valid arguments (fake, 16-byte aligned device pointers that are never dereferenced), one pointer displaced ----
A = 4096
BIG = 1 << 30
_dy, _dx = (ctypes.c_int8 * 1)(0), (ctypes.c_int8 * 1)(0)
_taps = (ctypes.cast(_dy, ctypes.c_void_p), ctypes.cast(_dx, ctypes.c_void_p))
_books = (ctypes.c_void_p * 2)(A + 0x10000, A + 0x20000)


_DISPLACE = {}                                       # struct field -> bytes: what the struct tests move, one field at a time


def _weights():
    """a VqvaeWeights of the default model whose device pointers are never followed (every refusal comes before)"""
    from vqvae_amd import _lib
    cw = _lib.VqvaeWeights()
    cw.dims = _lib.VqvaeDims(128, 32, 2, 512, 64, 3, 0.25)
    for i, f in enumerate(_lib._PACKED_FIELDS):
        setattr(cw, f, A + 0x40000000 + 0x100000 * i + _DISPLACE.get(("VqvaeWeights", f), 0))
    return ctypes.byref(cw)


def _adam_groups():
    from vqvae_amd import _lib
    return (_lib.VqvaeAdamGroup * 1)(_lib.VqvaeAdamGroup(1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 0))


def _raw_and_dims():
    from vqvae_amd import _lib
    raw = _lib.VqvaeRawWeights(**{f: A + 0x50000000 + 0x100000 * i + _DISPLACE.get(("VqvaeRawWeights", f), 0)
                                  for i, f in enumerate(_lib._RAW_FIELDS)})
    return ctypes.byref(_lib.VqvaeDims(128, 32, 2, 512, 64, 3, 0.25)), ctypes.byref(raw)


_sample_params = (ctypes.c_void_p * 14)(*[A + 0x60000000 + 0x100000 * i for i in range(14)])


def _p(i):
    return A + 0x100000 * (i + 1)                     # distinct, far apart: no entry sees an overlap


# entry -> (argument list with P(i) placeholders for its pointer rows in header order, as built by _valid)
VALID = {
    "vqvae_vq_forward_f32": lambda p: (p["z_e"], p["codebook"], 1, 64, 8, 8, 512, 0.25, 0, p["z_q"], p["idx"], p["hist"], p["loss"],
                                       p["perplexity"], p["workspace"], BIG, None),
    "vqvae_recon_loss_f32": lambda p: (p["x_hat"], p["x"], 16, 1.0, None, None, p["out3"], p["workspace"], BIG, None),
    "vqvae_conv_wgrad_f32": lambda p: (p["a"], p["bt"], 1, 8, 8, 128, 8, 8, 128, 3, 1, 1, 0, p["grad_w"], p["workspace"], BIG, None),
    "vqvae_conv_wgrad_ex_f32": lambda p: (p["a"], p["bt"], 1, 8, 8, 128, 8, 8, 128, 3, 1, 1, 0, 0, p["grad_w"], p["workspace"], BIG, None),
    "vqvae_relu_backward_f32": lambda p: (p["grad_out"], p["y"], 16, p["grad_in"], None),
    "vqvae_vq_residual_forward_f32": lambda p: (p["z_e"], _books, 1, 64, 8, 8, 512, 2, 0.25, 0, p["z_q"], p["idx"], p["hist"], p["loss_stage"],
                                                p["perplexity_stage"], p["loss"], p["residual_out"], p["workspace"], BIG, None),
    "vqvae_gather_rows_f32": lambda p: (p["idx"], p["table"], 4, 16, 8, p["out"], None),
    "vqvae_im2col_rows_f32": lambda p: (p["x"], 1, 4, 4, 16, 1, *_taps, p["out"], None),
    "vqvae_add_f32": lambda p: (p["a"], p["b"], 16, p["out"], None),
    "vqvae_conv_taps_wgrad_f32": lambda p: (p["grad_y"], p["x"], 1, 4, 4, 16, 16, 1, *_taps, p["grad_w"], p["workspace"], BIG, None),
    "vqvae_conv_forward_f32": lambda p: (1, p["x"], p["packed"], p["bias"], 1, 8, 8, 128, 128, 0, p["y"], None),
    "vqvae_conv_forward_ep_f32": lambda p: (1, p["x"], p["packed"], p["bias"], 1, 8, 8, 128, 128, 0, p["addend"], p["mask"], p["y"], None),
    "vqvae_conv_taps_forward_f32": lambda p: (p["x"], p["packed"], p["bias"], 1, 8, 8, 128, 128, 1, *_taps, 0, p["y"], None),
    "vqvae_conv_taps_forward_ep_f32": lambda p: (p["x"], p["packed"], p["bias"], 1, 8, 8, 128, 128, 1, *_taps, 0, p["addend"], p["mask"],
                                                 p["y"], None),
    "vqvae_conv_pack_f32": lambda p: (1, p["w"], 128, 128, p["packed"], None),
    "vqvae_conv_taps_pack_f32": lambda p: (p["w"], 1, *_taps, 128, 128, p["packed"], None),
    "vqvae_conv_taps_pack_dgrad_f32": lambda p: (p["w"], 1, 0, 1, *_taps, 16, 16, p["packed"], None),
    "vqvae_conv_in_pack_f32": lambda p: (p["w"], 3, 64, p["packed"], None),
    "vqvae_conv_in_forward_f32": lambda p: (p["x_nchw"], p["packed"], p["bias"], 1, 32, 32, 3, 64, 0, p["y"], None),
    "vqvae_conv_in_forward_ep_f32": lambda p: (p["x_nchw"], p["packed"], p["bias"], 1, 32, 32, 3, 64, 0, p["mask"], p["y"], None),
    "vqvae_convt_out_pack_f32": lambda p: (p["w"], 64, 3, p["packed"], None),
    "vqvae_convt_out_forward_f32": lambda p: (p["x"], p["packed"], p["bias"], 1, 16, 16, 64, 3, 0, p["y_nchw"], None),
    "vqvae_adam_step_f32": lambda p: (p["plan_dev"], BIG, 1, 1, _adam_groups(), 1, 0, p["clip_coef"], None),
    "vqvae_grad_norm_f32": lambda p: (p["plan_dev"], BIG, 1, 1, 1.0, p["total_norm_out"], p["clip_coef_out"], p["workspace"], BIG, None),
    "vqvae_pixelcnn_sample_pack_f32": lambda p: (_sample_params, 14, 64, 32, 1, 1, p["packed"], BIG, None),
    "vqvae_pixelcnn_sample_f32": lambda p: (p["packed"], BIG, p["label"], p["uniforms"], 1, 4, 4, 64, 32, 1, 1, p["samples"], p["logits"],
                                            p["status"], p["workspace"], BIG, None),
    "vqvae_pixelcnn_sample_ex_f32": lambda p: (p["packed"], BIG, p["label"], p["uniforms"], 1, 4, 4, 64, 32, 1, 1, 1.0, 0, 1.0, p["given"],
                                               p["samples"], p["logits"], p["status"], p["workspace"], BIG, None),
    "vqvae_weights_pack_f32": lambda p: (*_raw_and_dims(), p["packed"], BIG, _weights(), None),
    "vqvae_resstack_f32": lambda p: (p["packed_w1"], p["packed_w2"], p["x"], 1, 8, 8, 128, 32, 2, 0, p["y"], p["tmp"], None),
    "vqvae_encoder_f32": lambda p: (_weights(), p["x"], 1, 32, 32, p["z_e"], p["workspace"], BIG, None),
    "vqvae_encoder_ex_f32": lambda p: (_weights(), p["x"], 1, 32, 32, 0, p["z_e"], p["workspace"], BIG, None),
    "vqvae_decoder_f32": lambda p: (_weights(), p["z_q"], 1, 8, 8, p["x_hat"], p["workspace"], BIG, None),
    "vqvae_decoder_ex_f32": lambda p: (_weights(), p["z_q"], 1, 8, 8, 0, p["x_hat"], p["workspace"], BIG, None),
    "vqvae_forward_f32": lambda p: (_weights(), p["x"], 1, 32, 32, 0, p["x_hat"], p["loss"], p["perplexity"], p["idx"], p["workspace"], BIG,
                                    p["vq_workspace"], BIG, None),
    "vqvae_encode_f32": lambda p: (_weights(), p["x"], 1, 32, 32, 0, p["idx"], p["workspace"], BIG, p["vq_workspace"], BIG, None),
    "vqvae_decode_f32": lambda p: (_weights(), p["idx"], 1, 8, 8, 0, p["x_hat"], p["workspace"], BIG, None),
    "vqvae_forward_begin_f32": lambda p: (_weights(), 128, 32, 32, 0, p["workspace"], BIG, p["vq_workspace"], BIG, None),
    "vqvae_forward_part_f32": lambda p: (_weights(), p["x"], 128, 0, 128, 32, 32, 0, p["x_hat"], p["idx"], p["workspace"], BIG,
                                         p["vq_workspace"], BIG, None),
    "vqvae_forward_end_f32": lambda p: (_weights(), 128, 32, 32, p["loss"], p["perplexity"], p["workspace"], BIG, None),
    "vqvae_vq_grouped_forward_f32": lambda p: (p["z_e"], _books, 1, 64, 8, 8, 512, 2, 0.25, 0, p["z_q"], p["idx"], p["hist"], p["loss_group"],
                                               p["perplexity_group"], p["loss"], p["slabs_out"], p["workspace"], BIG, None),
    "vqvae_res_layer_forward_f32": lambda p: (p["x"], p["packed_w1"], p["packed_w2"], 1, 8, 8, 128, 32, 0, p["y"], None),
    "vqvae_res_layer_forward_ws_f32": lambda p: (p["x"], p["packed_w1"], p["packed_w2"], 1, 8, 8, 96, 48, 0, p["y"], p["scratch"], BIG, None),
    "vqvae_res_layer_forward_hidden_f32": lambda p: (p["x"], p["packed_w1"], p["packed_w2"], 1, 8, 8, 128, 32, 0, p["y"], p["hidden"], None),
}

OPTIONAL = {("vqvae_vq_forward_f32", "z_q"), ("vqvae_conv_forward_ep_f32", "addend"), ("vqvae_conv_forward_ep_f32", "mask"),
            ("vqvae_conv_taps_forward_ep_f32", "addend"), ("vqvae_conv_taps_forward_ep_f32", "mask"), ("vqvae_conv_in_forward_ep_f32", "mask"),
            ("vqvae_forward_f32", "vq_workspace"), ("vqvae_encode_f32", "vq_workspace"), ("vqvae_forward_begin_f32", "vq_workspace"),
            ("vqvae_forward_part_f32", "vq_workspace")}
REFUSING = [(e, n) for e, rows in TABLE.items() for n, c in rows.items() if c == R]


def test_every_refusing_row_has_valid_arguments():
    assert {e for e, _ in REFUSING} == set(VALID)


@pytest.mark.parametrize("entry,name", REFUSING, ids=lambda v: v)
def test_refusing_rows_refuse_a_displaced_pointer(entry, name):
    """The refusal comes back without a device: nothing was launched.  The same call with the pointer in place gets past every
    pointer test only to fail at a launch, so it is not made here; that the other arguments are valid shows in the displaced call
    returning UNSUPPORTED and not a NULL / shape / workspace code -- and in no other displaced pointer being needed for it."""
    from vqvae_amd import _lib
    L = _lib.load()
    rows = [n for n, c in TABLE[entry].items() if c != H]
    ptrs = {n: _p(i) for i, n in enumerate(rows)}
    assert all(v % 16 == 0 for v in ptrs.values())
    ptrs[name] += 4                                                           # (every refusing row is fp32: 4 bytes)
    assert getattr(L, entry)(*VALID[entry](ptrs)) == UNSUPPORTED
    # not a refusal of the shapes: with NULL in the same slot the same arguments get the NULL (or missing-workspace) code, which every
    # entry returns for a pointer it requires -- the optional ones, for which NULL is a legal call that would go on to launch, excepted
    if (entry, name) not in OPTIONAL:
        ptrs[name] = None
        assert getattr(L, entry)(*VALID[entry](ptrs)) in (-1, -4)


def _aligned_args(entry):
    rows = [n for n, c in TABLE[entry].items() if c != H]
    return VALID[entry]({n: _p(i) for i, n in enumerate(rows)})


def test_struct_tables_name_the_structs_fields():
    from vqvae_amd import _lib
    assert list(STRUCT_TABLE["VqvaeRawWeights"]) == _lib._RAW_FIELDS and list(STRUCT_TABLE["VqvaeWeights"]) == _lib._PACKED_FIELDS
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include/vqvae_hip.h")).read(), flags=re.S)
    for struct, fields in (("VqvaeRawWeights", _lib._RAW_FIELDS), ("VqvaeWeights", _lib._PACKED_FIELDS)):
        body = re.search(r"typedef struct[^{}]*\{([^{}]*)\}\s*" + struct + r"\s*;", hdr, flags=re.S).group(1)
        names = re.findall(r"\*\s*([a-z0-9_]+)", body)
        assert names == fields, f"{struct}: a device pointer of the header has no row"


@pytest.mark.parametrize("struct,field", [(s_, f) for s_, rows in STRUCT_TABLE.items() for f in rows], ids=lambda v: v)
def test_struct_pointers_are_tested_before_any_launch(struct, field):
    """vqvae_weights_pack_f32 with one raw pointer displaced, every whole-path entry with one pointer of its VqvaeWeights displaced:
    a refusing field 4 bytes off is refused, an element field 4 bytes off is not (the call goes on to its next check: the entries'
    own arguments are made to fail there, with a workspace of eight bytes), 2 bytes off is."""
    from vqvae_amd import _lib
    L = _lib.load()
    entries = ["vqvae_weights_pack_f32"] if struct == "VqvaeRawWeights" else WEIGHTS_ENTRIES
    cls = STRUCT_TABLE[struct][field]
    try:
        for entry in entries:
            _DISPLACE.clear()
            _DISPLACE[(struct, field)] = 4
            if cls == R:
                assert getattr(L, entry)(*_aligned_args(entry)) == UNSUPPORTED, entry
            _DISPLACE[(struct, field)] = 2
            assert getattr(L, entry)(*_aligned_args(entry)) == UNSUPPORTED, entry
        if cls == E and struct == "VqvaeRawWeights":
            # 4 bytes off is legal for a weight or a bias: the same call, its blob too small, gets as far as the size check
            _DISPLACE[(struct, field)] = 4
            args = list(_aligned_args("vqvae_weights_pack_f32"))
            args[3] = 8
            assert L.vqvae_weights_pack_f32(*args) == -4
    finally:
        _DISPLACE.clear()


def test_the_committed_table_is_this_table():
    """profiles/pointer_contract.md carries the audit's notes; its entry / pointer / class columns are TABLE and STRUCT_TABLE, row for row"""
    doc = open(os.path.join(ROOT, "profiles", "pointer_contract.md")).read()
    rows = re.findall(r"^\| `([A-Za-z0-9_]+)` \| `([^`]*?)([a-z0-9_]+)` \| [^|]* \| (narrow|refuses|element|host) \|", doc, flags=re.M)
    got = {}
    for entry, _type, name, cls in rows:
        got.setdefault(entry, {})[name] = cls
    want = dict(TABLE)
    want.update(STRUCT_TABLE)
    assert {e: dict(r) for e, r in want.items()} == got


def test_a_non_fixed_width_quantizer_call_is_not_refused_for_its_pointers():
    """vqvae_vq_forward_f32 refuses under-aligned z_e / codebook / z_q at the fixed widths only: at D = 48 the same displaced call gets
    past the pointer tests and stops at the next check, the workspace.  Both any-width kernels choose their access width from these
    pointers: vq_anyd_kernel from z_e, codebook and z_q, vq_generic_kernel (VQVAE_VQ_BF16_FILTER) from the codebook and, on row-major
    rows, z_e -- tests/test_views_gpu.py runs both on displaced views."""
    from vqvae_amd import _lib
    L = _lib.load()
    f = L.vqvae_vq_forward_f32
    assert f(A + 4, A + 0x1000, 1, 48, 8, 8, 512, 0.25, 0, A + 0x2000, A + 0x3000, A + 0x4000, A + 0x5000, A + 0x5004, A + 0x6000, 16, None) == -4
    assert f(A + 4, A + 0x1000, 1, 64, 8, 8, 512, 0.25, 0, A + 0x2000, A + 0x3000, A + 0x4000, A + 0x5000, A + 0x5004, A + 0x6000, 16, None) == UNSUPPORTED
    # bias_grad's four-channel form takes a 4-byte aligned gradient (an element-wise variant in the same order), not a 2-byte one
    assert L.vqvae_bias_grad_f32(A + 2, 1, 64, 32, 0, A, A, BIG, None) == UNSUPPORTED


# ---- the helper ------------------------------------------------------------------------------------------------------------------
def _displaced(t):
    buf = torch.empty(t.numel() + 4, dtype=t.dtype)
    while buf.data_ptr() % 16:                                                # (the CPU allocator aligns to 64 bytes; be sure)
        buf = torch.empty(t.numel() + 4, dtype=t.dtype)
    v = buf[1:1 + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def test_dense_returns_an_aligned_dense_tensor_itself():
    from vqvae_amd import _lib
    t = torch.arange(40.0).view(5, 8)
    assert t.data_ptr() % 16 == 0 and _lib.dense(t) is t
    assert _lib.dense(None) is None
    v = _displaced(t)
    assert _lib.dense(v, 4) is v and _lib.dense(v) is not v                    # an entry with an element-wise path takes it as it is
    i = _displaced(torch.arange(6))
    assert i.data_ptr() % 16 == 8 and _lib.dense(i, 8) is i and _lib.dense(i) is not i


@pytest.mark.parametrize("view", ["displaced", "permuted", "every-second-column", "expanded", "channels_last"])
def test_dense_copies_every_other_view(view):
    from vqvae_amd import _lib
    t = torch.randn(2, 6, 4, 8)
    v = {"displaced": lambda: _displaced(t), "permuted": lambda: t.permute(0, 2, 3, 1), "every-second-column": lambda: t[..., ::2],
         "expanded": lambda: t[:1, :1].expand(2, 6, 4, 8), "channels_last": lambda: t.to(memory_format=torch.channels_last)}[view]()
    assert not (v.is_contiguous() and v.data_ptr() % 16 == 0)
    d = _lib.dense(v)
    assert d is not v and d.is_contiguous() and d.data_ptr() % 16 == 0 and d.shape == v.shape and torch.equal(d, v)
    assert d.untyped_storage().data_ptr() != v.untyped_storage().data_ptr() and not d.requires_grad


def test_written_copies_back_and_keeps_the_callers_tensor():
    from vqvae_amd import _lib
    t = torch.arange(12.0).view(3, 4)
    with _lib.written(t) as w:                                                # aligned and dense: the tensor itself, no version bump of ours
        assert w is t
    for v in (_displaced(t), torch.zeros(3, 8)[:, ::2].copy_(t), torch.nn.Parameter(_displaced(t))):
        ptr, version, want = v.data_ptr(), v._version, v.detach().clone() + 1
        with _lib.written(v) as w:
            assert w is not v and w.is_contiguous() and w.data_ptr() % 16 == 0 and torch.equal(w, v)
            w.add_(1)                                                          # what a kernel does through w.data_ptr()
        assert torch.equal(v.detach(), want) and v.data_ptr() == ptr and v._version > version
    v = _displaced(t)
    with pytest.raises(RuntimeError, match="boom"):
        with _lib.written(v) as w:
            w.add_(1)
            raise RuntimeError("boom")
    assert torch.equal(v, t)                                                   # a failed call leaves the caller's state alone
