"""ctypes binding of libvqvae_hip.so (the C ABI declared in include/vqvae_hip.h).

There is deliberately NO fallback here: if the HIP library is missing or cannot be
loaded, importing the product path raises.  torch must be imported first so that
the library binds to the HIP runtime torch has already loaded (one runtime per
process is required for shared streams and device pointers).
"""
from __future__ import annotations

import collections
import ctypes as C
import os

import torch  # noqa: F401  (loads libamdhip64 first)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("VQVAE_HIP_LIB_OVERRIDE") or os.path.join(_HERE, "libvqvae_hip.so")   # override: A/B tools only

_i64, _i32, _f32, _vp, _sz = C.c_int64, C.c_int, C.c_float, C.c_void_p, C.c_size_t

class VqvaeDims(C.Structure):
    _fields_ = [("h_dim", _i32), ("res_h_dim", _i32), ("n_res_layers", _i32), ("n_embeddings", _i32),
                ("embedding_dim", _i32), ("in_ch", _i32), ("beta", _f32)]


_RAW_FIELDS = ["enc0_w", "enc0_b", "enc2_w", "enc2_b", "enc4_w", "enc4_b", "enc_res_w1", "enc_res_w2", "pre_w", "pre_b",
               "codebook", "dec0_w", "dec0_b", "dec_res_w1", "dec_res_w2", "dec2_w", "dec2_b", "dec4_w", "dec4_b"]
_PACKED_FIELDS = ["enc0", "enc0_b", "enc2", "enc2_b", "enc4", "enc4_b", "enc_res_w1", "enc_res_w2", "pre", "pre_b", "codebook",
                  "dec0", "dec0_b", "dec_res_w1", "dec_res_w2", "dec2", "dec2_b", "dec4", "dec4_b"]


class VqvaeAdamGroup(C.Structure):
    _fields_ = [("lr", C.c_double), ("beta1", C.c_double), ("beta2", C.c_double), ("eps", C.c_double), ("weight_decay", C.c_double),
                ("flags", _i32), ("reserved", _i32)]


class VqvaeRawWeights(C.Structure):
    _fields_ = [(n, _vp) for n in _RAW_FIELDS]


class VqvaeWeights(C.Structure):
    _fields_ = [("dims", VqvaeDims)] + [(n, _vp) for n in _PACKED_FIELDS]


_dimsp, _rawp, _wp = C.POINTER(VqvaeDims), C.POINTER(VqvaeRawWeights), C.POINTER(VqvaeWeights)

# name -> (restype, argtypes); mirrors include/vqvae_hip.h one to one
SIGNATURES = {
    "vqvae_abi_version": (_i32, []),
    "vqvae_source_fingerprint": (C.c_char_p, []),
    "vqvae_strerror": (C.c_char_p, [_i32]),
    "vqvae_profile_enable": (_i32, [_i32]),
    "vqvae_profile_collect": (_i32, [_i32, C.POINTER(C.c_double), C.POINTER(_i32)]),
    "vqvae_calibration_scratch_bytes": (_sz, []),
    "vqvae_calibration_flops": (C.c_double, [_i32]),
    "vqvae_calibration_mfma_f16": (_i32, [_i32, _vp, _sz, _vp]),
    "vqvae_vq_kernel_name": (C.c_char_p, [_i32, _i32, _i32]),
    "vqvae_vq_screen_sweeps": (_i32, [_i32, _i32, _i32]),
    "vqvae_vq_launch_form": (_i32, [_i64, _i32, _i32, _i32, _i32, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "vqvae_vq_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "vqvae_vq_forward_f32": (_i32, [_vp, _vp, _i64, _i32, _i32, _i32, _i32, _f32, _i32,
                                    _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "vqvae_vq_onehot_f32": (_i32, [_vp, _i64, _i32, _vp, _vp]),
    "vqvae_debug_row_sqnorm_f32": (_i32, [_vp, _i64, _i32, _i32, _vp, _vp]),
    "vqvae_vq_decode_indices_f32": (_i32, [_vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp]),
    "vqvae_conv_packed_bytes": (_sz, [_i32, _i32, _i32]),
    "vqvae_conv_term_products": (_i32, [_i32] * 6),
    "vqvae_conv_pack_f32": (_i32, [_i32, _vp, _i32, _i32, _vp, _vp]),
    "vqvae_conv_forward_f32": (_i32, [_i32, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "vqvae_res_layer_forward_f32": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "vqvae_res_layer_forward_ws_f32": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _sz, _vp]),
    "vqvae_res_layer_forward_hidden_f32": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "vqvae_conv_in_packed_bytes": (_sz, [_i32, _i32]),
    "vqvae_conv_in_pack_f32": (_i32, [_vp, _i32, _i32, _vp, _vp]),
    "vqvae_conv_in_forward_f32": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "vqvae_conv_taps_packed_bytes": (_sz, [_i32, _i32, _i32]),
    "vqvae_conv_taps_pack_f32": (_i32, [_vp, _i32, _vp, _vp, _i32, _i32, _vp, _vp]),
    "vqvae_conv_taps_forward_f32": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _vp]),
    "vqvae_conv_taps_forward_ep_f32": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    "vqvae_conv_forward_ep_f32": (_i32, [_i32, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "vqvae_conv_in_forward_ep_f32": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "vqvae_convt_out_packed_bytes": (_sz, [_i32, _i32]),
    "vqvae_convt_out_pack_f32": (_i32, [_vp, _i32, _i32, _vp, _vp]),
    "vqvae_convt_out_forward_f32": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "vqvae_transpose_f32": (_i32, [_vp, _i64, _i32, _i32, _vp, _vp]),
    "vqvae_vq_backward_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "vqvae_vq_backward_f32": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _f32, _i32,
                                     _vp, _vp, _vp, _sz, _vp]),
    "vqvae_vq_ema_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "vqvae_vq_ema_update_f32": (_i32, [_vp, _vp, _i64, _i32, _i32, _i32, _i32, C.c_double, C.c_double, C.c_double, _vp, _i32,
                                       _vp, _vp, _vp, _vp, _sz, _vp]),
    "vqvae_vq_ema_stats_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "vqvae_vq_ema_stats_f32": (_i32, [_vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _sz, _vp]),
    "vqvae_vq_ema_apply_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "vqvae_vq_ema_apply_f32": (_i32, [_vp, _i32, _i32, _i32, _i32, C.c_double, C.c_double, C.c_double, _vp, _vp, _vp, _vp,
                                      _vp, _sz, _vp]),
    "vqvae_vq_kmeans_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "vqvae_vq_kmeans_seed_f32": (_i32, [_vp, _i64, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _sz, _vp]),
    "vqvae_vq_kmeans_update_f32": (_i32, [_vp, _vp, _i64, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _sz, _vp]),
    "vqvae_l2norm_forward_f32": (_i32, [_vp, _i64, _i32, _i32, _i32, _f32, _i32, _vp, _vp, _vp]),
    "vqvae_l2norm_backward_f32": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _f32, _i32, _vp, _vp]),
    "vqvae_fsq_forward_f32": (_i32, [_vp] * 5 + [C.POINTER(_i32), _i32, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "vqvae_fsq_decode_indices_f32": (_i32, [_vp] * 3 + [C.POINTER(_i32), _i32, _i64, _i32, _i32, _i32, _i32, _vp, _vp]),
    "vqvae_fsq_backward_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "vqvae_fsq_backward_f32": (_i32, [_vp] * 5 + [C.POINTER(_i32), _i32, _i64, _i32, _i32, _i32, _i32] + [_vp] * 6 + [_sz, _vp]),
    "vqvae_linear_rows_forward_f32": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "vqvae_linear_rows_backward_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "vqvae_linear_rows_backward_f32": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "vqvae_vq_orthogonal_workspace_bytes": (_sz, [_i32, _i32]),
    "vqvae_vq_orthogonal_forward_f32": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "vqvae_vq_orthogonal_backward_f32": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp]),
    "vqvae_vq_entropy_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "vqvae_vq_entropy_forward_f32": (_i32, [_vp, _vp, _i64, _i32, _i32, _i32, _i32, C.c_double, C.c_double, _i32, _vp, _vp, _vp, _vp,
                                            _sz, _vp]),
    "vqvae_vq_entropy_backward_f32": (_i32, [_vp] * 5 + [_i64, _i32, _i32, _i32, _i32, C.c_double, C.c_double, _i32, _vp, _vp, _vp,
                                             _sz, _vp]),
    "vqvae_lfq_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "vqvae_lfq_forward_f32": (_i32, [_vp] * 5 + [_i32, _i64, _i32, _i32, _i32, _i32, _f32, _f32, _f32, _f32] + [_vp] * 7 + [_sz, _vp]),
    "vqvae_lfq_decode_indices_f32": (_i32, [_vp] * 3 + [_i32, _i64, _i32, _i32, _i32, _i32, _vp, _vp]),
    "vqvae_lfq_backward_f32": (_i32, [_vp] * 7 + [_i32, _i64, _i32, _i32, _i32, _i32, _f32, _f32, _f32, _f32] + [_vp] * 6 + [_sz, _vp]),
    "vqvae_vq_residual_workspace_bytes": (_sz, [_i64, _i32, _i32, _i32, _i32]),
    "vqvae_vq_residual_forward_f32": (_i32, [_vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _f32, _i32,
                                             _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "vqvae_vq_residual_decode_f32": (_i32, [_vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "vqvae_vq_residual_backward_workspace_bytes": (_sz, [_i64, _i32, _i32, _i32]),
    "vqvae_vq_residual_backward_f32": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _f32, _i32,
                                              _vp, _vp, _vp, _sz, _vp]),
    "vqvae_vq_grouped_workspace_bytes": (_sz, [_i64, _i32, _i32, _i32]),
    "vqvae_vq_grouped_forward_f32": (_i32, [_vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _f32, _i32,
                                            _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "vqvae_vq_grouped_decode_f32": (_i32, [_vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "vqvae_vq_grouped_backward_workspace_bytes": (_sz, [_i64, _i32, _i32, _i32]),
    "vqvae_vq_grouped_backward_f32": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _f32, _i32,
                                             _vp, _vp, _vp, _sz, _vp]),
    "vqvae_recon_loss_workspace_bytes": (_sz, []),
    "vqvae_recon_loss_f32": (_i32, [_vp, _vp, _i64, _f32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "vqvae_recon_loss_backward_f32": (_i32, [_vp, _vp, _i64, _f32, _vp, _vp, _vp]),
    "vqvae_conv_wgrad_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "vqvae_conv_wgrad_f32": (_i32, [_vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32,
                                    _vp, _vp, _sz, _vp]),
    "vqvae_conv_wgrad_ex_f32": (_i32, [_vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32,
                                       _vp, _vp, _sz, _vp]),
    "vqvae_bias_grad_workspace_bytes": (_sz, [_i32]),
    "vqvae_bias_grad_f32": (_i32, [_vp, _i64, _i32, _i32, _i32, _vp, _vp, _sz, _vp]),
    "vqvae_relu_backward_f32": (_i32, [_vp, _vp, _i64, _vp, _vp]),
    "vqvae_weights_packed_bytes": (_sz, [_dimsp]),
    "vqvae_weights_pack_f32": (_i32, [_dimsp, _rawp, _vp, _sz, _wp, _vp]),
    "vqvae_weights_range_check_f32": (_i32, [_dimsp, _rawp, _vp, C.POINTER(C.c_int), _vp, _sz, _vp]),
    "vqvae_workspace_bytes": (_sz, [_dimsp, _i64, _i32, _i32]),
    "vqvae_workspace_ze_offset": (_sz, [_dimsp, _i64, _i32, _i32]),
    "vqvae_resstack_f32": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "vqvae_encoder_f32": (_i32, [_wp, _vp, _i64, _i32, _i32, _vp, _vp, _sz, _vp]),
    "vqvae_decoder_f32": (_i32, [_wp, _vp, _i64, _i32, _i32, _vp, _vp, _sz, _vp]),
    "vqvae_encoder_ex_f32": (_i32, [_wp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _sz, _vp]),
    "vqvae_decoder_ex_f32": (_i32, [_wp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _sz, _vp]),
    "vqvae_forward_f32": (_i32, [_wp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _sz, _vp, _sz, _vp]),
    "vqvae_encode_f32": (_i32, [_wp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _sz, _vp, _sz, _vp]),
    "vqvae_decode_f32": (_i32, [_wp, _vp, _i64, _i32, _i32, _i32, _vp, _vp, _sz, _vp]),
    "vqvae_forward_begin_f32": (_i32, [_wp, _i64, _i32, _i32, _i32, _vp, _sz, _vp, _sz, _vp]),
    "vqvae_forward_part_f32": (_i32, [_wp, _vp, _i64, _i64, _i64, _i32, _i32, _i32, _vp, _vp, _vp, _sz, _vp, _sz, _vp]),
    "vqvae_forward_end_f32": (_i32, [_wp, _i64, _i32, _i32, _vp, _vp, _vp, _sz, _vp]),
    "vqvae_forward_abort_f32": (_i32, [_vp]),
    "vqvae_gather_rows_f32": (_i32, [_vp, _vp, _i64, _i32, _i32, _vp, _vp]),
    "vqvae_im2col_rows_f32": (_i32, [_vp, _i64, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "vqvae_gated_activation_f32": (_i32, [_vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp]),
    "vqvae_add_f32": (_i32, [_vp, _vp, _i64, _vp, _vp]),
    "vqvae_conv_taps_wgrad_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "vqvae_conv_taps_wgrad_f32": (_i32, [_vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "vqvae_conv_taps_pack_dgrad_bytes": (_sz, [_i32, _i32, _i32]),
    "vqvae_conv_taps_pack_dgrad_f32": (_i32, [_vp, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _vp, _vp]),
    "vqvae_gated_activation_backward_f32": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp]),
    "vqvae_gather_rows_backward_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "vqvae_gather_rows_backward_f32": (_i32, [_vp, _vp, _i64, _i32, _i32, _vp, _vp, _sz, _vp]),
    "vqvae_cross_entropy_workspace_bytes": (_sz, [_i64]),
    "vqvae_cross_entropy_f32": (_i32, [_vp, _vp, _i64, _i32, _vp, _vp, _sz, _vp]),
    "vqvae_cross_entropy_backward_f32": (_i32, [_vp, _vp, _i64, _i32, _vp, _vp, _vp]),
    "vqvae_bias_grad_wide_workspace_bytes": (_sz, [_i32]),
    "vqvae_bias_grad_wide_f32": (_i32, [_vp, _i64, _i32, _vp, _vp, _sz, _vp]),
    "vqvae_train_reduction_plan": (_i32, [_i32, C.POINTER(_i64), _i32, C.POINTER(_i64)]),
    "vqvae_pixelcnn_sample_packed_bytes": (_sz, [_i32, _i32, _i32, _i32]),
    "vqvae_pixelcnn_sample_pack_f32": (_i32, [C.POINTER(_vp), _i32, _i32, _i32, _i32, _i32, _vp, _sz, _vp]),
    "vqvae_pixelcnn_sample_workspace_bytes": (_sz, [_i64, _i32, _i32, _i32, _i32]),
    "vqvae_pixelcnn_sample_f32": (_i32, [_vp, _sz, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "vqvae_pixelcnn_sample_ex_f32": (_i32, [_vp, _sz, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _i32, _f32, _vp,
                                            _vp, _vp, _vp, _vp, _sz, _vp]),
    "vqvae_adam_chunk_elems": (_i32, []),
    "vqvae_adam_plan_bytes": (_sz, [_i32, C.POINTER(_i64)]),
    "vqvae_adam_plan_write": (_i32, [_i32, C.POINTER(_i64)] + [C.POINTER(_vp)] * 6 + [C.POINTER(_i32), _i32, _vp, _sz, C.POINTER(_i64)]),
    "vqvae_adam_step_f32": (_i32, [_vp, _sz, _i32, _i64, C.POINTER(VqvaeAdamGroup), _i32, _i32, _vp, _vp]),
    "vqvae_grad_norm_workspace_bytes": (_sz, [_i64]),
    "vqvae_grad_norm_f32": (_i32, [_vp, _sz, _i32, _i64, _f32, _vp, _vp, _vp, _sz, _vp]),
}

_lib = None


class VqvaeHipError(RuntimeError):
    pass


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise VqvaeHipError(
            f"{LIB_PATH} is missing: build it with `python -m vqvae_amd.build` "
            "(hipcc --offload-arch=gfx950).  There is no CPU or PyTorch fallback for this path.")
    lib = _open_checked()
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the ABI drifted
        fn.restype, fn.argtypes = res, args
    if lib.vqvae_abi_version() != 9:
        raise VqvaeHipError("libvqvae_hip.so ABI version mismatch")
    _lib = lib
    return lib


def _open_checked():
    """dlopen the in-tree library after making sure it was built from the csrc/ that lies next to it: a library left over from other
    sources (an experiment reverted without a rebuild, a checkout) is rebuilt where hipcc exists and refused where it does not --
    never silently measured or tested.  The library carries its sources' fingerprint as a marked string, read from the FILE: the
    stale one is never loaded.  Not checked: VQVAE_HIP_LIB_OVERRIDE (names an A/B build on purpose), VQVAE_HIP_TRUST_PREBUILT=1
    (a deployment that ships the built library and does not want its sources looked at), and a tree without csrc/*.hip at all
    (an installed package: there is nothing to compare with)."""
    if (os.environ.get("VQVAE_HIP_LIB_OVERRIDE") or os.environ.get("VQVAE_HIP_TRUST_PREBUILT", "0") not in ("", "0")):
        return C.CDLL(LIB_PATH)
    from . import build as _build
    if not _build.have_sources():
        return C.CDLL(LIB_PATH)
    want = _build.source_fingerprint()
    # Several ranks of one node may get here at once.  The comparison, a rebuild and the dlopen all happen under one lock, and
    # the build renames the finished file into place (build.link): nobody maps a half-written library.
    import fcntl
    try:
        lock = open(LIB_PATH + ".lock", "w")
    except OSError:                                   # read-only tree: nobody can be rebuilding it either
        lock = None
    try:
        if lock is not None:
            fcntl.flock(lock, fcntl.LOCK_EX)
        have = _build.library_fingerprint(LIB_PATH)
        if have != want:
            try:
                _build.hipcc()
            except RuntimeError:
                raise VqvaeHipError(f"{LIB_PATH} was built from other sources (fingerprint {have}, csrc/ is {want}) and hipcc is "
                                    "not here to rebuild it: run `python -m vqvae_amd.build -f` where it is, or set "
                                    "VQVAE_HIP_TRUST_PREBUILT=1 to use the library as it is") from None
            _build.build(force=True)
            if _build.library_fingerprint(LIB_PATH) != want:
                raise VqvaeHipError(f"{LIB_PATH}: rebuilt, and its fingerprint still differs from csrc/")
        return C.CDLL(LIB_PATH)
    finally:
        if lock is not None:
            fcntl.flock(lock, fcntl.LOCK_UN)
            lock.close()


ERR_UNSUPPORTED = -3      # VQVAE_ERR_UNSUPPORTED (include/vqvae_hip.h)


def check(code: int):
    if code != 0:
        raise VqvaeHipError(f"libvqvae_hip: {load().vqvae_strerror(code).decode()} (code {code})")


def dense(t, align: int = 16):
    """The tensor a raw data pointer may be taken from: `t` itself where it is contiguous and its first element lies on an
    `align`-byte boundary (the only case that costs nothing: one test on the host, no launch), else a fresh contiguous copy --
    torch's allocators hand out blocks aligned far beyond sixteen bytes.  Every front-end call that takes a tensor's data pointer
    takes it from what this returns, so a view (a slice of a batch, a parameter inside a flat buffer, a channels_last or expanded tensor) gives
    the bits its dense copy gives.  The copy is detached: it is storage for a kernel, not a node of a graph.  align: what the entry behind the call needs of this pointer (include/vqvae_hip.h, "Pointer
    contract"): 16 for the entries that refuse a narrower one, 4 or 8 for those that take an element-wise path themselves.
    None passes through."""
    if t is None or (t.is_contiguous() and not t.data_ptr() & (align - 1)):
        return t
    return t.detach().clone(memory_format=torch.contiguous_format)


class written:
    """`with written(t) as w:` -- the form of `dense` for a tensor an entry writes in place (EMA state, a codebook under EMA or
    k-means, an out=): `w` is `t` itself where `dense(t)` is, else a dense copy that is copied back into `t` with copy_ when the
    block ends without an exception.  The caller's tensor keeps its identity and its storage; where it was a view its _version
    moves, as after any in-place write."""

    def __init__(self, t, align: int = 16):
        self.t, self.w = t, dense(t, align)

    def __enter__(self):
        return self.w

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None and self.w is not self.t:
            with torch.no_grad():
                self.t.copy_(self.w)
        return False


def vq_align(D: int) -> int:
    """what vqvae_vq_forward_f32 needs of z_e and the codebook: 16 at the fixed widths (it refuses less), 4 at the others (the
    any-width kernels take their element-wise forms)"""
    return 16 if D in (32, 64, 128, 256) else 4


# ---- front-end helpers: the argument plumbing every tensor-taking wrapper shares ------------------------------------------------
# None of them launches a kernel, allocates on the device or synchronises, but for the allocation `workspace` and `like_map` exist
# to make and the min / max `check_index_range` exists to make; every pointer they hand out is taken from what `dense` returned.

def stream_ptr(t) -> int:
    """the current HIP stream of t's device, as the entries take it"""
    return torch.cuda.current_stream(t.device).cuda_stream


def check_dev(name, t, dtype=torch.float32):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise VqvaeHipError(f"{name} must be a CUDA(HIP) tensor on the GPU: the MI355X path has no CPU path and no fallback")
    if t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype} (the reference path is fp32 only)")


def ptr(t):
    """t's data pointer; None passes through (an optional argument of an entry)"""
    return None if t is None else t.data_ptr()


def ptr_array(tensors):
    """the HOST array of device pointers an entry takes for a list of tensors (read during the call only); None passes through"""
    return None if tensors is None else (C.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def ws_args(ws):
    """(pointer, bytes) of a workspace of any dtype, (None, 0) of none"""
    return (None, 0) if ws is None else (ws.data_ptr(), ws.numel() * ws.element_size())


def workspace(bytes_fn_name, what, envelope, dims, device):
    """a uint8 workspace of the size the entry `bytes_fn_name` gives for dims (a dict, in the entry's argument order); a size of 0
    says the dimensions are outside the kernels' envelope: VqvaeHipError, nothing allocated"""
    n = getattr(load(), bytes_fn_name)(*dims.values())
    if n == 0:
        raise VqvaeHipError(f"{what}: {', '.join(f'{k}={v}' for k, v in dims.items())} not supported by the gfx950 kernels ({envelope})")
    return torch.empty(n, dtype=torch.uint8, device=device)


def map_dims(name, x, rowmajor, allow_2d=False):
    """-> (B, D, H, W) of x, a device fp32 map: (B,D,H,W), or (B,H,W,D) when rowmajor.  allow_2d: a 2-D (K, D) table counts as K
    row-major rows, and the layout the entry is to be told comes back as a fifth value.  ValueError for any other rank."""
    check_dev(name, x)
    if allow_2d and x.dim() == 2:
        return x.shape[0], x.shape[1], 1, 1, True
    if x.dim() != 4:
        raise ValueError(f"{name} must be a 4-D map: (B, D, H, W), or (B, H, W, D) when rowmajor" + (", or a 2-D (K, D) tensor" * allow_2d))
    B, D, H, W = (x.shape[0], x.shape[3], x.shape[1], x.shape[2]) if rowmajor else x.shape
    return (B, D, H, W, bool(rowmajor)) if allow_2d else (B, D, H, W)


def like_map(x, C, rowmajor, bhw=None, device=None):
    """an empty fp32 tensor of x's rows and layout with C channels (x: a map, or a 2-D table); bhw: the map's (B, H, W) where x is
    no map (a decoder's indices) and gives the device alone; device: "meta" for the shape alone"""
    if bhw is not None:
        shape = (bhw[0], bhw[1], bhw[2], C) if rowmajor else (bhw[0], C, bhw[1], bhw[2])
    elif x.dim() == 2:
        shape = (x.shape[0], C)
    else:
        shape = (*x.shape[:3], C) if rowmajor else (x.shape[0], C, *x.shape[2:])
    return torch.empty(shape, dtype=torch.float32, device=device or x.device)


def check_index_range(idx, K, who):
    """IndexError unless every index lies in [0, K): the reference's embedding lookup raises on an index out of range, the kernels
    cannot (they write NaN rows and read nothing out of range).  One host sync, skipped while a graph is being captured."""
    if torch.cuda.is_current_stream_capturing():
        return
    lo, hi = int(idx.min()), int(idx.max())
    if lo < 0 or hi >= K:
        raise IndexError(f"index out of range in {who}: [{lo}, {hi}] not within [0, {K})")


def k_values(name, t, K):
    """K values in a device fp32 tensor (a draw of uniforms, one per code), dense; None passes through"""
    if t is None:
        return None
    check_dev(name, t)
    if t.numel() != K:
        raise ValueError(f"{name} must hold K = {K} values")
    return dense(t, 4)


def device_scalar(name, t):
    """one fp32 value on the device (an upstream loss gradient), dense; None passes through"""
    if t is None:
        return None
    check_dev(name, t)
    if t.numel() != 1:
        raise ValueError(f"{name} must be a scalar")
    return dense(t, 4)


def same_shape(name, t, like):
    """a device fp32 tensor of `like`'s shape (an upstream gradient), dense for an entry that picks its width by the pointer; None
    passes through"""
    if t is None:
        return None
    check_dev(name, t)
    if t.shape != like.shape:
        raise ValueError(f"{name} must have the shape {tuple(like.shape)}, got {tuple(t.shape)}")
    return dense(t, 4)


def books(codebooks, lo, hi, align):
    """-> the dense (K, D) codebooks of a residual or grouped quantizer: a sequence of tensors, one (K, D) tensor, or one (n, K, D)
    tensor; between lo and hi (None: no bound) of them, all device fp32 of one shape"""
    if isinstance(codebooks, torch.Tensor):
        codebooks = [codebooks] if codebooks.dim() == 2 else list(codebooks.unbind(0))
    out = list(codebooks)
    if len(out) < lo or (hi is not None and len(out) > hi):
        raise ValueError(f"{len(out)} codebooks: at least {lo}" + (f" and at most {hi}" if hi is not None else ""))
    for i, c in enumerate(out):
        check_dev(f"codebooks[{i}]", c)
        if c.dim() != 2 or c.shape != out[0].shape:
            raise ValueError("every codebook must be (K, D) with the same K and D")
    return [dense(c, align) for c in out]


def vq_kernel_name(K: int, D: int, flags: int = 0x1) -> str:
    """kernel vqvae_vq_forward_f32 launches for this shape (default flags: row-major rows, the fused path's layout)"""
    return load().vqvae_vq_kernel_name(K, D, flags).decode()


def vq_sweeps(K: int, D: int, flags: int = 0x1) -> int:
    return load().vqvae_vq_screen_sweeps(K, D, flags)


def vq_launch_form(n_rows: int, K: int, D: int, HW: int = 64, flags: int = 0x1):
    """(waves per CU, rows per unit, pooled tail units in per cent) of vq_track_kernel_d64 for this problem on the current device,
    or None where another kernel runs"""
    w, r, p = _i32(), _i32(), _i32()
    if load().vqvae_vq_launch_form(n_rows, K, D, HW, flags, C.byref(w), C.byref(r), C.byref(p)) != 0:
        return None
    return w.value, r.value, p.value


def vq_kernel_instance(n_rows: int, K: int, D: int, HW: int = 64, flags: int = 0x1) -> str:
    """the kernel's name with the template instance that runs for n_rows rows, e.g. vq_track_kernel_d64<16, false, 1>"""
    name = vq_kernel_name(K, D, flags)
    f = vq_launch_form(n_rows, K, D, HW, flags)
    if f is None:
        return name
    # (codebooks of exactly sixteen 32-code tiles, K in 481 .. 512, run instances with the sweep fully unrolled -- every launch form
    # but 64-row units on eight waves of row-major rows, which the rule no longer picks for such codebooks)
    unrolled = ", 16" if 480 < K <= 512 and not (f[0] == 8 and f[1] == 64 and flags & 0x1) and f[0] != 12 else ""
    return f"{name}<{f[0]}, {'false' if flags & 0x1 else 'true'}, {f[1] // 32}{unrolled}>" + (f" (last {f[2]} % of the units pooled)" if f[2] else "")


TRAIN_PLANS = {"conv_wgrad": 0, "conv_taps_wgrad": 1, "bias_grad": 2, "bias_grad_wide": 3, "segsum": 4}   # VQVAE_TRAIN_PLAN_*
TRAIN_KERNELS = [None, "conv_wgrad_img", "conv_wgrad_map8_h2", "conv_wgrad_map8", "conv_wgrad", "taps_wgrad_map", "taps_wgrad_blk",
                 "bias_grad", "bias_grad_wide", "segsum"]                                                  # VQVAE_TRAIN_KERNEL_*
TrainPlan = collections.namedtuple("TrainPlan", "kernel items splits per_split last want aux0 aux1")


def train_reduction_plan(what: str, *dims):
    """what a training reduction would launch for these dimensions (vqvae_train_reduction_plan in include/vqvae_hip.h lists them
    per reduction; a tap list is passed as its dy values, then its dx values), or None where the entry point refuses them"""
    d, out = (_i64 * len(dims))(*dims), (_i64 * 8)()
    if load().vqvae_train_reduction_plan(TRAIN_PLANS[what], d, len(dims), out) != 0:
        return None
    return TrainPlan(TRAIN_KERNELS[out[0]], *out[1:])


PROF_IDS = {"vq_main": 0, "conv_igemm": 1, "res_layer": 2, "conv_in": 3, "conv_out": 4}


def profile_enable(on: bool):
    check(load().vqvae_profile_enable(1 if on else 0))


def profile_collect(name: str):
    """-> (total_ms, launches) of one instrumented kernel since the last collect (synchronises)."""
    ms, n = C.c_double(), _i32()
    check(load().vqvae_profile_collect(PROF_IDS[name], C.byref(ms), C.byref(n)))
    return ms.value, n.value
