"""Every kernel under vqvae_amd/csrc whose work loop depends on gridDim.x, with the launch cap of its grid and the test that runs it past
that cap (tests/test_grid_caps_cpu.py keeps this table complete and live, tests/test_grid_caps_gpu.py holds the covering tests that
did not exist before)  --  TEST INFRASTRUCTURE ONLY; nothing under vqvae_amd/ imports it.

Most elementwise, gather and pack kernels launch min(ceil(units / 256), cap) workgroups of 256 threads and walk the rest of their
units in a `+= gridDim.x * 256` loop.  At small shapes every thread runs that loop body once: the stride, the 64-bit index of the
second lap, the ragged end of the last lap and the `blockIdx.x == 0` tail loops are reached only past cap * 256 units.  A row says
where that is and which test goes there.

Row fields
  kernel     the function that holds the gridDim.x expression: a __global__ kernel, or the header body several kernels wrap
  file       its source file under vqvae_amd/csrc
  entries    the C entries that launch it
  cap        workgroups: a number; CUS (a persistent grid sized from the CU count, `formula` says how); UNREACHABLE (the loop cannot
             lap inside the entry's accepted envelope, `proof` is the arithmetic); NO_LOOP (gridDim.x only decodes a 2-D grid)
  formula    the grid as the host code computes it
  unit       what one thread handles per lap
  anchors    (file, literal source text) of the clamp and of the constants behind it: a retuned cap breaks the anchor, and the CPU test
             then names the row that lost its purpose
  covers     Cover(node, units, elements): the pytest node id of a test past the cap, the units its shape gives the loop, and for
             kernels with a scalar tail behind 4-wide laps the element count (which must not be a multiple of 4).  For CUS rows
             `units` are the blocks / tiles the shape yields and `elements` the workgroups of the grid at 256 CUs.
  aligned    the unit count is a multiple of 256 by construction (padded operand images): the last lap can be partial, but never
             ends inside a workgroup

The shapes of the new tests live here (the GPU tests import them); the shapes of older tests are imported from their modules."""
import collections

CUS, UNREACHABLE, NO_LOOP = "cus", "unreachable", "no_loop"
NUM_CUS = 256                                    # MI355X, unpartitioned
WG = 256                                         # threads per workgroup of every capped kernel

Row = collections.namedtuple("Row", "kernel file entries cap formula unit anchors covers aligned proof note")
Cover = collections.namedtuple("Cover", "node units elements")


def cdiv(a, b):
    return -(-a // b)


def row(kernel, file, entries, cap, formula, unit, anchors, covers=(), aligned=False, proof=None, note=""):
    return Row(kernel, file, tuple(entries), cap, formula, unit, tuple(anchors), tuple(covers), aligned, proof, note)


def wraps_at(r):
    """the smallest unit count that gives some thread a second lap"""
    return r.cap * WG + 1


NEW = "tests/test_grid_caps_gpu.py::"
GRID_OF = ("common.h", "inline unsigned grid_of(long long total, long long cap = 65536) {")

# ------------------------------------------------------------------------------------------------- shapes of the new GPU tests
# training.vq_backward -> vqb_gradz_kernel: id -> (B, D, H, W, K, rowmajor, displaced); displaced: z_e starts one float past a
# 16-byte boundary, which sends D % 4 == 0 rows down the element path
VQB = {
    "rows_vec4": (16777805, 4, 1, 1, 3, True, False),
    "rows_element_path": (4194454, 4, 1, 1, 3, True, True),
    "nchw": (1118482, 3, 1, 5, 3, False, False),
}


def vqb_units(B, D, H, W, K, rowmajor, displaced):
    total = B * H * W * D
    return total // 4 if rowmajor and D % 4 == 0 and not displaced else total


# the codebook gradient's sorted segmented sum -> segsum_keys_kernel, one row per unit: (B, D, H, W, K)
SEGSUM_VQ = (1048909, 4, 1, 1, 3)
# pixelcnn.gather_rows_backward -> the same kernel: (n, rows, C)
SEGSUM_GATHER = (1048909, 7, 4)
SUM_PATTERNS = ("random", "spike")               # spike: one value 10^6 times the rest, in the second lap's range
# training.step_losses: elements of x_hat; the forward's partial sums (4-wide laps + a scalar tail) and the backward (elements)
RECON_FORWARD = 1049623
RECON_PATTERNS = ("random", "spike", "tail_spike")  # tail_spike: the large value is the last element, in block 0's scalar tail
RECON_BACKWARD = 16777516
RELU_BACKWARD = 67109926                         # autograd_conv.relu_backward: 4-wide laps + a scalar tail
ORTH_BACKWARD = (4099, 128)                      # functional.vq_orthogonal_backward: (K, D)
# training.vq_backward(rotation=True) -> rot_gradz_body, one ROW per unit: id -> (B, D, H, W, K, rowmajor)
ROT = {
    "rows_vec4": (16777486, 4, 1, 1, 5, True),
    "rows_element": (16777486, 1, 1, 1, 5, True),
    "nchw": (2396746, 1, 1, 7, 5, False),
}
ONEHOT = (349700, 3)                             # functional.vq_onehot: (N, K)
DECODE_INDICES = (69940, 3, 1, 5, 5)             # functional.vq_decode_indices: (B, D, H, W, K)
# VQVAE.decode_indices on maps without the gathering decoder kernel -> decode_gather_kernel (rows * D elements) and, for the
# per-image maxima of 6 B ints, fill_words_kernel: (h_dim, res_h, n_res, K, D, B, h4, w4)
DECODE_MODEL = (32, 8, 2, 5, 20, 52441, 4, 4)
# one image whose z_q has more than 64 * 16384 4-vectors -> act_absmax_kernel past its 64 parts per image:
# (h_dim, res_h, n_res, K, D, h4, w4); where the maximum sits: id -> (latent pixel, channel)
ABSMAX_MODEL = (128, 32, 2, 8, 52, 143, 142)
ABSMAX_AT = {"last_lap": (20200, 0), "last_vector": (143 * 142 - 1, 51)}
# the GatedPixelCNN helpers (pixelcnn._gather_rows, _im2col, _gate, _add)
PRIOR_GATHER = (16777486, 7, 4)                  # (n, rows, C): n * C / 4 units
PRIOR_IM2COL = (199729, 1, 3, 4, "t28")          # (B, H, W, C, taps): B H W * taps * C / 4 units
PRIOR_GATE = (1118482, 5, 3)                     # (B, HW, dim): B HW dim units
PRIOR_ADD = 67109924                             # elements, n / 4 units
RES_COMBINE = (4, 4, 32769, 8, 8)                # conv_hip.res_layer outside the fused widths: (C, Rh, B, H, W), B H W C / 4 units
# weight images.  conv_in: (Cin, Cout, B, H, W); convt_out: (Cin, Cout, B, H, W); conv: (kind, Cin, Cout, B, H, W)
CONV_IN_PACK = (3, 96, 1, 8, 8)
CONVT_OUT_PACK = (160, 3, 1, 4, 4)
CONV_PACK = ("conv3x3", 352, 352, 1, 4, 4)
TAPS_DGRAD = (1, 4, 252, 504, "t28")             # pixelcnn.taps_dgrad: (B, side, Cin, Cout, taps) -> taps_transpose_kernel per slice
TAPS_WGRAD = (2, 4, 4, 204, 188, "t28")          # pixelcnn.taps_wgrad: (B, H, W, Cin, Cout, taps) -> split_reduce_kernel
SAMPLE_PACK = (8, 252, 1, 2, 4, 8, None)         # a SAMPLE_CASES row of tests/pixelcnn_envelope.py: K, dim, layers, classes, B, side
VQ_ANYD = (5, 3, 70003, 1, 1, 1.0)               # test_vq_generic_matches_oracle_fresh's (K, D, B, H, W, scale)


def conv_in_pack_units(Cin, Cout):
    """conv_in_pack_kernel: n_tile * ceil(8 Cin / 4) * 256 floats; conv_in_pack_bf3_kernel: n_tile * Cin * 512 bf16 triples;
    conv_in_pack_h2_kernel: n_tile * Cin * 64 lanes"""
    nt = cdiv(Cout, 32)
    return nt * cdiv(8 * Cin, 4) * 256, nt * Cin * 512, nt * Cin * 64


def convt_out_pack_units(Cin, Cout):
    """convt_out_pack_kernel and convt_out_pack_bf3_kernel: ceil(Cin / 32) * ceil(16 Cout / 32) * 1024"""
    return cdiv(Cin, 32) * cdiv(16 * Cout, 32) * 1024


def conv_pack_units(kind, Cin, Cout):
    """packed_floats of conv_host.h for the one-phase kinds: taps * ceil(Cin / 32) * ceil(Cout / 32) * 1024"""
    taps = {"conv3x3": 9, "conv1x1": 1, "convT3x3": 9}[kind]
    return taps * cdiv(Cin, 32) * cdiv(Cout, 32) * 1024


def taps_slice(ntaps):
    """taps per launch of conv_hip.conv_taps / pixelcnn.taps_dgrad: slices of at most 16"""
    return cdiv(ntaps, cdiv(ntaps, 16))


def sample_pack_units(K, dim, nl, ncls):
    """the largest (O, T, Cin) copy of vqvae_pixelcnn_sample_pack_f32: layer 0's vertical stack, 21 of its 28 taps"""
    return 2 * dim * 21 * dim


def absmax_units(D, h4, w4):
    return h4 * w4 * D // 4


# envelope constants the UNREACHABLE proofs and the pack rows rest on (each stands in an anchor of its row)
CONV_IN_MAX_CIN, CONV_IN_MAX_COUT = 4, 128       # vqvae_conv_in_packed_bytes


# --------------------------------------------------------------------------------------------------------- older tests' shapes
def _residual_cap_units():
    from tests import test_vq_residual_gpu as T
    B, H, W, D, K = T.CAP_SHAPE
    return B * H * W * D


def _grouped_cap_units():
    from tests import test_vq_grouped_gpu as T
    K, D, G, B, H, W = T.CAP_SHAPE
    return B * H * W * D // 4


def _grouped_covers():
    """the 4-wide form on CAP_SHAPE's row-major rows (its NCHW case runs element by element too, but 256 channels end every lap
    on a workgroup boundary); the element path on CAP_SHAPE_ELEMENT in both layouts"""
    from tests import test_vq_grouped_gpu as T
    K, D, G, B, H, W = T.CAP_SHAPE_ELEMENT
    node = "tests/test_vq_grouped_gpu.py::test_grid_stride_past_the_launch_cap"
    return [Cover(node + "[True]", _grouped_cap_units(), None)] + [Cover(node + f"_element_path[{rm}]", B * H * W * D, None) for rm in (False, True)]


def _grouped_cap_rows():
    from tests import test_vq_grouped_gpu as T
    K, D, G, B, H, W = T.CAP_SHAPE
    return B * H * W, K, D // G


def _headline(i):
    from tests import test_vq_gpu as T
    B, H, W = T.HEADLINE_SHAPES[i]
    return B * H * W, H * W


def _groups_rows():
    from tests import test_vq_gpu as T
    return T.GROUPS_CASE[2]


def _full_size(name):
    from tests import test_model_gpu as T
    return {c[0]: c for c in T.FULL_SIZE_CONFIGS}[name]


# (waves per workgroup, rows per unit) of every launch form vq_track_form can choose (vq_track.hip)
TRACK_FORMS = ((16, 32), (12, 32), (8, 32), (8, 64), (4, 32))


def track_blocks(n_rows):
    """vq_track_form: units of unit_rows rows, `waves` of them per workgroup -> (workgroups needed, grid at 256 CUs) for the form
    that needs the FEWEST workgroups: which form runs depends on the device's CU count, and the figure here must not"""
    need = min(cdiv(cdiv(n_rows, unit_rows), waves) for waves, unit_rows in TRACK_FORMS)
    return need, min(need, NUM_CUS, 1024)


def _cus_covers():
    n_rag, hw_rag = _headline(1)
    need, grid = track_blocks(n_rag)
    n_grp, K_grp, d_grp = _grouped_cap_rows()
    slab = min(n_grp, 1 << 18)
    n17 = _groups_rows()
    c4 = _full_size("c4")
    tiles = c4[1] * cdiv(c4[2] // 2, 14) ** 2                 # B * 14 x 14 tiles of the (S / 2) x (S / 2) map the last layer reads
    return {
        "vq_track_kernel_d64": [Cover("tests/test_vq_gpu.py::test_vq_headline_size_bit_exact_vs_oracle[ragged_132300rows]", need, grid)],
        "vq_filter_kernel_d64": [Cover("tests/test_vq_gpu.py::test_vq_headline_size_bit_exact_vs_oracle[ragged_132300rows]",
                                       cdiv(n_rag, 512), min(cdiv(n_rag, 512), NUM_CUS))],
        "vq_exact_kernel": [Cover("tests/test_vq_gpu.py::test_vq_stream_more_than_one_group_of_slabs_equals_the_exhaustive_kernel",
                                  cdiv(n17, 512), min(cdiv(n17, 512), NUM_CUS))],
        "vq_stream_sweep_kernel": [Cover("tests/test_vq_grouped_gpu.py::test_grid_stride_past_the_launch_cap[True]",
                                         cdiv(slab, 512), min(cdiv(slab, 512), NUM_CUS))],
        "vq_stream_gather_kernel": [Cover("tests/test_vq_grouped_gpu.py::test_grid_stride_past_the_launch_cap[True]",
                                          cdiv(n_grp, 1024 // (d_grp // 4)), min(cdiv(n_grp, 2 * (1024 // (d_grp // 4))), 2 * NUM_CUS))],
        "vq_anyd_kernel": [Cover(NEW + "test_any_width_quantizers_lap_their_persistent_grids[mfma_fp32]",
                                 cdiv(VQ_ANYD[2] * VQ_ANYD[3] * VQ_ANYD[4], 64), 4 * NUM_CUS)],
        "vq_generic_kernel": [Cover(NEW + "test_any_width_quantizers_lap_their_persistent_grids[vector_units]",
                                    cdiv(VQ_ANYD[2] * VQ_ANYD[3] * VQ_ANYD[4], 8), 8 * NUM_CUS)],
        "convt_out_kernel": [Cover("tests/test_model_gpu.py::test_baseline_configs_4_and_5_at_full_size_properties[c4-512-224-1024-64]",
                                   tiles, 2 * NUM_CUS)],
    }


# -------------------------------------------------------------------------------------------------------------------- the table
def rows():
    cus = _cus_covers()
    B_, D_, H_, W_, K_ = SEGSUM_VQ
    r = [
        # ---- train.hip
        row("vqb_gradz_kernel", "train.hip", ["vqvae_vq_backward_f32"], 65536, "grid_of(vec4 ? total >> 2 : total)",
            "4 channels of a row-major row (D % 4 == 0, aligned tensors), else one element (row-major or NCHW)",
            [("train.hip", "hipLaunchKernelGGL(vqb_gradz_kernel, dim3(grid_of(vec4 ? total >> 2 : total)), dim3(256)"), GRID_OF],
            [Cover(NEW + f"test_vq_backward_grad_z[{k}]", vqb_units(*v), None) for k, v in VQB.items()]),
        row("recon_partial_kernel", "train.hip", ["vqvae_recon_loss_f32"], 1024, "grid_of(n >> 2, kReconGrid)",
            "a 4-vector; block 0 adds the n % 4 tail",
            [("train.hip", "constexpr int kReconGrid = 1024;"), ("train.hip", "const unsigned grid = grid_of(n >> 2, kReconGrid);")],
            [Cover(NEW + f"test_step_losses_forward[{p}]", RECON_FORWARD // 4, RECON_FORWARD) for p in RECON_PATTERNS]),
        row("recon_backward_kernel", "train.hip", ["vqvae_recon_loss_backward_f32"], 65536, "grid_of(n)", "an element",
            [("train.hip", "hipLaunchKernelGGL(recon_backward_kernel, dim3(grid_of(n)), dim3(256)"), GRID_OF],
            [Cover(NEW + "test_step_losses_backward", RECON_BACKWARD, None)]),
        # ---- train_reduce.hip
        row("segsum_keys_kernel", "train_reduce.hip",
            ["vqvae_vq_backward_f32", "vqvae_vq_ema_update_f32", "vqvae_gather_rows_backward_f32", "vqvae_vq_residual_backward_f32",
             "vqvae_vq_grouped_backward_f32"], 4096, "grid_of(n, 4096)", "a row (its sort key and value)",
            [("train_reduce.hip", "hipLaunchKernelGGL(segsum_keys_kernel, dim3(grid_of(n, 4096)), dim3(256)")],
            [Cover(NEW + f"test_vq_backward_codebook_gradient[{p}]", B_ * H_ * W_, None) for p in SUM_PATTERNS] +
            [Cover(NEW + f"test_gather_rows_backward[{p}]", SEGSUM_GATHER[0], None) for p in SUM_PATTERNS]),
        row("split_reduce_kernel", "train_reduce.hip", ["vqvae_conv_wgrad_ex_f32", "vqvae_conv_taps_wgrad_f32"], 4096,
            "grid_of(ntap * CA * CB, 4096)", "an element of the weight gradient",
            [("train_reduce.hip", "hipLaunchKernelGGL(split_reduce_kernel, dim3(grid_of((long long)ntap * CA * CB, 4096)), dim3(256)")],
            [Cover(NEW + "test_taps_weight_gradient_split_reduce", 28 * TAPS_WGRAD[3] * TAPS_WGRAD[4], None)],
            note="reachable: 28 taps of a 204 -> 188 masked conv are 1 073 856 elements; the entries bound neither width"),
        # ---- backward.hip
        row("relu_backward_kernel", "backward.hip", ["vqvae_relu_backward_f32"], 65536, "grid_of(n >> 2)",
            "a 4-vector; block 0 handles the n % 4 tail",
            [("backward.hip", "hipLaunchKernelGGL(relu_backward_kernel, dim3(grid_of(n >> 2)), dim3(256)"), GRID_OF],
            [Cover(NEW + "test_relu_backward", RELU_BACKWARD // 4, RELU_BACKWARD)]),
        # ---- vq_orthogonal.hip / .h
        row("orth_backward_kernel", "vq_orthogonal.hip", ["vqvae_vq_orthogonal_backward_f32"], 2048, "grid_of(K * D, 2048)",
            "an element (orth_backward_body of vq_orthogonal.h strides by the grid size it is handed)",
            [("vq_orthogonal.hip", "hipLaunchKernelGGL(orth_backward_kernel, dim3(grid_of((long long)K * D, 2048)), dim3(kOrthThreads)"),
             ("vq_orthogonal.hip", "orth_backward_body(saved, selected, count, grad_loss, K, D, grad_rows, gridDim.x);"),
             ("vq_orthogonal.h", "step = (size_t)nblocks * kOrthThreads;"), ("vq_orthogonal.h", "constexpr int kOrthThreads = 256;")],
            [Cover(NEW + "test_orthogonal_backward", ORTH_BACKWARD[0] * ORTH_BACKWARD[1], None)]),
        # ---- vq_residual.h (rvq_advance_kernel, rvq_finish_kernel, rvq_gradz_kernel of vq_residual.hip wrap it)
        row("rvq_walk", "vq_residual.h", ["vqvae_vq_residual_forward_f32", "vqvae_vq_residual_decode_f32", "vqvae_vq_residual_backward_f32"],
            65536, "grid_of(total >> 2) 4-wide, grid_of(total) element by element", "4 elements, or one",
            [("vq_residual.hip", "if (VEC) hipLaunchKernelGGL(KERNEL<4>, dim3(grid_of((A).total >> 2)), dim3(256)"),
             ("vq_residual.hip", "else hipLaunchKernelGGL(KERNEL<1>, dim3(grid_of((A).total)), dim3(256)"), GRID_OF],
            [Cover("tests/test_vq_residual_gpu.py::test_grid_stride_past_the_launch_cap", _residual_cap_units(), None),
             Cover("tests/test_vq_residual_gpu.py::test_grid_stride_past_the_launch_cap_4_wide", RVQ_WIDE_UNITS(), None),
             Cover("tests/test_vq_residual_gpu.py::test_grid_stride_past_the_launch_cap_4_wide_codebooks", RVQ_WIDE_UNITS(), None)]),
        # ---- vq_grouped.h (grp_split_kernel, grp_finish_kernel, grp_gradz_kernel of vq_grouped.hip wrap them)
        row("grp_split_body", "vq_grouped.h", ["vqvae_vq_grouped_forward_f32", "vqvae_vq_grouped_backward_f32"], 65536,
            "grid_of(total >> 2) 4-wide, grid_of(total) element by element", "4 elements, or one",
            [("vq_grouped.hip", "if (vec) hipLaunchKernelGGL((grp_split_kernel<4, unsigned>), dim3(grid_of(a.total >> 2)), dim3(256)"),
             ("vq_grouped.hip", "else hipLaunchKernelGGL((grp_split_kernel<1, unsigned>), dim3(grid_of(a.total)), dim3(256)"), GRID_OF],
            _grouped_covers()),
        row("grp_walk", "vq_grouped.h", ["vqvae_vq_grouped_forward_f32", "vqvae_vq_grouped_decode_f32", "vqvae_vq_grouped_backward_f32"],
            65536, "grid_of(total >> 2) 4-wide, grid_of(total) element by element", "4 elements, or one",
            [("vq_grouped.hip", "if (VEC) hipLaunchKernelGGL((KERNEL<4, unsigned>), dim3(grid_of((A).total >> 2)), dim3(256)"),
             ("vq_grouped.hip", "else hipLaunchKernelGGL((KERNEL<1, unsigned>), dim3(grid_of((A).total)), dim3(256)"), GRID_OF],
            _grouped_covers()),
        # ---- vq_rotation.h (vq_rotation_gradz_kernel of vq_rotation.hip wraps it)
        row("rot_gradz_body", "vq_rotation.h", ["vqvae_vq_backward_f32"], 65536, "grid_of(N)", "a row of D channels",
            [("vq_rotation.hip", "const dim3 grid(grid_of(a.N)), block(256);"), GRID_OF],
            [Cover(NEW + f"test_rotation_gradient[{k}]", v[0] * v[2] * v[3], None) for k, v in ROT.items()]),
        # ---- vq_exact.hip
        row("vq_onehot_kernel", "vq_exact.hip", ["vqvae_vq_onehot_f32"], 4096, "min(ceil(N K / 256), 256 * 16)", "an element",
            [("vq_exact.hip", "if (grid > 256 * 16) grid = 256 * 16;\n    hipLaunchKernelGGL(vq_onehot_kernel,")],
            [Cover(NEW + "test_onehot", ONEHOT[0] * ONEHOT[1], None)]),
        row("vq_decode_indices_kernel", "vq_exact.hip", ["vqvae_vq_decode_indices_f32"], 4096, "min(ceil(B D H W / 256), 256 * 16)",
            "an element",
            [("vq_exact.hip", "if (grid > 256 * 16) grid = 256 * 16;\n    hipLaunchKernelGGL(vq_decode_indices_kernel,")],
            [Cover(NEW + "test_decode_indices", DECODE_INDICES[0] * DECODE_INDICES[1] * DECODE_INDICES[2] * DECODE_INDICES[3], None)]),
        row("fill_words_kernel", "vq_exact.hip", ["vqvae_decode_f32", "vqvae_forward_f32", "vqvae_encoder_f32", "vqvae_decoder_f32",
                                                  "vqvae_vq_forward_f32"], 1024, "grid_of(bytes / 4, 1024)", "a 32-bit word",
            [("vq_exact.hip", "hipLaunchKernelGGL(fill_words_kernel, dim3(grid_of((long long)n, 1024)), dim3(256)")],
            [Cover(NEW + "test_decode_gathers_rows_and_clears_maxima", cdiv((4 + DECODE_MODEL[2]) * DECODE_MODEL[5] * 4, 256) * 64, None)],
            note="the largest clears are the per-image maxima of the layerwise whole path: (4 + n_res) ints per image, 256-byte aligned.  "
                 "A maximum that is not cleared makes its consumer form fp16 operand terms unscaled, so the covering test's "
                 "activations lie beyond fp16's range: a lost lap gives infinities"),
        row("vq_exact_kernel", "vq_exact.hip", ["vqvae_vq_forward_f32"], CUS, "min(ceil(N / (256 rt)), CUs), rt = 2 from 1024 CUs' rows on",
            "a block of 256 rt rows", [("vq_exact.hip", "long long grid = nblocks < cus ? nblocks : cus;")], cus["vq_exact_kernel"]),
        # ---- vq_filter.hip, vq_track.hip, vq_chunk.hip, vq_generic.hip: persistent quantizers
        row("vq_filter_kernel_d64", "vq_filter.hip", ["vqvae_vq_forward_f32"], CUS, "min(ceil(N / 512), CUs)", "a 512-row super-block",
            [("vq_filter.hip", "long long grid = nblocks < (long long)cus * per_cu ? nblocks : (long long)cus * per_cu;")],
            cus["vq_filter_kernel_d64"]),
        row("vq_track_kernel_d64", "vq_track.hip", ["vqvae_vq_forward_f32", "vqvae_forward_f32", "vqvae_encode_f32"], CUS,
            "min(ceil(units / waves), CUs), units of 32 or 64 rows (vq_track_form)", "a unit per wave",
            [("vq_track.hip", "if (grid > cus) grid = cus;")], cus["vq_track_kernel_d64"]),
        row("vq_stream_sweep_kernel", "vq_chunk.hip", ["vqvae_vq_forward_f32"], CUS, "min(ceil(slab rows / 512), CUs) per slab of 2^18 rows",
            "a 512-row block", [("vq_chunk.hip", "dim3(nblk < cus ? nblk : cus), dim3(512)")], cus["vq_stream_sweep_kernel"]),
        row("vq_stream_resolve_kernel", "vq_chunk.hip", ["vqvae_vq_forward_f32"], CUS, "4 CUs",
            "an open (row, tile) pair per thread, a hard row per wave: counts that depend on the data, not on the shape",
            [("vq_chunk.hip", "hipLaunchKernelGGL(vq_stream_resolve_kernel<D>, dim3(4 * cus), dim3(256)")],
            [Cover("tests/test_vq_gpu.py::test_vq_stream_more_than_one_group_of_slabs_equals_the_exhaustive_kernel", None, 4 * NUM_CUS)],
            note="its loops run over the open pairs and hard rows the sweep leaves (a few thousand per slab): no shape forces a second "
                 "lap of 4 CUs * 256 threads; the named test is the one with the most of them (4.4 M rows, planted near-ties)"),
        row("vq_stream_gather_kernel", "vq_chunk.hip", ["vqvae_vq_forward_f32"], CUS, "min(ceil(N / (2 rows per pass)), 2 CUs)",
            "ceil(passes / grid) consecutive passes of 1024 / (D / 4) rows per workgroup",
            [("vq_chunk.hip", "if (g > 2 * cus) g = 2 * cus;")], cus["vq_stream_gather_kernel"]),
        row("vq_generic_kernel", "vq_generic.hip", ["vqvae_vq_forward_f32"], CUS, "min(ceil(N / 8), 8 CUs, 4096)", "a tile of 8 rows",
            [("vq_generic.hip", "long long grid = ntiles < 8LL * num_cus() ? ntiles : 8LL * num_cus();")], cus["vq_generic_kernel"]),
        row("vq_anyd_kernel", "vq_generic.hip", ["vqvae_vq_forward_f32"], CUS, "min(ceil(N / 64), per_cu CUs, 4096), per_cu = 4 / 2 / 1 by LDS",
            "a tile of 64 rows",
            [("vq_generic.hip", "long long grid = ntiles < per_cu * num_cus() ? ntiles : per_cu * num_cus();")], cus["vq_anyd_kernel"]),
        # ---- model.hip
        row("decode_gather_kernel", "model.hip", ["vqvae_decode_f32"], 65536, "min(ceil(rows D / 256), 65536)", "an element",
            [("model.hip", "dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256)")],
            [Cover(NEW + "test_decode_gathers_rows_and_clears_maxima", DECODE_MODEL[5] * DECODE_MODEL[6] * DECODE_MODEL[7] * DECODE_MODEL[4], None)]),
        # ---- pixelcnn.hip
        row("gather_rows_kernel", "pixelcnn.hip", ["vqvae_gather_rows_f32"], 65536, "grid_for(n * (C / 4))", "a 4-vector",
            [("pixelcnn.hip", "if (g > 65536) g = 65536;"), ("pixelcnn.hip", "hipLaunchKernelGGL(gather_rows_kernel, dim3(grid_for(n * (C / 4))), dim3(256)")],
            [Cover(NEW + "test_prior_gather_rows", PRIOR_GATHER[0] * PRIOR_GATHER[2] // 4, None)]),
        row("im2col_rows_kernel", "pixelcnn.hip", ["vqvae_im2col_rows_f32"], 65536, "grid_for(B * H * W * ntaps * (C / 4))", "a 4-vector",
            [("pixelcnn.hip", "if (g > 65536) g = 65536;"),
             ("pixelcnn.hip", "hipLaunchKernelGGL(im2col_rows_kernel, dim3(grid_for(B * H * W * ntaps * (C / 4))), dim3(256)")],
            [Cover(NEW + "test_prior_im2col", PRIOR_IM2COL[0] * PRIOR_IM2COL[1] * PRIOR_IM2COL[2] * 28 * PRIOR_IM2COL[3] // 4, None)]),
        row("gated_activation_kernel", "pixelcnn.hip", ["vqvae_gated_activation_f32"], 65536, "grid_for(B * HW * dim)", "an element",
            [("pixelcnn.hip", "if (g > 65536) g = 65536;"),
             ("pixelcnn.hip", "hipLaunchKernelGGL(gated_activation_kernel, dim3(grid_for(B * HW * dim)), dim3(256)")],
            [Cover(NEW + "test_prior_gate", PRIOR_GATE[0] * PRIOR_GATE[1] * PRIOR_GATE[2], None)]),
        row("add_kernel", "pixelcnn.hip", ["vqvae_add_f32"], 65536, "grid_for(n / 4)", "a 4-vector",
            [("pixelcnn.hip", "if (g > 65536) g = 65536;"), ("pixelcnn.hip", "hipLaunchKernelGGL(add_kernel, dim3(grid_for(n / 4)), dim3(256)")],
            [Cover(NEW + "test_prior_add", PRIOR_ADD // 4, None)]),
        # ---- pixelcnn_backward.hip, pixelcnn_sample.hip
        row("taps_transpose_kernel", "pixelcnn_backward.hip", ["vqvae_conv_taps_pack_dgrad_f32"], 4096, "grid_of(Cin * Cout * ntaps, 4096)",
            "an element of a slice's staged weight",
            [("pixelcnn_backward.hip", "hipLaunchKernelGGL(taps_transpose_kernel, dim3(grid_of((long long)Cin * Cout * ntaps, 4096)), dim3(256)")],
            [Cover(NEW + "test_taps_data_gradient_staging", TAPS_DGRAD[2] * TAPS_DGRAD[3] * taps_slice(28), None)]),
        row("pixelcnn_sample_pack_kernel", "pixelcnn_sample.hip", ["vqvae_pixelcnn_sample_pack_f32"], 4096, "min(ceil(O T Cin / 256), 4096)",
            "an element of a weight copy", [("pixelcnn_sample.hip", "grid = grid > 4096 ? 4096 : grid;")],
            [Cover(NEW + "test_sampler_weight_image", sample_pack_units(*SAMPLE_PACK[:4]), None)]),
        # ---- conv.hip
        row("act_absmax_kernel", "conv.hip", ["vqvae_decode_f32", "vqvae_decoder_f32", "vqvae_forward_f32", "vqvae_encoder_f32"], 64,
            "(min(ceil(elements / 16384), 64), B): parts per image", "a 4-vector of one image",
            [("conv.hip", "parts = parts < 1 ? 1 : (parts > 64 ? 64 : parts);"),
             ("conv.hip", "long long parts = (elems_per_image + 256 * 4 * 16 - 1) / (256 * 4 * 16);"),
             ("conv.hip", "if (Cin % 4) return VQVAE_ERR_UNSUPPORTED;          // float4 activation loads")],
            [Cover(NEW + f"test_image_maximum_in_the_last_lap[{k}]", absmax_units(*ABSMAX_MODEL[4:]), None) for k in ABSMAX_AT],
            note="below the cap every image already takes 16 laps of its parts: the row is about more than 16.  The kernel's scalar "
                 "tail (elements % 4) cannot run: both callers measure maps of pixels x channels whose consumer is a conv that refuses "
                 "Cin % 4 != 0, so the element count is always a multiple of 4"),
        row("conv_pack_images_kernel", "conv.hip", ["vqvae_conv_pack_f32"], 4096, "min(ceil(packed floats / 256), 4096)",
            "an element of the fp32 image (and of both 16-bit images)", [("conv.hip", "if (grid > 4096) grid = 4096;")],
            [Cover(NEW + "test_conv_weight_image", conv_pack_units(*CONV_PACK[:3]), None)], aligned=True),
        row("conv_tile8_bf3_kernel", "conv.hip", ["vqvae_conv_forward_f32", "vqvae_conv_taps_forward_f32"], NO_LOOP,
            "gx * ny workgroups in one dimension", "-", [("conv.hip", "const unsigned id = blockIdx.x, nxb = gridDim.x / (unsigned)ny;")],
            note="gridDim.x / ny recovers the x extent of a flattened 2-D grid; every workgroup handles one tile, there is no loop"),
        row("conv_halo8_h2_kernel", "conv.hip", ["vqvae_forward_f32", "vqvae_encoder_f32", "vqvae_decoder_f32"], NO_LOOP,
            "gx * ny workgroups in one dimension", "-", [("conv.hip", "const unsigned id = blockIdx.x, nxb = gridDim.x / (unsigned)ny;")],
            note="as conv_tile8_bf3_kernel"),
        # ---- conv_res.hip
        row("res_combine_kernel", "conv_res.hip", ["vqvae_res_layer_forward_ws_f32", "vqvae_forward_f32", "vqvae_encoder_f32", "vqvae_decoder_f32"],
            8192, "min(ceil(B H W C / 4 / 256), 8192)", "a 4-vector", [("conv_res.hip", "if (grid > 8192) grid = 8192;")],
            [Cover(NEW + "test_residual_layer_outside_the_fused_widths", RES_COMBINE[2] * RES_COMBINE[3] * RES_COMBINE[4] * RES_COMBINE[0] // 4, None)]),
        # ---- conv_ends.hip: fixed grids
        row("conv_in_pack_kernel", "conv_ends.hip", ["vqvae_conv_in_pack_f32"], 16, "16 workgroups", "an element of the fp32 image",
            [("conv_ends.hip", "hipLaunchKernelGGL((conv_in_pack_kernel<3>), dim3(16), dim3(256)"),
             ("conv_ends.hip", "const int total = ntile * JG * 256;")],
            [Cover(NEW + "test_first_layer_weight_images", conv_in_pack_units(*CONV_IN_PACK[:2])[0], None)], aligned=True),
        row("conv_in_pack_bf3_kernel", "conv_ends.hip", ["vqvae_conv_in_pack_f32"], 16, "16 workgroups", "an element of the bf16 image",
            [("conv_ends.hip", "hipLaunchKernelGGL((conv_in_pack_bf3_kernel<3>), dim3(16), dim3(256)"),
             ("conv_ends.hip", "const int total = ntile * CIN * 512;")],
            [Cover(NEW + "test_first_layer_weight_images", conv_in_pack_units(*CONV_IN_PACK[:2])[1], None)], aligned=True),
        row("conv_in_pack_h2_kernel", "conv_ends.hip", ["vqvae_conv_in_pack_f32"], UNREACHABLE, "4 workgroups", "a lane of the fp16 image",
            [("conv_ends.hip", "hipLaunchKernelGGL((conv_in_pack_h2_kernel<4>), dim3(4), dim3(256)"),
             ("conv_ends.hip", "const int total = ntile * CIN * 64;"),
             ("conv_ends.hip", "if (!(Cin == 1 || Cin == 3 || Cin == 4) || Cout < 1 || Cout > 128) return 0;")],
            proof=lambda: conv_in_pack_units(CONV_IN_MAX_CIN, CONV_IN_MAX_COUT)[2] <= 4 * WG,
            note="Cin <= 4 and Cout <= 128 give at most 4 tiles * 4 channels * 64 lanes = 1024 = 4 workgroups of 256"),
        row("convt_out_pack_kernel", "conv_ends.hip", ["vqvae_convt_out_pack_f32"], 32, "32 workgroups", "an element of the fp32 image",
            [("conv_ends.hip", "hipLaunchKernelGGL(convt_out_pack_kernel, dim3(32), dim3(256)"), ("conv_ends.hip", "const int total = cpt * ntile * 1024;")],
            [Cover(NEW + "test_last_layer_weight_images", convt_out_pack_units(*CONVT_OUT_PACK[:2]), None)], aligned=True),
        row("convt_out_pack_bf3_kernel", "conv_ends.hip", ["vqvae_convt_out_pack_f32"], 32, "32 workgroups", "an element of a 16-bit image",
            [("conv_ends.hip", "hipLaunchKernelGGL(convt_out_pack_bf3_kernel<false>, dim3(32), dim3(256)"),
             ("conv_ends.hip", "hipLaunchKernelGGL(convt_out_pack_bf3_kernel<true>, dim3(32), dim3(256)")],
            [Cover(NEW + "test_last_layer_weight_images", convt_out_pack_units(*CONVT_OUT_PACK[:2]), None)], aligned=True),
        row("convt_out_pack_a_kernel", "conv_ends.hip", ["vqvae_convt_out_pack_f32"], UNREACHABLE, "2 workgroups", "a lane of the A-operand image",
            [("conv_ends.hip", "hipLaunchKernelGGL(convt_out_pack_a_kernel, dim3(2), dim3(256)"),
             ("conv_ends.hip", "for (int e = blockIdx.x * 256 + threadIdx.x; e < 8 * 64; e += gridDim.x * 256) {")],
            proof=lambda: 8 * 64 <= 2 * WG, note="the loop bound is the constant 8 * 64 = 512 = 2 workgroups of 256"),
        row("convt_out_kernel", "conv_ends.hip", ["vqvae_convt_out_forward_f32", "vqvae_forward_f32", "vqvae_decoder_f32"], CUS,
            "min(tiles, CUs * (2 if LDS <= 80 KiB else 1))", "a 14 x 14 (or whole-map) input tile",
            [("conv_ends.hip", "const long long grid = ntiles < resident ? ntiles : resident;")], cus["convt_out_kernel"]),
    ]
    return r


def RVQ_WIDE_UNITS():
    from tests import test_vq_residual_gpu as T
    B, H, W, D, K = T.CAP_SHAPE_WIDE
    return B * H * W * D // 4


# ------------------------------------------------------------------------------------------------ guarded device allocations
GUARD = 4096                                     # 32-bit words of pattern in front of and behind every buffer (16 KiB: views stay aligned)
PATTERN = 0x7FC0BEEF                             # a quiet NaN as fp32, and as the low half of an fp64 NaN's neighbour: never a result


class guarded:
    """`with guarded() as g: out = front_end(...)` -- while the block runs, every device buffer the front end allocates with
    torch.empty / torch.empty_like (outputs and workspaces alike) is a view into a larger buffer: the view and GUARD words on both
    sides hold PATTERN.  (The replacement is process-wide while the block runs, so keep the block to the call under test; a call
    that passes other keywords than dtype and device gets a plain buffer, which `check(*outputs)` notices.)  So an element no lap wrote is a NaN in the result, and
    `g.check()` afterwards finds a store that landed in front of a buffer or past its end (a last lap that ran beyond `total`).  The front end is the one the small-shape tests call:
    nothing about the call changes but where its buffers lie."""

    def __enter__(self):
        import torch
        self.torch, self.empty, self.empty_like, self.buffers = torch, torch.empty, torch.empty_like, []
        torch.empty, torch.empty_like = self._empty, self._empty_like
        return self

    def __exit__(self, *exc):
        self.torch.empty, self.torch.empty_like = self.empty, self.empty_like
        return False

    def _empty(self, *size, dtype=None, device=None, **kw):
        torch = self.torch
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            size = tuple(size[0])
        dev = torch.device(device) if device is not None else None
        if dev is None or dev.type != "cuda" or kw:
            return self.empty(size, dtype=dtype, device=device, **kw)
        dtype = dtype or torch.get_default_dtype()
        n = 1
        for s in size:
            n *= int(s)
        nbytes = n * self.empty((), dtype=dtype).element_size()
        words = cdiv(nbytes, 4)
        buf = self.empty(words + 2 * GUARD, dtype=torch.int32, device=dev).fill_(PATTERN)
        self.buffers.append((buf, words))
        return buf[GUARD:GUARD + words].view(torch.uint8)[:nbytes].view(dtype).view(size)

    def _empty_like(self, t, **kw):
        if not t.is_cuda or kw:
            return self.empty_like(t, **kw)
        return self._empty(tuple(t.shape), dtype=t.dtype, device=t.device)

    def owns(self, t):
        """is `t` a view into one of the guarded buffers?"""
        p = t.untyped_storage().data_ptr()
        return any(buf.untyped_storage().data_ptr() == p for buf, _ in self.buffers)

    def check(self, *outputs):
        """every guard still holds the pattern, and every tensor of `outputs` (the results under test) lies in a guarded buffer: a
        front end that came to allocate some other way would otherwise run unguarded without any test noticing"""
        torch = self.torch
        torch.cuda.synchronize()
        assert self.buffers, "the front end allocated nothing on the device"
        for i, t in enumerate(outputs):
            assert self.owns(t), f"output {i} {tuple(t.shape)} does not lie in a guarded buffer"
        for i, (buf, words) in enumerate(self.buffers):
            front, back = buf[:GUARD], buf[GUARD + words:]
            assert bool((front == PATTERN).all()), f"buffer {i} ({words} words): a store in front of it"
            assert bool((back == PATTERN).all()), f"buffer {i} ({words} words): a store past its end"


def nan_filled(shape, device, displaced=0):
    """an input buffer with guards of its own: a contiguous fp32 tensor of `shape` that starts `displaced` floats past a 16-byte
    boundary, to be filled by the caller"""
    import torch
    n = 1
    for s in shape:
        n *= int(s)
    buf = torch.empty(n + 2 * GUARD + 4, dtype=torch.int32, device=device).fill_(PATTERN)
    v = buf[GUARD + displaced:GUARD + displaced + n].view(torch.float32).view(shape)
    assert v.data_ptr() % 16 == 4 * displaced and v.is_contiguous()
    return v
