/*
 * vqvae_hip.h -- C ABI of libvqvae_hip.so: the MI355X (gfx950) implementation of
 * the VQ-VAE forward hot path of MishaLaskin/vqvae.
 *
 * The reference has no FFI or plugin interface; its seam for this path is the
 * nn.Module.forward boundary of five Python classes.  Each entry
 * point below names the reference interface it replaces (file:line under the
 * reference tree).  INTEGRATION.md shows the ctypes stub a maintainer of the
 * reference would add.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless
 *     its name says host; all tensors are dense, contiguous fp32 unless noted.
 *   - the caller owns and allocates every buffer, including the workspace
 *     (size from the matching *_workspace_bytes()); the library never allocates,
 *     frees or synchronises; all work is enqueued on `stream` (a hipStream_t
 *     passed as void*; NULL = the null stream).
 *   - inputs are const and never written.
 *   - return value: 0 on success, a negative VQVAE_ERR_* on argument errors
 *     (nothing is launched), a positive hipError_t if a launch failed.
 *     No exceptions cross this boundary.  vqvae_strerror() names any of them.
 *
 * Pointer contract
 *   - an fp32 or int32 pointer must be 4-byte aligned, an int64 or fp64 pointer 8-byte aligned.
 *   - many kernels move sixteen bytes per access.  Where an entry's kernels do that on a caller's pointer, the entry
 *     either takes an element-wise path that gives the same result when the pointer is not 16-byte aligned, or it
 *     returns VQVAE_ERR_UNSUPPORTED before anything is launched.  No entry launches a 16-byte access on a pointer that
 *     is not 16-byte aligned.  Which entry does which, pointer by pointer, is tabulated in profiles/pointer_contract.md
 *     (tests/test_views_cpu.py holds the same table and calls every refusing row).
 *   - the same holds for the device pointers inside VqvaeRawWeights and VqvaeWeights: the codebook (handed on unpacked, and
 *     read 16 bytes at a time) and the packed images are 16-byte aligned, weights and biases 4-byte aligned;
 *     vqvae_weights_pack_f32 and every entry that takes a VqvaeWeights test them before their first launch.
 *   - workspaces and packed images are 16-byte aligned (the *_bytes() functions size them; any hipMalloc result is).
 *   - a tensor is dense: a strided view has no meaning at this boundary.  The Python front end (vqvae_amd/_lib.py:
 *     dense / written) copies a strided or under-aligned tensor to fresh storage where the entry behind a call would
 *     refuse it, so every public Python call accepts any view and returns the bits of its dense copy.
 */
#ifndef VQVAE_HIP_H
#define VQVAE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VQVAE_HIP_ABI_VERSION 9   /* 2: round 2's packed-weight layout, whole-path entries; 3: quantizer flag 0x10 = VQVAE_VQ_TOP3_KEYS;
                                    4: forward in parts (begin / part / end), residual layer with hidden output, larger
                                       weight-gradient and streamed-quantizer workspaces (always ask the *_bytes functions);
                                    5-6: round 4's headers in front of the two-term images, whole-path product flags, removed
                                       quantizer flags; 7: data-gradient epilogues (vqvae_conv_forward_ep_f32);
                                    8: vqvae_vq_launch_form, unit counters in the quantizer workspace (its size changed: ask
                                       vqvae_vq_workspace_bytes), K up to 1024 on the resident-image and the fused quantizer;
                                    9: round 5 -- vqvae_encode_f32 / vqvae_decode_f32 (the index wire format as fused entry points),
                                       VQVAE_VQ_UNITS32_8WAVES, the sixteen-wave quantizer form at every size */

#define VQVAE_OK               0
#define VQVAE_ERR_NULL        -1   /* a required pointer is NULL                       */
#define VQVAE_ERR_SHAPE       -2   /* non-positive or inconsistent dimension           */
#define VQVAE_ERR_UNSUPPORTED -3   /* shape outside what the kernels are built for     */
#define VQVAE_ERR_WORKSPACE   -4   /* workspace missing or smaller than required       */
#define VQVAE_ERR_OVERFLOW    -5   /* an element count does not fit the index type     */

typedef void *vqvae_stream_t;      /* hipStream_t */

#if defined(__GNUC__)
#define VQVAE_API __attribute__((visibility("default")))
#else
#define VQVAE_API
#endif

VQVAE_API int vqvae_abi_version(void);
/* sha256 (16 hex digits) over the names and bytes of the kernel sources (vqvae_amd/csrc) this library was built from; the same string
 * follows the marker "VQVAE_SRC_FP=" inside the library FILE, so a loader can tell a stale build without loading it (vqvae_amd/_lib.py
 * rebuilds or refuses; bench.py stamps its profiles with it).  Round 5; no ABI change for existing callers.                          */
VQVAE_API const char *vqvae_source_fingerprint(void);
VQVAE_API const char *vqvae_strerror(int code);

/* ---------------------------------------------------------------- profiling
 * Measurement aid for bench.py (never used on the product path): while enabled,
 * every launch of an instrumented kernel is bracketed by a pair of hipEvents
 * recorded on the launch stream.  vqvae_profile_collect() is the only call in
 * this library that synchronises: it waits for the recorded events of one
 * kernel id, returns the summed kernel time and launch count, and resets them.
 * At most 256 launches per id are recorded between collects.                  */
#define VQVAE_PROF_VQ_MAIN     0   /* fused VectorQuantizer kernel                     */
#define VQVAE_PROF_CONV_IGEMM  1   /* implicit-GEMM conv / conv-transpose kernels      */
#define VQVAE_PROF_RES_LAYER   2   /* fused residual-layer kernel                      */
#define VQVAE_PROF_CONV_IN     3   /* first conv (NCHW image in)                       */
#define VQVAE_PROF_CONV_OUT    4   /* last conv-transpose (NCHW image out)             */
#define VQVAE_PROF_NUM_IDS     5
VQVAE_API int vqvae_profile_enable(int on);
VQVAE_API int vqvae_profile_collect(int kernel_id, double *total_ms, int *launches);

/* Box calibration (bench.py): one launch of a bare fp16 MFMA stream on random operands (512 workgroups x 4 waves, `iters` x 4
 * v_mfma_f32_32x32x16_f16 per wave = vqvae_calibration_flops(iters) flop); the caller times it with events.  scratch (at least
 * vqvae_calibration_scratch_bytes()): afterwards 512 pairs of uint64 {shader cycles, 100 MHz ticks} of each workgroup's loop
 * -- cycles / (ticks * 10 ns) = the clock the chip held under this load -- followed by the kernel's (meaningless) sums.       */
VQVAE_API size_t vqvae_calibration_scratch_bytes(void);
VQVAE_API double vqvae_calibration_flops(int iters);
VQVAE_API int vqvae_calibration_mfma_f16(int iters, void *scratch, size_t scratch_bytes, vqvae_stream_t stream);

/* ---------------------------------------------------------------- quantizer */

/* flags for vqvae_vq_forward_f32 */
#define VQVAE_VQ_NCHW          0x0  /* z_e / z_q are (B,D,H,W): the module boundary   */
#define VQVAE_VQ_ROWMAJOR      0x1  /* z_e / z_q are (B,H,W,D) = (N,D) rows (internal) */
#define VQVAE_VQ_CODEBOOK_PREPARED 0x2 /* workspace already holds this codebook's image
                                        (a previous call with the same codebook, K, D
                                        and workspace): skip the prepare kernel        */

#define VQVAE_VQ_EXACT_SWEEP    0x4  /* force the exhaustive exact-fp32 MFMA sweep instead of the
                                        16-bit-screened + exactly-refined kernels (identical outputs) */
#define VQVAE_VQ_BF16_FILTER    0x8  /* use round 1's two-sweep bf16 filter kernel where the default would be the
                                        single-sweep fp16 kernel (identical outputs; A/B timing and tests) */

#define VQVAE_VQ_REMOVED_FLAGS  0x30 /* 0x10 / 0x20 selected round 2's tracker kernel (vq_sweep_kernel_d64: index-carrying top-3 keys; 32-row units
                                        on sixteen waves) for A/B runs.  Round 4 removed that kernel: VQVAE_ERR_UNSUPPORTED */

#define VQVAE_VQ_UNITS64_8WAVES  0x100 /* vq_track_kernel_d64's launch form, forced (identical outputs; tests and A/B timing): 64-row units on */
#define VQVAE_VQ_UNITS32_16WAVES 0x200 /* eight waves per CU / 32-row units on sixteen waves per CU (row-major rows, K <= 512).  Default: the
                                        * 32-row units on eight waves up to 8 units per CU (every CU busy before any wave gets a second unit),
                                        * the sixteen-wave form where a wave gets at most two units (N <= 2 x 16 x CUs x 32 rows), else 64-row
                                        * units on eight waves */

#define VQVAE_VQ_UNITS32_8WAVES  0x400 /* 32-row units on eight waves per CU, forced (the rule takes this form up to 8 units per CU) */

#define VQVAE_VQ_BWD_COMMITMENT 0x800 /* vqvae_vq_backward_f32 only: the gradient of VectorQuantizerEMA's loss beta * mean((z_q - z)^2)
                                        (grad_z only, scale 2 beta / (N D); grad_codebook must be NULL) */
#define VQVAE_VQ_BWD_ROTATION   0x20000 /* vqvae_vq_backward_f32 only: grad_zq reaches grad_z through the rotation trick (arXiv 2410.06424)
                                        instead of unchanged; grad_z must not be NULL, grad_codebook is what it is without the flag */

#define VQVAE_VQ_UNFUSED        0x40 /* vqvae_forward_f32 only: run the quantizer as its own launch even where the encoder's last
                                        kernel would quantize its z_e in place (32x32 images, h_dim 128, K = 128 k <= 1024, D = 64: z_e is
                                        then never written); identical outputs, A/B timing and tests */

/* Which kernel vqvae_vq_forward_f32 launches for this shape / flags ("vq_track_kernel_d64" (codebook image resident in LDS: D = 64,
 * K <= 1024 -- up to ~600 beside eight or sixteen waves' tiles, beyond that with four waves per CU; row-major rows or, since round 5 for
 * every such K, NCHW maps whose pixel count is a multiple of 32),
 * "vq_stream_sweep_kernel" (image streamed through LDS: D = 64 / 128, K <= 16384),
 * "vq_filter_kernel_d64", "vq_exact_kernel"), and how many times that kernel sweeps the codebook on the 16-bit matrix
 * cores per row (0 for the exact-fp32 kernel).  For reporting (bench.py). */
VQVAE_API const char *vqvae_vq_kernel_name(int K, int D, int flags);
VQVAE_API int vqvae_vq_screen_sweeps(int K, int D, int flags);
/* Where vqvae_vq_kernel_name says "vq_track_kernel_d64": the launch form that kernel takes for n_rows rows (HW = pixels per image,
 * which matters for NCHW maps only) on the CURRENT device -- waves per CU (4 / 8 / 16), rows per unit (32 / 64) and the share of
 * the units (per cent) that waves draw from per-group pools at the end; VQVAE_ERR_UNSUPPORTED where another kernel runs.
 * For reporting and tests (bench.py names the template instance that ran). */
VQVAE_API int vqvae_vq_launch_form(int64_t n_rows, int K, int D, int HW, int flags, int *waves, int *unit_rows, int *pool_pct);

/* Bytes of workspace vqvae_vq_forward_f32 needs (any number of rows: the streamed-codebook kernels work through the rows
 * in slabs of 2^18 and resolve the open rows of up to sixteen slabs per launch, so their scratch -- 221 MB at D = 64,
 * 254 MB at D = 128: a slab's fp16 rows + 44 bytes of records per row of a sixteen-slab group -- does not grow with n_rows). */
VQVAE_API size_t vqvae_vq_workspace_bytes(int64_t n_rows, int K, int D);

/*
 * Fused VectorQuantizer forward.  Replaces VectorQuantizer.forward
 * (models/quantizer.py:29-76): NCHW->rows (:45-46), the distance matrix
 * ||z||^2 + ||e||^2 - 2 z.E^T (:49-51), argmin (:54), the one-hot @ E gather
 * (:55-60), the loss (:63-64), the straight-through value z + (z_q - z) (:67),
 * the perplexity (:70-71) and rows->NCHW (:74) -- one pass over z_e.
 *
 *   z_e        (B,D,H,W) fp32 [or (B,H,W,D) with VQVAE_VQ_ROWMAJOR]        in
 *   codebook   (K,D) fp32 row-major = embedding.weight (:26)               in
 *   z_q        same shape/layout as z_e; may be NULL (index-only encode)   out
 *   idx        (N) int64, N = B*H*W, row order (b,h,w) = min_encoding_indices (N,1)  out
 *   hist       (K) int32: how many rows chose each code (column sums of
 *              min_encodings, :55-57)                                      out
 *   loss       1 fp32  = mean((z_q-z)^2) + beta*mean((z_q-z)^2)  (:63-64)  out
 *   perplexity 1 fp32  = exp(-sum p log(p + 1e-10)), p = hist/N  (:70-71)  out
 *
 * Bit-exactness contract (tests/test_vq_gpu.py): idx and z_q are bit-identical
 * to the reference's for identical z_e bits, including first-index tie-breaking
 * and NaN-counts-as-minimum; loss / perplexity agree to rtol 1e-6.
 * Supported: 1 <= K <= 16384; D in {32, 64, 128, 256} on the kernels named by vqvae_vq_kernel_name; any other 1 <= D <= 256
 * (main.py:21 leaves --embedding_dim free and the reference "just runs") with the same contract on the fp32 matrix cores (round 6,
 * vq_anyd_kernel: rows and codes zero-padded to a multiple of eight channels -- fmaf(0, 0, acc) = acc, so v_mfma_f32_32x32x2_f32 stays
 * the reference's k-ordered chain; ~60-80 TFLOP/s of distance arithmetic); VQVAE_VQ_BF16_FILTER selects round 5's per-thread vector
 * chains there (vq_generic_kernel, 16 TFLOP/s; kept for A/B runs), the other kernel-selection flags select nothing for these widths.
 * D > 256 stays VQVAE_ERR_UNSUPPORTED: from D = 384 on the reference's own z @ E^T is no longer one k-ordered fmaf chain (its sgemm
 * blocks the reduction), so there are no pinned bits to be exact against.
 */
VQVAE_API int vqvae_vq_forward_f32(const float *z_e, const float *codebook,
                         int64_t B, int D, int H, int W, int K, float beta, int flags,
                         float *z_q, int64_t *idx, int32_t *hist,
                         float *loss, float *perplexity,
                         void *workspace, size_t workspace_bytes, vqvae_stream_t stream);

/* min_encodings, the (N,K) fp32 one-hot (models/quantizer.py:55-57).  Optional:
 * VQVAE.forward discards it (models/vqvae.py:34); N*K must fit in int64.       */
/* Test hook (round 5): out[r] = torch.sum(x[r] ** 2) of `rows` row-major rows of any width D <= 1024, in the order ATen's CPU kernel
 * uses (models/quantizer.py:49-50 delegates it; the tests' CPU oracle restates it) -- mode 0: one thread per row (the codebook term of
 * vq_generic_kernel), mode 1: the workgroup-cooperative form (its row term).  tests/test_vq_generic_gpu.py compares both with
 * torch.sum bit for bit.                                                                                                               */
VQVAE_API int vqvae_debug_row_sqnorm_f32(const float *x, int64_t rows, int D, int mode, float *out, vqvae_stream_t stream);

VQVAE_API int vqvae_vq_onehot_f32(const int64_t *idx, int64_t N, int K, float *onehot,
                        vqvae_stream_t stream);

/* indices -> z_q (B,D,H,W): the one-hot @ embedding.weight -> view -> permute
 * sequence of the notebook's generate_samples (visualization.ipynb:358-365).
 * An index outside [0, K) never reads the codebook: its D elements become NaN
 * (the reference raises; a launch cannot -- validate on the host if the indices
 * are not your own, as the Python front end does).                             */
VQVAE_API int vqvae_vq_decode_indices_f32(const int64_t *idx, const float *codebook,
                                int64_t B, int D, int H, int W, int K,
                                float *z_q, vqvae_stream_t stream);

/* ------------------------------------------------------- conv / residual stacks
 * Activations between layers are ROW-MAJOR (B,H,W,C): one contiguous C-vector per
 * pixel.  NCHW appears only at the image boundaries (vqvae_conv_in_*, vqvae_convt_out_*)
 * and, for callers that use sub-modules directly, through vqvae_transpose_f32.
 * Weights are passed PACKED: vqvae_*_pack_f32 rewrites a torch-layout weight into the
 * MFMA B-operand image once per weight version (bytes from vqvae_*_packed_bytes).
 * fp32 in, fp32 out, fp32 accumulation.  Products are formed from 16-bit splits of both fp32 operands on the
 * 16-bit matrix cores: two fp16 terms per operand and three term products on 8x8 maps (operands carry exact
 * power-of-two scales: per layer for the weights, per image for the activations, measured by the kernel itself) --
 * relative error per product <= 2^-21 (representation 2^-23 per operand, dropped term pair 2^-22; fp32's own is 2^-24);
 * three bf16 terms (an exact split) and six term products on other map sizes and everywhere with VQVAE_CONV_BF16_SPLIT --
 * per product <= 3*2^-24.  The whole-path entry points (vqvae_forward_f32 ...) hand the per-image maxima from layer
 * to layer and use the fp16 scheme on every map size.  VQVAE_CONV_EXACT_FP32 selects the exact-fp32 MFMA kernels.  Parity with the reference is
 * tolerance-level either way (oneDNN's summation order is opaque): |y - y_ref| <= 1e-5 + 1e-4|y_ref|.
 * All activation pointers must be 16-byte aligned (VQVAE_ERR_UNSUPPORTED otherwise).
 * Shapes the reference uses at 32x32 images (8x8 maps, and the 4x4 s2 conv on 16x16 maps) take
 * tile-resident kernels (one image per wavefront); every other shape takes the generic implicit-GEMM ones. */
#define VQVAE_CONV_4x4_S2   0   /* nn.Conv2d(k=4,s=2,p=1), weight (Cout,Cin,4,4)   encoder.py:29-33 */
#define VQVAE_CONV_3x3_S1   1   /* nn.Conv2d(k=3,s=1,p=1), weight (Cout,Cin,3,3)   encoder.py:35, residual.py:20 */
#define VQVAE_CONV_1x1      2   /* nn.Conv2d(k=1),         weight (Cout,Cin,1,1)   vqvae.py:16, residual.py:23 */
#define VQVAE_CONVT_3x3_S1  3   /* nn.ConvTranspose2d(k=3,s=1,p=1), weight (Cin,Cout,3,3)  decoder.py:28 */
#define VQVAE_CONVT_4x4_S2  4   /* nn.ConvTranspose2d(k=4,s=2,p=1), weight (Cin,Cout,4,4)  decoder.py:31 */
#define VQVAE_CONV_TAPS     6   /* stride-1 conv over an explicit tap list: only through the vqvae_conv_taps_* entry points below */
#define VQVAE_CONVT_1x1     5   /* nn.ConvTranspose2d(k=1), weight (Cin,Cout,1,1): the data gradient of a 1x1 nn.Conv2d */

#define VQVAE_CONV_RELU_IN  0x1 /* apply ReLU to the input as it is read (the in-place nn.ReLU(True)
                                   in front of a conv, residual.py:19,22)                          */
#define VQVAE_CONV_RELU_OUT 0x2 /* ReLU on the result (encoder.py:31,34, decoder.py:33)           */
#define VQVAE_CONV_BF16_SPLIT 0x8 /* use round 1's three-term bf16 products (6 per fp32 product) where the default on 8x8
                                    maps is the two-term fp16 scheme (3 per product, same error bound; A/B and tests) */
#define VQVAE_CONV_EXACT_FP32 0x4 /* use the exact-fp32 MFMA kernels (157 TF peak) instead of the default 16-bit
                                   split products (see above)                                                  */

VQVAE_API size_t vqvae_conv_packed_bytes(int kind, int Cin, int Cout);
VQVAE_API int vqvae_conv_pack_f32(int kind, const float *w, int Cin, int Cout, float *packed,
                                  vqvae_stream_t stream);
/* y = conv(x) + bias [ReLU]; x (B,H,W,Cin) row-major, y (B,Hout,Wout,Cout) row-major; bias may be
 * NULL.  Cin must be a multiple of 4.  Replaces one nn.Conv2d / nn.ConvTranspose2d call.
 * packed: [fp32 image][three-term bf16 image][4x4 s2 only: the same in space-to-depth chunk order]
 *         [header {weight scale exponent}][two-term fp16 image][4x4 s2 only: the same in space-to-depth chunk order]. */
/* How many 16-bit MFMA term products vqvae_conv_forward_f32 issues per fp32 multiply-add for this layer shape: 3 (two-term
 * fp16, 8x8 maps), 6 (three-term bf16), 1 (VQVAE_CONV_EXACT_FP32), 0 = unsupported shape.  With
 * VQVAE_CONV_QUERY_WHOLE_PATH in flags: what the whole-path entry points (vqvae_forward_f32 ...) launch for the layer --
 * they hand the per-image maxima over, so every map size runs the two-term fp16 products (3).  For reporting (bench.py). */
#define VQVAE_CONV_QUERY_WHOLE_PATH 0x100
VQVAE_API int vqvae_conv_term_products(int kind, int H, int W, int Cin, int Cout, int flags);

VQVAE_API int vqvae_conv_forward_f32(int kind, const float *x, const float *packed, const float *bias,
                                     int64_t B, int H, int W, int Cin, int Cout, int flags,
                                     float *y, vqvae_stream_t stream);

/* One ResidualLayer.forward (models/residual.py:27-29) as a single kernel:
 *   y = r(x) + W2 (*) relu(W1 (*) r(x)),  r = ReLU if VQVAE_CONV_RELU_IN else identity,
 *   followed by ReLU if VQVAE_CONV_RELU_OUT (the stack's final F.relu, residual.py:50, or the
 *   next layer's in-place ReLU hoisted into this one).
 * packed_w1 = pack(VQVAE_CONV_3x3_S1, res_block[1].weight (Rh,C,3,3)), packed_w2 =
 * pack(VQVAE_CONV_1x1, res_block[3].weight (C,Rh,1,1)).  C in {32,64,128}, Rh <= 32, x != y (other widths:
 * vqvae_res_layer_forward_ws_f32 below; here VQVAE_ERR_UNSUPPORTED).                                */
VQVAE_API int vqvae_res_layer_forward_f32(const float *x, const float *packed_w1,
                                          const float *packed_w2, int64_t B, int H, int W, int C,
                                          int Rh, int flags, float *y, vqvae_stream_t stream);

/* The same for ANY width with C % 4 == 0 and Rh % 4 == 0 (round 4: main.py's --n_hiddens / --n_residual_hiddens are free):
 * widths outside the fused kernels (C not in {32,64,128} or Rh > 32) run as 3x3 conv -> 1x1 conv -> skip + ReLU through the conv
 * kernels, the hidden map in `scratch` (at least B*H*W*Rh floats; unused and may be NULL for the fused widths).              */
VQVAE_API int vqvae_res_layer_forward_ws_f32(const float *x, const float *packed_w1, const float *packed_w2, int64_t B, int H,
                                             int W, int C, int Rh, int flags, float *y, float *scratch, size_t scratch_bytes,
                                             vqvae_stream_t stream);
/* The same layer for a training step (main.py:74-78 through models/residual.py:27-29): also writes the hidden
 * activation relu(W1 (*) r(x)) as hidden (B,H,W,Rh) row-major, which the backward pass needs for the ReLU mask and the
 * 1x1 weight gradient -- instead of recomputing the 3x3 conv there.  Only where a wave owns whole images:
 * H = W = 8, Rh = 32 (VQVAE_ERR_UNSUPPORTED otherwise: the caller recomputes with vqvae_conv_forward_f32).     */
VQVAE_API int vqvae_res_layer_forward_hidden_f32(const float *x, const float *packed_w1,
                                                 const float *packed_w2, int64_t B, int H, int W, int C,
                                                 int Rh, int flags, float *y, float *hidden,
                                                 vqvae_stream_t stream);

/* First encoder conv, nn.Conv2d(Cin,Cout,k=4,s=2,p=1) (models/encoder.py:29-31), reading the NCHW
 * image x (B,Cin,H,W) and writing row-major (B,H/2,W/2,Cout).  Cin in {1,3,4}, Cout <= 128.
 * flags: VQVAE_CONV_RELU_OUT, VQVAE_CONV_EXACT_FP32 (fp32 MFMA instead of the split-bf16 products).
 * (The packed image also carries the two-term fp16 operand image of the fused encoder front, see vqvae_encoder_f32.)  */
VQVAE_API size_t vqvae_conv_in_packed_bytes(int Cin, int Cout);
VQVAE_API int vqvae_conv_in_pack_f32(const float *w, int Cin, int Cout, float *packed,
                                     vqvae_stream_t stream);
VQVAE_API int vqvae_conv_in_forward_f32(const float *x_nchw, const float *packed, const float *bias,
                                        int64_t B, int H, int W, int Cin, int Cout, int flags,
                                        float *y, vqvae_stream_t stream);

/* Last decoder layer, nn.ConvTranspose2d(Cin,Cout,k=4,s=2,p=1) (models/decoder.py:34-35), reading
 * row-major (B,H,W,Cin) and writing the NCHW image (B,Cout,2H,2W).  Cout <= 4, Cin % 4 == 0,
 * Cin <= 256.  Runs as GEMM (pixels x Cin x 16*Cout on the MFMA) + in-LDS col2im.  flags: 0, or
 * VQVAE_CONV_EXACT_FP32 for the fp32 MFMA instead of the split-bf16 products.                      */
VQVAE_API size_t vqvae_convt_out_packed_bytes(int Cin, int Cout);
VQVAE_API int vqvae_convt_out_pack_f32(const float *w, int Cin, int Cout, float *packed,
                                       vqvae_stream_t stream);
VQVAE_API int vqvae_convt_out_forward_f32(const float *x, const float *packed, const float *bias,
                                          int64_t B, int H, int W, int Cin, int Cout, int flags,
                                          float *y_nchw, vqvae_stream_t stream);

/* Batched transpose x[batch][R][C] -> y[batch][C][R]: (B,C,HW) <-> (B,HW,C) layout changes for
 * callers that enter or leave the path at a sub-module boundary (visualization.ipynb:84-90).     */
VQVAE_API int vqvae_transpose_f32(const float *x, int64_t batch, int R, int C, float *y,
                                  vqvae_stream_t stream);

/* ------------------------------------------------------- training-step companions
 * what main.py:74-83 needs around the forward path.
 *
 * vqvae_vq_backward_f32 -- the gradients autograd derives from models/quantizer.py:63-67:
 *     grad_z        = grad_zq + g * 2 (z - e_idx) / (N D)             (:63 first term, :67 straight-through)
 *     grad_codebook = g * 2 beta * sum_{i: idx_i=k} (e_k - z_i) / (N D)   (:63-64; beta sits on the codebook
 *                     term in the reference, the reverse of the paper -- reproduced as written)
 *   g = *grad_loss (device scalar; NULL = 1), grad_zq = upstream gradient of the returned z_q (NULL = 0).
 *   z_e / grad_zq / grad_z share the layout selected by VQVAE_VQ_ROWMAJOR.  Either output may be NULL.
 *   The codebook gradient uses no floating-point atomics: rows are stably sorted by code and summed in a
 *   fixed order in fp64, so it is bit-reproducible run to run.  Parity with torch autograd: rtol 1e-5.
 *   flags | VQVAE_VQ_BWD_COMMITMENT: grad_z = grad_zq + g * 2 beta (z - e_idx) / (N D) only (VectorQuantizerEMA's loss).
 *   flags | VQVAE_VQ_BWD_ROTATION (alone or with VQVAE_VQ_BWD_COMMITMENT): grad_z = rot(grad_zq) + the same loss term, where for
 *   each row e of z with code q = E[idx] and upstream row g, rot(g) = lam R^T g = lam [g - 2 r (r^T g) + 2 e^ (q^^T g)] with
 *   e^ = e/||e||, q^ = q/||q||, r = (e^ + q^)/||e^ + q^||, lam = ||q||/||e||: the gradient of z~_q = sg[lam R] e (Fifty et al.,
 *   arXiv 2410.06424), whose value is q.  Evaluated per row in fp64 from five dot products added in ascending channel order and
 *   rounded to fp32 once (the exact operation order: csrc/vq_rotation.hip's header); the same bits in both layouts and in every
 *   run.  Fallback rule: a row whose z is all zeros, whose code is all zeros, whose norms are not finite, or that is antipodal to
 *   its code (||e^ + q^||^2 < 2^-20: the reflection axis is undefined) keeps grad_zq unchanged, as without the flag.  A NaN in
 *   grad_zq or z stays in its own row.  grad_codebook is untouched by the flag; grad_zq == NULL gives the unflagged result
 *   (rot(0) = 0) from the unflagged kernel; grad_z == NULL with the flag is VQVAE_ERR_NULL.  Without the flag the entry launches
 *   exactly what it always did.                                                                                                 */
VQVAE_API size_t vqvae_vq_backward_workspace_bytes(int64_t N, int K, int D);
VQVAE_API int vqvae_vq_backward_f32(const float *z_e, const float *codebook, const int64_t *idx,
                                    const float *grad_zq, const float *grad_loss,
                                    int64_t B, int D, int H, int W, int K, float beta, int flags,
                                    float *grad_z, float *grad_codebook,
                                    void *workspace, size_t workspace_bytes, vqvae_stream_t stream);

/* EMA codebook update (arXiv 1711.00937 Appendix A.1; Sonnet's VectorQuantizerEMA): the codebook follows exponential moving
 * averages of the encoder outputs assigned to each code instead of a gradient.  With c_k = #{i : idx_i = k}, s_k = sum of those z_i:
 *     N_k <- decay N_k + (1 - decay) c_k                       ema_cluster_size (K) fp32, in/out
 *     m_k <- decay m_k + (1 - decay) s_k                       ema_w (K, D) fp32, in/out
 *     n = sum_k N_k;  e_k = m_k / ((N_k + eps) / (n + K eps) n)   codebook (K, D) fp32, out (Laplace-smoothed counts)
 * Restart: with threshold >= 0 and uniforms (K fp32 in [0, 1)) given, a code with N_k < threshold takes row
 * r_k = min(floor(u_k N), N - 1) of z_e instead (N_k and m_k stay as updated); threshold < 0 or uniforms == NULL: no restart.
 *   idx: the forward's indices (against the codebook before this update).  z_e layout by VQVAE_VQ_ROWMAJOR (no other flag).
 *   Sums s_k in fp64 in a fixed order (the backward's sort and segmented sum), update and normalisation in fp64, one rounding per
 *   store; no floating-point atomics, no host sync: bit-reproducible.  codebook must not alias ema_w or z_e.
 *   Envelope: K <= 16384, D <= 256, N <= INT32_MAX (VQVAE_ERR_UNSUPPORTED outside it; the sizing call then returns 0).  */
VQVAE_API size_t vqvae_vq_ema_workspace_bytes(int64_t N, int K, int D);
VQVAE_API int vqvae_vq_ema_update_f32(const float *z_e, const int64_t *idx, int64_t B, int D, int H, int W, int K,
                                      double decay, double eps, double threshold, const float *uniforms, int flags,
                                      float *ema_cluster_size, float *ema_w, float *codebook,
                                      void *workspace, size_t workspace_bytes, vqvae_stream_t stream);

/* The same update cut in two (csrc/vq_ema_merge.hip; its header is the numeric contract), so that the statistics of R shards --
 * other ranks' batches, or earlier micro-batches of this rank -- are merged before the codebook moves.
 * vqvae_vq_ema_stats_f32: one shard's record, stats (K, C) fp64, every element written: column 0 the count c_k (an exact integer),
 *   columns 1 .. D the fp64 sum s_k of the code's rows exactly as vqvae_vq_ema_update_f32 forms it (unrounded), and, with
 *   row_uniforms (K fp32 in [0, 1)), columns D + 1 .. 2 D the shard's restart candidate: row clamp(floor(u_k N_s), 0, N_s - 1) of
 *   z_e as doubles.  C = D + 1 without row_uniforms, 2 D + 1 with them.  The same bits in either layout of z_e.
 * vqvae_vq_ema_apply_f32: stats (R, K, C), shard-major.  c_k = sum_s c_{s,k}; S_k = ((s_0 + s_1) + ...) in fp64 in shard order;
 *   then vqvae_vq_ema_update_f32's update, operation for operation.  Restart (shard_uniforms K fp32, threshold >= 0, C = 2 D + 1):
 *   a code with N_k < threshold takes the candidate of shard clamp(floor(v_k R), 0, R - 1).  R = 1: the bits of
 *   vqvae_vq_ema_update_f32 with row_uniforms as its uniforms.  codebook must not alias ema_w or stats.
 * Envelope: stats as vqvae_vq_ema_update_f32 (flags: VQVAE_VQ_ROWMAJOR only); apply 1 <= R <= 1024, C in {D + 1, 2 D + 1}, decay in
 * [0, 1], eps > 0, shard_uniforms only with C = 2 D + 1: VQVAE_ERR_UNSUPPORTED outside it and for a stats pointer that is not 8-byte
 * aligned; the sizing calls then return 0.  No host sync, no allocation, no memset, no floating-point atomics; every launch on
 * `stream` in one linear chain (capturable); the same bits in every run.                                                      */
VQVAE_API size_t vqvae_vq_ema_stats_workspace_bytes(int64_t N, int K, int D);
VQVAE_API int vqvae_vq_ema_stats_f32(const float *z_e, const int64_t *idx, int64_t B, int D, int H, int W, int K,
                                     const float *row_uniforms, int flags, double *stats,
                                     void *workspace, size_t workspace_bytes, vqvae_stream_t stream);
VQVAE_API size_t vqvae_vq_ema_apply_workspace_bytes(int R, int K, int D);
VQVAE_API int vqvae_vq_ema_apply_f32(const double *stats, int R, int K, int D, int C, double decay, double eps, double threshold,
                                     const float *shard_uniforms, float *ema_cluster_size, float *ema_w, float *codebook,
                                     void *workspace, size_t workspace_bytes, vqvae_stream_t stream);

/* k-means initialisation of the codebook (csrc/vq_kmeans.hip; its header is the numeric contract): a data-dependent start instead of
 * uniform(-1/K, 1/K) (models/quantizer.py:26-27).  Both calls take z_e in the layout VQVAE_VQ_ROWMAJOR selects (no other flag); rows
 * are the N = B H W rows in the quantizer's order.  One workspace size serves both.  No RNG of their own: the caller supplies K fp32
 * uniforms in [0, 1).  No host sync, no atomics, no workgroup waits on another: bit-reproducible, the same bits in either layout.
 * Envelope: 1 <= D <= 256, 1 <= K <= 16384, 1 <= N <= INT32_MAX (VQVAE_ERR_UNSUPPORTED outside it; the sizing call then returns 0).
 *
 * vqvae_vq_kmeans_seed_f32 -- k-means++ (Arthur & Vassilvitskii 2007): rows[0] = min(floor(u_0 N), N - 1); round k >= 1 keeps
 *   w_n = min over the chosen centres of the fp64 squared distance (channels added in order) and picks the first row whose
 *   inclusive prefix sum of w exceeds u_k T (T the total; blocks of 256 rows, groups of blocks, sequential scans: the order is
 *   written in the source's header) with w_n > 0, so a copy of a chosen centre is never picked while T > 0; T = 0 (fewer distinct
 *   rows than centres): rows[k] = min(floor(u_k N), N - 1).  codebook (K, D) out: codebook[k] = row rows[k] bit for bit;
 *   rows (K) int64 out.  1 + 2 (K - 1) launches.
 * vqvae_vq_kmeans_update_f32 -- one Lloyd mean update from the indices vqvae_vq_forward_f32 assigned: counts (K) int32 out = c_k;
 *   codebook (K, D) in/out: c_k > 0: e_k = s_k / c_k (the EMA update's sorted fp64 sums, one fp64 division, one rounding); c_k = 0:
 *   unchanged, or with uniforms (may be NULL) row min(floor(u_k N), N - 1) of z_e.  codebook must not alias z_e.              */
VQVAE_API size_t vqvae_vq_kmeans_workspace_bytes(int64_t N, int K, int D);
VQVAE_API int vqvae_vq_kmeans_seed_f32(const float *z_e, int64_t B, int D, int H, int W, int K, const float *uniforms, int flags,
                                       float *codebook, int64_t *rows, void *workspace, size_t workspace_bytes,
                                       vqvae_stream_t stream);
VQVAE_API int vqvae_vq_kmeans_update_f32(const float *z_e, const int64_t *idx, int64_t B, int D, int H, int W, int K,
                                         const float *uniforms, int flags, float *codebook, int32_t *counts,
                                         void *workspace, size_t workspace_bytes, vqvae_stream_t stream);

/* l2-normalisation of rows and its backward (csrc/vq_cosine.hip; its header is the numeric contract): what a cosine-similarity
 * codebook (ViT-VQGAN, arXiv 2110.04627 section 3.2) puts in front of the quantizer, for encoder outputs and for codes.
 *     forward:   d = max(||x||, eps) per row (fp64 sum of squares in channel order, fp64 sqrt, rounded to fp32, clamped by
 *                (d < eps) ? eps : d);  y = x / d (one fp32 division);  denom (N) fp32 out = d
 *     backward:  t = sum_c y_c g_c in fp64;  grad_x = (g - y t) / d in fp64, rounded once, where d > eps;  g / eps elsewhere
 *   Rows and layouts are vqvae_vq_forward_f32's: N = B H W rows of D channels, (B,D,H,W) maps, or (N,D) rows with
 *   VQVAE_VQ_ROWMAJOR (no other flag); a (K, D) codebook is the row-major case B = K, H = W = 1.  No workspace, no host sync, no
 *   atomics, one launch on `stream`: bit-reproducible, the same bits in either layout.  eps: 1e-12 is torch.nn.functional.normalize's.
 *   Envelope: 1 <= D <= 256, N <= INT32_MAX.  VQVAE_ERR_UNSUPPORTED outside it, for a pointer that is not 4-byte aligned and for an
 *   output that overlaps an input (y and x; grad_x and y or grad_y).                                                               */
VQVAE_API int vqvae_l2norm_forward_f32(const float *x, int64_t B, int D, int H, int W, float eps, int flags,
                                       float *y, float *denom, vqvae_stream_t stream);
VQVAE_API int vqvae_l2norm_backward_f32(const float *y, const float *denom, const float *grad_y,
                                        int64_t B, int D, int H, int W, float eps, int flags,
                                        float *grad_x, vqvae_stream_t stream);

/* Finite scalar quantization (csrc/vq_fsq.hip; its header is the numeric contract): the quantizer without a learned codebook
 * (arXiv 2309.15505; vector-quantize-pytorch's FSQ and its `bound`).  A row is projected to d = n_levels channels (w_in (d, D), b_in
 * (d)), channel j is bounded with tanh and rounded to one of levels[j] values, and projected back (w_out (D, d), b_out (D)); the
 * projections run inside the kernels, all in fp64 with one rounding per output.  The implicit codebook has K = prod levels[j] entries.
 *     forward:   z_q (may be NULL; then w_out / b_out may be too), idx (N) int64 in [0, K), first level least significant;
 *                hist (K) int32 counts (may be NULL), perplexity = exp(-sum p log(p + 1e-10)) (may be NULL, needs hist)
 *     decode:    idx -> z_q; an index outside [0, K) writes a NaN row and reads nothing out of range
 *     backward:  grad_zq -> grad_z (straight-through rounding, through tanh and both projections) and the four parameter gradients,
 *                fp64 sums over the rows in an order that depends on N alone (blocks of 256 rows in row order, then the blocks in
 *                order): the same bits in both layouts and in every run.  Every gradient pointer may be NULL (not all); `workspace`
 *                (vqvae_fsq_backward_workspace_bytes; 0 = outside the envelope) is needed for the parameter gradients only.
 *   `levels` is a HOST array, read during the call.  Rows and layouts are vqvae_vq_forward_f32's; the only flag is
 *   VQVAE_VQ_ROWMAJOR.  No host sync, no allocation, every launch on `stream` in one chain: capturable.
 *   Envelope: 1 <= n_levels <= 8, 2 <= levels[j] <= 256, K <= 65536, 1 <= D <= 256, N <= INT32_MAX.  VQVAE_ERR_UNSUPPORTED outside
 *   it, for a pointer that is not 4-byte aligned (idx, workspace: 8-byte) and for an output that overlaps an input.                */
VQVAE_API int vqvae_fsq_forward_f32(const float *z_e, const float *w_in, const float *b_in, const float *w_out, const float *b_out,
                                    const int *levels, int n_levels, int64_t B, int D, int H, int W, int flags,
                                    float *z_q, int64_t *idx, int32_t *hist, float *perplexity, vqvae_stream_t stream);
VQVAE_API int vqvae_fsq_decode_indices_f32(const int64_t *idx, const float *w_out, const float *b_out, const int *levels,
                                           int n_levels, int64_t B, int D, int H, int W, int flags, float *z_q,
                                           vqvae_stream_t stream);
VQVAE_API size_t vqvae_fsq_backward_workspace_bytes(int64_t N, int D, int n_levels);
VQVAE_API int vqvae_fsq_backward_f32(const float *z_e, const float *grad_zq, const float *w_in, const float *b_in,
                                     const float *w_out, const int *levels, int n_levels, int64_t B, int D, int H, int W, int flags,
                                     float *grad_z, float *grad_w_in, float *grad_b_in, float *grad_w_out, float *grad_b_out,
                                     void *workspace, size_t workspace_bytes, vqvae_stream_t stream);

/* The per-row linear map of latent rows, y = W x + b, forward and backward (csrc/vq_linear.hip; its header is the numeric
 * contract): the projections of a factorized (low-dimensional) codebook (ViT-VQGAN, arXiv 2110.04627 section 3.2; `codebook_dim` in
 * vector-quantize-pytorch).  x and grad_x have Cin channels, y and grad_y Cout channels, in the same layout; w is (Cout, Cin)
 * row-major (nn.Linear.weight), b is (Cout).
 *     y[n][j]      = float(double(b[j]) + sum_c double(w[j][c]) double(x[n][c]))    fp64 from b[j], c ascending, one rounding to fp32
 *     grad_x[n][c] = float(sum_j double(w[j][c]) double(grad_y[n][j]))              fp64 from 0.0, j ascending, one rounding
 *     grad_w[j][c] = float(sum_n double(grad_y[n][j]) double(x[n][c])),  grad_b[j] = float(sum_n double(grad_y[n][j])), in FSQ's
 *                    order: blocks of 256 consecutive rows; inside a block one row after the other from 0.0; then the blocks in
 *                    order from 0.0, by a second launch; one rounding
 *   The order depends on N alone: every output has the same bits in both layouts, on the 16-byte and the element path, in every
 *   run and in a graph replay; there is no floating-point atomic.  The product of two fp32 values is exact in fp64, so the kernels'
 *   fused multiply-adds round as a multiplication and an addition do.  A non-finite x or grad_y stays in its own row of y / grad_x;
 *   the parameter gradients follow IEEE through the stated order.
 *   Rows and layouts are vqvae_vq_forward_f32's: N = B H W rows, (B,C,H,W) maps, or (N,C) rows with VQVAE_VQ_ROWMAJOR, the only flag.
 *   backward: any of grad_x, grad_w, grad_b may be NULL (not all three); `workspace` (vqvae_linear_rows_backward_workspace_bytes; 0 =
 *   outside the envelope) is needed for grad_w / grad_b only (VQVAE_ERR_WORKSPACE when it is missing or too small).
 *   No host sync, no allocation, no memset, every launch on `stream` in one chain: capturable.
 *   Envelope: 1 <= Cin, Cout <= 256, 1 <= N <= INT32_MAX.  VQVAE_ERR_UNSUPPORTED outside it, for a pointer that is not 4-byte aligned
 *   (workspace: 8-byte) and for an output that overlaps an input or another output.                                              */
VQVAE_API int vqvae_linear_rows_forward_f32(const float *x, const float *w, const float *b, int64_t B, int Cin, int H, int W,
                                            int Cout, int flags, float *y, vqvae_stream_t stream);
VQVAE_API size_t vqvae_linear_rows_backward_workspace_bytes(int64_t N, int Cin, int Cout);
VQVAE_API int vqvae_linear_rows_backward_f32(const float *x, const float *grad_y, const float *w, int64_t B, int Cin, int H, int W,
                                             int Cout, int flags, float *grad_x, float *grad_w, float *grad_b, void *workspace,
                                             size_t workspace_bytes, vqvae_stream_t stream);

/* The orthogonal regularization loss of a codebook and its gradient (csrc/vq_orthogonal.hip; its header is the numeric contract):
 * L = |E^ E^T|_F^2 / M^2 - 1 / M over the M selected codes (arXiv 2112.00384 section 3.2; `orthogonal_reg_weight`,
 * `orthogonal_reg_active_codes_only`, `orthogonal_reg_max_codes` in vector-quantize-pytorch).  `rows` (K, D) are taken as they stand:
 * the caller normalises.  One K^2 D pass, no (K, K) array.  Every line is one IEEE operation in the stated precision:
 *     candidate(k) = hist == NULL or hist[k] > 0;  under a cap (uniforms != NULL and max_codes > 0) the max_codes candidates that
 *                    come first in the order (u_k ascending, then k ascending) are kept; selected[k] is 0 / 1, *count = M
 *     G_ij = sum_c double(n_ic) double(n_jc)                 from 0.0, c ascending
 *     R_i  = sum_{j selected} fl(G_ij G_ij),  V_ic = sum_{j selected} fl(G_ij double(n_jc))      from 0.0, j ascending, for selected
 *            i; 0.0 for an unselected i
 *     T    = the R_i of blocks of 256 consecutive codes added in ascending i from 0.0, then the blocks' sums in ascending order
 *            from 0.0: an order that depends on K alone
 *     loss = float(T / (double(M) double(M)) - 1.0 / double(M)),  0 where M = 0
 *     grad_rows[i][c] = float((double(g) (4.0 / (double(M) double(M)))) V_ic) for selected i, +0.0 otherwise; g = *grad_loss, or 1
 *   saved (K, D) fp64 receives V, or is NULL (the V sums are then not formed).  A non-finite value in a selected row makes the
 *   loss and the selected rows' gradients non-finite (which NaN is unspecified) and never reaches an unselected row.
 *   No host sync, no allocation, no memset, no atomic, one chain of launches on `stream`: capturable; the same bits in every run,
 *   at every pointer alignment and in a graph replay.
 *   Envelope: 1 <= K <= 16384, 1 <= D <= 256 (vqvae_vq_orthogonal_workspace_bytes: 0 outside it).  VQVAE_ERR_UNSUPPORTED outside
 *   it, for flags != 0, for a pointer that is not 4-byte aligned (saved, workspace: 8-byte) and for an output that overlaps an input
 *   or another output; VQVAE_ERR_WORKSPACE for a missing or short workspace.                                                     */
VQVAE_API size_t vqvae_vq_orthogonal_workspace_bytes(int K, int D);
VQVAE_API int vqvae_vq_orthogonal_forward_f32(const float *rows, const int32_t *hist, const float *uniforms, int max_codes, int K,
                                              int D, int flags, float *loss, int32_t *count, int32_t *selected, double *saved,
                                              void *workspace, size_t workspace_bytes, vqvae_stream_t stream);
VQVAE_API int vqvae_vq_orthogonal_backward_f32(const double *saved, const int32_t *selected, const int32_t *count,
                                               const float *grad_loss, int K, int D, float *grad_rows, vqvae_stream_t stream);

/* The code-entropy loss of a learned codebook and its gradients (csrc/vq_entropy.hip; its header is the numeric contract): the
 * entropy penalty of MaskGIT's VQGAN tokenizer, MAGVIT and LlamaGen (`entropy_loss_ratio`; `codebook_diversity_loss_weight` in
 * vector-quantize-pytorch), streamed: no (N, K) array, O(N + K D) memory.  Rows and layouts are vqvae_vq_forward_f32's (N = B H W
 * rows z_n; (B, D, H, W) maps, or (N, D) rows with VQVAE_VQ_ROWMAJOR, the only flag); codebook e_k (K, D).  s = inv_temperature.
 * Everything in fp64 from the fp32 inputs:
 *     l_nk = -s ((zz_n + ee_k) - 2 dot_nk);  p_nk = softmax_k(l_nk), shifted by the row maximum
 *     H_n = -sum_k p_nk log p_nk;  P = (1 / N) sum_n H_n;  avg_k = (1 / N) sum_n p_nk;  H = -sum_k avg_k log avg_k  (0 log 0 = 0)
 *     losses = float(P - gamma H, P, H);  avg (K) fp64;  rowstat (N, 2) fp64: the row's log-sum-exp and H_n, or NULL
 *   backward, g = *grad_loss (NULL = 1), L_k = log avg_k (0 where avg_k = 0), M_n = sum_j p_nj L_j; avg and rowstat are the forward's:
 *     a_nk = (g / N) p_nk [-(log p_nk + H_n) + gamma (L_k - M_n)]
 *     grad_z_n = float(-2 s sum_k a_nk (z_n - e_k));  grad_codebook_k = float(2 s sum_n a_nk (z_n - e_k));  either may be NULL, not both
 *   exp and log on the device are not correctly rounded: the results agree with a restatement within a derived bound, not by bits.
 *   The order of every sum is a function of (N, K, D) alone; no floating-point atomics, no host sync, no allocation, no memset, one
 *   chain of launches on `stream`: capturable; the same bits in both layouts, at every pointer alignment, in every run and in a graph
 *   replay.  The losses and gradients of a batch that holds a non-finite value are unspecified (nothing is read out of bounds).
 *   Envelope: 1 <= K <= 16384, 1 <= D <= 256, N < 2^31, s > 0 and finite, gamma finite (vqvae_vq_entropy_workspace_bytes: 0 outside
 *   it; one size for both calls).  VQVAE_ERR_UNSUPPORTED outside it, for another flag, for a pointer that is not 4-byte aligned
 *   (avg, rowstat, workspace: 8-byte) and for an output that overlaps an input or another output; VQVAE_ERR_WORKSPACE for a missing
 *   or short workspace.                                                                                                          */
VQVAE_API size_t vqvae_vq_entropy_workspace_bytes(int64_t N, int K, int D);
VQVAE_API int vqvae_vq_entropy_forward_f32(const float *z_e, const float *codebook, int64_t B, int D, int H, int W, int K,
                                           double inv_temperature, double gamma, int flags, float *losses, double *avg,
                                           double *rowstat, void *workspace, size_t workspace_bytes, vqvae_stream_t stream);
VQVAE_API int vqvae_vq_entropy_backward_f32(const float *z_e, const float *codebook, const double *avg, const double *rowstat,
                                            const float *grad_loss, int64_t B, int D, int H, int W, int K, double inv_temperature,
                                            double gamma, int flags, float *grad_z, float *grad_codebook, void *workspace,
                                            size_t workspace_bytes, vqvae_stream_t stream);

/* Lookup-free quantization (csrc/vq_lfq.hip; its header is the numeric contract): the codebook is {-1, +1}^d, K = 2^d (MAGVIT-v2,
 * arXiv 2310.05737 section 3.1; vector-quantize-pytorch's LFQ).  A row is projected to d channels (w_in (d, D), b_in (d)), every
 * channel keeps its sign (c_j = +1 where y_j > 0, else -1), and the signs are projected back (w_out (D, d), b_out (D)); the
 * projections run inside the kernels in fp64 with one rounding per output.  beta weighs the commitment term, entropy_weight the
 * entropy penalty, diversity_gamma the codebook entropy inside it; inv_temperature (the library's 100) scales the logits.
 *     workspace_bytes: one size for forward and backward; 0 = outside the envelope.
 *     forward:   z_q (may be NULL; then w_out / b_out may be too), idx (N) int64 in [0, K), FIRST channel LEAST significant;
 *                hist (K) int32 counts (may be NULL), perplexity = exp(-sum p log(p + 1e-10)) (may be NULL, needs hist);
 *                losses (4) fp32 = (loss, commitment C, per-sample entropy P, codebook entropy H), loss = beta C + w_e (P - gamma H),
 *                and avg (K) fp64, the batch-averaged code distribution.  losses and avg may be NULL together: then no entropy work
 *                runs and no workspace is needed.  The sums over the rows are fp64 in an order that depends on (N, K) alone: every
 *                output has the same bits in both layouts and in every run.  No (N, K) array is formed.
 *     decode:    idx -> z_q; an index outside [0, K) writes a NaN row.
 *     backward:  from grad_zq (NULL = 0) and g = *grad_loss (device scalar, NULL = 1) to grad_z (straight-through rounding) and the
 *                four parameter gradients (fp64 sums: blocks of 256 rows in row order, then the blocks in order).  avg is the
 *                forward's; with avg NULL the loss contributes nothing.  Every gradient pointer may be NULL (not all); the
 *                workspace is always needed.
 *   Rows and layouts are vqvae_vq_forward_f32's; the only flag is VQVAE_VQ_ROWMAJOR.  No host sync, no allocation, every launch on
 *   `stream` in one chain, every clear a kernel: capturable.
 *   Envelope: 1 <= d <= 16, 1 <= D <= 256, N <= INT32_MAX.  VQVAE_ERR_UNSUPPORTED outside it, for a pointer that is not 4-byte
 *   aligned (idx, avg, workspace: 8-byte) and for an output that overlaps an input.                                              */
VQVAE_API size_t vqvae_lfq_workspace_bytes(int64_t N, int D, int d);
VQVAE_API int vqvae_lfq_forward_f32(const float *z_e, const float *w_in, const float *b_in, const float *w_out, const float *b_out,
                                    int d, int64_t B, int D, int H, int W, int flags, float beta, float entropy_weight,
                                    float diversity_gamma, float inv_temperature, float *z_q, int64_t *idx, int32_t *hist,
                                    float *perplexity, float *losses, double *avg, void *workspace, size_t workspace_bytes,
                                    vqvae_stream_t stream);
VQVAE_API int vqvae_lfq_decode_indices_f32(const int64_t *idx, const float *w_out, const float *b_out, int d, int64_t B, int D,
                                           int H, int W, int flags, float *z_q, vqvae_stream_t stream);
VQVAE_API int vqvae_lfq_backward_f32(const float *z_e, const float *grad_zq, const float *grad_loss, const double *avg,
                                     const float *w_in, const float *b_in, const float *w_out, int d, int64_t B, int D, int H, int W,
                                     int flags, float beta, float entropy_weight, float diversity_gamma, float inv_temperature,
                                     float *grad_z, float *grad_w_in, float *grad_b_in, float *grad_w_out, float *grad_b_out,
                                     void *workspace, size_t workspace_bytes, vqvae_stream_t stream);

/* Residual vector quantization (csrc/vq_residual.hip; its header is the numeric contract): Q codebooks E_0 .. E_{Q-1}, each (K, D),
 * quantize the same latent position, stage q what stage q - 1 left over (RQ-VAE, arXiv 2203.01941; SoundStream's RVQ):
 *     r_0 = z;   idx_q = vqvae_vq_forward_f32's indices of r_q against E_q;   r_{q+1} = r_q - E_q[idx_q]
 *     S = ((e_0 + e_1) + ...) in stage order;   z_q = z + (S - z);   loss = ((loss_0 + loss_1) + ...) on the device
 * 1 <= Q <= 16; the quantizer's envelope (K <= 16384, D <= 256) and N <= INT32_MAX: VQVAE_ERR_UNSUPPORTED outside it, and the sizing
 * calls then return 0.  `codebooks` is a HOST array of Q device pointers (read during the call only); with
 * VQVAE_VQ_RESIDUAL_SHARED every stage uses codebooks[0] and only that entry is read.  No host sync, no allocation, no
 * floating-point atomics; every launch on `stream` in one linear chain (capturable); the same bits in every run and either layout.
 *
 * forward:  flags = the quantizer's own (VQVAE_VQ_ROWMAJOR, VQVAE_VQ_CODEBOOK_PREPARED, the kernel-selection flags), passed to every
 *   stage, | VQVAE_VQ_RESIDUAL_SHARED.  The workspace holds one prepared codebook image per distinct codebook and one residual map,
 *   so VQVAE_VQ_CODEBOOK_PREPARED means: every stage's image is there from a previous call with the same codebooks and workspace.
 *     idx (Q, N) int64 stage-major;  hist (Q, K) int32;  loss_stage, perplexity_stage (Q) fp32: each stage's quantizer outputs;
 *     loss 1 fp32;  z_q like z_e, may be NULL;  residual_out = r_Q like z_e, may be NULL.
 *   Launches: Q quantizer calls (index-only), Q - 1 advance kernels, one finish kernel.  Q = 1: the bits of vqvae_vq_forward_f32.
 * decode:   indices (Q, N) -> z_q = S, (B,D,H,W) or rows with VQVAE_VQ_ROWMAJOR.  An index outside [0, K) never reads a codebook:
 *   the D elements of its row become NaN (the rule of vqvae_vq_decode_indices_f32).
 * backward: the gradients autograd derives when every stage is the reference quantizer and r_{q+1} = r_q - e_q.detach():
 *     grad_z      = grad_zq + g * 2 / (N D) * sum_q (r_q - e_q)
 *     grad_E_q[k] = g * 2 beta / (N D) * sum_{i: idx_q,i = k} (e_k - r_q,i)        shared: the stage results added in stage order
 *   g = *grad_loss (NULL = 1), grad_zq may be NULL (= 0).  grad_z may be NULL; grad_codebooks (a HOST array of Q device pointers, one
 *   when shared) may be NULL, and the workspace is needed only with it.  The codebook gradients come from the sorted segmented sum of
 *   vqvae_vq_backward_f32 on each stage's re-materialised residual: fp64, fixed order.  flags: VQVAE_VQ_ROWMAJOR,
 *   VQVAE_VQ_RESIDUAL_SHARED.                                                                                                   */
#define VQVAE_VQ_RESIDUAL_SHARED 0x10000 /* the residual entries: one codebook for every stage */
VQVAE_API size_t vqvae_vq_residual_workspace_bytes(int64_t N, int K, int D, int Q, int shared);
VQVAE_API int vqvae_vq_residual_forward_f32(const float *z_e, const float *const *codebooks, int64_t B, int D, int H, int W, int K,
                                            int Q, float beta, int flags, float *z_q, int64_t *idx, int32_t *hist,
                                            float *loss_stage, float *perplexity_stage, float *loss, float *residual_out,
                                            void *workspace, size_t workspace_bytes, vqvae_stream_t stream);
VQVAE_API int vqvae_vq_residual_decode_f32(const int64_t *idx, const float *const *codebooks, int64_t B, int D, int H, int W, int K,
                                           int Q, int flags, float *z_q, vqvae_stream_t stream);
VQVAE_API size_t vqvae_vq_residual_backward_workspace_bytes(int64_t N, int K, int D, int Q);
VQVAE_API int vqvae_vq_residual_backward_f32(const float *z_e, const float *const *codebooks, const int64_t *idx,
                                             const float *grad_zq, const float *grad_loss, int64_t B, int D, int H, int W, int K,
                                             int Q, float beta, int flags, float *grad_z, float *const *grad_codebooks,
                                             void *workspace, size_t workspace_bytes, vqvae_stream_t stream);

/* Grouped (product) vector quantization (csrc/vq_grouped.hip; its header is the numeric contract): the D channels of a row are cut
 * into G groups of d = D / G channels, group g is quantized against its own (K, d) codebook E_g (wav2vec 2.0's groups; heads with a
 * codebook each).  A position carries G indices:
 *     slab_g = the channels [g d, (g + 1) d) of every row, dense, in the layout of the input
 *     idx_g, hist_g, loss_g, perplexity_g = vqvae_vq_forward_f32's outputs for (slab_g, E_g, beta)
 *     z_q[row][g d + c] = z + (E_g[idx_g[row]][c] - z);   loss = ((loss_0 + loss_1) + ...) / (float)G on the device
 * 1 <= G <= 16, D % G == 0, 1 <= D <= 256, K <= 16384, N <= INT32_MAX: VQVAE_ERR_UNSUPPORTED outside it, and the sizing calls then
 * return 0.  The same error for a pointer that is not 4-byte aligned (idx, workspace: 8-byte) and for an output that overlaps an
 * input.  `codebooks` is a HOST array of G device pointers (read during the call only).  No host sync, no allocation, no
 * floating-point atomics; every launch on `stream` in one linear chain (capturable); the same bits in every run.
 *
 * forward:  flags = the quantizer's own (VQVAE_VQ_ROWMAJOR, VQVAE_VQ_CODEBOOK_PREPARED, the kernel-selection flags), passed to every
 *   group.  The workspace holds one prepared codebook image per group and the G slabs, so VQVAE_VQ_CODEBOOK_PREPARED means: every
 *   group's image is there from a previous call with the same codebooks and workspace.
 *     idx (G, N) int64 group-major;  hist (G, K) int32;  loss_group, perplexity_group (G) fp32: each group's quantizer outputs;
 *     loss 1 fp32;  z_q like z_e, may be NULL;  slabs_out, may be NULL: the G slabs one after the other, (G, B, d, H, W) or (G, N, d)
 *     with VQVAE_VQ_ROWMAJOR -- what vqvae_vq_ema_update_f32 and the k-means entries take per group.
 *   Launches: one split kernel, G quantizer calls (index-only), one finish kernel.  G = 1: the bits of vqvae_vq_forward_f32.
 * decode:   indices (G, N) -> z_q[row][g d + c] = E_g[idx_g[row]][c], (B,D,H,W) or rows with VQVAE_VQ_ROWMAJOR.  An index outside
 *   [0, K) never reads a codebook: the d elements of that group's segment become NaN, and only those.
 * backward: per group the gradients of vqvae_vq_backward_f32 on (slab_g, E_g, idx_g, grad_zq's channels, g / (float)G), written into
 *   grad_z's channels of the group and grad_codebooks[g] (a HOST array of G device pointers; may be NULL, and the workspace is
 *   needed only with it).  g = *grad_loss (NULL = 1), grad_zq may be NULL (= 0), grad_z may be NULL.  flags: VQVAE_VQ_ROWMAJOR,
 *   VQVAE_VQ_BWD_COMMITMENT (grad_z of beta * mse only; with grad_codebooks: VQVAE_ERR_UNSUPPORTED).                            */
VQVAE_API size_t vqvae_vq_grouped_workspace_bytes(int64_t N, int K, int D, int G);
VQVAE_API int vqvae_vq_grouped_forward_f32(const float *z_e, const float *const *codebooks, int64_t B, int D, int H, int W, int K,
                                           int G, float beta, int flags, float *z_q, int64_t *idx, int32_t *hist,
                                           float *loss_group, float *perplexity_group, float *loss, float *slabs_out,
                                           void *workspace, size_t workspace_bytes, vqvae_stream_t stream);
VQVAE_API int vqvae_vq_grouped_decode_f32(const int64_t *idx, const float *const *codebooks, int64_t B, int D, int H, int W, int K,
                                          int G, int flags, float *z_q, vqvae_stream_t stream);
VQVAE_API size_t vqvae_vq_grouped_backward_workspace_bytes(int64_t N, int K, int D, int G);
VQVAE_API int vqvae_vq_grouped_backward_f32(const float *z_e, const float *const *codebooks, const int64_t *idx,
                                            const float *grad_zq, const float *grad_loss, int64_t B, int D, int H, int W, int K,
                                            int G, float beta, int flags, float *grad_z, float *const *grad_codebooks,
                                            void *workspace, size_t workspace_bytes, vqvae_stream_t stream);

/* recon_loss = mean((x_hat - x)^2) / x_train_var; loss = recon_loss + embedding_loss (main.py:75-76).
 * out3 = {recon_loss, loss, perplexity}: the three values main.py:81-83 copies to the host one by one,
 * packed so that a step needs one D2H copy.  embedding_loss / perplexity are device scalars (NULL = 0);
 * x_hat and x must be 16-byte aligned.  inv_var = 1 / x_train_var.                                    */
VQVAE_API size_t vqvae_recon_loss_workspace_bytes(void);
VQVAE_API int vqvae_recon_loss_f32(const float *x_hat, const float *x, int64_t n, float inv_var,
                                   const float *embedding_loss, const float *perplexity, float *out3,
                                   void *workspace, size_t workspace_bytes, vqvae_stream_t stream);
/* grad_x_hat = g * 2 (x_hat - x) inv_var / n,  g = *grad_loss (NULL = 1) */
VQVAE_API int vqvae_recon_loss_backward_f32(const float *x_hat, const float *x, int64_t n, float inv_var,
                                            const float *grad_loss, float *grad_x_hat,
                                            vqvae_stream_t stream);

/* ------------------------------------------------------- conv backward
 * Data gradients reuse the forward kernels: d/dx of nn.Conv2d(k,s,p) is the ConvTranspose2d with the SAME weight
 * tensor and vice versa (kinds 0<->4, 1<->3, 2<->5; ReLU masks via vqvae_relu_backward_f32); d/dx of the last
 * layer (convT 4x4 s2, Cout<=4) is vqvae_conv_in_forward_f32 on the NCHW gradient with that layer's weight.
 *
 * vqvae_conv_wgrad_f32 -- weight gradient of one conv / conv-transpose layer:
 *     grad_w[ca][cb][ky][kx] = sum_{b,y,x} a[b,y,x,ca] * bt[b, y*stride + ky - pad, x*stride + kx - pad, cb]
 *   nn.Conv2d:          a = grad_y (B,Ho,Wo,Cout), bt = x (B,H,W,Cin)        -> grad_w is (Cout,Cin,k,k)
 *   nn.ConvTranspose2d: a = x (B,H,W,Cin),         bt = grad_y (B,Ho,Wo,Cout) -> grad_w is (Cin,Cout,k,k)
 *   a is row-major; bt is row-major, or an NCHW image tensor when bt_nchw != 0 (first / last layer).
 *   Exact fp32 products (fp32 MFMA), fixed-order reduction: bit-reproducible.  k <= 4.
 *   8x8 a maps with 32-channel multiples (every layer of the path between the first and the last at 32x32 images):
 *   both maps of an image resident in LDS, all taps from one staging (conv_wgrad_map8_kernel); else pixel blocks
 *   per tap.  The workspace holds the per-range partial sums ([range][tap][ca][cb]).                          */
VQVAE_API size_t vqvae_conv_wgrad_workspace_bytes(int CA, int CB, int k);
VQVAE_API int vqvae_conv_wgrad_f32(const float *a, const float *bt, int64_t B, int HA, int WA, int CA,
                                   int HB, int WB, int CB, int k, int stride, int pad, int bt_nchw,
                                   float *grad_w, void *workspace, size_t workspace_bytes,
                                   vqvae_stream_t stream);
/* The same with a product-scheme flag (round 4).  flags = 0: on the map-resident shapes (8x8 a maps, 32-channel multiples) with
 * k >= 3 the products are formed from two fp16 terms per operand on the fp16 matrix cores (conv_wgrad_map8_h2_kernel: <= 2^-21 relative per
 * product, one power-of-two scale per image and operand tile measured inside the kernel, accumulators rescaled exactly between
 * images, still a fixed summation order) -- about three times the fp32 pipe's rate; every other shape runs the fp32 kernels
 * either way.  flags = VQVAE_CONV_EXACT_FP32: vqvae_conv_wgrad_f32 (which is this call with that flag).  Same workspace. */
VQVAE_API int vqvae_conv_wgrad_ex_f32(const float *a, const float *bt, int64_t B, int HA, int WA, int CA,
                                      int HB, int WB, int CB, int k, int stride, int pad, int bt_nchw, int flags,
                                      float *grad_w, void *workspace, size_t workspace_bytes,
                                      vqvae_stream_t stream);
/* grad_b[c] = sum over pixels of grad_y[.., c]; grad_y (B*HW, C) row-major, or (B,C,HW) when nchw != 0.  C <= 256. */
VQVAE_API size_t vqvae_bias_grad_workspace_bytes(int C);
VQVAE_API int vqvae_bias_grad_f32(const float *grad_y, int64_t B, int HW, int C, int nchw, float *grad_b,
                                  void *workspace, size_t workspace_bytes, vqvae_stream_t stream);
/* grad_in = grad_out * (y > 0): backward of y = relu(.)                                                      */
VQVAE_API int vqvae_relu_backward_f32(const float *grad_out, const float *y, int64_t n, float *grad_in,
                                      vqvae_stream_t stream);

/* Data-gradient launches with the element-wise tail of the backward chain in the conv's epilogue (round 4):
 *     y = (mask > 0) ? conv(x) + addend : 0
 *   addend (or NULL): the gradient arriving over a residual layer's skip (models/residual.py:28: d(x + block(x)));
 *   mask   (or NULL): the activation whose ReLU sits below this layer in the forward order -- the conv's own INPUT in the
 *                     forward pass is relu(.) of the layer below, so its data gradient times (input > 0) is that ReLU's
 *                     backward (what vqvae_relu_backward_f32 did in a pass of its own);
 *   both row-major with y's shape, 16-byte aligned, distinct from y.  Split-product kernels only: VQVAE_ERR_UNSUPPORTED with
 *   VQVAE_CONV_EXACT_FP32, and for the first-layer kernel outside its row-band form (the caller then uses the separate passes). */
VQVAE_API int vqvae_conv_forward_ep_f32(int kind, const float *x, const float *packed, const float *bias, int64_t B, int H,
                                        int W, int Cin, int Cout, int flags, const float *addend, const float *mask,
                                        float *y, vqvae_stream_t stream);
VQVAE_API int vqvae_conv_in_forward_ep_f32(const float *x_nchw, const float *packed, const float *bias, int64_t B, int H,
                                           int W, int Cin, int Cout, int flags, const float *mask, float *y,
                                           vqvae_stream_t stream);

/* ------------------------------------------------------- GatedPixelCNN prior
 * pixelcnn/models.py: the masked convolutions run as im2col over their causal tap list followed by the 1x1 conv
 * (vqvae_conv_forward_f32, kind VQVAE_CONV_1x1); these are the memory-bound pieces around it, all on row-major
 * (B,H,W,C) activations, C % 4 == 0, pointers 16-byte aligned.
 *   gather_rows       out[i][:] = table[idx[i]][:]            nn.Embedding (:119-121; class_cond_embedding :68)
 *   im2col_rows       out[b,y,x,t*C+c] = x[b,y+dy[t],x+dx[t],c], 0 outside the map; dy/dx are HOST arrays, ntaps <= 32
 *   gated_activation  out[.., c] = tanh(a) * sigmoid(g), a = t1[.., c] (+ t2[.., c]) (+ cond[b][c]),
 *                     g = the same at channel dim + c (GatedActivation :21-27 with the sums of :71 / :77);
 *                     t1, t2 (B,HW,2*dim), cond (B,2*dim), out (B,HW,dim); t2 and cond may be NULL
 *   add               out = a + b                              the horizontal residual (:79)                 */
VQVAE_API int vqvae_gather_rows_f32(const int64_t *idx, const float *table, int64_t n, int C, int rows,
                                    float *out, vqvae_stream_t stream);
VQVAE_API int vqvae_im2col_rows_f32(const float *x, int64_t B, int H, int W, int C, int ntaps,
                                    const int8_t *dy, const int8_t *dx, float *out, vqvae_stream_t stream);
/* A masked convolution WITHOUT the im2col pass (round 4): a stride-1 conv over an explicit list of ntaps <= 16 taps, tap t reading
 * the input at (y + dy[t], x + dx[t]) (zero outside the map; |dy|, |dx| <= 7).  w is (Cout, Cin, ntaps) contiguous -- a masked
 * conv's own (Cout, Cin, kh, kw) tensor when the list enumerates (ky, kx) in row-major order (GatedMaskedConv2d's vertical
 * (k//2+1) x k and horizontal 1 x (k//2+1) stacks, pixelcnn/models.py:45-58).  dy / dx are HOST arrays.  Same kernels, packed
 * image and flags as vqvae_conv_forward_f32 (on 8x8 maps with 32-channel multiples: the tile-resident kernel, every tap from
 * one parked image).                                                                                                   */
VQVAE_API size_t vqvae_conv_taps_packed_bytes(int ntaps, int Cin, int Cout);
VQVAE_API int vqvae_conv_taps_pack_f32(const float *w, int ntaps, const int8_t *dy, const int8_t *dx, int Cin, int Cout,
                                       float *packed, vqvae_stream_t stream);
VQVAE_API int vqvae_conv_taps_forward_f32(const float *x, const float *packed, const float *bias, int64_t B, int H, int W,
                                          int Cin, int Cout, int ntaps, const int8_t *dy, const int8_t *dx, int flags,
                                          float *y, vqvae_stream_t stream);
/* the same with vqvae_conv_forward_ep_f32's epilogue, y = (mask > 0) ? conv + addend : 0: a tap list longer than 16 runs as a chain of
 * launches over slices of it, each adding to the previous one's result (the first GatedMaskedConv2d's 4 x 7 vertical stack)      */
VQVAE_API int vqvae_conv_taps_forward_ep_f32(const float *x, const float *packed, const float *bias, int64_t B, int H, int W,
                                             int Cin, int Cout, int ntaps, const int8_t *dy, const int8_t *dx, int flags,
                                             const float *addend, const float *mask, float *y, vqvae_stream_t stream);
VQVAE_API int vqvae_gated_activation_f32(const float *t1, const float *t2, const float *cond, int64_t B,
                                         int HW, int dim, float *out, vqvae_stream_t stream);
VQVAE_API int vqvae_add_f32(const float *a, const float *b, int64_t n, float *out, vqvae_stream_t stream);

/* ------------------------------------------------------- GatedPixelCNN prior: backward (csrc/pixelcnn_backward.hip)
 * What loss.backward() of pixelcnn/gated_pixelcnn.py:78-111 needs beyond the conv path's entries.  Row-major activations, channel
 * counts % 4 == 0 and 16-byte aligned tensors where noted.  No floating-point atomics: every result is bit-reproducible.
 *
 * vqvae_conv_taps_wgrad_f32 -- weight gradient of a tap-list convolution (vqvae_conv_taps_forward_f32's tap semantics):
 *     grad_w[co][ci][t] = sum_{b,y,x} grad_y[b,y,x,co] * x[b, y+dy[t], x+dx[t], ci]      (0 outside the map)
 *   grad_w is the weight's own (Cout, Cin, kh, kw) tensor for a list in (ky, kx) order.  ntaps <= 32, |dy|, |dx| <= 7 (HOST arrays),
 *   Cin, Cout % 4 == 0, grad_y / x 16-byte aligned.  Exact fp32 products (fp32 MFMA, the pixel as the reduction index); maps of at
 *   most 8 x 8 with 32-channel multiples stage both maps of an image in LDS once and serve every tap from there, other shapes run
 *   per tap over 32-pixel blocks.  Partial sums per image / pixel range in the workspace, combined in a fixed order.  The workspace
 *   size depends on (ntaps, Cin, Cout) only; 0 = unsupported.                                                                  */
VQVAE_API size_t vqvae_conv_taps_wgrad_workspace_bytes(int ntaps, int Cin, int Cout);
VQVAE_API int vqvae_conv_taps_wgrad_f32(const float *grad_y, const float *x, int64_t B, int H, int W, int Cin, int Cout, int ntaps,
                                        const int8_t *dy, const int8_t *dx, float *grad_w, void *workspace, size_t workspace_bytes,
                                        vqvae_stream_t stream);
/* Data gradient of a tap-list convolution: grad_x = conv over the NEGATED taps of grad_y with the per-tap transposed weight, i.e.
 * vqvae_conv_taps_forward_ep_f32(grad_y, packed, NULL, B, H, W, Cout, Cin, ntaps, -dy, -dx, 0, addend, NULL, grad_x) -- the
 * forward's kernels and product scheme; the addend epilogue adds the other gradient terms of the same tensor.  This packs taps
 * [t0, t0 + ntaps) of the forward weight w (Cout, Cin, wtaps) for that call (ntaps <= 16: longer lists run as slices, like the
 * forward); dy / dx are the FORWARD offsets of the slice (HOST arrays).  The buffer holds the packed image and, behind it, the
 * transposed weight the pack reads (no temporary allocation): vqvae_conv_taps_pack_dgrad_bytes.                               */
VQVAE_API size_t vqvae_conv_taps_pack_dgrad_bytes(int ntaps, int Cin, int Cout);
VQVAE_API int vqvae_conv_taps_pack_dgrad_f32(const float *w, int wtaps, int t0, int ntaps, const int8_t *dy, const int8_t *dx, int Cin,
                                             int Cout, float *packed, vqvae_stream_t stream);
/* Backward of vqvae_gated_activation_f32: (a|g) recomputed in the forward's order ((t1 + t2) + cond, same device functions),
 *     grad_pre[.., c] = go sigma(g) (1 - tanh^2 a),   grad_pre[.., dim + c] = go tanh(a) sigma(g) (1 - sigma(g))
 *   grad_out (B,HW,dim), grad_pre (B,HW,2*dim).  With cond: grad_cond[b] = [grad_cond_in[b] +] sum over HW of grad_pre[b] (fp64 in a
 *   fixed order), (B, 2*dim) -- the class embedding's gradient per image; grad_cond_in may alias grad_cond, so that the two gates
 *   of one layer share one buffer.  grad_cond / grad_cond_in may be NULL; they need cond.                                      */
VQVAE_API int vqvae_gated_activation_backward_f32(const float *t1, const float *t2, const float *cond, const float *grad_out, int64_t B,
                                                  int HW, int dim, float *grad_pre, const float *grad_cond_in, float *grad_cond,
                                                  vqvae_stream_t stream);
/* Backward of vqvae_gather_rows_f32 (nn.Embedding): grad_table[k] = sum_{i: idx_i = k} grad_out[i], (rows, C); rows nobody read are 0.
 * Out-of-range indices: the forward clamps them into [0, rows), and so does this -- the gradient goes to the row the forward read.
 * The stable-sort segmented sum of vqvae_vq_backward_f32: indices radix-sorted by row (ascending source order within a row),
 * chunks of 512 sorted rows summed in fp64 by one workgroup, a row's chunks combined in order.  Any C.                       */
VQVAE_API size_t vqvae_gather_rows_backward_workspace_bytes(int64_t n, int C, int rows);
VQVAE_API int vqvae_gather_rows_backward_f32(const int64_t *idx, const float *grad_out, int64_t n, int C, int rows, float *grad_table,
                                             void *workspace, size_t workspace_bytes, vqvae_stream_t stream);
/* nn.CrossEntropyLoss() (mean) over N rows of K logits, row-major (B,H,W,K) as the prior's last conv writes them; int64 targets.
 *   loss: one device float, the mean of (m + log sum exp(l - m)) - l[target] with m the row maximum, summed in fp64 in a fixed
 *   order.  backward: grad_logits = g (softmax - onehot) / N, g = *grad_loss (device scalar; NULL = 1).  A target outside [0, K)
 *   makes the loss and that row's gradient NaN (no host check: nothing synchronises).                                          */
VQVAE_API size_t vqvae_cross_entropy_workspace_bytes(int64_t N);
VQVAE_API int vqvae_cross_entropy_f32(const float *logits, const int64_t *targets, int64_t N, int K, float *loss, void *workspace,
                                      size_t workspace_bytes, vqvae_stream_t stream);
VQVAE_API int vqvae_cross_entropy_backward_f32(const float *logits, const int64_t *targets, int64_t N, int K, const float *grad_loss,
                                               float *grad_logits, vqvae_stream_t stream);
/* grad_b[c] = sum over the P rows of grad_y (P, C) row-major, any C (vqvae_bias_grad_f32 stops at 256): fp64, fixed order.       */
VQVAE_API size_t vqvae_bias_grad_wide_workspace_bytes(int C);
VQVAE_API int vqvae_bias_grad_wide_f32(const float *grad_y, int64_t P, int C, float *grad_b, void *workspace, size_t workspace_bytes,
                                       vqvae_stream_t stream);

/* ------------------------------------------------------- what a training reduction would launch (csrc/train_reduce.hip)
 * Host logic only (no GPU needed; without a device it assumes 256 CUs): the plan the entry point itself launches from, for tests and
 * tools that must know how a batch is split.  `what` selects the reduction and the meaning of dims[0 .. ndims):
 *   VQVAE_TRAIN_PLAN_CONV_WGRAD       B, HA, WA, CA, HB, WB, CB, k, stride, pad, bt_nchw, flags      (vqvae_conv_wgrad_ex_f32)
 *   VQVAE_TRAIN_PLAN_CONV_TAPS_WGRAD  B, H, W, Cin, Cout, ntaps, dy[0 .. ntaps), dx[0 .. ntaps)      (vqvae_conv_taps_wgrad_f32)
 *   VQVAE_TRAIN_PLAN_BIAS_GRAD        P = B * HW, C                                                  (vqvae_bias_grad_f32)
 *   VQVAE_TRAIN_PLAN_BIAS_GRAD_WIDE   P, C                                                           (vqvae_bias_grad_wide_f32)
 *   VQVAE_TRAIN_PLAN_SEGSUM           n, keys, C      (the sorted segmented sum of vqvae_vq_backward_f32: N, K, D; of
 *                                                      vqvae_vq_ema_update_f32: N, K, D; of vqvae_gather_rows_backward_f32: n, rows, C)
 * out[0 .. 8): the kernel (VQVAE_TRAIN_KERNEL_*); the items that are split (images for the map-resident and image-operand kernels,
 * 32-pixel blocks for the per-tap kernels, rows); splits; items per split; items in the last split (0: it is empty); the split count
 * the rule asks for before it is clamped to its cap and to the items; and two kernel-specific values: waves along ca and cb
 * (CONV_WGRAD_MAP8*), tap groups and taps per group (CONV_TAPS_WGRAD_MAP), rows per unit and the unit bound (SEGSUM: its splits are
 * the unit bound too -- how many units hold rows depends on the data, ceil(count_k / rows per unit) per key), else 0.
 * Returns VQVAE_OK, or the error the entry point gives for these dimensions (VQVAE_ERR_SHAPE also for a wrong ndims).             */
#define VQVAE_TRAIN_PLAN_CONV_WGRAD      0
#define VQVAE_TRAIN_PLAN_CONV_TAPS_WGRAD 1
#define VQVAE_TRAIN_PLAN_BIAS_GRAD       2
#define VQVAE_TRAIN_PLAN_BIAS_GRAD_WIDE  3
#define VQVAE_TRAIN_PLAN_SEGSUM          4
#define VQVAE_TRAIN_KERNEL_CONV_WGRAD_IMG      1   /* conv_wgrad_img_kernel                                  */
#define VQVAE_TRAIN_KERNEL_CONV_WGRAD_MAP8_H2  2   /* conv_wgrad_map8_h2_kernel (two-term fp16 products)      */
#define VQVAE_TRAIN_KERNEL_CONV_WGRAD_MAP8     3   /* conv_wgrad_map8_kernel (fp32 products)                  */
#define VQVAE_TRAIN_KERNEL_CONV_WGRAD          4   /* conv_wgrad_kernel: any map, per tap                     */
#define VQVAE_TRAIN_KERNEL_CONV_TAPS_WGRAD_MAP 5   /* taps_wgrad_map_kernel                                   */
#define VQVAE_TRAIN_KERNEL_CONV_TAPS_WGRAD_BLK 6   /* taps_wgrad_blk_kernel                                   */
#define VQVAE_TRAIN_KERNEL_BIAS_GRAD           7   /* bias_grad_partial_kernel                                */
#define VQVAE_TRAIN_KERNEL_BIAS_GRAD_WIDE      8   /* bias_wide_partial_kernel                                */
#define VQVAE_TRAIN_KERNEL_SEGSUM              9   /* segsum_kernel                                           */
VQVAE_API int vqvae_train_reduction_plan(int what, const int64_t *dims, int ndims, int64_t *out);

/* ------------------------------------------------------- GatedPixelCNN prior: cached sampler (csrc/pixelcnn_sample.hip)
 * GatedPixelCNN.generate (pixelcnn/models.py:129-142) without its H*W full forwards.  The prior is causal, so the sampler keeps each
 * layer's state and computes only what the next pixel needs: per row, the vertical stacks (hv_L, out_v) and vert_to_horiz of every
 * layer and column; per position, the horizontal stacks (out_h) of every layer, the output head, and one draw.  One workgroup per
 * image loops over the whole map; nothing is shared between images, nothing synchronises across workgroups.  fp32 products with
 * fp32 accumulation (fmaf chains); the gate is vqvae_gated_activation_f32's expression in the reference's order of sums.
 *
 * Supported (VQVAE_ERR_UNSUPPORTED otherwise): GatedPixelCNN's own structure (layer 0: k = 7, mask 'A', no residual; the others:
 * k = 3, mask 'B'; output head 512 wide); dim % 4 == 0 and dim <= 256; 2 <= K <= 8192; any n_classes >= 1 and n_layers >= 1;
 * square maps H = W from 1 to 128 (the reference's crops :70, :74 only make sense for square maps); packed image and workspace
 * 16-byte aligned.
 *
 * vqvae_pixelcnn_sample_pack_f32 -- writes every parameter into the caller-owned sampler image (vqvae_pixelcnn_sample_packed_bytes;
 *   0 = unsupported).  params: a HOST array of 9 n_layers + 5 device pointers in GatedPixelCNN.named_parameters() order:
 *   embedding.weight; per layer class_cond_embedding.weight, vert_stack.{weight,bias}, vert_to_horiz.{weight,bias},
 *   horiz_stack.{weight,bias}, horiz_resid.{weight,bias}; output_conv.0.{weight,bias}, output_conv.2.{weight,bias}.  The taps
 *   make_causal zeroes are never read and not packed.
 * vqvae_pixelcnn_sample_f32 -- label (B,) int64 (clamped into [0, n_classes) like vqvae_gather_rows_f32), uniforms (B, H, W) fp32
 *   in [0, 1) -> samples (B, H, W) int64; logits (B, K, H, W), the NCHW logits each position was drawn from (may be NULL);
 *   status (B,) int32, 0 or VQVAE_SAMPLE_* bits.  The draw: m = max l, e_k = exp(l_k - m), C_k the running sums of e_k in ascending
 *   k (a fixed order), S = C_{K-1}; the code is the smallest k with u S < C_k, or, where rounding leaves none, the largest k with
 *   e_k > 0.  A position whose logits are not all finite sets VQVAE_SAMPLE_NONFINITE and that image gets code 0 from there on.
 *   workspace: vqvae_pixelcnn_sample_workspace_bytes (0 = unsupported), never read before the call writes it.
 * vqvae_pixelcnn_sample_ex_f32 -- the same call with sampling controls; vqvae_pixelcnn_sample_f32 is it with (1, 0, 1, NULL), which
 *   runs the plain kernel.  VQVAE_ERR_SHAPE for a temperature that is not finite and > 0, top_k < 0, top_p outside (0, 1] or NaN;
 *   every other check as above, all before any HIP call.  Same packed image, same workspace size.  In order, per position:
 *     top_k (1 <= top_k < K; 0 or >= K: off): code j stays iff #{i : l_i > l_j or (l_i == l_j and i < j)} < top_k, on the raw fp32
 *       logits: exactly top_k codes, ties at the threshold go to the lower index; top_k = 1 is greedy decoding.
 *     temperature: m = max l, e_k = expf((l_k - m) / temperature) for the codes that stay (a correctly rounded divide, exact at 1),
 *       0 for the others.
 *     top_p (1: off): rank the codes by (l descending, index ascending); with S the sum of all e_k, code k stays iff the mass of
 *       the codes ranked before it is < top_p S, so the first always stays; the others get e_k = 0.  The masses are fp32 sums in a
 *       fixed order that depends on K and the logits only (no floating-point atomics): the same bits in every run and batch.
 *     the draw: the rule above over the e_k that remain (running sums in ascending k, the smallest k with u S' < C_k, the same
 *       fallback).
 *   given (B, H, W) int64, may be NULL: a value >= 0 fixes the code of that position -- it is written to samples, the uniform is
 *   ignored and the layers' state advances as after a draw of that code; a negative value means draw.  A value >= K sets
 *   VQVAE_SAMPLE_GIVEN_RANGE and that image gets code 0 from there on.  logits, when asked for, are written at given positions
 *   too (teacher-forced logits); when they are not, the head is not computed there, which changes no other output.  Logits are
 *   not checked for VQVAE_SAMPLE_NONFINITE at given positions.                                                                   */
#define VQVAE_SAMPLE_NONFINITE 1
#define VQVAE_SAMPLE_GIVEN_RANGE 2
VQVAE_API size_t vqvae_pixelcnn_sample_packed_bytes(int K, int dim, int n_layers, int n_classes);
VQVAE_API int vqvae_pixelcnn_sample_pack_f32(const float *const *params, int n_params, int K, int dim, int n_layers, int n_classes,
                                             void *packed, size_t packed_bytes, vqvae_stream_t stream);
VQVAE_API size_t vqvae_pixelcnn_sample_workspace_bytes(int64_t B, int H, int W, int dim, int n_layers);
VQVAE_API int vqvae_pixelcnn_sample_f32(const void *packed, size_t packed_bytes, const int64_t *label, const float *uniforms, int64_t B,
                                        int H, int W, int K, int dim, int n_layers, int n_classes, int64_t *samples, float *logits,
                                        int32_t *status, void *workspace, size_t workspace_bytes, vqvae_stream_t stream);
VQVAE_API int vqvae_pixelcnn_sample_ex_f32(const void *packed, size_t packed_bytes, const int64_t *label, const float *uniforms,
                                           int64_t B, int H, int W, int K, int dim, int n_layers, int n_classes, float temperature,
                                           int top_k, float top_p, const int64_t *given, int64_t *samples, float *logits,
                                           int32_t *status, void *workspace, size_t workspace_bytes, vqvae_stream_t stream);

/* ------------------------------------------------------------------- whole path
 * models/vqvae.py:29-44 as ONE call: Encoder (models/encoder.py:28-43) -> pre_quantization_conv (models/vqvae.py:33)
 * -> VectorQuantizer (models/quantizer.py:45-76) -> Decoder (models/decoder.py:27-39).  The caller owns every buffer:
 * the packed weights (built once per weight version with vqvae_weights_pack_f32), the activation workspace
 * (vqvae_workspace_bytes) and, optionally, a persistent quantizer workspace that keeps the prepared codebook images
 * across calls.  Nothing is allocated or synchronised; every kernel goes to `stream`.                                 */
typedef struct VqvaeDims {          /* VQVAE(h_dim, res_h_dim, n_res_layers, n_embeddings, embedding_dim, beta), vqvae.py:11-12 */
    int h_dim, res_h_dim, n_res_layers, n_embeddings, embedding_dim, in_ch;
    float beta;
} VqvaeDims;

typedef struct VqvaeRawWeights {    /* device pointers to the parameters in torch's layouts; names = state_dict keys */
    const float *enc0_w, *enc0_b;           /* encoder.conv_stack.0  (h/2, in_ch, 4, 4), (h/2)                      */
    const float *enc2_w, *enc2_b;           /* encoder.conv_stack.2  (h, h/2, 4, 4), (h)                            */
    const float *enc4_w, *enc4_b;           /* encoder.conv_stack.4  (h, h, 3, 3), (h)                              */
    const float *enc_res_w1, *enc_res_w2;   /* encoder.conv_stack.5.stack.0.res_block.{1,3}  (Rh, h, 3, 3), (h, Rh, 1, 1) */
    const float *pre_w, *pre_b;             /* pre_quantization_conv (D, h, 1, 1), (D)                              */
    const float *codebook;                  /* vector_quantization.embedding.weight (K, D)                          */
    const float *dec0_w, *dec0_b;           /* decoder.inverse_conv_stack.0  (D, h, 3, 3), (h)   [ConvTranspose2d]  */
    const float *dec_res_w1, *dec_res_w2;   /* decoder.inverse_conv_stack.1.stack.0.res_block.{1,3}                 */
    const float *dec2_w, *dec2_b;           /* decoder.inverse_conv_stack.2  (h, h/2, 4, 4), (h/2)                  */
    const float *dec4_w, *dec4_b;           /* decoder.inverse_conv_stack.4  (h/2, in_ch, 4, 4), (in_ch)            */
} VqvaeRawWeights;

typedef struct VqvaeWeights {       /* what the whole-path entry points consume: packed images + biases + codebook */
    VqvaeDims dims;
    const float *enc0, *enc0_b, *enc2, *enc2_b, *enc4, *enc4_b, *enc_res_w1, *enc_res_w2, *pre, *pre_b, *codebook;
    const float *dec0, *dec0_b, *dec_res_w1, *dec_res_w2, *dec2, *dec2_b, *dec4, *dec4_b;
} VqvaeWeights;

/* Which product scheme do these WEIGHTS call for?  (round 5)  The default two-term fp16 scheme carries one power-of-two scale per output
 * channel of every weight tensor and one per image of every activation map; a layer whose INPUT channels still differ by many binades
 * after that normalisation pairs its largest weights with activations far below their image's maximum, whose second fp16 term
 * underflows -- the regime in which the default path is 100x further from fp64 than the reference's fp32.  That is a
 * property of the checkpoint: this call measures, per layer, log2(max_c r[c] / min_c r[c]) with r[c] = max over (o, taps) of
 * |w[o, c]| / max |w[o, ., .]| (spread_log2_host: 11 floats in VqvaeRawWeights' order of the weight tensors, may be NULL) and sets
 * *recommended_flags to VQVAE_FWD_CONV_BF16_SPLIT when any layer behind the first exceeds VQVAE_RANGE_SPREAD_LIMIT_LOG2 binades, else 0.
 * OR it into vqvae_forward_f32's vq_flags / the _ex_ entries' flags (the Python layer and integration/vqvae_hip_stub.py do, once per
 * weight version).  Launches 11 one-workgroup kernels on `stream` and SYNCHRONISES it; scratch_device: >= 64 bytes of device memory. */
#define VQVAE_RANGE_SPREAD_LIMIT_LOG2 10.0f
VQVAE_API int vqvae_weights_range_check_f32(const VqvaeDims *dims, const VqvaeRawWeights *raw, float *spread_log2_host,
                                            int *recommended_flags, void *scratch_device, size_t scratch_bytes, vqvae_stream_t stream);

/* Bytes of the one buffer that holds every packed weight image (0: unsupported dims). */
VQVAE_API size_t vqvae_weights_packed_bytes(const VqvaeDims *dims);
/* Packs every layer into `packed` and fills `out` (its bias / codebook pointers alias `raw`'s: keep those alive). */
VQVAE_API int vqvae_weights_pack_f32(const VqvaeDims *dims, const VqvaeRawWeights *raw, void *packed, size_t packed_bytes,
                                     VqvaeWeights *out, vqvae_stream_t stream);
/* Bytes of activation workspace for a (B, in_ch, H, W) batch (H, W multiples of 4; 0: unsupported). */
VQVAE_API size_t vqvae_workspace_bytes(const VqvaeDims *dims, int64_t B, int H, int W);
VQVAE_API size_t vqvae_workspace_ze_offset(const VqvaeDims *dims, int64_t B, int H, int W);   /* bytes from the workspace's start to z_e (0: unsupported shape) */

/* ResidualStack.forward (models/residual.py:47-51): n_layers applications of the SAME layer, then F.relu if
 * VQVAE_CONV_RELU_OUT; VQVAE_CONV_RELU_IN applies the first layer's in-place ReLU on read.  x, y, tmp row-major
 * (B,H,W,C); the result is in y; tmp (same size) is needed when n_layers > 1; x is not modified.                    */
VQVAE_API int vqvae_resstack_f32(const float *packed_w1, const float *packed_w2, const float *x, int64_t B, int H, int W,
                                 int C, int Rh, int n_layers, int flags, float *y, float *tmp, vqvae_stream_t stream);

/* Encoder + pre_quantization_conv: x (B,in_ch,H,W) NCHW -> z_e (B,H/4,W/4,D) ROW-MAJOR (the layout vqvae_vq_forward_f32
 * takes with VQVAE_VQ_ROWMAJOR).  workspace: vqvae_workspace_bytes(dims, B, H, W) is always enough; the entry itself needs the two
 * activation buffers, plus -- where h_dim is not 32 / 64 / 128 or res_h_dim > 32 (the generic residual path) -- one hidden map of
 * B * H/4 * W/4 * res_h_dim floats, and uses room beyond that for the per-image maxima (without them every layer measures its own).
 * On 32x32 RGB images with h_dim 128 and two residual layers (the reference's defaults) the encoder is two launches
 * (models/encoder.py:29-34, then :35-38 + models/vqvae.py:33) and the decoder two (models/decoder.py:28-30, :31-35): no
 * intermediate map is written inside a launch; other shapes run layer by layer through the kernels of the per-layer
 * entry points above.                                                                                                  */
VQVAE_API int vqvae_encoder_f32(const VqvaeWeights *w, const float *x, int64_t B, int H, int W, float *z_e,
                                void *workspace, size_t workspace_bytes, vqvae_stream_t stream);
/* Decoder: z_q (B,h,w,D) row-major -> x_hat (B,in_ch,4h,4w) NCHW. */
VQVAE_API int vqvae_decoder_f32(const VqvaeWeights *w, const float *z_q, int64_t B, int h, int w_, float *x_hat,
                                void *workspace, size_t workspace_bytes, vqvae_stream_t stream);
/* The same two with a product-scheme selector (flags: 0, VQVAE_FWD_CONV_BF16_SPLIT or VQVAE_FWD_CONV_EXACT_FP32, below). */
VQVAE_API int vqvae_encoder_ex_f32(const VqvaeWeights *w, const float *x, int64_t B, int H, int W, int flags, float *z_e,
                                   void *workspace, size_t workspace_bytes, vqvae_stream_t stream);
VQVAE_API int vqvae_decoder_ex_f32(const VqvaeWeights *w, const float *z_q, int64_t B, int h, int w_, int flags, float *x_hat,
                                   void *workspace, size_t workspace_bytes, vqvae_stream_t stream);

/* Whole-path product scheme (round 4), OR-ed into vqvae_forward_f32's vq_flags / the flags of the _ex_ entries above:
 *   default (neither bit)       two-term fp16 products (3 MFMAs per fp32 product, <= 2^-21 relative per product) with one
 *                               power-of-two scale per OUTPUT CHANNEL of every weight tensor and one per image for the
 *                               activations; on the reference's default shapes the four fused kernels;
 *   VQVAE_FWD_CONV_BF16_SPLIT   every layer through the per-layer kernels with three-term bf16 products (6 MFMAs per fp32
 *                               product, <= 3 * 2^-24 relative per product, fp32's exponent range: no operand scales at all);
 *   VQVAE_FWD_CONV_EXACT_FP32   every layer through the exact-fp32 MFMA kernels (v_mfma_f32_32x32x2_f32: fp32 products,
 *                               fp32 accumulation -- the reference's own arithmetic up to summation order).
 * The two selectors are the escape hatch for callers whose data defeats the fp16 scheme's range assumptions (DESIGN.md section 5,
 * "error bound per output channel") and the honest side-by-side legs of bench.py.  Both at once: VQVAE_ERR_UNSUPPORTED.   */
#define VQVAE_FWD_CONV_BF16_SPLIT 0x1000
#define VQVAE_FWD_CONV_EXACT_FP32 0x2000
/* Test hook (round 5): on the default shapes' fused path -- where the encoder's last kernel quantizes a z_e that never leaves the chip --
 * vqvae_forward_f32 ALSO writes the very z_e rows that kernel quantizes, row-major (B*H/4*W/4, D), at vqvae_workspace_ze_offset() of the
 * workspace (a separate instance of the kernel; idx must be given).  tests/test_model_gpu.py feeds those bits to the CPU oracle.
 * Ignored where the quantizer runs as its own launch (z_e is in the workspace there anyway).                                          */
#define VQVAE_FWD_DEBUG_ZE        0x4000

/* VQVAE.forward: x -> (embedding_loss, x_hat, perplexity) (models/vqvae.py:44); idx (B*H/4*W/4 int64) is optional.
 * vq_flags: VQVAE_VQ_CODEBOOK_PREPARED (only meaningful with a persistent vq_workspace of vqvae_vq_workspace_bytes),
 * VQVAE_VQ_EXACT_SWEEP / _BF16_FILTER, VQVAE_FWD_CONV_BF16_SPLIT / _EXACT_FP32.  vq_workspace may
 * be NULL (then the codebook images are rebuilt inside `workspace` on every call).                                                                       */
VQVAE_API int vqvae_forward_f32(const VqvaeWeights *w, const float *x, int64_t B, int H, int W, int vq_flags,
                                float *x_hat, float *loss, float *perplexity, int64_t *idx, void *workspace,
                                size_t workspace_bytes, void *vq_workspace, size_t vq_workspace_bytes,
                                vqvae_stream_t stream);

/* The index wire format as single entry points -- what the PixelCNN prior is trained on and sampled into:
 *   vqvae_encode_f32   x (B,C,H,W) -> min_encoding_indices (B*H/4*W/4 int64), README.md:56 / visualization.ipynb:84-90 (encode_data);
 *   vqvae_decode_f32   indices -> x_hat (B,C,4h,4w), visualization.ipynb:358-365 / 642-650 (one-hot @ embedding -> decoder).
 * On the default shapes' fused path (32x32 images, h_dim 128, two residual layers, K a multiple of 128 up to 1024, D = 64) neither
 * touches a latent map: the encoder's last kernel quantizes its own z_e and writes 512 bytes of indices per image (no z_e, no z_q:
 * 12 KiB in, 0.5 KiB out), and the decoder's first kernel takes each latent pixel's row straight from the codebook (0.5 KiB in, 12 KiB
 * out).  Other shapes run encoder -> stand-alone quantizer / row gather -> decoder through the workspace.  Indices equal
 * vqvae_forward_f32's bit for bit; x_hat equals the decoder's on the same z_q bit for bit.  An index outside [0, K) never reads the
 * codebook: that latent pixel enters the first conv as NaN on EVERY path (fused gather and workspace gather alike) and -- the fused
 * ReLUs keep a NaN as nn.ReLU does -- shows as NaN pixels of its image's x_hat; no other image is affected.  The Python layer
 * validates foreign indices on the host and raises, as the reference's scatter does.  workspace: vqvae_workspace_bytes(dims, B, H, W) (decode: H = 4h, W = 4w); vq_workspace /
 * vq_flags as for vqvae_forward_f32; decode's flags: VQVAE_FWD_CONV_BF16_SPLIT / _EXACT_FP32 or 0.                                   */
VQVAE_API int vqvae_encode_f32(const VqvaeWeights *w, const float *x, int64_t B, int H, int W, int vq_flags, int64_t *idx,
                               void *workspace, size_t workspace_bytes, void *vq_workspace, size_t vq_workspace_bytes,
                               vqvae_stream_t stream);
VQVAE_API int vqvae_decode_f32(const VqvaeWeights *w, const int64_t *idx, int64_t B, int h, int w_, int flags, float *x_hat,
                               void *workspace, size_t workspace_bytes, vqvae_stream_t stream);

/* The same step in PARTS, for callers that spread a large batch over several streams (the default shapes' path only: 32x32
 * images, h_dim 128, two residual layers, K a multiple of 128 up to 1024, D = 64; VQVAE_ERR_UNSUPPORTED otherwise -- use vqvae_forward_f32):
 *   vqvae_forward_begin_f32   codebook images + cleared histogram, on `stream`;
 *   vqvae_forward_part_f32    images [b0, b0 + Bc) of the batch of B, on ANY stream ordered behind the begin (b0 and every Bc
 *                             but the last multiples of 64); x, x_hat, idx and both workspaces are the WHOLE batch's, as
 *                             vqvae_forward_f32 would get them; parts must not overlap;
 *   vqvae_forward_end_f32     loss and perplexity of the whole batch, on a stream ordered behind every part.
 * Results are bit-identical to one vqvae_forward_f32 call.  Why: with the four kernels of the whole batch one after the other,
 * 10-15 % of every kernel's workgroup slots stand empty while it ramps up and while its last workgroups finish; kernels of
 * different parts on different streams can fill those ends -- measured between -7 % and +9 % per step depending on the box
 * (profiles/r03_notes.txt section 11), which is why the Python host layer does not do it by default.
 * The library creates no streams or events: ordering between the streams is the caller's (hipStreamWaitEvent / torch
 * wait_stream).
 * Checked on the host since round 5 (a record per workspace pointer, opened by begin and closed by end; VQVAE_ERR_SHAPE on violation):
 * every part repeats begin's B, H, W, flags and quantizer workspace; parts do not overlap; end finds [0, B) covered exactly once (a part
 * leaves one loss partial per four images and adds to the histogram atomically: a gap or a repeat would give wrong loss / perplexity).
 * What stays the caller's, because no launch-time check can see it: begin / parts / end are ORDERED on their streams as described, and
 * every buffer stays alive, untouched by other work, until the stream of `end` has passed it.  With vq_workspace == NULL the codebook
 * images live inside `workspace`, prepared by begin -- parts never prepare them. */
VQVAE_API int vqvae_forward_begin_f32(const VqvaeWeights *w, int64_t B, int H, int W, int vq_flags, void *workspace,
                                      size_t workspace_bytes, void *vq_workspace, size_t vq_workspace_bytes,
                                      vqvae_stream_t stream);
VQVAE_API int vqvae_forward_part_f32(const VqvaeWeights *w, const float *x, int64_t B, int64_t b0, int64_t Bc, int H, int W,
                                     int vq_flags, float *x_hat, int64_t *idx, void *workspace, size_t workspace_bytes,
                                     void *vq_workspace, size_t vq_workspace_bytes, vqvae_stream_t stream);
VQVAE_API int vqvae_forward_end_f32(const VqvaeWeights *w, int64_t B, int H, int W, float *loss, float *perplexity,
                                    void *workspace, size_t workspace_bytes, vqvae_stream_t stream);
/* Host-side state of the step in parts (the only state the library keeps): one record per `workspace` pointer in a process-wide table,
 * opened by begin, closed by end.  A part whose launches fail gives its claim back (it may be retried); a step that will not be
 * finished is dropped with vqvae_forward_abort_f32(workspace) -- otherwise its record stays until the next begin on the same pointer
 * replaces it (a freed and reused pointer would inherit it only until that begin).  Always VQVAE_OK. */
VQVAE_API int vqvae_forward_abort_f32(void *workspace);

/* ---------------------------------------------------------------- optimizer
 * torch.optim.Adam(...).step() (main.py:59,80; pixelcnn/gated_pixelcnn.py:78-99) -- Adam, AMSGrad and AdamW -- over every tensor of an
 * optimizer in ONE elementwise launch, plus the global gradient norm of torch.nn.utils.clip_grad_norm_.  Additive to ABI 9.
 *
 * The plan is a blob the caller builds on the host (vqvae_adam_plan_write, pure host code) and copies to the device:
 *   [header: 8 int64 = magic, n_tensors, n_chunks, chunk elements, offset of the tensor table, of the chunk list, of the scratch, bytes]
 *   [tensor table: per tensor 64 bytes = param, grad, exp_avg, exp_avg_sq, max_exp_avg_sq, step (device pointers), int64 numel,
 *    int32 group, int32 0]
 *   [chunk list: per chunk 2 int32 = tensor, index: elements [index * chunk, ...) of that tensor; tensors in table order, a tensor's
 *    chunks in ascending order; a tensor with numel 0 or a NULL grad has none]
 *   [scratch: 80 bytes per tensor, written by the step's first kernel on the device]
 * grad[i] == NULL skips tensor i: its parameter, state and counter are untouched.  max_exp_avg_sq == NULL (the array, or an entry) turns
 * AMSGrad off for that tensor.  step[i] is ONE fp32 scalar on the device per tensor (torch's capturable / fused state layout), advanced
 * by the step itself: nothing reads device memory from the host.  All arrays fp32, 4-byte aligned; tensors whose arrays are all
 * 16-byte aligned run on 16-byte accesses.  Per-element arithmetic and its order: the header comment of vqvae_amd/csrc/optim.hip
 * (evaluated in fp64 from the fp32 inputs and the device counter, each result rounded to fp32 once).  An element's bits do not depend
 * on how the data is split into tensors.                                                                                                     */
#define VQVAE_ADAM_CHUNK        4096    /* elements per workgroup                                                                     */
#define VQVAE_ADAM_MAX_GROUPS   16      /* parameter groups per step (their hyper-parameters travel as launch arguments)              */
#define VQVAE_ADAM_ZERO_GRAD    0x1     /* step flag: overwrite the consumed gradients with zeros (the update's bits do not change)   */
#define VQVAE_ADAM_DECOUPLED_WD 0x1     /* group flag: p *= 1 - lr * wd (AdamW) instead of g += wd * p                                */
typedef struct VqvaeAdamGroup {
    double lr, beta1, beta2, eps, weight_decay;     /* lr, eps > 0 and finite; betas in [0, 1); weight_decay >= 0                      */
    int flags, reserved;
} VqvaeAdamGroup;
VQVAE_API int vqvae_adam_chunk_elems(void);
/* Bytes that hold the plan of these tensors when every one has a gradient (0: n_tensors < 1, NULL or a negative count). */
VQVAE_API size_t vqvae_adam_plan_bytes(int n_tensors, const int64_t *numel_host);
/* Fills plan_host from HOST arrays of n_tensors device pointers / sizes / group indices; *n_chunks_out = chunks (= workgroups). */
VQVAE_API int vqvae_adam_plan_write(int n_tensors, const int64_t *numel_host, void *const *param, void *const *grad,
                                    void *const *exp_avg, void *const *exp_avg_sq, void *const *max_exp_avg_sq, void *const *step,
                                    const int *group, int n_groups, void *plan_host, size_t plan_bytes, int64_t *n_chunks_out);
/* One optimizer step: a one-workgroup kernel (counters, bias corrections) and the update kernel, in that order on `stream`.  The groups'
 * hyper-parameters are read from groups_host during the call and travel as launch arguments: the caller may change them right after
 * (an lr scheduler), and a captured step keeps those of capture time.  clip_coef: NULL, or a device scalar every gradient element is
 * multiplied by (vqvae_grad_norm_f32's output); the gradients in memory stay unscaled -- torch's clip_grad_norm_ scales them in place. */
VQVAE_API int vqvae_adam_step_f32(void *plan_dev, size_t plan_bytes, int n_tensors, int64_t n_chunks,
                                  const VqvaeAdamGroup *groups_host, int n_groups, int flags, const float *clip_coef,
                                  vqvae_stream_t stream);
/* Global L2 norm of the plan's gradients: fp64 partial sums per chunk, added in a fixed order by one workgroup (no atomics: the same
 * bits in every run).  total_norm_out = fp32(sqrt(sum)); clip_coef_out (may be NULL) = min(1, max_norm / (total_norm + 1e-6)).        */
VQVAE_API size_t vqvae_grad_norm_workspace_bytes(int64_t n_chunks);
VQVAE_API int vqvae_grad_norm_f32(const void *plan_dev, size_t plan_bytes, int n_tensors, int64_t n_chunks, float max_norm,
                                  float *total_norm_out, float *clip_coef_out, void *workspace, size_t workspace_bytes,
                                  vqvae_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VQVAE_HIP_H */
