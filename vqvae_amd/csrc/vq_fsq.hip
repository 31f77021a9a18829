// Finite scalar quantization (gfx950): the quantizer without a learned codebook (Mentzer et al., "Finite Scalar Quantization: VQ-VAE
// Made Simple", arXiv 2309.15505; `FSQ` in vector-quantize-pytorch).  Each latent row is projected to d channels, every channel is
// bounded with tanh and rounded to one of L_j levels; the implicit codebook has K = prod L_j entries.  The two projections run INSIDE
// these kernels: one kernel reads z once and writes z_q once.
//   vqvae_fsq_forward_f32          z -> z_q, idx, hist, perplexity
//   vqvae_fsq_decode_indices_f32   idx -> z_q
//   vqvae_fsq_backward_f32         (z, grad_zq) -> grad_z and the gradients of the four projection parameters
// Rows and layouts are vqvae_vq_forward_f32's: N = B H W rows of D channels, (B, D, H, W) maps, or (N, D) rows with
// VQVAE_VQ_ROWMAJOR.  levels = (L_0 .. L_{d-1}), 1 <= d <= 8, 2 <= L_j <= 256, K <= 65536; 1 <= D <= 256; N <= INT32_MAX.
// W_in (d, D), b_in (d), W_out (D, d), b_out (D): fp32 in nn.Linear's layouts.
//
// THE ARITHMETIC IS THE CONTRACT (tests/vq_fsq_ref.py restates it on the CPU; the library is compiled with -ffp-contract=off, so every
// operation written below is one IEEE operation).  Host constants, computed in fp64 and passed to the kernels as doubles -- they are
// vector-quantize-pytorch's FSQ.bound (the paper's listing differs in the sign of eps and uses tan):
//
//   eps = 1e-3;  half_l_j = (L_j - 1) (1 + eps) / 2;  offset_j = 0.5 if L_j is even else 0;  shift_j = atanh(offset_j / half_l_j)
//   hw_j = L_j / 2 (integer);  basis_0 = 1, basis_j = prod_{i<j} L_i
//
// Forward, per row, every operation in fp64:
//
//   s = double(b_in[j]); for c = 0 .. D-1 ascending: s = s + double(W_in[j][c]) * double(z_c)   (the product is exact);  y_j = float(s)
//   t_j = tanh(double(y_j) + shift_j);  b_j = t_j * half_l_j - offset_j;  q_j = rint(b_j)         (half-even; q_j in [-hw_j, L_j-1-hw_j])
//   c^_j = float(double(q_j) / double(hw_j))
//   idx = sum_j (q_j + hw_j) basis_j                                                              (int64, first level least significant)
//   s = double(b_out[c]); for j ascending: s = s + double(W_out[c][j]) * double(c^_j);  zq_c = float(s)
//
// A non-finite y_j (NaN or +-Inf) contributes digit 0 to idx and makes c^_j NaN: that row of z_q is NaN, idx stays in [0, K), and a
// NaN stays in its own row.  hist (K) counts the indices with int32 atomics (exact in any order); there is no floating-point atomic
// anywhere.  perplexity = exp(-sum_k p_k log(p_k + 1e-10)), p_k = double(hist_k) / double(N) (the reference's formula,
// models/quantizer.py:71), in fp64: thread t of 256 adds k = t, t + 256, .. in ascending order, the 256 sums meet in a fixed tree
// (common.h's block_sum_f64), one rounding to fp32.  There is no loss term.
//
// Decode, per index: digit_j = (idx / basis_j) % L_j, q_j = digit_j - hw_j, then the forward's last two lines.  An index outside
// [0, K) writes a NaN row and reads nothing out of range (vqvae_vq_decode_indices_f32's rule).
//
// Backward, from the upstream gradient g of z_q; rounding is straight-through, t and c^ are recomputed from z as the forward does:
//
//   gc_j = 0.0; for c ascending: gc_j = gc_j + double(W_out[c][j]) * double(g_c)
//   gy_j = gc_j / double(hw_j) * half_l_j * (1.0 - t_j * t_j)                                    (left to right, kept in fp64)
//   s = 0.0; for j ascending: s = s + double(W_in[j][c]) * gy_j;  gz_c = float(s)
//   grad_W_out[c][j] = sum_n g_{n,c} c^_{n,j}   grad_b_out[c] = sum_n g_{n,c}   grad_W_in[j][c] = sum_n gy_{n,j} z_{n,c}   grad_b_in[j] = sum_n gy_{n,j}
//
// THE ORDER OF THE FOUR SUMS depends on N alone: rows are cut into blocks of 256 consecutive rows (the last one ragged); inside a
// block the terms are added in fp64 one row after the other, in ascending row order, starting from 0.0; a second launch adds the
// blocks' partials in ascending block order, starting from 0.0, and rounds once to fp32.  Both layouts and both access paths cut the
// same blocks and add in the same order: the same bits in all of them and in every run.  A gradient pointer that is NULL is skipped.
//
// z_q depends only on idx, W_out and b_out through correctly rounded operations, so it is bit-equal to the restatement wherever the
// indices agree; the device's fp64 tanh is not guaranteed correctly rounded, so idx can differ on rows within an ulp of a rounding
// boundary, and grad_z carries tanh's error through 1 - t^2.
//
// Mappings (bodies in vq_proj.h, which LFQ's row kernels share; the bound, the rounding and the backward bodies in vq_fsq.h; kernels
// and launches in vq_proj_kernels.h): NCHW maps one pixel per lane, every channel one coalesced access of the wave; row-major rows are
// staged through vq_cosine.h's LDS tile, 64 rows per wave, in 16-byte accesses (D % 4 == 0 and 16-byte aligned pointers) or element
// by element, and each lane walks its own row of the tile.  The projection weights lie in LDS and are read as broadcasts.  No
// scratch.  Every launch is on the caller's stream in one chain; no host sync, no allocation: capturable.
#include <cmath>

#include "common.h"
#include "vq_fsq.h"
#include "vq_proj_kernels.h"

namespace vqvae {

// levels and the constants that follow from them -> a; VQVAE_ERR_UNSUPPORTED outside the envelope
static int fsq_levels(const int *levels, int n_levels, int D, FsqArgs &a) {
    if (n_levels < 1 || n_levels > kFsqMaxLevels || D < 1 || D > 256) return VQVAE_ERR_UNSUPPORTED;
    long long K = 1;
    for (int j = 0; j < n_levels; ++j) {
        const int L = levels[j];
        if (L < 2 || L > 256) return VQVAE_ERR_UNSUPPORTED;
        a.L[j] = L;
        a.hw[j] = L / 2;
        a.basis[j] = (int)K;
        const double eps = 1e-3;
        a.half_l[j] = (double)(L - 1) * (1.0 + eps) / 2.0;
        a.offset[j] = (L % 2 == 0) ? 0.5 : 0.0;
        a.shift[j] = std::atanh(a.offset[j] / a.half_l[j]);
        K *= L;
        if (K > 65536) return VQVAE_ERR_UNSUPPORTED;
    }
    a.K = (int)K;
    a.d = n_levels;
    a.D = D;
    return VQVAE_OK;
}

// the entries' first checks, in the header's order: the shape, then the levels
static int fsq_shape(int64_t B, int H, int W, const int *levels, int n_levels, int D, FsqArgs &a) {
    const int rc = check_rows_shape(B, H, W, a.N, a.HW);
    return rc != VQVAE_OK ? rc : fsq_levels(levels, n_levels, D, a);
}

}  // namespace vqvae

using namespace vqvae;

extern "C" {

int vqvae_fsq_forward_f32(const float *z_e, const float *w_in, const float *b_in, const float *w_out, const float *b_out,
                          const int *levels, int n_levels, int64_t B, int D, int H, int W, int flags, float *z_q, int64_t *idx,
                          int32_t *hist, float *perplexity, vqvae_stream_t stream) {
    if (!z_e || !w_in || !b_in || !levels || !idx || (z_q && (!w_out || !b_out)) || (perplexity && !hist)) return VQVAE_ERR_NULL;
    if (flags & ~VQVAE_VQ_ROWMAJOR) return VQVAE_ERR_UNSUPPORTED;
    FsqArgs a = {};
    int rc = fsq_shape(B, H, W, levels, n_levels, D, a);
    if (rc != VQVAE_OK) return rc;
    const size_t nd = (size_t)a.N * D * 4, wd = (size_t)a.d * D * 4;
    const Span in[] = {{z_e, nd, 4}, {w_in, wd, 4}, {b_in, (size_t)a.d * 4, 4}, {w_out, wd, 4}, {b_out, (size_t)D * 4, 4}};
    const Span out[] = {{z_q, nd, 4}, {idx, (size_t)a.N * 8, 8}, {hist, (size_t)a.K * 4, 4}, {perplexity, 4, 4}};
    if ((rc = check_pointers(in, 5, out, 4)) != VQVAE_OK) return rc;
    a.z = z_e; a.w_in = w_in; a.b_in = b_in; a.w_out = z_q ? w_out : nullptr; a.b_out = z_q ? b_out : nullptr;
    a.out = z_q; a.idx = reinterpret_cast<long long *>(idx); a.hist = hist;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // hist = 0 in front of the forward, by a kernel (common.h: fill_bytes_async): a captured hipMemsetAsync of its K * 4 bytes (4000 for
    // levels (8, 5, 5, 5)) came back from a graph replay with other values than zero in it
    if (hist && (rc = fill_bytes_async(hist, 0, (size_t)a.K * 4, st)) != 0) return rc;
    proj_launch_fwd<Fsq, false>(a, (flags & VQVAE_VQ_ROWMAJOR) != 0, st);
    if (perplexity) hipLaunchKernelGGL(proj_perplexity_kernel<Fsq>, dim3(1), dim3(256), 0, st, hist, a.K, a.N, perplexity);
    return (int)hipGetLastError();
}

int vqvae_fsq_decode_indices_f32(const int64_t *idx, const float *w_out, const float *b_out, const int *levels, int n_levels,
                                 int64_t B, int D, int H, int W, int flags, float *z_q, vqvae_stream_t stream) {
    if (!idx || !w_out || !b_out || !levels || !z_q) return VQVAE_ERR_NULL;
    if (flags & ~VQVAE_VQ_ROWMAJOR) return VQVAE_ERR_UNSUPPORTED;
    FsqArgs a = {};
    int rc = fsq_shape(B, H, W, levels, n_levels, D, a);
    if (rc != VQVAE_OK) return rc;
    const Span in[] = {{idx, (size_t)a.N * 8, 8}, {w_out, (size_t)a.d * D * 4, 4}, {b_out, (size_t)D * 4, 4}};
    const Span out[] = {{z_q, (size_t)a.N * D * 4, 4}};
    if ((rc = check_pointers(in, 3, out, 1)) != VQVAE_OK) return rc;
    a.idx_in = reinterpret_cast<const long long *>(idx); a.w_out = w_out; a.b_out = b_out; a.out = z_q;
    proj_launch_fwd<Fsq, true>(a, (flags & VQVAE_VQ_ROWMAJOR) != 0, static_cast<hipStream_t>(stream));
    return (int)hipGetLastError();
}

size_t vqvae_fsq_backward_workspace_bytes(int64_t N, int D, int n_levels) {
    if (N < 1 || N > INT32_MAX || D < 1 || D > 256 || n_levels < 1 || n_levels > kFsqMaxLevels) return 0;
    return proj_partial_bytes(N, D, n_levels);
}

int vqvae_fsq_backward_f32(const float *z_e, const float *grad_zq, const float *w_in, const float *b_in, const float *w_out,
                           const int *levels, int n_levels, int64_t B, int D, int H, int W, int flags, float *grad_z,
                           float *grad_w_in, float *grad_b_in, float *grad_w_out, float *grad_b_out, void *workspace,
                           size_t workspace_bytes, vqvae_stream_t stream) {
    const bool params = grad_w_in || grad_b_in || grad_w_out || grad_b_out;
    if (!z_e || !grad_zq || !w_in || !b_in || !w_out || !levels || (!grad_z && !params)) return VQVAE_ERR_NULL;
    if (flags & ~VQVAE_VQ_ROWMAJOR) return VQVAE_ERR_UNSUPPORTED;
    FsqArgs a = {};
    int rc = fsq_shape(B, H, W, levels, n_levels, D, a);
    if (rc != VQVAE_OK) return rc;
    const size_t nd = (size_t)a.N * D * 4, wd = (size_t)a.d * D * 4, need = params ? proj_partial_bytes(a.N, D, a.d) : 0;
    const Span in[] = {{z_e, nd, 4}, {grad_zq, nd, 4}, {w_in, wd, 4}, {b_in, (size_t)a.d * 4, 4}, {w_out, wd, 4}};
    const Span out[] = {{grad_z, nd, 4}, {grad_w_in, wd, 4}, {grad_b_in, (size_t)a.d * 4, 4}, {grad_w_out, wd, 4},
                        {grad_b_out, (size_t)D * 4, 4}, {params ? workspace : nullptr, need, 8}};
    if ((rc = check_pointers(in, 5, out, 6)) != VQVAE_OK) return rc;
    if (params && (!workspace || workspace_bytes < need)) return VQVAE_ERR_WORKSPACE;
    a.z = z_e; a.g = grad_zq; a.w_in = w_in; a.b_in = b_in; a.w_out = w_out; a.out = grad_z;
    a.partials = params ? static_cast<double *>(workspace) : nullptr;
    proj_launch_bwd<Fsq>(a, (flags & VQVAE_VQ_ROWMAJOR) != 0, grad_w_in, grad_b_in, grad_w_out, grad_b_out, static_cast<hipStream_t>(stream));
    return (int)hipGetLastError();
}

}  // extern "C"
