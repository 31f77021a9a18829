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
// Mappings (bodies in vq_fsq.h): NCHW maps one pixel per lane, every channel one coalesced access of the wave; row-major rows are
// staged through vq_cosine.h's LDS tile, 64 rows per wave, in 16-byte accesses (D % 4 == 0 and 16-byte aligned pointers) or element
// by element, and each lane walks its own row of the tile.  The projection weights lie in LDS and are read as broadcasts.  No
// scratch.  Every launch is on the caller's stream in one chain; no host sync, no allocation: capturable.
#include <cmath>

#include "common.h"
#include "vq_fsq.h"

namespace vqvae {

template <bool DECODE, int WF>
__global__ __launch_bounds__(kFsqBlockRows) void fsq_fwd_nchw_kernel(FsqArgs a) {
    __shared__ float wl[WF];
    fsq_fwd_nchw_body<DECODE>(a, wl);
}

template <bool DECODE, int V, int WF>
__global__ __launch_bounds__(kFsqBlockRows) void fsq_fwd_rows_kernel(FsqArgs a) {
    __shared__ __attribute__((aligned(16))) float tiles[kL2Waves * kL2TileFloats];
    __shared__ float wl[WF];
    fsq_fwd_rows_body<DECODE, V>(a, tiles, wl);
}

template <bool PARAMS, int WF>
__global__ __launch_bounds__(kFsqBlockRows) void fsq_bwd_nchw_kernel(FsqArgs a) {
    __shared__ float tile[PARAMS ? kL2Chunk * kFsqNchwStride : 1];
    __shared__ float wl[WF];
    __shared__ float chat_l[PARAMS ? kFsqBlockRows * kFsqMaxLevels : 1];
    __shared__ double gy_l[PARAMS ? kFsqBlockRows * kFsqMaxLevels : 1];
    fsq_bwd_nchw_body<PARAMS>(a, tile, wl, chat_l, gy_l);
}

template <bool PARAMS, int V, int WF>
__global__ __launch_bounds__(kFsqBlockRows) void fsq_bwd_rows_kernel(FsqArgs a) {
    __shared__ __attribute__((aligned(16))) float tiles[kL2Waves * kL2TileFloats];
    __shared__ float wl[WF];
    __shared__ float chat_l[PARAMS ? kFsqBlockRows * kFsqMaxLevels : 1];
    __shared__ double gy_l[PARAMS ? kFsqBlockRows * kFsqMaxLevels : 1];
    fsq_bwd_rows_body<PARAMS, V>(a, tiles, wl, chat_l, gy_l);
}

__global__ __launch_bounds__(kFsqBlockRows) void fsq_param_finalize_kernel(const double *partials, long long nblocks, int D, int d,
                                                                           float *g_w_in, float *g_b_in, float *g_w_out, float *g_b_out) {
    fsq_param_finalize_body(partials, nblocks, D, d, g_w_in, g_b_in, g_w_out, g_b_out);
}

__global__ __launch_bounds__(256) void fsq_perplexity_kernel(const int *hist, int K, long long N, float *perplexity) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (int k = tid; k < K; k += 256) {
        const double p = (double)hist[k] / (double)N;
        s = s + p * log(p + 1e-10);
    }
    block_sum_f64(red, tid, s);
    if (tid == 0) *perplexity = (float)exp(-red[0]);
}

static bool fsq_small(const FsqArgs &a) { return a.D <= 64; }
static unsigned fsq_grid(const FsqArgs &a) { return (unsigned)((a.N + kFsqBlockRows - 1) / kFsqBlockRows); }
static bool fsq_wide(const FsqArgs &a, uintptr_t bits) { return (a.D & 3) == 0 && !(bits & 15); }

template <bool DECODE>
static void fsq_launch_fwd(const FsqArgs &a, bool rowmajor, hipStream_t st) {
    const dim3 grid(fsq_grid(a)), block(kFsqBlockRows);
    constexpr int S = kFsqWeightFloatsSmall, M = kFsqWeightFloatsMax;
    if (!rowmajor) {
        if (fsq_small(a)) hipLaunchKernelGGL((fsq_fwd_nchw_kernel<DECODE, S>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((fsq_fwd_nchw_kernel<DECODE, M>), grid, block, 0, st, a);
        return;
    }
    const bool wide = fsq_wide(a, reinterpret_cast<uintptr_t>(a.z) | reinterpret_cast<uintptr_t>(a.out));
    if (wide && fsq_small(a)) hipLaunchKernelGGL((fsq_fwd_rows_kernel<DECODE, 4, S>), grid, block, 0, st, a);
    else if (wide) hipLaunchKernelGGL((fsq_fwd_rows_kernel<DECODE, 4, M>), grid, block, 0, st, a);
    else if (fsq_small(a)) hipLaunchKernelGGL((fsq_fwd_rows_kernel<DECODE, 1, S>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((fsq_fwd_rows_kernel<DECODE, 1, M>), grid, block, 0, st, a);
}

void launch_fsq_forward(const FsqArgs &a, bool rowmajor, hipStream_t st) { fsq_launch_fwd<false>(a, rowmajor, st); }
void launch_fsq_decode(const FsqArgs &a, bool rowmajor, hipStream_t st) { fsq_launch_fwd<true>(a, rowmajor, st); }

template <bool PARAMS>
static void fsq_launch_bwd(const FsqArgs &a, bool rowmajor, hipStream_t st) {
    const dim3 grid(fsq_grid(a)), block(kFsqBlockRows);
    constexpr int S = kFsqWeightFloatsSmall, M = kFsqWeightFloatsMax;
    if (!rowmajor) {
        if (fsq_small(a)) hipLaunchKernelGGL((fsq_bwd_nchw_kernel<PARAMS, S>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((fsq_bwd_nchw_kernel<PARAMS, M>), grid, block, 0, st, a);
        return;
    }
    const bool wide = fsq_wide(a, reinterpret_cast<uintptr_t>(a.z) | reinterpret_cast<uintptr_t>(a.g) | reinterpret_cast<uintptr_t>(a.out));
    if (wide && fsq_small(a)) hipLaunchKernelGGL((fsq_bwd_rows_kernel<PARAMS, 4, S>), grid, block, 0, st, a);
    else if (wide) hipLaunchKernelGGL((fsq_bwd_rows_kernel<PARAMS, 4, M>), grid, block, 0, st, a);
    else if (fsq_small(a)) hipLaunchKernelGGL((fsq_bwd_rows_kernel<PARAMS, 1, S>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((fsq_bwd_rows_kernel<PARAMS, 1, M>), grid, block, 0, st, a);
}

void launch_fsq_backward(const FsqArgs &a, bool rowmajor, hipStream_t st) {
    if (a.partials) fsq_launch_bwd<true>(a, rowmajor, st);
    else fsq_launch_bwd<false>(a, rowmajor, st);
}

// ---- the entries' checks: the header's codes, before any launch ---------------------------------------------------------------------

struct FsqSpan { const void *p; size_t bytes; };

static bool fsq_overlap(const FsqSpan &x, const FsqSpan &y) {
    if (!x.p || !y.p) return false;
    const uintptr_t a = reinterpret_cast<uintptr_t>(x.p), b = reinterpret_cast<uintptr_t>(y.p);
    return a < b + y.bytes && b < a + x.bytes;
}

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

static int fsq_shape(int64_t B, int H, int W, FsqArgs &a) {
    if (B < 1 || H < 1 || W < 1) return VQVAE_ERR_SHAPE;
    if ((long long)H * W > INT32_MAX) return VQVAE_ERR_UNSUPPORTED;
    const long long HW = (long long)H * W;
    if (B > INT32_MAX / HW) return VQVAE_ERR_UNSUPPORTED;
    a.HW = (int)HW;
    a.N = B * HW;
    return VQVAE_OK;
}

// every pointer aligned to `align` of its span (NULL passes), and no output on an input
static int fsq_pointers(const FsqSpan *in, const int *in_align, int n_in, const FsqSpan *out, const int *out_align, int n_out) {
    for (int i = 0; i < n_in; ++i)
        if (reinterpret_cast<uintptr_t>(in[i].p) & (uintptr_t)(in_align[i] - 1)) return VQVAE_ERR_UNSUPPORTED;
    for (int o = 0; o < n_out; ++o) {
        if (reinterpret_cast<uintptr_t>(out[o].p) & (uintptr_t)(out_align[o] - 1)) return VQVAE_ERR_UNSUPPORTED;
        for (int i = 0; i < n_in; ++i)
            if (fsq_overlap(out[o], in[i])) return VQVAE_ERR_UNSUPPORTED;
    }
    return VQVAE_OK;
}

static size_t fsq_backward_ws(long long N, int D, int d) {
    const size_t nblocks = (size_t)((N + kFsqBlockRows - 1) / kFsqBlockRows);
    return nblocks * (size_t)(2 * D * d + D + d) * sizeof(double);
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
    int rc = fsq_shape(B, H, W, a);
    if (rc == VQVAE_OK) rc = fsq_levels(levels, n_levels, D, a);
    if (rc != VQVAE_OK) return rc;
    const size_t nd = (size_t)a.N * D * 4, wd = (size_t)a.d * D * 4;
    const FsqSpan in[] = {{z_e, nd}, {w_in, wd}, {b_in, (size_t)a.d * 4}, {w_out, wd}, {b_out, (size_t)D * 4}};
    const int in_al[] = {4, 4, 4, 4, 4};
    const FsqSpan out[] = {{z_q, nd}, {idx, (size_t)a.N * 8}, {hist, (size_t)a.K * 4}, {perplexity, 4}};
    const int out_al[] = {4, 8, 4, 4};
    if ((rc = fsq_pointers(in, in_al, 5, out, out_al, 4)) != VQVAE_OK) return rc;
    a.z = z_e; a.w_in = w_in; a.b_in = b_in; a.w_out = z_q ? w_out : nullptr; a.b_out = z_q ? b_out : nullptr;
    a.out = z_q; a.idx = reinterpret_cast<long long *>(idx); a.hist = hist;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // hist = 0 in front of the forward, by a kernel (common.h: fill_bytes_async): a captured hipMemsetAsync of its K * 4 bytes (4000 for
    // levels (8, 5, 5, 5)) came back from a graph replay with other values than zero in it
    if (hist && (rc = fill_bytes_async(hist, 0, (size_t)a.K * 4, st)) != 0) return rc;
    launch_fsq_forward(a, (flags & VQVAE_VQ_ROWMAJOR) != 0, st);
    if (perplexity) hipLaunchKernelGGL(fsq_perplexity_kernel, dim3(1), dim3(256), 0, st, hist, a.K, a.N, perplexity);
    return (int)hipGetLastError();
}

int vqvae_fsq_decode_indices_f32(const int64_t *idx, const float *w_out, const float *b_out, const int *levels, int n_levels,
                                 int64_t B, int D, int H, int W, int flags, float *z_q, vqvae_stream_t stream) {
    if (!idx || !w_out || !b_out || !levels || !z_q) return VQVAE_ERR_NULL;
    if (flags & ~VQVAE_VQ_ROWMAJOR) return VQVAE_ERR_UNSUPPORTED;
    FsqArgs a = {};
    int rc = fsq_shape(B, H, W, a);
    if (rc == VQVAE_OK) rc = fsq_levels(levels, n_levels, D, a);
    if (rc != VQVAE_OK) return rc;
    const FsqSpan in[] = {{idx, (size_t)a.N * 8}, {w_out, (size_t)a.d * D * 4}, {b_out, (size_t)D * 4}};
    const int in_al[] = {8, 4, 4};
    const FsqSpan out[] = {{z_q, (size_t)a.N * D * 4}};
    const int out_al[] = {4};
    if ((rc = fsq_pointers(in, in_al, 3, out, out_al, 1)) != VQVAE_OK) return rc;
    a.idx_in = reinterpret_cast<const long long *>(idx); a.w_out = w_out; a.b_out = b_out; a.out = z_q;
    launch_fsq_decode(a, (flags & VQVAE_VQ_ROWMAJOR) != 0, static_cast<hipStream_t>(stream));
    return (int)hipGetLastError();
}

size_t vqvae_fsq_backward_workspace_bytes(int64_t N, int D, int n_levels) {
    if (N < 1 || N > INT32_MAX || D < 1 || D > 256 || n_levels < 1 || n_levels > kFsqMaxLevels) return 0;
    return fsq_backward_ws(N, D, n_levels);
}

int vqvae_fsq_backward_f32(const float *z_e, const float *grad_zq, const float *w_in, const float *b_in, const float *w_out,
                           const int *levels, int n_levels, int64_t B, int D, int H, int W, int flags, float *grad_z,
                           float *grad_w_in, float *grad_b_in, float *grad_w_out, float *grad_b_out, void *workspace,
                           size_t workspace_bytes, vqvae_stream_t stream) {
    const bool params = grad_w_in || grad_b_in || grad_w_out || grad_b_out;
    if (!z_e || !grad_zq || !w_in || !b_in || !w_out || !levels || (!grad_z && !params)) return VQVAE_ERR_NULL;
    if (flags & ~VQVAE_VQ_ROWMAJOR) return VQVAE_ERR_UNSUPPORTED;
    FsqArgs a = {};
    int rc = fsq_shape(B, H, W, a);
    if (rc == VQVAE_OK) rc = fsq_levels(levels, n_levels, D, a);
    if (rc != VQVAE_OK) return rc;
    const size_t nd = (size_t)a.N * D * 4, wd = (size_t)a.d * D * 4, need = params ? fsq_backward_ws(a.N, D, a.d) : 0;
    const FsqSpan in[] = {{z_e, nd}, {grad_zq, nd}, {w_in, wd}, {b_in, (size_t)a.d * 4}, {w_out, wd}};
    const int in_al[] = {4, 4, 4, 4, 4};
    const FsqSpan out[] = {{grad_z, nd}, {grad_w_in, wd}, {grad_b_in, (size_t)a.d * 4}, {grad_w_out, wd}, {grad_b_out, (size_t)D * 4},
                           {params ? workspace : nullptr, need}};
    const int out_al[] = {4, 4, 4, 4, 4, 8};
    if ((rc = fsq_pointers(in, in_al, 5, out, out_al, 6)) != VQVAE_OK) return rc;
    if (params && (!workspace || workspace_bytes < need)) return VQVAE_ERR_WORKSPACE;
    a.z = z_e; a.g = grad_zq; a.w_in = w_in; a.b_in = b_in; a.w_out = w_out; a.out = grad_z;
    a.partials = params ? static_cast<double *>(workspace) : nullptr;
    hipStream_t st = static_cast<hipStream_t>(stream);
    launch_fsq_backward(a, (flags & VQVAE_VQ_ROWMAJOR) != 0, st);
    if (params) {
        const int P = 2 * D * a.d + D + a.d;
        hipLaunchKernelGGL(fsq_param_finalize_kernel, dim3((unsigned)((P + kFsqBlockRows - 1) / kFsqBlockRows)), dim3(kFsqBlockRows), 0,
                           st, a.partials, (long long)((a.N + kFsqBlockRows - 1) / kFsqBlockRows), D, a.d, grad_w_in, grad_b_in,
                           grad_w_out, grad_b_out);
    }
    return (int)hipGetLastError();
}

}  // extern "C"
