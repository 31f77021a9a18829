// Lookup-free quantization (gfx950): the quantizer whose codebook is {-1, +1}^d (Yu et al., "Language Model Beats Diffusion --
// Tokenizer is Key to Visual Generation", MAGVIT-v2, arXiv 2310.05737, section 3.1; `LFQ` in vector-quantize-pytorch) with its
// commitment term and its entropy penalty.  Each latent row is projected to d = log2 K channels, every channel keeps its sign, and the
// signs are projected back.  The two projections run INSIDE these kernels.
//   vqvae_lfq_forward_f32          z -> z_q, idx, hist, perplexity, losses (loss, C, P, H), avg
//   vqvae_lfq_decode_indices_f32   idx -> z_q
//   vqvae_lfq_backward_f32         (z, grad_zq, grad_loss, avg) -> grad_z and the gradients of the four projection parameters
// Rows and layouts are vqvae_vq_forward_f32's: N = B H W rows of D channels, (B, D, H, W) maps, or (N, D) rows with
// VQVAE_VQ_ROWMAJOR.  1 <= d <= 16, K = 2^d; 1 <= D <= 256; N <= INT32_MAX.  W_in (d, D), b_in (d), W_out (D, d), b_out (D): fp32 in
// nn.Linear's layouts.  The scalars beta (commitment weight), w_e (entropy weight), gamma (diversity weight) and inv_temperature
// (the library's default: 100) are passed as floats and used as doubles; s = 4.0 * inv_temperature.
//
// THE ARITHMETIC IS THE CONTRACT (tests/vq_lfq_ref.py restates it on the CPU; the library is compiled with -ffp-contract=off, so every
// operation written below is one IEEE operation).
//
// Forward, per row, every operation in fp64:
//
//   t = double(b_in[j]); for c = 0 .. D-1 ascending: t = t + double(W_in[j][c]) * double(z_c)   (the product is exact);  y_j = float(t)
//   bit_j = (y_j > 0);  c_j = bit_j ? +1 : -1        (a y of exactly 0 gives -1, as torch.where(x > 0, 1, -1); +-Inf keep their sign)
//   idx = sum_j bit_j 2^j                              (int64, FIRST channel LEAST significant -- the library puts it most significant)
//   t = double(b_out[c]); for j ascending: t = t + double(W_out[c][j]) * double(c_j);  zq_c = float(t)
//
// y is defined bit for bit (FSQ's projection), and so are idx, hist and z_q.  A NaN y_j gives bit 0 and c_j = NaN: that row of z_q is
// NaN, idx stays in [0, K), and a NaN stays in its own row of z_q.  hist (K) counts the indices with int32 atomics (exact in any
// order); there is no floating-point atomic anywhere.  perplexity = exp(-sum_k p_k log(p_k + 1e-10)), p_k = hist_k / N, in fp64: thread
// t of 256 adds k = t, t + 256, .. in ascending order, the 256 sums meet in a fixed tree, one rounding to fp32 (vq_fsq.hip's).
//
// Losses, per call, fp64, each returned scalar rounded to fp32 once.  With a = s * double(y_nj):
//
//   e = exp(-|a|);  big = 1 / (1 + e);  small = e / (1 + e);  p+ = sigma(a) = (a >= 0 ? big : small);  p- = sigma(-a) = the other one
//   h(a) = log1p(e) + |a| * small                       (the entropy of the channel's two-way softmax)
//   C = (1 / (N d)) sum_{n,j} (y_nj - c_nj)^2           commitment
//   P = (1 / N) sum_n sum_j h(a_nj)                     per-sample entropy: the exact entropy of the row's softmax over all K codes with
//                                                       logits 2 inv_temperature y . c_k, which factorises over the channels
//   p_n(k) = ((..(1 * p_0) * p_1 ..) * p_{d-1}),  p_j = p+ if bit j of k is set, p- if not
//   avg[k] = (1 / N) sum_n p_n(k)                       K fp64 values, an output
//   H = -sum_k avg[k] log avg[k]                        a term with avg[k] == 0 is 0
//   loss = beta * C + w_e * (P - gamma * H);  losses = (loss, C, P, H)
//
// vector-quantize-pytorch clamps probabilities at 1e-5 inside its logs and computes the losses in training mode only; this does neither.
// The scalar losses and avg of a batch that holds a non-finite y are unspecified (nothing faults).
//
// THE ORDER OF THE SUMS OVER n depends on (N, K) alone.  Rows are cut into blocks of 256 consecutive rows; P_max = max(16, min(1024,
// 2^20 / K)); bpp = ceil(blocks / P_max) blocks make one partition (the last one ragged), so that the (partitions, K) fp64 partials
// never take more than 8 MiB.  Inside a partition every sum (avg[k]; per channel j the sums of h and of (y - c)^2) adds its rows one
// after the other in ascending order from 0.0; a second launch adds avg's partitions in ascending order from 0.0 and divides by N; a
// one-workgroup launch adds the partitions of P and C per channel, then the channels in ascending order, and adds H as the
// perplexity's sum is added (thread t: k = t, t + 256, ..; then the fixed tree).  The loss kernels read the y the row kernel left in
// the workspace, so every output has the same bits in both layouts, on both access paths and in every run.
//
// Backward.  g = *grad_loss (a device scalar, NULL = 1.0), grad_zq may be NULL (= 0).  Rounding is straight-through,
// z_q = project_out(y + sg(c - y)).  With L[k] = log avg[k] (log 0 = 0) and avg an INPUT (the forward's):
//
//   gc_j = 0.0; for c ascending: gc_j = gc_j + double(W_out[c][j]) * double(grad_zq_c)
//   T_j^+ (T_j^-) = sum over the k whose bit j is set (clear) of L[k] prod_{i != j} p_i^{bit_i(k)}
//   e_j = beta * 2 * (y_j - c_j) / (N d) - w_e * (s s / N) * y_j * (p+ p-) + w_e * gamma * (s / N) * (p+ p-) * (T_j^+ - T_j^-)
//   gy_j = gc_j + g * e_j                                (fp64, unrounded)
//   t = 0.0; for j ascending: t = t + double(W_in[j][c]) * gy_j;  grad_z_c = float(t)
//   grad_W_out[c][j] = sum_n grad_zq_{n,c} c_{n,j}   grad_b_out[c] = sum_n grad_zq_{n,c}   grad_W_in[j][c] = sum_n gy_{n,j} z_{n,c}   grad_b_in[j] = sum_n gy_{n,j}
//
// T is computed by halves (vq_lfq.h, lfq_entgrad_body): the bits are split into ceil(d / 2) low and the other high ones, the products
// over each half are tables A[lo], B[hi], u[lo] = sum_hi L[hi][lo] B[hi] and v[hi] = sum_lo L[hi][lo] A[lo] in ascending order, and T
// of a low (high) bit is a sum over the low (high) half's entries of u (v) times the half's other channels -- about 2 K
// multiply-adds a row, no (N, K) array anywhere.  With avg NULL the loss has no gradient (gy_j = gc_j) and no entropy work runs.
// The four parameter gradients are fp64 sums in an order fixed by N alone: blocks of 256 consecutive rows, rows in order inside a
// block from 0.0, then the blocks in order from 0.0, rounded once to fp32 (vq_fsq.hip's scheme).  A NULL gradient pointer is skipped.
//
// Launch chains, each on the caller's stream, no host sync, no allocation, capturable, every clear a kernel (fill_bytes_async):
//   forward:   [clear hist] row kernel (z -> y into the workspace, idx, hist, z_q)  [perplexity]  [avg partials; avg; loss finalize]
//   backward:  row kernel (z -> y)  [log avg; entropy gradient -> e (N, d) fp64]  row kernel (grad_z, partials)  [parameter finalize]
// Workspace (vqvae_lfq_workspace_bytes(N, D, d), one size for both chains): y (N, d) fp32, then the larger of
// {avg partials (P, K), scalar partials (P, 32)} and {L (K), e (N, d), parameter partials (ceil(N / 256), 2 D d + D + d)}, all fp64.
//
// Mappings (the row kernels' bodies in vq_proj.h, their kernels and launches in vq_proj_kernels.h; the sign code, the loss kernels
// and the backward bodies in vq_lfq.h): the row kernels are vq_fsq.hip's -- NCHW maps one pixel per lane, row-major rows staged through
// vq_cosine.h's LDS tile, 64 rows per wave, 16-byte or element accesses.  avg partials: workgroup (partition, 1024 codes), 4 codes per
// thread, rows staged 64 at a time as fp64 probabilities.  Entropy gradient: one wave per row, L in LDS up to K = 4096 (rows padded by
// one double), read from memory above.  No scratch.
#include <cmath>

#include "common.h"
#include "vq_lfq.h"
#include "vq_proj_kernels.h"

namespace vqvae {

__global__ __launch_bounds__(256) void lfq_avg_kernel(LfqLossArgs a) {
    __shared__ double pp[2 * kLfqChunkRows * kLfqMaxBits], hh[kLfqChunkRows * kLfqMaxBits], cc[kLfqChunkRows * kLfqMaxBits];
    lfq_avg_body(a, pp, hh, cc);
}

__global__ __launch_bounds__(256) void lfq_avg_reduce_kernel(LfqLossArgs a) { lfq_avg_reduce_body(a); }

__global__ __launch_bounds__(256) void lfq_loss_finalize_kernel(LfqLossArgs a) {
    __shared__ double red[256], ch[kLfqScalarSlots];
    lfq_loss_finalize_body(a, red, ch);
}

__global__ __launch_bounds__(256) void lfq_logavg_kernel(LfqLossArgs a) { lfq_logavg_body(a); }

template <int LN>
__global__ __launch_bounds__(kLfqGradThreads) void lfq_entgrad_kernel(LfqLossArgs a) {
    __shared__ double l_lds[LN], pb[2 * kLfqMaxBits], A[256], B[256], u[256], v[256], T[2 * kLfqMaxBits];
    lfq_entgrad_body(a, l_lds, pb, A, B, u, v, T);
}

// the entries' first checks, in the header's order
static int lfq_shape(int64_t B, int D, int H, int W, int d, LfqArgs &a) {
    const int rc = check_rows_shape(B, H, W, a.N, a.HW);
    if (rc != VQVAE_OK) return rc;
    if (d < 1 || d > kLfqMaxBits || D < 1 || D > 256) return VQVAE_ERR_UNSUPPORTED;
    a.D = D;
    a.d = d;
    a.K = 1 << d;
    return VQVAE_OK;
}

// the workspace: [y (N, d) fp32, padded to 8 bytes] then forward {avg_part, sc_part} or backward {logavg, e, partials}
struct LfqPlan {
    long long rows_per_part;
    int P;
    size_t off_a, avg_part, sc_part, logavg, e, partials, total;
};

static LfqPlan lfq_plan(long long N, int D, int d) {
    LfqPlan p = {};
    const int K = 1 << d;
    lfq_partition(N, K, p.rows_per_part, p.P);
    p.off_a = ((size_t)N * d * 4 + 7) & ~(size_t)7;
    p.avg_part = p.off_a;
    p.sc_part = p.avg_part + (size_t)p.P * K * 8;
    const size_t fwd_end = p.sc_part + (size_t)p.P * kLfqScalarSlots * 8;
    p.logavg = p.off_a;
    p.e = p.logavg + (size_t)K * 8;
    p.partials = p.e + (size_t)N * d * 8;
    const size_t bwd_end = p.partials + proj_partial_bytes(N, D, d);
    p.total = fwd_end > bwd_end ? fwd_end : bwd_end;
    return p;
}

}  // namespace vqvae

using namespace vqvae;

extern "C" {

size_t vqvae_lfq_workspace_bytes(int64_t N, int D, int d) {
    if (N < 1 || N > INT32_MAX || D < 1 || D > 256 || d < 1 || d > kLfqMaxBits) return 0;
    return lfq_plan(N, D, d).total;
}

int vqvae_lfq_forward_f32(const float *z_e, const float *w_in, const float *b_in, const float *w_out, const float *b_out, int d,
                          int64_t B, int D, int H, int W, int flags, float beta, float entropy_weight, float diversity_gamma,
                          float inv_temperature, float *z_q, int64_t *idx, int32_t *hist, float *perplexity, float *losses,
                          double *avg, void *workspace, size_t workspace_bytes, vqvae_stream_t stream) {
    if (!z_e || !w_in || !b_in || !idx || (z_q && (!w_out || !b_out)) || (perplexity && !hist) || (!losses != !avg))
        return VQVAE_ERR_NULL;
    if (flags & ~VQVAE_VQ_ROWMAJOR) return VQVAE_ERR_UNSUPPORTED;
    LfqArgs a = {};
    int rc = lfq_shape(B, D, H, W, d, a);
    if (rc != VQVAE_OK) return rc;
    const LfqPlan plan = lfq_plan(a.N, D, d);
    const size_t nd = (size_t)a.N * D * 4, wd = (size_t)d * D * 4;
    const Span in[] = {{z_e, nd, 4}, {w_in, wd, 4}, {b_in, (size_t)d * 4, 4}, {w_out, wd, 4}, {b_out, (size_t)D * 4, 4}};
    const Span out[] = {{z_q, nd, 4}, {idx, (size_t)a.N * 8, 8}, {hist, (size_t)a.K * 4, 4}, {perplexity, 4, 4}, {losses, 16, 4},
                        {avg, (size_t)a.K * 8, 8}, {losses ? workspace : nullptr, plan.total, 8}};
    if ((rc = check_pointers(in, 5, out, 7)) != VQVAE_OK) return rc;
    if (losses && (!workspace || workspace_bytes < plan.total)) return VQVAE_ERR_WORKSPACE;
    char *ws = static_cast<char *>(workspace);
    a.z = z_e; a.w_in = w_in; a.b_in = b_in; a.w_out = z_q ? w_out : nullptr; a.b_out = z_q ? b_out : nullptr;
    a.out = z_q; a.idx = reinterpret_cast<long long *>(idx); a.hist = hist;
    a.y = losses ? reinterpret_cast<float *>(ws) : nullptr;
    hipStream_t st = static_cast<hipStream_t>(stream);
    // hist = 0 by a kernel, not hipMemsetAsync: the chain is captured and replayed
    if (hist && (rc = fill_bytes_async(hist, 0, (size_t)a.K * 4, st)) != 0) return rc;
    proj_launch_fwd<Lfq, false>(a, (flags & VQVAE_VQ_ROWMAJOR) != 0, st);
    if (perplexity) hipLaunchKernelGGL(proj_perplexity_kernel<Lfq>, dim3(1), dim3(256), 0, st, hist, a.K, a.N, perplexity);
    if (losses) {
        LfqLossArgs l = {};
        l.y = a.y; l.N = a.N; l.rows_per_part = plan.rows_per_part; l.d = d; l.K = a.K; l.P = plan.P;
        l.s = 4.0 * (double)inv_temperature; l.beta = (double)beta; l.we = (double)entropy_weight; l.gamma = (double)diversity_gamma;
        l.avg_part = reinterpret_cast<double *>(ws + plan.avg_part); l.sc_part = reinterpret_cast<double *>(ws + plan.sc_part);
        l.avg_out = avg; l.losses = losses;
        const unsigned tiles = (unsigned)((a.K + kLfqTileCodes - 1) / kLfqTileCodes);
        hipLaunchKernelGGL(lfq_avg_kernel, dim3((unsigned)plan.P, tiles), dim3(256), 0, st, l);
        hipLaunchKernelGGL(lfq_avg_reduce_kernel, dim3((unsigned)((a.K + 255) / 256)), dim3(256), 0, st, l);
        hipLaunchKernelGGL(lfq_loss_finalize_kernel, dim3(1), dim3(256), 0, st, l);
    }
    return (int)hipGetLastError();
}

int vqvae_lfq_decode_indices_f32(const int64_t *idx, const float *w_out, const float *b_out, int d, int64_t B, int D, int H, int W,
                                 int flags, float *z_q, vqvae_stream_t stream) {
    if (!idx || !w_out || !b_out || !z_q) return VQVAE_ERR_NULL;
    if (flags & ~VQVAE_VQ_ROWMAJOR) return VQVAE_ERR_UNSUPPORTED;
    LfqArgs a = {};
    int rc = lfq_shape(B, D, H, W, d, a);
    if (rc != VQVAE_OK) return rc;
    const Span in[] = {{idx, (size_t)a.N * 8, 8}, {w_out, (size_t)d * D * 4, 4}, {b_out, (size_t)D * 4, 4}};
    const Span out[] = {{z_q, (size_t)a.N * D * 4, 4}};
    if ((rc = check_pointers(in, 3, out, 1)) != VQVAE_OK) return rc;
    a.idx_in = reinterpret_cast<const long long *>(idx); a.w_out = w_out; a.b_out = b_out; a.out = z_q;
    proj_launch_fwd<Lfq, true>(a, (flags & VQVAE_VQ_ROWMAJOR) != 0, static_cast<hipStream_t>(stream));
    return (int)hipGetLastError();
}

int vqvae_lfq_backward_f32(const float *z_e, const float *grad_zq, const float *grad_loss, const double *avg, const float *w_in,
                           const float *b_in, const float *w_out, int d, int64_t B, int D, int H, int W, int flags, float beta,
                           float entropy_weight, float diversity_gamma, float inv_temperature, float *grad_z, float *grad_w_in,
                           float *grad_b_in, float *grad_w_out, float *grad_b_out, void *workspace, size_t workspace_bytes,
                           vqvae_stream_t stream) {
    const bool params = grad_w_in || grad_b_in || grad_w_out || grad_b_out;
    if (!z_e || !w_in || !b_in || !w_out || (!grad_z && !params) || (!grad_zq && !avg)) return VQVAE_ERR_NULL;
    if (flags & ~VQVAE_VQ_ROWMAJOR) return VQVAE_ERR_UNSUPPORTED;
    LfqArgs a = {};
    int rc = lfq_shape(B, D, H, W, d, a);
    if (rc != VQVAE_OK) return rc;
    const LfqPlan plan = lfq_plan(a.N, D, d);
    const size_t nd = (size_t)a.N * D * 4, wd = (size_t)d * D * 4;
    const Span in[] = {{z_e, nd, 4}, {grad_zq, nd, 4}, {grad_loss, 4, 4}, {avg, (size_t)a.K * 8, 8}, {w_in, wd, 4}, {b_in, (size_t)d * 4, 4},
                       {w_out, wd, 4}};
    const Span out[] = {{grad_z, nd, 4}, {grad_w_in, wd, 4}, {grad_b_in, (size_t)d * 4, 4}, {grad_w_out, wd, 4},
                        {grad_b_out, (size_t)D * 4, 4}, {workspace, plan.total, 8}};
    if ((rc = check_pointers(in, 7, out, 6)) != VQVAE_OK) return rc;
    if (!workspace || workspace_bytes < plan.total) return VQVAE_ERR_WORKSPACE;
    char *ws = static_cast<char *>(workspace);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool rowmajor = (flags & VQVAE_VQ_ROWMAJOR) != 0;
    // 1: y of every row, as the forward computes it
    LfqArgs f = a;
    f.z = z_e; f.w_in = w_in; f.b_in = b_in; f.y = reinterpret_cast<float *>(ws);
    proj_launch_fwd<Lfq, false>(f, rowmajor, st);
    // 2: the loss's gradient with respect to y
    double *e = nullptr;
    if (avg) {
        LfqLossArgs l = {};
        l.y = f.y; l.N = a.N; l.d = d; l.K = a.K;
        l.s = 4.0 * (double)inv_temperature; l.beta = (double)beta; l.we = (double)entropy_weight; l.gamma = (double)diversity_gamma;
        l.avg = avg; l.logavg = reinterpret_cast<double *>(ws + plan.logavg); l.e = e = reinterpret_cast<double *>(ws + plan.e);
        l.nwg = (int)(a.N < 8192 ? a.N : 8192);
        hipLaunchKernelGGL(lfq_logavg_kernel, dim3((unsigned)((a.K + 255) / 256)), dim3(256), 0, st, l);
        if (a.K <= 1024) hipLaunchKernelGGL((lfq_entgrad_kernel<kLfqLogLdsDoublesSmall>), dim3((unsigned)l.nwg), dim3(kLfqGradThreads), 0, st, l);
        else if (a.K <= kLfqLdsLogK) hipLaunchKernelGGL((lfq_entgrad_kernel<kLfqLogLdsDoubles>), dim3((unsigned)l.nwg), dim3(kLfqGradThreads), 0, st, l);
        else hipLaunchKernelGGL((lfq_entgrad_kernel<1>), dim3((unsigned)l.nwg), dim3(kLfqGradThreads), 0, st, l);
    }
    // 3: the rows' gradients, the parameter gradients' partials and their sums
    a.z = z_e; a.g = grad_zq; a.w_in = w_in; a.w_out = w_out; a.out = grad_z; a.y = f.y; a.e = e; a.gl = grad_loss;
    a.partials = params ? reinterpret_cast<double *>(ws + plan.partials) : nullptr;
    proj_launch_bwd<Lfq>(a, rowmajor, grad_w_in, grad_b_in, grad_w_out, grad_b_out, st);
    return (int)hipGetLastError();
}

}  // extern "C"
