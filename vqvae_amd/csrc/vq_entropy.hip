// The code-entropy loss of a learned codebook (gfx950): the entropy penalty of MaskGIT's VQGAN tokenizer, MAGVIT and LlamaGen
// (`entropy_loss_ratio`, temperature 0.01; vector-quantize-pytorch's `codebook_diversity_loss_weight` is its second half) --
// every row's softmax over the K codes confident, the batch's average softmax uniform -- and its gradient with respect to the rows
// and the codebook, streamed: no (N, K) array exists, the memory is O(N + K D).
//   vqvae_vq_entropy_workspace_bytes
//   vqvae_vq_entropy_forward_f32     (z, E) -> losses (term, P, H), avg (K), rowstat (N, 2)
//   vqvae_vq_entropy_backward_f32    (z, E, avg, rowstat, grad_loss) -> grad_z, grad_codebook
// Rows and layouts are vqvae_vq_forward_f32's: N = B H W rows z_n of D channels, (B, D, H, W) maps, or (N, D) rows with
// VQVAE_VQ_ROWMAJOR; the codebook e_k is (K, D).  1 <= K <= 16384, 1 <= D <= 256, N < 2^31, s = inv_temperature > 0 and finite,
// gamma finite.
//
// THE NUMERIC CONTRACT (tests/vq_entropy_ref.py restates it on the CPU).  Everything is fp64, computed from the fp32 inputs.
//
// Forward:
//   d_nk  = (zz_n + ee_k) - 2 dot_nk          dot, zz, ee: fp64 sums over the channels c (a product of two fp32 values is exact)
//   l_nk  = -s d_nk
//   p_nk  = softmax_k(l_nk)                    shifted by the row maximum: no exponential overflows
//   H_n   = -sum_k p_nk log p_nk               a term with p = 0 is 0
//   P     = (1 / N) sum_n H_n
//   avg_k = (1 / N) sum_n p_nk
//   H     = -sum_k avg_k log avg_k             0 log 0 = 0
//   term  = P - gamma H
//   losses = float(term, P, H);  avg (K doubles);  rowstat (N x 2 doubles): the row's log-sum-exp and H_n
//
// Backward, with g = *grad_loss (NULL = 1), L_k = log avg_k (0 where avg_k = 0), M_n = sum_j p_nj L_j, avg and rowstat INPUTS
// (the forward's), p_nk = exp(l_nk - lse_n):
//   a_nk      = (g / N) p_nk [-(log p_nk + H_n) + gamma (L_k - M_n)]
//   grad_z_n  = float(-2 s sum_k a_nk (z_n - e_k))
//   grad_E_k  = float( 2 s sum_n a_nk (z_n - e_k))
//
// exp and log on the device are not correctly rounded, so the comparison with the restatement is by a bound derived in
// tests/test_vq_entropy_gpu.py, not by bits.  What IS fixed is the order of every sum, a function of (N, K, D) alone:
//   over c   ascending, one fma per channel (the product is exact, so the fma is the contract's multiply and add)
//   over k   (row maximum, S = sum e^x, T = sum e^x x with x = l - max, M_n, A_n = sum_k a_nk, G_nc = sum_k a_nk e_kc) sixteen
//            interleaved classes -- class q holds the codes k with (k mod 64) / 4 = q -- each in ascending k, then the classes in
//            ascending q from 0.0.  H_n = log S - T / S, lse_n = max + log S.
//   over n   LFQ's scheme: blocks of 256 rows grouped into partitions (whole blocks; avg: at most max(16, min(256, 2^20 / K))
//            partitions, so the (partitions, K) partials take at most 8 MiB; grad_E: at most max(1, min(1024, 2^22 / (K D))), so the
//            (partitions, K, D) partials take at most 32 MiB).  Inside a partition a sum over rows (avg_k, sum_n a_nk,
//            sum_n a_nk z_nc) is split into sixteen classes -- class q holds the rows n with (n mod 64) / 4 = q -- each in ascending
//            n (the second contraction: all 64 rows of a tile in ascending n), the classes in ascending q; then the partitions in
//            ascending order from 0.0.  P: per partition, thread t of 256 adds H_n of the rows t, t + 256, .. in ascending order,
//            the 256 sums meet in the fixed tree; then the partitions in order.  H: as the perplexity's sum (k = t, t + 256, ..).
//   the gradients are formed as -2 s (z_nc A_n - G_nc) and 2 s (sum_n a_nk z_nc - e_kc sum_n a_nk): the same sums, grouped so that
//   both are contractions.
// No floating-point atomics, no host sync, no allocation, no memset (every output and every partial is written by a kernel): one
// linear chain of launches on the caller's stream, capturable.  The kernels read z through one element path in either layout and
// stage it as the same doubles, so every output has the same bits in both layouts, at every pointer alignment, in every run and in
// a graph replay.
//
// The contractions run on the vector ALU (v_fma_f64), sixteen independent chains per lane in the dot tiles and 16 - 64 in the second
// contraction; v_mfma_f64_16x16x4_f64 is not used.
// The scalar losses and the gradients of a batch that holds a non-finite value are unspecified; no index depends on the data, so
// nothing is read out of bounds.
//
// Launch chains:
//   forward:   zz; ee; row kernel (max, S, T -> lse, H_n); avg partials (partition x 64 codes); avg; finalize
//   backward:  zz; ee; log avg; row kernel (M_n [, grad_z]); [grad_E partials (partition x 64 codes); grad_E]
// Workspace (vqvae_vq_entropy_workspace_bytes(N, K, D), one size for both chains), all fp64: zz (N), ee (K), rowstat (N, 2), then
// the larger of {avg partials (P, K), P sums (P)} and {L (K), M (N), grad_E partials (P', K, D), a sums (P', K)}.
#include <cmath>

#include "common.h"
#include "vq_entropy.h"

namespace vqvae {

__global__ __launch_bounds__(kEntThreads) void ent_sqnorm_kernel(EntSrc s, double *out) { ent_sqnorm_body(s, out); }

__global__ __launch_bounds__(kEntThreads) void ent_row_fwd_kernel(EntArgs a) {
    __shared__ __attribute__((aligned(16))) double buf[kEntBufDoubles];
    ent_row_fwd_body(a, buf);
}

__global__ __launch_bounds__(kEntThreads) void ent_avg_kernel(EntArgs a) {
    __shared__ __attribute__((aligned(16))) double buf[kEntBufDoubles];
    ent_avg_body(a, buf);
}

__global__ __launch_bounds__(kEntThreads) void ent_avg_reduce_kernel(EntArgs a) { ent_avg_reduce_body(a); }

__global__ __launch_bounds__(kEntThreads) void ent_finalize_kernel(EntArgs a) {
    __shared__ double red[kEntThreads];
    ent_finalize_body(a, red);
}

__global__ __launch_bounds__(kEntThreads) void ent_logavg_kernel(EntArgs a) { ent_logavg_body(a); }

template <int DT, bool WANT_Z>
__global__ __launch_bounds__(kEntThreads) void ent_row_bwd_kernel(EntArgs a) {
    __shared__ __attribute__((aligned(16))) double buf[kEntBufDoubles], w[kEntWDoubles];
    ent_row_bwd_body<DT, WANT_Z>(a, buf, w);
}

template <int DT>
__global__ __launch_bounds__(kEntThreads) void ent_grad_e_kernel(EntArgs a) {
    __shared__ __attribute__((aligned(16))) double buf[kEntBufDoubles], w[kEntWDoubles];
    ent_grad_e_body<DT>(a, buf, w);
}

__global__ __launch_bounds__(kEntThreads) void ent_grad_e_reduce_kernel(EntArgs a) { ent_grad_e_reduce_body(a); }

struct EntPlan {
    long long rpp_avg, rpp_grad;
    int P_avg, P_grad;
    size_t zz, ee, rs, avg_part, sc_part, logavg, m, ge_part, as_part, total;
};

static EntPlan ent_plan(long long N, int K, int D) {
    EntPlan p = {};
    ent_partition_avg(N, K, p.rpp_avg, p.P_avg);
    ent_partition_grad(N, K, D, p.rpp_grad, p.P_grad);
    p.zz = 0;
    p.ee = p.zz + (size_t)N * 8;
    p.rs = p.ee + (size_t)K * 8;
    const size_t u = p.rs + (size_t)N * 16;
    p.avg_part = u;
    p.sc_part = p.avg_part + (size_t)p.P_avg * K * 8;
    const size_t fwd_end = p.sc_part + (size_t)p.P_avg * 8;
    p.logavg = u;
    p.m = p.logavg + (size_t)K * 8;
    p.ge_part = p.m + (size_t)N * 8;
    p.as_part = p.ge_part + (size_t)p.P_grad * K * D * 8;
    const size_t bwd_end = p.as_part + (size_t)p.P_grad * K * 8;
    p.total = fwd_end > bwd_end ? fwd_end : bwd_end;
    return p;
}

// the entries' first checks; N and HW out
static int ent_shape(int64_t B, int D, int H, int W, int K, double s, double gamma, int flags, long long &N, int &HW) {
    const int rc = check_rows_shape(B, H, W, N, HW);
    if (rc != VQVAE_OK) return rc;
    if (K < 1 || D < 1 || K > kEntMaxK || D > kEntMaxD || (flags & ~VQVAE_VQ_ROWMAJOR)) return VQVAE_ERR_UNSUPPORTED;
    if (!(s > 0.0) || !std::isfinite(s) || !std::isfinite(gamma)) return VQVAE_ERR_UNSUPPORTED;
    return VQVAE_OK;
}

static void ent_common(EntArgs &a, const float *z_e, const float *codebook, long long N, int HW, int K, int D, double s, double gamma,
                       int flags, char *ws, const EntPlan &plan) {
    a.z = EntSrc{z_e, N, D, HW, (flags & VQVAE_VQ_ROWMAJOR) ? 1 : 0};
    a.e = EntSrc{codebook, K, D, 1, 1};
    a.N = N; a.K = K; a.D = D; a.s = s; a.gamma = gamma;
    a.zz = reinterpret_cast<double *>(ws + plan.zz);
    a.ee = reinterpret_cast<double *>(ws + plan.ee);
    a.rs = reinterpret_cast<double *>(ws + plan.rs);
}

static void ent_launch_norms(const EntArgs &a, hipStream_t st) {
    hipLaunchKernelGGL(ent_sqnorm_kernel, dim3((unsigned)((a.N + kEntThreads - 1) / kEntThreads)), dim3(kEntThreads), 0, st, a.z, a.zz);
    hipLaunchKernelGGL(ent_sqnorm_kernel, dim3((unsigned)((a.K + kEntThreads - 1) / kEntThreads)), dim3(kEntThreads), 0, st, a.e, a.ee);
}

template <int DT>
static void ent_launch_bwd(EntArgs a, const EntPlan &plan, hipStream_t st) {
    const dim3 rows((unsigned)((a.N + kEntTile - 1) / kEntTile)), block(kEntThreads);
    if (a.grad_z) hipLaunchKernelGGL((ent_row_bwd_kernel<DT, true>), rows, block, 0, st, a);
    else hipLaunchKernelGGL((ent_row_bwd_kernel<DT, false>), rows, block, 0, st, a);
    if (!a.grad_e) return;
    a.rows_per_part = plan.rpp_grad;
    a.P = plan.P_grad;
    hipLaunchKernelGGL((ent_grad_e_kernel<DT>), dim3((unsigned)a.P, (unsigned)((a.K + kEntTile - 1) / kEntTile)), block, 0, st, a);
    hipLaunchKernelGGL(ent_grad_e_reduce_kernel, dim3((unsigned)(((long long)a.K * a.D + kEntThreads - 1) / kEntThreads)), block, 0, st, a);
}

}  // namespace vqvae

using namespace vqvae;

extern "C" {

size_t vqvae_vq_entropy_workspace_bytes(int64_t N, int K, int D) {
    if (N < 1 || N > INT32_MAX || K < 1 || K > kEntMaxK || D < 1 || D > kEntMaxD) return 0;
    return ent_plan(N, K, D).total;
}

int vqvae_vq_entropy_forward_f32(const float *z_e, const float *codebook, int64_t B, int D, int H, int W, int K, double inv_temperature,
                                 double gamma, int flags, float *losses, double *avg, double *rowstat, void *workspace,
                                 size_t workspace_bytes, vqvae_stream_t stream) {
    if (!z_e || !codebook || !losses || !avg) return VQVAE_ERR_NULL;
    long long N;
    int HW;
    int rc = ent_shape(B, D, H, W, K, inv_temperature, gamma, flags, N, HW);
    if (rc != VQVAE_OK) return rc;
    const EntPlan plan = ent_plan(N, K, D);
    const Span in[] = {{z_e, (size_t)N * D * 4, 4}, {codebook, (size_t)K * D * 4, 4}};
    const Span out[] = {{losses, 12, 4}, {avg, (size_t)K * 8, 8}, {rowstat, (size_t)N * 16, 8}, {workspace, plan.total, 8}};
    if ((rc = check_pointers(in, 2, out, 4)) != VQVAE_OK || (rc = check_outputs_apart(out, 4)) != VQVAE_OK) return rc;
    if (!workspace || workspace_bytes < plan.total) return VQVAE_ERR_WORKSPACE;
    char *ws = static_cast<char *>(workspace);
    hipStream_t st = static_cast<hipStream_t>(stream);
    EntArgs a = {};
    ent_common(a, z_e, codebook, N, HW, K, D, inv_temperature, gamma, flags, ws, plan);
    a.rows_per_part = plan.rpp_avg; a.P = plan.P_avg;
    a.rs_out = rowstat; a.avg = avg; a.losses = losses;
    a.avg_part = reinterpret_cast<double *>(ws + plan.avg_part);
    a.sc_part = reinterpret_cast<double *>(ws + plan.sc_part);
    const dim3 block(kEntThreads);
    ent_launch_norms(a, st);
    hipLaunchKernelGGL(ent_row_fwd_kernel, dim3((unsigned)((N + kEntTile - 1) / kEntTile)), block, 0, st, a);
    hipLaunchKernelGGL(ent_avg_kernel, dim3((unsigned)a.P, (unsigned)((K + kEntTile - 1) / kEntTile)), block, 0, st, a);
    hipLaunchKernelGGL(ent_avg_reduce_kernel, dim3((unsigned)((K + kEntThreads - 1) / kEntThreads)), block, 0, st, a);
    hipLaunchKernelGGL(ent_finalize_kernel, dim3(1), block, 0, st, a);
    return (int)hipGetLastError();
}

int vqvae_vq_entropy_backward_f32(const float *z_e, const float *codebook, const double *avg, const double *rowstat,
                                  const float *grad_loss, int64_t B, int D, int H, int W, int K, double inv_temperature, double gamma,
                                  int flags, float *grad_z, float *grad_codebook, void *workspace, size_t workspace_bytes,
                                  vqvae_stream_t stream) {
    if (!z_e || !codebook || !avg || !rowstat || (!grad_z && !grad_codebook)) return VQVAE_ERR_NULL;
    long long N;
    int HW;
    int rc = ent_shape(B, D, H, W, K, inv_temperature, gamma, flags, N, HW);
    if (rc != VQVAE_OK) return rc;
    const EntPlan plan = ent_plan(N, K, D);
    const Span in[] = {{z_e, (size_t)N * D * 4, 4}, {codebook, (size_t)K * D * 4, 4}, {avg, (size_t)K * 8, 8},
                       {rowstat, (size_t)N * 16, 8}, {grad_loss, 4, 4}};
    const Span out[] = {{grad_z, (size_t)N * D * 4, 4}, {grad_codebook, (size_t)K * D * 4, 4}, {workspace, plan.total, 8}};
    if ((rc = check_pointers(in, 5, out, 3)) != VQVAE_OK || (rc = check_outputs_apart(out, 3)) != VQVAE_OK) return rc;
    if (!workspace || workspace_bytes < plan.total) return VQVAE_ERR_WORKSPACE;
    char *ws = static_cast<char *>(workspace);
    hipStream_t st = static_cast<hipStream_t>(stream);
    EntArgs a = {};
    ent_common(a, z_e, codebook, N, HW, K, D, inv_temperature, gamma, flags, ws, plan);
    a.rs = const_cast<double *>(rowstat);                                     // read only in this chain
    a.avg = const_cast<double *>(avg);
    a.gl = grad_loss; a.grad_z = grad_z; a.grad_e = grad_codebook;
    a.logavg = reinterpret_cast<double *>(ws + plan.logavg);
    a.m = reinterpret_cast<double *>(ws + plan.m);
    a.ge_part = reinterpret_cast<double *>(ws + plan.ge_part);
    a.as_part = reinterpret_cast<double *>(ws + plan.as_part);
    ent_launch_norms(a, st);
    hipLaunchKernelGGL(ent_logavg_kernel, dim3((unsigned)((K + kEntThreads - 1) / kEntThreads)), dim3(kEntThreads), 0, st, a);
    if (D <= 64) ent_launch_bwd<64>(a, plan, st);
    else if (D <= 128) ent_launch_bwd<128>(a, plan, st);
    else ent_launch_bwd<256>(a, plan, st);
    return (int)hipGetLastError();
}

}  // extern "C"
