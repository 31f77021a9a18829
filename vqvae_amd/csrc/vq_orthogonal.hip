// The orthogonal regularization loss of a codebook (gfx950): the squared cosine similarities between the selected codes,
// L = |E^ E^T|_F^2 / M^2 - 1 / M (arXiv 2112.00384 section 3.2; `orthogonal_reg_weight`, `orthogonal_reg_active_codes_only` and
// `orthogonal_reg_max_codes` in vector-quantize-pytorch), and its gradient, in one K^2 D pass with no (K, K) array.
//   vqvae_vq_orthogonal_workspace_bytes
//   vqvae_vq_orthogonal_forward_f32     rows (K, D), taken as they stand (the caller normalises) -> loss, M, selected, V
//   vqvae_vq_orthogonal_backward_f32    V -> grad_rows
// 1 <= K <= 16384, 1 <= D <= 256.
//
// THE ARITHMETIC IS THE CONTRACT (tests/vq_orthogonal_ref.py restates it on the CPU).  Every line is one IEEE operation in the
// stated precision; n is `rows`.
//
//   candidate(k) = hist == NULL or hist[k] > 0
//   selected[k]  = candidate(k), and, under a cap (uniforms != NULL and max_codes > 0), fewer than max_codes candidates j come before
//                  k in the order (u_j < u_k, or u_j == u_k and j < k).  M = sum_k selected[k].
//   G_ij    = sum_c double(n_ic) double(n_jc)            from 0.0, c ascending (each product is exact in fp64)
//   R_i     = sum_{j selected} fl(G_ij G_ij)             from 0.0, j ascending; the product rounded to fp64, then the add
//   V_ic    = sum_{j selected} fl(G_ij double(n_jc))     from 0.0, j ascending; the product rounded to fp64, then the add
//   both for selected i; R_i = 0.0 and V_ic = 0.0 for an unselected i.  An unselected j contributes nothing.
//   T       = see below
//   loss    = float(T / (double(M) double(M)) - 1.0 / double(M)),        0 where M = 0
//   grad_rows[i][c] = float((double(g) (4.0 / (double(M) double(M)))) V_ic) for selected i, +0.0 otherwise;  g = *grad_loss or 1
//
// THE ORDER OF THE TOTAL depends on K alone: the codes are cut into blocks of 256 consecutive codes (the last one ragged); inside a
// block the R_i are added in ascending i, starting from 0.0 -- every code's, an unselected one's being +0.0, which changes no bit of
// a sum of non-negative terms; then the blocks' sums are added in ascending block order, starting from 0.0.  Neither the launch
// shape nor the selection enters.
//
// `saved` receives V (all K rows).  With saved == NULL the V sums are not formed at all.
//
// A non-finite value in a selected row makes G non-finite in that row and column, hence every selected row's R and V and the loss
// (which NaN is unspecified); unselected rows are written as constants and never see it.
//
// The product of two fp32 values is exact in fp64, so the Gram sums use v_fma_f64 (__builtin_fma) although the library is compiled
// with -ffp-contract=off; G G and G n are NOT exact, and are a multiplication and an addition.  The fp64 matrix instructions are not
// used: the order in which they add the four products of a block internally is not documented, and the order is the contract.
//
// Launches, all on the caller's stream: the selection (one thread per code, the rank an O(K^2) comparison), the main kernel
// (vq_orthogonal.h), the total.  No host sync, no allocation, no memset, no atomic of any kind: capturable, and the same bits in
// every run, at every pointer alignment and in a graph replay.  The workspace holds the K row sums.
#include "common.h"
#include "vq_orthogonal.h"

namespace vqvae {

__global__ __launch_bounds__(kOrthThreads) void orth_select_kernel(const int32_t *hist, const float *u, int max_codes, int K,
                                                                   int32_t *selected) {
    orth_select_body(hist, u, max_codes, K, selected);
}

template <int DT, bool WANT_V>
__global__ __launch_bounds__(kOrthThreads) void orth_main_kernel(OrthArgs a) {
    __shared__ __attribute__((aligned(16))) float ni[kOrthRows * (DT + 4)];
    __shared__ __attribute__((aligned(16))) float nj[kOrthTile * (DT + 4)];
    __shared__ double g[kOrthRows * kOrthTile];
    __shared__ int selj[kOrthTile];
    orth_main_body<DT, WANT_V>(a, ni, nj, g, selj);
}

__global__ __launch_bounds__(kOrthThreads) void orth_finalize_kernel(const double *r, const int32_t *selected, int K, float *loss,
                                                                     int32_t *count) {
    __shared__ double part[kOrthSumBlocks];
    __shared__ int cnt[kOrthThreads];
    orth_finalize_body(r, selected, K, loss, count, part, cnt);
}

__global__ __launch_bounds__(kOrthThreads) void orth_backward_kernel(const double *saved, const int32_t *selected, const int32_t *count,
                                                                     const float *grad_loss, int K, int D, float *grad_rows) {
    orth_backward_body(saved, selected, count, grad_loss, K, D, grad_rows, gridDim.x);
}

template <int DT>
static void orth_launch_main(const OrthArgs &a, hipStream_t st) {
    const dim3 grid((unsigned)((a.K + kOrthRows - 1) / kOrthRows)), block(kOrthThreads);
    if (a.v) hipLaunchKernelGGL((orth_main_kernel<DT, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((orth_main_kernel<DT, false>), grid, block, 0, st, a);
}

// every pointer aligned (NULL passes), no output on an input, nor on another output
static int orth_pointers(const Span *in, int n_in, const Span *out, int n_out) {
    const int rc = check_pointers(in, n_in, out, n_out);
    return rc != VQVAE_OK ? rc : check_outputs_apart(out, n_out);
}

static int orth_shape(int K, int D) {
    if (K < 1 || D < 1) return VQVAE_ERR_SHAPE;
    if (K > kOrthMaxK || D > kOrthMaxD) return VQVAE_ERR_UNSUPPORTED;
    return VQVAE_OK;
}

}  // namespace vqvae

using namespace vqvae;

extern "C" {

size_t vqvae_vq_orthogonal_workspace_bytes(int K, int D) {
    if (orth_shape(K, D) != VQVAE_OK) return 0;
    return (size_t)K * sizeof(double);
}

int vqvae_vq_orthogonal_forward_f32(const float *rows, const int32_t *hist, const float *uniforms, int max_codes, int K, int D,
                                    int flags, float *loss, int32_t *count, int32_t *selected, double *saved, void *workspace,
                                    size_t workspace_bytes, vqvae_stream_t stream) {
    if (!rows || !loss || !count || !selected) return VQVAE_ERR_NULL;
    int rc = orth_shape(K, D);
    if (rc != VQVAE_OK) return rc;
    if (flags) return VQVAE_ERR_UNSUPPORTED;
    const size_t need = (size_t)K * sizeof(double);
    const Span in[] = {{rows, (size_t)K * D * 4, 4}, {hist, (size_t)K * 4, 4}, {uniforms, (size_t)K * 4, 4}};
    const Span out[] = {{loss, 4, 4}, {count, 4, 4}, {selected, (size_t)K * 4, 4}, {saved, (size_t)K * D * 8, 8},
                            {workspace, need, 8}};
    if ((rc = orth_pointers(in, 3, out, 5)) != VQVAE_OK) return rc;
    if (!workspace || workspace_bytes < need) return VQVAE_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(orth_select_kernel, dim3((unsigned)((K + kOrthThreads - 1) / kOrthThreads)), dim3(kOrthThreads), 0, st, hist,
                       uniforms, max_codes, K, selected);
    OrthArgs a = {};
    a.rows = rows; a.selected = selected; a.r = static_cast<double *>(workspace); a.v = saved; a.K = K; a.D = D;
    if (D <= 64) orth_launch_main<64>(a, st);
    else if (D <= 128) orth_launch_main<128>(a, st);
    else orth_launch_main<256>(a, st);
    hipLaunchKernelGGL(orth_finalize_kernel, dim3(1), dim3(kOrthThreads), 0, st, a.r, selected, K, loss, count);
    return (int)hipGetLastError();
}

int vqvae_vq_orthogonal_backward_f32(const double *saved, const int32_t *selected, const int32_t *count, const float *grad_loss, int K,
                                     int D, float *grad_rows, vqvae_stream_t stream) {
    if (!saved || !selected || !count || !grad_rows) return VQVAE_ERR_NULL;
    int rc = orth_shape(K, D);
    if (rc != VQVAE_OK) return rc;
    const Span in[] = {{saved, (size_t)K * D * 8, 8}, {selected, (size_t)K * 4, 4}, {count, 4, 4}, {grad_loss, 4, 4}};
    const Span out[] = {{grad_rows, (size_t)K * D * 4, 4}};
    if ((rc = orth_pointers(in, 4, out, 1)) != VQVAE_OK) return rc;
    hipLaunchKernelGGL(orth_backward_kernel, dim3(grid_of((long long)K * D, 2048)), dim3(kOrthThreads), 0, static_cast<hipStream_t>(stream),
                       saved, selected, count, grad_loss, K, D, grad_rows);
    return (int)hipGetLastError();
}

}  // extern "C"
