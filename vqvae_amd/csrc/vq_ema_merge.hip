// The EMA codebook update (train.hip, vqvae_vq_ema_update_f32) cut in two, so that the statistics of several shards -- the batches of
// other ranks, or earlier micro-batches of this rank -- can be merged before the codebook moves (include/vqvae_hip.h):
//
//   vqvae_vq_ema_stats_f32   (z_e, idx) of one shard -> its sufficient statistics, one fp64 record (K, C)
//   vqvae_vq_ema_apply_f32   the records of R shards, added in shard order -> ema_cluster_size, ema_w, codebook
//
// Numeric contract.
//
// stats, per shard of N_s = B H W rows.  C = D + 1 without row_uniforms, C = 2 D + 1 with them.  Row k of the record holds
//   c_k           column 0: #{i : idx_i = k}, an exact integer stored as a double (idx clamped into [0, K) as the sort clamps it);
//   s_k[0 .. D)   columns 1 .. D: the fp64 sum of the shard's rows of code k, exactly the value segsum_key_sum returns after
//                 launch_segsum, unrounded -- the order, the sort and the clamp of vqvae_vq_ema_update_f32;
//   cand_k[0 .. D)  columns D + 1 .. 2 D, only with row_uniforms: row rho_k = clamp(floor(double(u_k) N_s), 0, N_s - 1) of this
//                 shard's z_e, each fp32 value converted to double: the shard's restart candidate for code k.
// Every element of the record is written (no memset), nothing is added with a floating-point atomic, and both layouts of z_e give
// the same bits.
//
// apply, over R records laid out (R, K, C), shard-major.
//   c_k = sum_s c_{s,k}                        (exact integers)
//   S_k = ((s_{0,k} + s_{1,k}) + ...)          fp64, in shard order, starting from shard 0's value itself
//   N_k <- decay N_k + (1 - decay) c_k;  n = sum_k N_k in vqe_counts_kernel's order (contiguous codes per thread, its tree)
//   m_k <- decay m_k + (1 - decay) S_k;  e_k = m_k / ((N_k + eps) / (n + K eps) n)
// -- vqvae_vq_ema_update_f32's operations, operation for operation, in fp64 with one rounding per store.
// Restart is on with shard_uniforms != NULL, threshold >= 0 and C = 2 D + 1: a code with N_k < threshold takes
// float(cand_{j_k,k}), j_k = clamp(floor(double(v_k) R), 0, R - 1); N_k and m_k stay as updated.  A NaN in a candidate is read
// only for its own code: it stays in that code's row.  (shard_uniforms with C = D + 1: VQVAE_ERR_UNSUPPORTED.)
// R = 1: all three outputs have the bits of vqvae_vq_ema_update_f32 with row_uniforms as its `uniforms`.
//
// Envelope.  stats: that of vqvae_vq_ema_update_f32 (K <= 16384, D <= 256, 1 <= N_s <= INT32_MAX, no flag but VQVAE_VQ_ROWMAJOR).
// apply: 1 <= R <= 1024, C in {D + 1, 2 D + 1}, decay in [0, 1], eps > 0.  VQVAE_ERR_UNSUPPORTED outside either, and for a stats
// pointer that is not 8-byte aligned; the sizing calls then return 0.  A NULL mandatory pointer: VQVAE_ERR_NULL.  codebook must
// not alias ema_w or stats.
//
// Launches.  stats: launch_segsum, then ema_pack_kernel over (k, c).  apply: ema_count_kernel (one workgroup), then ema_apply_kernel
// over (k, c).  No host sync, no allocation, every launch on `stream` in one linear chain, no memset: both
// entries are capturable.
#include "train_reduce.h"
#include "vq_ema_merge.h"

namespace vqvae {

struct EmaApplyPlan {
    size_t off_nk, off_n, total;
};

static EmaApplyPlan ema_apply_plan(int K) {
    EmaApplyPlan p;
    p.off_nk = 0;
    p.off_n = align_up((size_t)K * sizeof(double), 256);
    p.total = align_up(p.off_n + sizeof(double), 256);
    return p;
}

__global__ __launch_bounds__(kEmaMergeThreads) void ema_pack_kernel(const float *__restrict__ z, const int *__restrict__ offsets,
                                                                    const int *__restrict__ unit_start,
                                                                    const double *__restrict__ partial,
                                                                    const float *__restrict__ row_uniforms, long long N, int K, int D,
                                                                    int C, int HW, int rowmajor, double *__restrict__ stats) {
    const long long e = (long long)blockIdx.x * kEmaMergeThreads + threadIdx.x;
    double sum = 0.0;
    if (e < (long long)K * C) {
        const int k = (int)(e / C), c = (int)(e - (long long)k * C);
        if (ema_stats_field(c, D) == 1) sum = segsum_key_sum(unit_start, partial, k, c - 1, D);
    }
    ema_pack_body(e, sum, offsets, z, row_uniforms, N, K, D, C, HW, rowmajor, stats);
}

__global__ __launch_bounds__(kEmaCountThreads) void ema_count_kernel(const double *__restrict__ stats, int R, int K, int C,
                                                                     const float *__restrict__ cluster_size, double decay,
                                                                     double *__restrict__ nk, double *__restrict__ n_total) {
    __shared__ double part[kEmaCountThreads];
    ema_count_body(stats, R, K, C, cluster_size, decay, nk, n_total, part);
}

__global__ __launch_bounds__(kEmaMergeThreads) void ema_apply_kernel(const double *__restrict__ stats, int R, int K, int D, int C,
                                                                     const double *__restrict__ nk,
                                                                     const double *__restrict__ n_total,
                                                                     const float *__restrict__ shard_uniforms, double decay, double eps,
                                                                     double threshold, float *__restrict__ cluster_size,
                                                                     float *__restrict__ ema_w, float *__restrict__ codebook) {
    const long long e = (long long)blockIdx.x * kEmaMergeThreads + threadIdx.x;
    ema_apply_body(e, stats, R, K, D, C, nk, n_total, shard_uniforms, decay, eps, threshold, cluster_size, ema_w, codebook);
}

static bool ema_stats_envelope(long long N, int K, int D) {
    return N >= 1 && N <= INT32_MAX && K >= 1 && K <= 16384 && D >= 1 && D <= 256;
}

static bool ema_apply_envelope(int R, int K, int D) {
    return R >= 1 && R <= kEmaMergeMaxR && K >= 1 && K <= 16384 && D >= 1 && D <= 256;
}

}  // namespace vqvae

using namespace vqvae;

extern "C" {

size_t vqvae_vq_ema_stats_workspace_bytes(int64_t N, int K, int D) {
    if (!ema_stats_envelope(N, K, D)) return 0;
    return segsum_plan(N, K, D).total;
}

int vqvae_vq_ema_stats_f32(const float *z_e, const int64_t *idx, int64_t B, int D, int H, int W, int K, const float *row_uniforms,
                           int flags, double *stats, void *workspace, size_t workspace_bytes, vqvae_stream_t stream) {
    if (!z_e || !idx || !stats) return VQVAE_ERR_NULL;
    if (B < 1 || D < 1 || H < 1 || W < 1 || K < 1) return VQVAE_ERR_SHAPE;
    const long long HW = (long long)H * W, N = (long long)B * HW;
    if (D > 256 || K > 16384 || N > INT32_MAX || (flags & ~VQVAE_VQ_ROWMAJOR)) return VQVAE_ERR_UNSUPPORTED;
    if (reinterpret_cast<uintptr_t>(stats) & 7) return VQVAE_ERR_UNSUPPORTED;
    const SegsumPlan p = segsum_plan(N, K, D);
    if (!workspace || workspace_bytes < p.total) return VQVAE_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rowmajor = (flags & VQVAE_VQ_ROWMAJOR) ? 1 : 0;
    char *ws = static_cast<char *>(workspace);
    const hipError_t e = launch_segsum(p, z_e, reinterpret_cast<const long long *>(idx), N, K, D, (int)HW, rowmajor, ws, st);
    if (e != hipSuccess) return (int)e;
    const int *offsets = reinterpret_cast<const int *>(ws + p.off_offsets);
    const int *unit_start = reinterpret_cast<const int *>(ws + p.off_units);
    const double *partial = reinterpret_cast<const double *>(ws + p.off_partials);
    const int C = row_uniforms ? 2 * D + 1 : D + 1;
    hipLaunchKernelGGL(ema_pack_kernel, dim3((unsigned)(((long long)K * C + kEmaMergeThreads - 1) / kEmaMergeThreads)),
                       dim3(kEmaMergeThreads), 0, st, z_e, offsets, unit_start, partial, row_uniforms, N, K, D, C, (int)HW, rowmajor,
                       stats);
    return (int)hipGetLastError();
}

size_t vqvae_vq_ema_apply_workspace_bytes(int R, int K, int D) {
    if (!ema_apply_envelope(R, K, D)) return 0;
    return ema_apply_plan(K).total;
}

int vqvae_vq_ema_apply_f32(const double *stats, int R, int K, int D, int C, double decay, double eps, double threshold,
                           const float *shard_uniforms, float *ema_cluster_size, float *ema_w, float *codebook, void *workspace,
                           size_t workspace_bytes, vqvae_stream_t stream) {
    if (!stats || !ema_cluster_size || !ema_w || !codebook) return VQVAE_ERR_NULL;
    if (K < 1 || D < 1) return VQVAE_ERR_SHAPE;
    if (!ema_apply_envelope(R, K, D) || (C != D + 1 && C != 2 * D + 1)) return VQVAE_ERR_UNSUPPORTED;
    if (!(decay >= 0.0 && decay <= 1.0) || !(eps > 0.0)) return VQVAE_ERR_UNSUPPORTED;
    if (shard_uniforms && C != 2 * D + 1) return VQVAE_ERR_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(stats) | reinterpret_cast<uintptr_t>(workspace)) & 7) return VQVAE_ERR_UNSUPPORTED;
    const EmaApplyPlan p = ema_apply_plan(K);
    if (!workspace || workspace_bytes < p.total) return VQVAE_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char *ws = static_cast<char *>(workspace);
    double *nk = reinterpret_cast<double *>(ws + p.off_nk);
    double *n_total = reinterpret_cast<double *>(ws + p.off_n);
    hipLaunchKernelGGL(ema_count_kernel, dim3(1), dim3(kEmaCountThreads), 0, st, stats, R, K, C, ema_cluster_size, decay, nk, n_total);
    const bool restart = shard_uniforms && threshold >= 0.0;
    hipLaunchKernelGGL(ema_apply_kernel, dim3((unsigned)(((long long)K * D + kEmaMergeThreads - 1) / kEmaMergeThreads)),
                       dim3(kEmaMergeThreads), 0, st, stats, R, K, D, C, nk, n_total, restart ? shard_uniforms : nullptr, decay, eps,
                       restart ? threshold : 0.0, ema_cluster_size, ema_w, codebook);
    return (int)hipGetLastError();
}

}  // extern "C"
