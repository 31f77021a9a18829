// Training-step companions of the forward path, gfx950.
//
//   vqvae_vq_backward_f32      gradients of VectorQuantizer.forward as autograd derives them from
//                              models/quantizer.py:63-67:
//                                dL/dz   = g_zq + g_loss * 2 (z - e_idx) / (N D)         (:63 first term, :67)
//                                dL/dE_k = g_loss * 2 beta * sum_{i: idx_i = k} (e_k - z_i) / (N D)   (:63-64)
//                              The codebook gradient is a segmented sum over the rows of each code.  It is
//                              computed WITHOUT floating-point atomics: rows are sorted by code (stable radix
//                              sort, so row order inside a code is ascending), every 512-row chunk of a code is
//                              added in a fixed order in fp64 by one workgroup, and a code's chunks are combined in a
//                              fixed order -- the result is bit-reproducible from run to run, and the work is
//                              proportional to the rows however skewed the code histogram is.
//                              With VQVAE_VQ_BWD_ROTATION the g_zq term of dL/dz goes through the rotation trick instead
//                              (vq_rotation.hip states the arithmetic and holds the kernel); nothing else changes.
//   vqvae_vq_ema_update_f32    the codebook update of VectorQuantizerEMA (arXiv 1711.00937 Appendix A.1): the same sorted,
//                              fixed-order fp64 per-code sums, then exponential moving averages of counts and sums and the
//                              Laplace-smoothed normalisation (optionally restarting codes whose average count is below a
//                              threshold on rows of the batch).  Bit-reproducible, no host sync.
//   vqvae_recon_loss_f32       main.py:75-76 and the three scalars of :81-83 packed into one 3-float buffer
//                              (one D2H copy per step instead of three).
//   vqvae_recon_loss_backward_f32   d/dx_hat of mean((x_hat - x)^2) / var.
#include "train_reduce.h"
#include "vq_rotation.h"

namespace vqvae {

constexpr int kReconGrid = 1024;      // partial sums of the reconstruction loss

// dL/dE_k from the units of the sorted segmented sum (launch_segsum, train_reduce.h): cnt_k e_k - sum of the code's rows
__global__ __launch_bounds__(256) void vqb_codebook_grad_kernel(const float *__restrict__ cb,
                                                                const int *__restrict__ offsets,
                                                                const int *__restrict__ unit_start,
                                                                const double *__restrict__ partial,
                                                                const float *__restrict__ g_loss, int K, int D,
                                                                double scale, float *__restrict__ grad_cb) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)K * D) return;
    const int k = (int)(e / D), c = (int)(e - (long long)k * D);
    const double zsum = segsum_key_sum(unit_start, partial, k, c, D);
    const double cnt = (double)(offsets[k + 1] - offsets[k]);
    const double gl = g_loss ? (double)g_loss[0] : 1.0;
    grad_cb[e] = (float)(gl * scale * (cnt * (double)cb[e] - zsum));
}

// grad_z = g_zq + g_loss * s * (z - e_idx); one thread per element, row-major or NCHW addressing
__global__ __launch_bounds__(256) void vqb_gradz_kernel(const float *__restrict__ z, const float *__restrict__ cb,
                                                        const long long *__restrict__ idx,
                                                        const float *__restrict__ g_zq,
                                                        const float *__restrict__ g_loss, long long total, int D,
                                                        int HW, int rowmajor, float scale,
                                                        float *__restrict__ grad_z) {
    const float gs = (g_loss ? g_loss[0] : 1.0f) * scale;
    if (rowmajor < 0) {
        // row-major rows with D % 4 == 0 and 16-byte aligned tensors (the launch checks): four channels per thread
        for (long long e4 = (long long)blockIdx.x * 256 + threadIdx.x; e4 < (total >> 2); e4 += (long long)gridDim.x * 256) {
            const long long e = e4 << 2, row = e / D;
            const int c = (int)(e - row * D);
            const f32x4 zv = *reinterpret_cast<const f32x4 *>(z + e);
            const f32x4 ev = *reinterpret_cast<const f32x4 *>(cb + (size_t)idx[row] * D + c);
            f32x4 o;
            o.x = gs * (zv.x - ev.x); o.y = gs * (zv.y - ev.y); o.z = gs * (zv.z - ev.z); o.w = gs * (zv.w - ev.w);
            if (g_zq) {
                const f32x4 gv = *reinterpret_cast<const f32x4 *>(g_zq + e);
                o.x = gv.x + o.x; o.y = gv.y + o.y; o.z = gv.z + o.z; o.w = gv.w + o.w;
            }
            *reinterpret_cast<f32x4 *>(grad_z + e) = o;
        }
        return;
    }
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        long long row;
        int c;
        if (rowmajor) {
            row = e / D;
            c = (int)(e - row * D);
        } else {
            const long long plane = e / HW;          // b*D + c
            const int hw = (int)(e - plane * HW);
            const long long b = plane / D;
            c = (int)(plane - b * D);
            row = b * HW + hw;
        }
        const long long k = idx[row];
        const float d = z[e] - cb[(size_t)k * D + c];
        const float g = gs * d;
        grad_z[e] = g_zq ? g_zq[e] + g : g;
    }
}

__global__ __launch_bounds__(256) void recon_partial_kernel(const float *__restrict__ a, const float *__restrict__ b,
                                                            long long n, double *__restrict__ partial) {
    __shared__ double red[256];
    double acc = 0.0;
    const long long n4 = n >> 2;
    const f32x4 *a4 = reinterpret_cast<const f32x4 *>(a), *b4 = reinterpret_cast<const f32x4 *>(b);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const f32x4 u = a4[i], v = b4[i];
        const float d0 = u.x - v.x, d1 = u.y - v.y, d2 = u.z - v.z, d3 = u.w - v.w;
        acc += (double)(d0 * d0) + (double)(d1 * d1) + (double)(d2 * d2) + (double)(d3 * d3);
    }
    if (blockIdx.x == 0)
        for (long long i = (n4 << 2) + threadIdx.x; i < n; i += 256) {
            const float d = a[i] - b[i];
            acc += (double)(d * d);
        }
    block_sum_f64(red, threadIdx.x, acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(256) void recon_final_kernel(const double *__restrict__ partial, int np, long long n,
                                                          float inv_var, const float *__restrict__ embedding_loss,
                                                          const float *__restrict__ perplexity,
                                                          float *__restrict__ out3) {
    __shared__ double red[256];
    double acc = 0.0;
    for (int i = threadIdx.x; i < np; i += 256) acc += partial[i];
    block_sum_f64(red, threadIdx.x, acc);
    if (threadIdx.x == 0) {
        const float mse = (float)(red[0] / (double)n);          // torch.mean((x_hat - x)**2)   main.py:75
        const float recon = mse * inv_var;                       //   / x_train_var
        out3[0] = recon;
        out3[1] = recon + (embedding_loss ? embedding_loss[0] : 0.0f);   // loss = recon + embedding   :76
        out3[2] = perplexity ? perplexity[0] : 0.0f;
    }
}

__global__ __launch_bounds__(256) void recon_backward_kernel(const float *__restrict__ a, const float *__restrict__ b,
                                                             long long n, float scale,
                                                             const float *__restrict__ g_loss,
                                                             float *__restrict__ grad) {
    const float s = (g_loss ? g_loss[0] : 1.0f) * scale;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256)
        grad[i] = s * (a[i] - b[i]);
}

// ---- EMA codebook update (arXiv 1711.00937 Appendix A.1; include/vqvae_hip.h, vqvae_vq_ema_update_f32) ----

struct EmaPlan {
    SegsumPlan seg;                 // the segmented sum's workspace, first
    size_t off_nk, off_n, total;
};

static EmaPlan ema_plan(long long N, int K, int D) {
    EmaPlan p;
    p.seg = segsum_plan(N, K, D);
    p.off_nk = align_up(p.seg.total, 256);
    p.off_n = align_up(p.off_nk + (size_t)K * sizeof(double), 256);
    p.total = align_up(p.off_n + sizeof(double), 256);
    return p;
}

// N_k <- decay N_k + (1 - decay) c_k in fp64 (c_k from the sorted offsets), kept unrounded in nk[]; n = sum_k N_k in a fixed
// order (contiguous codes per thread, then a fixed tree).  One block: K <= 16384.
__global__ __launch_bounds__(1024) void vqe_counts_kernel(const int *__restrict__ offsets, const float *__restrict__ cluster_size,
                                                          int K, double decay, double *__restrict__ nk,
                                                          double *__restrict__ n_total) {
    __shared__ double part[1024];
    const int tid = threadIdx.x;
    const int per = (K + 1023) / 1024;
    double local = 0.0;
    for (int j = 0; j < per; ++j) {
        const int k = tid * per + j;
        if (k < K) {
            const double v = decay * (double)cluster_size[k] + (1.0 - decay) * (double)(offsets[k + 1] - offsets[k]);
            nk[k] = v;
            local += v;
        }
    }
    part[tid] = local;
    __syncthreads();
    for (int o = 512; o > 0; o >>= 1) {
        if (tid < o) part[tid] += part[tid + o];
        __syncthreads();
    }
    if (tid == 0) *n_total = part[0];
}

// One thread per (k, c): s_k[c] from the code's unit partials (the codebook gradient's fixed order), m <- decay m + (1 - decay) s,
// then e_k = m / ((N_k + eps) / (n + K eps) * n), or, with restart on and N_k < threshold, row r_k = min(floor(u_k N), N - 1) of z.
// Everything in fp64, rounded once on the store.  Reads only ws / ema_w / z, so codebook may be any buffer of K x D floats.
__global__ __launch_bounds__(256) void vqe_update_kernel(const float *__restrict__ z, const int *__restrict__ unit_start,
                                                         const double *__restrict__ partial, const double *__restrict__ nk,
                                                         const double *__restrict__ n_total, const float *__restrict__ uniforms,
                                                         long long N, int K, int D, int HW, int rowmajor, double decay,
                                                         double eps, double threshold, float *__restrict__ cluster_size,
                                                         float *__restrict__ ema_w, float *__restrict__ codebook) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)K * D) return;
    const int k = (int)(e / D), c = (int)(e - (long long)k * D);
    const double s = segsum_key_sum(unit_start, partial, k, c, D);
    const double m = decay * (double)ema_w[e] + (1.0 - decay) * s;
    const double Nk = nk[k];
    double ek;
    if (uniforms && Nk < threshold) {
        long long r = (long long)floor((double)uniforms[k] * (double)N);
        r = r < 0 ? 0 : (r > N - 1 ? N - 1 : r);
        if (rowmajor) {
            ek = (double)z[(size_t)r * D + c];
        } else {
            const long long bb = r / HW;
            const int hw = (int)(r - bb * HW);
            ek = (double)z[((size_t)bb * D + c) * HW + hw];
        }
    } else {
        const double n = *n_total;
        const double smoothed = (Nk + eps) / (n + (double)K * eps) * n;
        ek = m / smoothed;
    }
    ema_w[e] = (float)m;
    codebook[e] = (float)ek;
    if (c == 0) cluster_size[k] = (float)Nk;
}

}  // namespace vqvae

using namespace vqvae;

extern "C" {

size_t vqvae_vq_backward_workspace_bytes(int64_t N, int K, int D) {
    if (N < 1 || N > INT32_MAX || K < 1 || K > 16384 || D < 1 || D > 256) return 0;
    return segsum_plan(N, K, D).total;
}

int vqvae_vq_backward_f32(const float *z_e, const float *codebook, const int64_t *idx, const float *grad_zq,
                          const float *grad_loss, int64_t B, int D, int H, int W, int K, float beta, int flags,
                          float *grad_z, float *grad_codebook, void *workspace, size_t workspace_bytes,
                          vqvae_stream_t stream) {
    const bool commitment = (flags & VQVAE_VQ_BWD_COMMITMENT) != 0, rotation = (flags & VQVAE_VQ_BWD_ROTATION) != 0;
    if (!z_e || !codebook || !idx || (!grad_z && !grad_codebook) || ((commitment || rotation) && !grad_z)) return VQVAE_ERR_NULL;
    if (B < 1 || D < 1 || H < 1 || W < 1 || K < 1) return VQVAE_ERR_SHAPE;
    if (D > 256 || K > 16384 || (commitment && grad_codebook)) return VQVAE_ERR_UNSUPPORTED;
    const long long HW = (long long)H * W, N = (long long)B * HW;
    if (N > INT32_MAX || N * D > ((long long)1 << 40)) return VQVAE_ERR_OVERFLOW;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rowmajor = (flags & VQVAE_VQ_ROWMAJOR) ? 1 : 0;
    const double nd = (double)N * (double)D;
    // the reference's z term is 2/(ND) (its commitment term carries no beta); the EMA quantizer's loss is beta * mse only
    const float gz_scale = commitment ? (float)(2.0 * (double)beta / nd) : (float)(2.0 / nd);
    if (grad_z && rotation && grad_zq) {
        // the rotation-trick gradient (vq_rotation.hip); without an upstream gradient rot(0) = 0: the launch below
        RotArgs a;
        a.z = z_e; a.cb = codebook; a.idx = reinterpret_cast<const long long *>(idx); a.g_zq = grad_zq; a.g_loss = grad_loss;
        a.N = N; a.D = D; a.HW = (int)HW; a.K = K; a.rowmajor = rowmajor; a.scale = gz_scale; a.out = grad_z;
        launch_vq_rotation_gradz(a, st);
    } else if (grad_z) {
        const long long total = N * D;
        const bool vec4 = rowmajor && (D & 3) == 0 &&
                          !((reinterpret_cast<uintptr_t>(z_e) | reinterpret_cast<uintptr_t>(codebook) | reinterpret_cast<uintptr_t>(grad_z) |
                             reinterpret_cast<uintptr_t>(grad_zq)) & 15);
        hipLaunchKernelGGL(vqb_gradz_kernel, dim3(grid_of(vec4 ? total >> 2 : total)), dim3(256), 0, st, z_e, codebook,
                           reinterpret_cast<const long long *>(idx), grad_zq, grad_loss, total, D, (int)HW, vec4 ? -1 : rowmajor,
                           gz_scale, grad_z);
    }
    if (grad_codebook) {
        const SegsumPlan p = segsum_plan(N, K, D);
        if (!workspace || workspace_bytes < p.total) return VQVAE_ERR_WORKSPACE;
        char *ws = static_cast<char *>(workspace);
        const hipError_t e = launch_segsum(p, z_e, reinterpret_cast<const long long *>(idx), N, K, D, (int)HW, rowmajor, ws, st);
        if (e != hipSuccess) return (int)e;
        const int *offsets = reinterpret_cast<const int *>(ws + p.off_offsets);
        const int *unit_start = reinterpret_cast<const int *>(ws + p.off_units);
        const double *partial = reinterpret_cast<const double *>(ws + p.off_partials);
        hipLaunchKernelGGL(vqb_codebook_grad_kernel, dim3((unsigned)(((long long)K * D + 255) / 256)), dim3(256), 0,
                           st, codebook, offsets, unit_start, partial, grad_loss, K, D, 2.0 * (double)beta / nd,
                           grad_codebook);
    }
    return (int)hipGetLastError();
}

size_t vqvae_vq_ema_workspace_bytes(int64_t N, int K, int D) {
    if (N < 1 || N > INT32_MAX || K < 1 || K > 16384 || D < 1 || D > 256) return 0;
    return ema_plan(N, K, D).total;
}

int vqvae_vq_ema_update_f32(const float *z_e, const int64_t *idx, int64_t B, int D, int H, int W, int K, double decay,
                            double eps, double threshold, const float *uniforms, int flags, float *ema_cluster_size,
                            float *ema_w, float *codebook, void *workspace, size_t workspace_bytes, vqvae_stream_t stream) {
    if (!z_e || !idx || !ema_cluster_size || !ema_w || !codebook) return VQVAE_ERR_NULL;
    if (B < 1 || D < 1 || H < 1 || W < 1 || K < 1) return VQVAE_ERR_SHAPE;
    const long long HW = (long long)H * W, N = (long long)B * HW;
    if (D > 256 || K > 16384 || N > INT32_MAX || (flags & ~VQVAE_VQ_ROWMAJOR)) return VQVAE_ERR_UNSUPPORTED;
    if (!(decay >= 0.0 && decay <= 1.0) || !(eps > 0.0)) return VQVAE_ERR_UNSUPPORTED;
    const EmaPlan p = ema_plan(N, K, D);
    if (!workspace || workspace_bytes < p.total) return VQVAE_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rowmajor = (flags & VQVAE_VQ_ROWMAJOR) ? 1 : 0;
    char *ws = static_cast<char *>(workspace);
    const hipError_t e = launch_segsum(p.seg, z_e, reinterpret_cast<const long long *>(idx), N, K, D, (int)HW, rowmajor, ws, st);
    if (e != hipSuccess) return (int)e;
    const int *offsets = reinterpret_cast<const int *>(ws + p.seg.off_offsets);
    const int *unit_start = reinterpret_cast<const int *>(ws + p.seg.off_units);
    const double *partial = reinterpret_cast<const double *>(ws + p.seg.off_partials);
    double *nk = reinterpret_cast<double *>(ws + p.off_nk);
    double *n_total = reinterpret_cast<double *>(ws + p.off_n);
    hipLaunchKernelGGL(vqe_counts_kernel, dim3(1), dim3(1024), 0, st, offsets, ema_cluster_size, K, decay, nk, n_total);
    const bool restart = uniforms && threshold >= 0.0;
    hipLaunchKernelGGL(vqe_update_kernel, dim3((unsigned)(((long long)K * D + 255) / 256)), dim3(256), 0, st, z_e, unit_start,
                       partial, nk, n_total, restart ? uniforms : nullptr, N, K, D, (int)HW, rowmajor, decay, eps,
                       restart ? threshold : 0.0, ema_cluster_size, ema_w, codebook);
    return (int)hipGetLastError();
}

size_t vqvae_recon_loss_workspace_bytes(void) { return (size_t)kReconGrid * sizeof(double); }

int vqvae_recon_loss_f32(const float *x_hat, const float *x, int64_t n, float inv_var,
                         const float *embedding_loss, const float *perplexity, float *out3, void *workspace,
                         size_t workspace_bytes, vqvae_stream_t stream) {
    if (!x_hat || !x || !out3) return VQVAE_ERR_NULL;
    if (n < 1) return VQVAE_ERR_SHAPE;
    if (!workspace || workspace_bytes < vqvae_recon_loss_workspace_bytes()) return VQVAE_ERR_WORKSPACE;
    if ((reinterpret_cast<uintptr_t>(x_hat) | reinterpret_cast<uintptr_t>(x)) & 15) return VQVAE_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const unsigned grid = grid_of(n >> 2, kReconGrid);
    double *partial = static_cast<double *>(workspace);
    hipLaunchKernelGGL(recon_partial_kernel, dim3(grid), dim3(256), 0, st, x_hat, x, (long long)n, partial);
    hipLaunchKernelGGL(recon_final_kernel, dim3(1), dim3(256), 0, st, partial, (int)grid, (long long)n, inv_var,
                       embedding_loss, perplexity, out3);
    return (int)hipGetLastError();
}

int vqvae_recon_loss_backward_f32(const float *x_hat, const float *x, int64_t n, float inv_var,
                                  const float *grad_loss, float *grad_x_hat, vqvae_stream_t stream) {
    if (!x_hat || !x || !grad_x_hat) return VQVAE_ERR_NULL;
    if (n < 1) return VQVAE_ERR_SHAPE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(recon_backward_kernel, dim3(grid_of(n)), dim3(256), 0, st, x_hat, x, (long long)n,
                       (float)(2.0 * (double)inv_var / (double)n), grad_loss, grad_x_hat);
    return (int)hipGetLastError();
}

}  // extern "C"
