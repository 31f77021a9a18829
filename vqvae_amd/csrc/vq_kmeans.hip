// k-means initialisation of the codebook (gfx950): k-means++ seeding (Arthur & Vassilvitskii 2007) and one Lloyd mean update.
//   vqvae_vq_kmeans_workspace_bytes   host only: the larger of the two calls' workspaces
//   vqvae_vq_kmeans_seed_f32          kms_first_kernel, then per round kms_weights_kernel (one workgroup per selection block)
//                                     + kms_pick_kernel (one workgroup): 1 + 2 (K - 1) launches, a plain chain on the stream
//   vqvae_vq_kmeans_update_f32        the shared sorted segmented sum (launch_segsum, train_reduce.h) + kmu_update_kernel
// Assignment between the two is the quantizer itself (vqvae_vq_forward_f32); nothing of it is repeated here.
//
// THE OPERATION ORDER IS THE CONTRACT (tests/kmeans_ref.py restates it on the CPU; the library is compiled with
// -ffp-contract=off, so every multiply and add below is one IEEE fp64 operation).  Rows are the N = B H W rows of z_e in the
// quantizer's row order (NCHW: row r is pixel r % HW of image r / HW); u_k are the K caller-supplied fp32 uniforms in [0, 1),
// taken to fp64 exactly.  Inputs are expected to be finite.
//
//   Round 0:  rows[0] = min(floor(u_0 * N), N - 1).
//   Round k >= 1, weights.  With e = row rows[k - 1]:
//       dist_n = 0;  for c = 0 .. D - 1 in this order:  d = double(z_n[c]) - double(e[c]);  dist_n = dist_n + d * d
//       w_n = dist_n (k = 1), else dist_n if dist_n < w_n, else w_n          -- w_n >= 0, and 0 exactly on a chosen centre's copies
//   Round k >= 1, sums.  Three levels, none of which depends on the grid, the launch form or the layout -- only on N:
//       block b  = rows [256 b, 256 b + 256) (nb = ceil(N / 256) blocks, rows past N count as 0.0);
//                  S_b = block_sum_f64's tree over the 256 weights (red[i] += red[i + o] for o = 128, 64 ... 1);
//       group t  = blocks [t per, min((t + 1) per, nb)), per = ceil(nb / 256), t = 0 .. 255 (trailing groups may be empty: 0.0);
//                  G_t = ((S_first + S_next) + ...) sequentially in block order, starting from 0.0;
//       total    T = ((G_0 + G_1) + ...) + G_255 sequentially, starting from 0.0.
//   Round k >= 1, pick.  T == 0 (not T > 0: fewer than k + 1 distinct rows): rows[k] = min(floor(u_k * N), N - 1).  Otherwise
//   thr = u_k * T and one descent through the same three levels.  A level scans its items (groups; then the blocks of the selected
//   group; then the rows of the selected block, whose "sum" is w_n) in order with a running prefix that starts at `base` (0.0 at
//   the top):
//       for each item i with sum s:  inc = run + s;  if s > 0 and inc > thr: select i, its base is run, stop;  run = inc
//       nothing selected: select the LAST item with s > 0, its base being the prefix in front of it
//   and the next level starts from the selected item's base.  The selected row is rows[k].  So a row's inclusive prefix is the
//   sequential sum of the groups before its group, then of the blocks before its block inside the group, then of the rows up to it
//   inside the block; the row picked is the first whose prefix exceeds u_k T with w_n > 0, rounding between the levels (S_b is a
//   tree, the scan inside a block is sequential) resolved by the last positive item.  An item with a positive sum contains a row
//   with w_n > 0 (sums of non-negative terms), so while T > 0 a row with w_n = 0 -- a copy of a chosen centre -- is never picked.
//   Output.  codebook[k] = row rows[k], bit for bit.
//
// The dependency between rounds goes through device memory (rows[k - 1], the weights): the host reads nothing back, no workgroup
// waits on another one, no atomics.  The weights kernel streams z once per round (its roof is HBM, or L2 / MALL for the subsamples
// people initialise from); the pick kernel is one workgroup's latency.
//
//   Update (one Lloyd step from the quantizer's indices).  c_k = rows of code k, s_k = their sum from the segmented sum's units
//   (fp64, rows ascending inside a unit), a code's units combined in vqe_update_kernel's order: four interleaved running sums over
//   the units, then (z0 + z1) + (z2 + z3).  c_k > 0: e_k = fp32(s_k / double(c_k)), one division in fp64, one rounding.
//   c_k = 0: the code keeps its bits, or with uniforms takes row min(floor(u_k * N), N - 1).  counts[k] = c_k.
#include <math.h>

#include "train_reduce.h"

namespace vqvae {

constexpr int kKmBlockRows = 256;        // rows per selection block = threads per workgroup
constexpr int kKmGroups = 256;           // groups of consecutive blocks the pick kernel's threads sum

struct KmSeedPlan {
    long long nb, per;                   // selection blocks; blocks per group
    size_t off_w, off_bsum, total;
};

static KmSeedPlan km_seed_plan(long long N) {
    KmSeedPlan p;
    p.nb = (N + kKmBlockRows - 1) / kKmBlockRows;
    p.per = (p.nb + kKmGroups - 1) / kKmGroups;
    p.off_w = 0;
    p.off_bsum = align_up((size_t)N * sizeof(double), 256);
    p.total = align_up(p.off_bsum + (size_t)p.nb * sizeof(double), 256);
    return p;
}

// element c of row r; layout: 0 = NCHW images of HW pixels, else row-major
__device__ __forceinline__ float km_at(const float *__restrict__ z, long long r, int c, int D, int HW, int layout) {
    if (layout) return z[(size_t)r * D + c];
    const long long bb = r / HW;
    const int hw = (int)(r - bb * HW);
    return z[((size_t)bb * D + c) * HW + hw];
}

__device__ __forceinline__ long long km_uniform_row(float u, long long N) {
    long long r = (long long)floor((double)u * (double)N);
    return r < 0 ? 0 : (r > N - 1 ? N - 1 : r);
}

// round 0: rows[0] = min(floor(u_0 N), N - 1), codebook[0] = that row.  One workgroup.
__global__ __launch_bounds__(256) void kms_first_kernel(const float *__restrict__ z, const float *__restrict__ uniforms, long long N,
                                                        int D, int HW, int layout, long long *__restrict__ rows,
                                                        float *__restrict__ codebook) {
    const long long r = km_uniform_row(uniforms[0], N);
    if (threadIdx.x == 0) rows[0] = r;
    if ((int)threadIdx.x < D) codebook[threadIdx.x] = km_at(z, r, threadIdx.x, D, HW, layout);
}

// one workgroup per selection block, one thread per row: w_n against the centre of the previous round, and the block's sum.
// layout 2: row-major rows with D % 4 == 0 and a 16-byte aligned z (the launch checks): four channels per load.
__global__ __launch_bounds__(256) void kms_weights_kernel(const float *__restrict__ z, const long long *__restrict__ rows, int k,
                                                          long long N, int D, int HW, int layout, double *__restrict__ w,
                                                          double *__restrict__ bsum) {
    __shared__ double red[256];
    __shared__ float e[256];
    const int tid = threadIdx.x;
    long long centre = rows[k - 1];
    centre = centre < 0 ? 0 : (centre > N - 1 ? N - 1 : centre);          // (the pick kernel only writes rows inside [0, N))
    if (tid < D) e[tid] = km_at(z, centre, tid, D, HW, layout);
    __syncthreads();
    const long long r = (long long)blockIdx.x * kKmBlockRows + tid;
    double v = 0.0;
    if (r < N) {
        double acc = 0.0;
        if (layout == 2) {
            const f32x4 *zr = reinterpret_cast<const f32x4 *>(z + (size_t)r * D);
            for (int c4 = 0; c4 < (D >> 2); ++c4) {
                const f32x4 q = zr[c4];
                const double d0 = (double)q.x - (double)e[4 * c4], d1 = (double)q.y - (double)e[4 * c4 + 1];
                const double d2 = (double)q.z - (double)e[4 * c4 + 2], d3 = (double)q.w - (double)e[4 * c4 + 3];
                acc = acc + d0 * d0;
                acc = acc + d1 * d1;
                acc = acc + d2 * d2;
                acc = acc + d3 * d3;
            }
        } else {
            for (int c = 0; c < D; ++c) {
                const double d = (double)km_at(z, r, c, D, HW, layout) - (double)e[c];
                acc = acc + d * d;
            }
        }
        if (k > 1) {
            const double old = w[r];
            acc = acc < old ? acc : old;
        }
        w[r] = acc;
        v = acc;
    }
    block_sum_f64(red, tid, v);
    if (tid == 0) bsum[blockIdx.x] = red[0];
}

// One workgroup: group sums, total, the descent of the file header, rows[k] and codebook[k].
__global__ __launch_bounds__(256) void kms_pick_kernel(const float *__restrict__ z, const float *__restrict__ uniforms,
                                                       const double *__restrict__ w, const double *__restrict__ bsum, long long nb,
                                                       long long per, int k, long long N, int D, int HW, int layout,
                                                       long long *__restrict__ rows, float *__restrict__ codebook) {
    __shared__ double grp[kKmGroups];
    __shared__ double wrow[kKmBlockRows];
    __shared__ long long sh_blk, sh_row;
    __shared__ double sh_base, sh_thr;
    const int tid = threadIdx.x;
    {
        const long long b0 = (long long)tid * per;
        const long long b1 = b0 + per < nb ? b0 + per : nb;
        double g = 0.0;
        for (long long b = b0; b < b1; ++b) g = g + bsum[b];
        grp[tid] = g;
    }
    __syncthreads();
    if (tid == 0) {
        double T = 0.0;
        for (int t = 0; t < kKmGroups; ++t) T = T + grp[t];
        long long blk = -1;
        double base = 0.0, thr = 0.0;
        if (T > 0.0) {
            thr = (double)uniforms[k] * T;
            // groups
            int sel = -1, last = -1;
            double run = 0.0, last_base = 0.0;
            for (int t = 0; t < kKmGroups; ++t) {
                const double s = grp[t], inc = run + s;
                if (s > 0.0) {
                    last = t;
                    last_base = run;
                    if (inc > thr) { sel = t; base = run; break; }
                }
                run = inc;
            }
            if (sel < 0) { sel = last; base = last_base; }
            if (sel >= 0) {
                // the blocks of the selected group
                const long long b0 = (long long)sel * per;
                const long long b1 = b0 + per < nb ? b0 + per : nb;
                long long lastb = -1;
                run = base;
                last_base = base;
                for (long long b = b0; b < b1; ++b) {
                    const double s = bsum[b], inc = run + s;
                    if (s > 0.0) {
                        lastb = b;
                        last_base = run;
                        if (inc > thr) { blk = b; base = run; break; }
                    }
                    run = inc;
                }
                if (blk < 0) { blk = lastb; base = last_base; }
            }
        }
        sh_blk = blk;
        sh_base = base;
        sh_thr = thr;
        if (blk < 0) sh_row = km_uniform_row(uniforms[k], N);        // T == 0: fewer distinct rows than centres
    }
    __syncthreads();
    const long long blk = sh_blk;                                     // the same value in every thread: the barriers below are uniform
    if (blk >= 0) {
        const long long r = blk * kKmBlockRows + tid;
        wrow[tid] = r < N ? w[r] : 0.0;
        __syncthreads();
        if (tid == 0) {
            const double thr = sh_thr;
            double run = sh_base;
            int sel = -1, last = -1;
            for (int i = 0; i < kKmBlockRows; ++i) {
                const double s = wrow[i], inc = run + s;
                if (s > 0.0) {
                    last = i;
                    if (inc > thr) { sel = i; break; }
                }
                run = inc;
            }
            if (sel < 0) sel = last;
            long long row = sel >= 0 ? blk * kKmBlockRows + sel : km_uniform_row(uniforms[k], N);
            sh_row = row < 0 ? 0 : (row > N - 1 ? N - 1 : row);
        }
    }
    __syncthreads();
    const long long row = sh_row;
    if (tid == 0) rows[k] = row;
    if (tid < D) codebook[(size_t)k * D + tid] = km_at(z, row, tid, D, HW, layout);
}

// One thread per (k, c): the code's mean from its units, or its old bits / a row of the batch where no row chose it.
__global__ __launch_bounds__(256) void kmu_update_kernel(const float *__restrict__ z, const int *__restrict__ offsets,
                                                         const int *__restrict__ unit_start, const double *__restrict__ partial,
                                                         const float *__restrict__ uniforms, long long N, int K, int D, int HW,
                                                         int layout, float *__restrict__ codebook, int *__restrict__ counts) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)K * D) return;
    const int k = (int)(e / D), c = (int)(e - (long long)k * D);
    const int cnt = offsets[k + 1] - offsets[k];
    if (c == 0) counts[k] = cnt;
    if (cnt > 0) {
        const double s = segsum_key_sum(unit_start, partial, k, c, D);
        codebook[e] = (float)(s / (double)cnt);
    } else if (uniforms) {
        codebook[e] = km_at(z, km_uniform_row(uniforms[k], N), c, D, HW, layout);
    }
}

// shared argument checks: 0, or the error; N and HW on success
static int km_check(int64_t B, int D, int H, int W, int K, int flags, long long &HW, long long &N) {
    if (B < 1 || H < 1 || W < 1) return VQVAE_ERR_SHAPE;
    if (D < 1 || D > 256 || K < 1 || K > 16384 || (flags & ~VQVAE_VQ_ROWMAJOR)) return VQVAE_ERR_UNSUPPORTED;
    HW = (long long)H * W;
    if (B > INT32_MAX || HW > INT32_MAX) return VQVAE_ERR_UNSUPPORTED;
    N = (long long)B * HW;
    if (N > INT32_MAX) return VQVAE_ERR_UNSUPPORTED;
    return VQVAE_OK;
}

}  // namespace vqvae

using namespace vqvae;

extern "C" {

size_t vqvae_vq_kmeans_workspace_bytes(int64_t N, int K, int D) {
    if (N < 1 || N > INT32_MAX || K < 1 || K > 16384 || D < 1 || D > 256) return 0;
    const size_t a = km_seed_plan(N).total, b = segsum_plan(N, K, D).total;
    return a > b ? a : b;
}

int vqvae_vq_kmeans_seed_f32(const float *z_e, int64_t B, int D, int H, int W, int K, const float *uniforms, int flags,
                             float *codebook, int64_t *rows, void *workspace, size_t workspace_bytes, vqvae_stream_t stream) {
    if (!z_e || !uniforms || !codebook || !rows) return VQVAE_ERR_NULL;
    long long HW = 0, N = 0;
    const int rc = km_check(B, D, H, W, K, flags, HW, N);
    if (rc != VQVAE_OK) return rc;
    const KmSeedPlan p = km_seed_plan(N);
    if (!workspace || workspace_bytes < p.total) return VQVAE_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char *ws = static_cast<char *>(workspace);
    double *w = reinterpret_cast<double *>(ws + p.off_w);
    double *bsum = reinterpret_cast<double *>(ws + p.off_bsum);
    long long *rows_ll = reinterpret_cast<long long *>(rows);
    const int layout = (flags & VQVAE_VQ_ROWMAJOR) ? 1 : 0;
    const int layout_w = layout && (D & 3) == 0 && !(reinterpret_cast<uintptr_t>(z_e) & 15) ? 2 : layout;
    hipLaunchKernelGGL(kms_first_kernel, dim3(1), dim3(256), 0, st, z_e, uniforms, N, D, (int)HW, layout, rows_ll, codebook);
    for (int k = 1; k < K; ++k) {
        hipLaunchKernelGGL(kms_weights_kernel, dim3((unsigned)p.nb), dim3(256), 0, st, z_e, rows_ll, k, N, D, (int)HW, layout_w, w,
                           bsum);
        hipLaunchKernelGGL(kms_pick_kernel, dim3(1), dim3(256), 0, st, z_e, uniforms, w, bsum, p.nb, p.per, k, N, D, (int)HW, layout,
                           rows_ll, codebook);
    }
    return (int)hipGetLastError();
}

int vqvae_vq_kmeans_update_f32(const float *z_e, const int64_t *idx, int64_t B, int D, int H, int W, int K, const float *uniforms,
                               int flags, float *codebook, int32_t *counts, void *workspace, size_t workspace_bytes,
                               vqvae_stream_t stream) {
    if (!z_e || !idx || !codebook || !counts) return VQVAE_ERR_NULL;
    long long HW = 0, N = 0;
    const int rc = km_check(B, D, H, W, K, flags, HW, N);
    if (rc != VQVAE_OK) return rc;
    const SegsumPlan p = segsum_plan(N, K, D);
    if (!workspace || workspace_bytes < p.total) return VQVAE_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char *ws = static_cast<char *>(workspace);
    const int layout = (flags & VQVAE_VQ_ROWMAJOR) ? 1 : 0;
    const hipError_t e = launch_segsum(p, z_e, reinterpret_cast<const long long *>(idx), N, K, D, (int)HW, layout, ws, st);
    if (e != hipSuccess) return (int)e;
    const int *offsets = reinterpret_cast<const int *>(ws + p.off_offsets);
    const int *unit_start = reinterpret_cast<const int *>(ws + p.off_units);
    const double *partial = reinterpret_cast<const double *>(ws + p.off_partials);
    hipLaunchKernelGGL(kmu_update_kernel, dim3((unsigned)(((long long)K * D + 255) / 256)), dim3(256), 0, st, z_e, offsets,
                       unit_start, partial, uniforms, N, K, D, (int)HW, layout, codebook, counts);
    return (int)hipGetLastError();
}

}  // extern "C"
