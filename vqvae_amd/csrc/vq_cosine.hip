// l2-normalisation of rows and its backward (gfx950): what a cosine-similarity codebook (ViT-VQGAN, arXiv 2110.04627 section 3.2;
// vector-quantize-pytorch's use_cosine_sim) puts in front of the quantizer.  Encoder outputs and codes are divided by their l2 norm,
// and the quantizer -- unchanged, bit for bit -- then runs on the unit rows.
//   vqvae_l2norm_forward_f32    x -> y = x / max(||x||, eps), denom = max(||x||, eps)        (torch.nn.functional.normalize)
//   vqvae_l2norm_backward_f32   (y, denom, grad_y) -> grad_x                                  (its autograd)
// Rows and layouts are vqvae_vq_forward_f32's: N = B H W rows of D channels, (B, D, H, W) maps, or (N, D) rows with
// VQVAE_VQ_ROWMAJOR; a codebook is the row-major case B = K, H = W = 1.  1 <= D <= 256, N < 2^31.
//
// THE ARITHMETIC IS THE CONTRACT (tests/vq_cosine_ref.py restates it on the CPU; the library is compiled with -ffp-contract=off, so
// every operation written below is one IEEE operation).  Forward, per row:
//
//   s = 0.0; for c = 0 .. D-1 in ascending order: s = s + double(x_c) * double(x_c)      (the product is exact in fp64)
//   n = sqrt(s) in fp64;  d = float(n)
//   d = (d < eps) ? eps : d             (written as that comparison: a NaN norm stays NaN, as torch.clamp_min keeps it)
//   y_c = x_c / d                       (one fp32 division);  denom = d
//
// Backward, per row, from the forward's y and denom:
//
//   t = 0.0; for c ascending: t = t + double(y_c) * double(g_c)
//   d >  eps:  grad_x_c = float((double(g_c) - double(y_c) * t) / double(d))             (three fp64 operations, one rounding)
//   otherwise: grad_x_c = float(double(g_c) / double(eps))     (the clamp was active: what autograd gives clamp_min there; a NaN
//                                                               denom also lands here)
//
// A NaN or Inf stays in its own row.  The fp32 division is the correctly rounded one (hipcc's default; build.FLAGS sets nothing that
// relaxes it: no -ffast-math, no -fno-hip-fp32-correctly-rounded-divide-sqrt) and the device's fp64 sqrt and division are correctly
// rounded (vq_rotation.hip and optim.hip rely on the same), so the results have the restatement's bits.
//
// One lane owns one row's sum in either layout and adds in ascending channel order: the same bits in row-major and NCHW, on the
// 16-byte and the element-by-element access paths, and from run to run.  No workspace, no allocation, no host sync, no atomics; one
// launch on the caller's stream, capturable.  The mappings are described in vq_cosine.h next to their bodies: NCHW maps one pixel
// (or four, with 16-byte accesses) per lane, row-major rows staged through LDS a wave's 64 rows at a time.  Every thread has one
// item and the grid covers all rows: no capped grid, no stride loop.
#include "common.h"
#include "vq_cosine.h"

namespace vqvae {

template <bool BWD, int DREG, int V>
__global__ __launch_bounds__(256) void vq_l2norm_nchw_kernel(L2nArgs a) { l2n_nchw_body<BWD, DREG, V>(a); }

template <bool BWD, int V>
__global__ __launch_bounds__(64 * kL2Waves) void vq_l2norm_rows_kernel(L2nArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[kL2Waves * (BWD ? 2 : 1) * kL2TileFloats];
    l2n_rows_body<BWD, V>(a, lds);
}

template <bool BWD>
static void l2n_launch(const L2nArgs &a, bool rowmajor, hipStream_t st) {
    uintptr_t bits = reinterpret_cast<uintptr_t>(a.x) | reinterpret_cast<uintptr_t>(a.out);
    if (BWD) bits |= reinterpret_cast<uintptr_t>(a.g);
    const dim3 block(256);
    if (rowmajor) {
        const dim3 grid((unsigned)((a.N + 64 * kL2Waves - 1) / (64 * kL2Waves)));
        if ((a.D & 3) == 0 && !(bits & 15)) hipLaunchKernelGGL((vq_l2norm_rows_kernel<BWD, 4>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((vq_l2norm_rows_kernel<BWD, 1>), grid, block, 0, st, a);
        return;
    }
    bits |= reinterpret_cast<uintptr_t>(BWD ? a.denom_in : a.denom_out);      // a lane's four pixels share one access of denom too
    // Four pixels per lane wherever the maps allow 16-byte accesses -- except the forward at 16 < D <= 64, where one pixel per lane
    // with the row in registers reads x once and runs four times as many waves.  The backward's register form at that width holds
    // y and grad_y (2 waves per SIMD) and is the slower of its two.  Both choices were measured: profiles/vq_cosine_notes.txt.
    if ((a.HW & 3) == 0 && !(bits & 15) && (BWD || a.D <= 16 || a.D > 64)) {
        const dim3 grid((unsigned)((a.N / 4 + 255) / 256));
        if (a.D <= 16) hipLaunchKernelGGL((vq_l2norm_nchw_kernel<BWD, 16, 4>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((vq_l2norm_nchw_kernel<BWD, 0, 4>), grid, block, 0, st, a);
    } else {
        const dim3 grid((unsigned)((a.N + 255) / 256));
        if (a.D <= 16) hipLaunchKernelGGL((vq_l2norm_nchw_kernel<BWD, 16, 1>), grid, block, 0, st, a);
        else if (a.D <= 64) hipLaunchKernelGGL((vq_l2norm_nchw_kernel<BWD, 64, 1>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((vq_l2norm_nchw_kernel<BWD, 0, 1>), grid, block, 0, st, a);
    }
}

void launch_l2norm(const L2nArgs &a, bool backward, bool rowmajor, hipStream_t st) {
    if (backward) l2n_launch<true>(a, rowmajor, st);
    else l2n_launch<false>(a, rowmajor, st);
}

static bool l2n_overlap(const float *p, const float *q, long long elems) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q), n = (uintptr_t)elems * 4;
    return a < b + n && b < a + n;
}

// shapes and pointers of both entries: the header's codes, before any launch
static int l2n_check(int64_t B, int D, int H, int W, long long &HW, long long &N) {
    if (B < 1 || H < 1 || W < 1) return VQVAE_ERR_SHAPE;
    if (D < 1 || D > 256) return VQVAE_ERR_UNSUPPORTED;
    if ((long long)H * W > INT32_MAX) return VQVAE_ERR_UNSUPPORTED;
    HW = (long long)H * W;
    if (B > INT32_MAX / HW) return VQVAE_ERR_UNSUPPORTED;
    N = B * HW;
    return VQVAE_OK;
}

}  // namespace vqvae

using namespace vqvae;

extern "C" {

int vqvae_l2norm_forward_f32(const float *x, int64_t B, int D, int H, int W, float eps, int flags, float *y, float *denom,
                             vqvae_stream_t stream) {
    if (!x || !y || !denom) return VQVAE_ERR_NULL;
    long long HW = 0, N = 0;
    const int rc = l2n_check(B, D, H, W, HW, N);
    if (rc != VQVAE_OK) return rc;
    if ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(denom)) & 3)
        return VQVAE_ERR_UNSUPPORTED;
    if (l2n_overlap(x, y, N * D)) return VQVAE_ERR_UNSUPPORTED;       // the second pass over wide rows reads x again
    L2nArgs a = {};
    a.x = x; a.out = y; a.denom_out = denom; a.N = N; a.D = D; a.HW = (int)HW; a.eps = eps;
    launch_l2norm(a, false, (flags & VQVAE_VQ_ROWMAJOR) != 0, static_cast<hipStream_t>(stream));
    return (int)hipGetLastError();
}

int vqvae_l2norm_backward_f32(const float *y, const float *denom, const float *grad_y, int64_t B, int D, int H, int W, float eps,
                              int flags, float *grad_x, vqvae_stream_t stream) {
    if (!y || !denom || !grad_y || !grad_x) return VQVAE_ERR_NULL;
    long long HW = 0, N = 0;
    const int rc = l2n_check(B, D, H, W, HW, N);
    if (rc != VQVAE_OK) return rc;
    if ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(denom) | reinterpret_cast<uintptr_t>(grad_y) |
         reinterpret_cast<uintptr_t>(grad_x)) & 3)
        return VQVAE_ERR_UNSUPPORTED;
    if (l2n_overlap(y, grad_x, N * D) || l2n_overlap(grad_y, grad_x, N * D)) return VQVAE_ERR_UNSUPPORTED;
    L2nArgs a = {};
    a.x = y; a.g = grad_y; a.denom_in = denom; a.out = grad_x; a.N = N; a.D = D; a.HW = (int)HW; a.eps = eps;
    launch_l2norm(a, true, (flags & VQVAE_VQ_ROWMAJOR) != 0, static_cast<hipStream_t>(stream));
    return (int)hipGetLastError();
}

}  // extern "C"
