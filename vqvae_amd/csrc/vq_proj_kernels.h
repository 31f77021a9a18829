// The kernels and launches over vq_proj.h's bodies, for a policy P (vq_fsq.hip: Fsq, vq_lfq.hip: Lfq).  Every kernel is an
// instantiation of its own per quantizer; its LDS arrays are sized by P::kMaxD and the weight capacity WF.
#pragma once

#include "common.h"
#include "vq_proj.h"

namespace vqvae {

template <typename P, bool DECODE, int WF>
__global__ __launch_bounds__(kProjBlockRows) void proj_fwd_nchw_kernel(typename P::Args a) {
    __shared__ float wl[WF];
    proj_fwd_nchw_body<P, DECODE>(a, wl);
}

template <typename P, bool DECODE, int V, int WF>
__global__ __launch_bounds__(kProjBlockRows) void proj_fwd_rows_kernel(typename P::Args a) {
    __shared__ __attribute__((aligned(16))) float tiles[kL2Waves * kL2TileFloats];
    __shared__ float wl[WF];
    proj_fwd_rows_body<P, DECODE, V>(a, tiles, wl);
}

template <typename P, bool PARAMS, int WF>
__global__ __launch_bounds__(kProjBlockRows) void proj_bwd_nchw_kernel(typename P::Args a) {
    __shared__ float tile[PARAMS ? kL2Chunk * kProjNchwStride : 1];
    __shared__ float wl[WF];
    __shared__ float code_l[PARAMS ? kProjBlockRows * P::kMaxD : 1];
    __shared__ double gy_l[PARAMS ? kProjBlockRows * P::kMaxD : 1];
    P::template bwd_nchw_body<PARAMS>(a, tile, wl, code_l, gy_l);
}

template <typename P, bool PARAMS, int V, int WF>
__global__ __launch_bounds__(kProjBlockRows) void proj_bwd_rows_kernel(typename P::Args a) {
    __shared__ __attribute__((aligned(16))) float tiles[kL2Waves * kL2TileFloats];
    __shared__ float wl[WF];
    __shared__ float code_l[PARAMS ? kProjBlockRows * P::kMaxD : 1];
    __shared__ double gy_l[PARAMS ? kProjBlockRows * P::kMaxD : 1];
    P::template bwd_rows_body<PARAMS, V>(a, tiles, wl, code_l, gy_l);
}

template <typename P>
__global__ __launch_bounds__(kProjBlockRows) void proj_param_finalize_kernel(const double *partials, long long nblocks, int D, int d,
                                                                            float *g_w_in, float *g_b_in, float *g_w_out, float *g_b_out) {
    proj_param_finalize_body(partials, nblocks, D, d, g_w_in, g_b_in, g_w_out, g_b_out);
}

// perplexity = exp(-sum_k p_k log(p_k + 1e-10)), p_k = hist_k / N, in fp64: thread t adds k = t, t + 256, .. in ascending order, the
// 256 sums meet in the fixed tree, one rounding to fp32
template <typename P>
__global__ __launch_bounds__(256) void proj_perplexity_kernel(const int *hist, int K, long long N, float *perplexity) {
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

// ---- the launches: pick the access width (16-byte aligned pointers, D % 4 == 0) and the weight capacity ----------------------------

inline unsigned proj_grid(long long N) { return (unsigned)((N + kProjBlockRows - 1) / kProjBlockRows); }
inline bool proj_wide(const ProjArgs &a, const void *p0, const void *p1, const void *p2 = nullptr) {
    const uintptr_t bits = reinterpret_cast<uintptr_t>(p0) | reinterpret_cast<uintptr_t>(p1) | reinterpret_cast<uintptr_t>(p2);
    return (a.D & 3) == 0 && !(bits & 15);
}
// bytes of the backward's partials: one record per block of rows
inline size_t proj_partial_bytes(long long N, int D, int d) { return (size_t)proj_grid(N) * (size_t)proj_partial_count(D, d) * sizeof(double); }

template <typename P, bool DECODE>
void proj_launch_fwd(const typename P::Args &a, bool rowmajor, hipStream_t st) {
    const dim3 grid(proj_grid(a.N)), block(kProjBlockRows);
    constexpr int S = proj_weight_floats_small(P::kMaxD), M = proj_weight_floats_max(P::kMaxD);
    const bool small = a.D <= kProjSmallD;
    if (!rowmajor) {
        if (small) hipLaunchKernelGGL((proj_fwd_nchw_kernel<P, DECODE, S>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((proj_fwd_nchw_kernel<P, DECODE, M>), grid, block, 0, st, a);
        return;
    }
    const bool wide = proj_wide(a, a.z, a.out);
    if (wide && small) hipLaunchKernelGGL((proj_fwd_rows_kernel<P, DECODE, 4, S>), grid, block, 0, st, a);
    else if (wide) hipLaunchKernelGGL((proj_fwd_rows_kernel<P, DECODE, 4, M>), grid, block, 0, st, a);
    else if (small) hipLaunchKernelGGL((proj_fwd_rows_kernel<P, DECODE, 1, S>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((proj_fwd_rows_kernel<P, DECODE, 1, M>), grid, block, 0, st, a);
}

template <typename P, bool PARAMS>
void proj_launch_bwd_rows(const typename P::Args &a, bool rowmajor, hipStream_t st) {
    const dim3 grid(proj_grid(a.N)), block(kProjBlockRows);
    constexpr int S = proj_weight_floats_small(P::kMaxD), M = proj_weight_floats_max(P::kMaxD);
    const bool small = a.D <= kProjSmallD;
    if (!rowmajor) {
        if (small) hipLaunchKernelGGL((proj_bwd_nchw_kernel<P, PARAMS, S>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((proj_bwd_nchw_kernel<P, PARAMS, M>), grid, block, 0, st, a);
        return;
    }
    const bool wide = proj_wide(a, a.z, a.g, a.out);
    if (wide && small) hipLaunchKernelGGL((proj_bwd_rows_kernel<P, PARAMS, 4, S>), grid, block, 0, st, a);
    else if (wide) hipLaunchKernelGGL((proj_bwd_rows_kernel<P, PARAMS, 4, M>), grid, block, 0, st, a);
    else if (small) hipLaunchKernelGGL((proj_bwd_rows_kernel<P, PARAMS, 1, S>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((proj_bwd_rows_kernel<P, PARAMS, 1, M>), grid, block, 0, st, a);
}

// the row kernel of the backward and, with a.partials, the second launch that adds the workgroups' records into the four gradients
template <typename P>
void proj_launch_bwd(const typename P::Args &a, bool rowmajor, float *g_w_in, float *g_b_in, float *g_w_out, float *g_b_out,
                     hipStream_t st) {
    if (!a.partials) {
        proj_launch_bwd_rows<P, false>(a, rowmajor, st);
        return;
    }
    proj_launch_bwd_rows<P, true>(a, rowmajor, st);
    const int n = proj_partial_count(a.D, a.d);
    hipLaunchKernelGGL(proj_param_finalize_kernel<P>, dim3((unsigned)((n + kProjBlockRows - 1) / kProjBlockRows)), dim3(kProjBlockRows), 0,
                       st, a.partials, (long long)proj_grid(a.N), a.D, a.d, g_w_in, g_b_in, g_w_out, g_b_out);
}

}  // namespace vqvae
