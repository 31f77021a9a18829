// Finite scalar quantization (vq_fsq.hip, whose header states the arithmetic): what FSQ does with the finished sums of a row -- the
// tanh bound and the rounding -- and its backward bodies, which re-project z and g together.  The kernel skeleton around them (the
// weights in LDS, the projections, the forward / decode bodies, the parameter-gradient reductions and their second launch) is
// vq_proj.h's, which takes `Fsq` below as its policy.  Plain C++ over `__device__ __forceinline__`, so that tests/host/fsq_harness.cpp
// compiles THIS text for the host and compares it with a scalar loop under the sanitizers.
#pragma once

#include "vq_proj.h"

namespace vqvae {

constexpr int kFsqMaxLevels = 8;

struct FsqArgs : ProjArgs {
    int L[kFsqMaxLevels], hw[kFsqMaxLevels], basis[kFsqMaxLevels];
    double half_l[kFsqMaxLevels], shift[kFsqMaxLevels], offset[kFsqMaxLevels];
};

// ---- the per-row operations, one IEEE operation each -----------------------------------------------------------------------------

// FSQ.bound and the rounding of channel j: t = tanh(y + shift), q = rint(t half_l - offset)
__device__ __forceinline__ void fsq_bound_round(const FsqArgs &a, int j, float y, double &t, double &q) {
    t = tanh((double)y + a.shift[j]);
    const double b = t * a.half_l[j] - a.offset[j];
    q = rint(b);
}

// acc (the d sums, b_in included) -> codes c^ (fp32), the row's index, and t (for the backward).  A non-finite y_j: digit 0, c^_j NaN.
__device__ __forceinline__ long long fsq_quantize(const FsqArgs &a, const double *acc, float *chat, double *t) {
    long long idx = 0;
#pragma unroll
    for (int j = 0; j < kFsqMaxLevels; ++j)
        if (j < a.d) {
            const float y = (float)acc[j];
            double q;
            fsq_bound_round(a, j, y, t[j], q);
            const bool fin = (y - y) == 0.0f;
            chat[j] = fin ? (float)(q / (double)a.hw[j]) : __builtin_nanf("");
            idx += fin ? (long long)(((int)q + a.hw[j]) * a.basis[j]) : 0;
        }
    return idx;
}

__device__ __forceinline__ void fsq_gy(const FsqArgs &a, const double *gc, const double *t, double *gy) {
#pragma unroll
    for (int j = 0; j < kFsqMaxLevels; ++j)
        if (j < a.d) gy[j] = gc[j] / (double)a.hw[j] * a.half_l[j] * (1.0 - t[j] * t[j]);
}

// what both backward bodies do with the finished sums of a row: codes and gy, to registers and (PARAMS) to the workgroup's LDS
__device__ __forceinline__ void fsq_bwd_row(const FsqArgs &a, const double *acc_y, const double *acc_g, bool params, bool mine,
                                            float *chat_l, double *gy_l, double *gy) {
    float chat[kFsqMaxLevels];
    double t[kFsqMaxLevels];
    fsq_quantize(a, acc_y, chat, t);
    fsq_gy(a, acc_g, t, gy);
    if (params && mine) {
#pragma unroll
        for (int j = 0; j < kFsqMaxLevels; ++j)
            if (j < a.d) {
                chat_l[threadIdx.x * kFsqMaxLevels + j] = chat[j];
                gy_l[threadIdx.x * kFsqMaxLevels + j] = gy[j];
            }
    }
}

// ---- vq_proj.h's policy ------------------------------------------------------------------------------------------------------------
struct Fsq {
    using Args = FsqArgs;
    static constexpr int kMaxD = kFsqMaxLevels, kNchwUnroll = 8;
    using Side = double[kFsqMaxLevels];              // t

    // an index -> codes; outside [0, K): NaN codes, nothing read
    static __device__ __forceinline__ void codes_of_index(const FsqArgs &a, long long idx, float *chat) {
        const bool ok = idx >= 0 && idx < (long long)a.K;
        const unsigned u = ok ? (unsigned)idx : 0u;
#pragma unroll
        for (int j = 0; j < kFsqMaxLevels; ++j)
            if (j < a.d) {
                const int q = (int)((u / (unsigned)a.basis[j]) % (unsigned)a.L[j]) - a.hw[j];
                chat[j] = ok ? (float)((double)q / (double)a.hw[j]) : __builtin_nanf("");
            }
    }

    static __device__ __forceinline__ void quantize_row(const FsqArgs &a, const double *acc, long long row, bool mine, float *chat,
                                                        double *t) {
        const long long idx = fsq_quantize(a, acc, chat, t);
        if (mine) {
            a.idx[row] = idx;
            if (a.hist) atomicAdd(a.hist + idx, 1);
        }
    }

    // the backward: y and gc of the row in one pass over z and g, as the forward projects; then grad_z and the workgroup's record
    template <bool PARAMS>
    static __device__ __forceinline__ void bwd_nchw_body(const FsqArgs &a, float *tile, float *wl, float *chat_l, double *gy_l) {
        const ProjLdsW w = proj_stage_weights<kMaxD>(a, wl);
        const ProjNchwPos p = proj_nchw_pos(a);
        const int D = a.D, d = a.d;
        double acc_y[kMaxD], acc_g[kMaxD], gy[kMaxD];
#pragma unroll
        for (int j = 0; j < kMaxD; ++j) {
            acc_y[j] = j < d ? (double)w.b_in[j] : 0.0;
            acc_g[j] = 0.0;
        }
        if (p.mine) {
#pragma unroll 4
            for (int c = 0; c < D; ++c) {
                proj_project<kMaxD>(acc_y, w.w_in, D, 1, c, d, a.z[p.base + c * p.stride]);
                proj_project<kMaxD>(acc_g, w.w_out, 1, d, c, d, a.g[p.base + c * p.stride]);
            }
        }
        fsq_bwd_row(a, acc_y, acc_g, PARAMS, p.mine, chat_l, gy_l, gy);
        if (a.out && p.mine) {
#pragma unroll 4
            for (int c = 0; c < D; ++c) a.out[p.base + c * p.stride] = proj_gz<kMaxD>(w, c, D, d, gy);
        }
        if constexpr (PARAMS) {
            double *part = a.partials + (size_t)blockIdx.x * proj_partial_count(D, d);
            for (int c0 = 0; c0 < D; c0 += kL2Chunk) {
                const int cw = D - c0 < kL2Chunk ? D - c0 : kL2Chunk;
                __syncthreads();                                              // chat_l / gy_l written; the tile's last readers are done
                if (p.mine)
                    for (int c = 0; c < cw; ++c) tile[c * kProjNchwStride + threadIdx.x] = a.g[p.base + (c0 + c) * p.stride];
                __syncthreads();
                proj_reduce_w_out<kMaxD, 1, kProjNchwStride, false>(a, tile, chat_l, c0, cw, p.nrb, part);
                __syncthreads();
                if (p.mine)
                    for (int c = 0; c < cw; ++c) tile[c * kProjNchwStride + threadIdx.x] = a.z[p.base + (c0 + c) * p.stride];
                __syncthreads();
                proj_reduce_w_in<kMaxD, 1, kProjNchwStride>(a, tile, gy_l, c0, cw, p.nrb, part);
            }
        }
    }

    template <bool PARAMS, int V>
    static __device__ __forceinline__ void bwd_rows_body(const FsqArgs &a, float *tiles, float *wl, float *chat_l, double *gy_l) {
        const ProjLdsW w = proj_stage_weights<kMaxD>(a, wl);
        const ProjRowsPos p = proj_rows_pos(a, tiles);
        const int D = a.D, d = a.d, nch = (D + kL2Chunk - 1) / kL2Chunk;
        double acc_y[kMaxD], acc_g[kMaxD], gy[kMaxD];
#pragma unroll
        for (int j = 0; j < kMaxD; ++j) {
            acc_y[j] = j < d ? (double)w.b_in[j] : 0.0;
            acc_g[j] = 0.0;
        }
        // the lane walks the chunk of its row that lies in the tile: into the y sums (G = false) or the gc sums
        auto walk = [&](bool G, int c0, int cw) {
            if (p.mine)
                for (int c = 0; c < cw; c += 4) {
                    float xv[4];
                    l2n_load<4>(p.mx, (size_t)c, xv);
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (c + k < cw) {
                            if (G) proj_project<kMaxD>(acc_g, w.w_out, 1, d, c0 + c + k, d, xv[k]);
                            else proj_project<kMaxD>(acc_y, w.w_in, D, 1, c0 + c + k, d, xv[k]);
                        }
                }
        };
        for (int ch = 0; ch < nch; ++ch) {
            const int c0 = ch * kL2Chunk, cw = D - c0 < kL2Chunk ? D - c0 : kL2Chunk;
            l2n_copy<V, true>(const_cast<float *>(a.z), p.tx, p.r0, p.nr, D, c0, cw, p.lane);
            __syncthreads();
            walk(false, c0, cw);
            __syncthreads();
            l2n_copy<V, true>(const_cast<float *>(a.g), p.tx, p.r0, p.nr, D, c0, cw, p.lane);
            __syncthreads();
            walk(true, c0, cw);
            __syncthreads();
        }
        fsq_bwd_row(a, acc_y, acc_g, PARAMS, p.mine, chat_l, gy_l, gy);
        double *part = PARAMS ? a.partials + (size_t)blockIdx.x * proj_partial_count(D, d) : nullptr;
        for (int ch = 0; ch < nch; ++ch) {
            const int c0 = ch * kL2Chunk, cw = D - c0 < kL2Chunk ? D - c0 : kL2Chunk;
            if constexpr (PARAMS) {
                l2n_copy<V, true>(const_cast<float *>(a.g), p.tx, p.r0, p.nr, D, c0, cw, p.lane);
                __syncthreads();                                              // (and chat_l / gy_l are written)
                proj_reduce_w_out<kMaxD, kL2Stride, 1, false>(a, tiles, chat_l, c0, cw, p.nrb, part);
                __syncthreads();
                l2n_copy<V, true>(const_cast<float *>(a.z), p.tx, p.r0, p.nr, D, c0, cw, p.lane);
                __syncthreads();
                proj_reduce_w_in<kMaxD, kL2Stride, 1>(a, tiles, gy_l, c0, cw, p.nrb, part);
                __syncthreads();
            }
            if (a.out) {
                if (p.mine)
                    for (int c = 0; c < cw; c += 4) {
                        float o[4];
#pragma unroll
                        for (int k = 0; k < 4; ++k) o[k] = c + k < cw ? proj_gz<kMaxD>(w, c0 + c + k, D, d, gy) : 0.0f;
                        l2n_store<4>(p.mx, (size_t)c, o);
                    }
                __syncthreads();
                l2n_copy<V, false>(a.out, p.tx, p.r0, p.nr, D, c0, cw, p.lane);
                __syncthreads();
            }
        }
    }
};

}  // namespace vqvae
