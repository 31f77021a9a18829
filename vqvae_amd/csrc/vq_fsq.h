// Finite scalar quantization (vq_fsq.hip, whose header states the arithmetic): the per-row operations and the whole bodies of the
// kernels.  Plain C++ over `__device__ __forceinline__`, so that tests/host/fsq_harness.cpp compiles THIS text for the host (blockIdx /
// threadIdx, f32x4, __syncthreads, atomicAdd and <cmath> supplied by the harness) and compares it with a scalar loop under the
// sanitizers.  The LDS tile, its 16-byte / element copies and the lane-walks-its-own-row scheme are vq_cosine.h's.
#pragma once

#include "vq_cosine.h"

namespace vqvae {

constexpr int kFsqMaxLevels = 8;
constexpr int kFsqBlockRows = 64 * kL2Waves;                          // rows of one workgroup, in either layout: 256
constexpr int kFsqWeightFloatsMax = 2 * kFsqMaxLevels * 256 + kFsqMaxLevels + 256;   // W_in, b_in (8 slots), W_out, b_out at D = 256
constexpr int kFsqWeightFloatsSmall = 2 * kFsqMaxLevels * 64 + kFsqMaxLevels + 64;   // ... at D <= 64: the tile's workgroup fits a CU twice
constexpr int kFsqNchwStride = kFsqBlockRows + 1;                     // dwords between two channels of the backward's NCHW tile

struct FsqArgs {
    const float *z;                                  // forward / backward: z_e.  (N, D) rows or (B, D, HW) maps
    const float *g;                                  // backward: grad_zq, z's layout
    const float *w_in, *b_in, *w_out, *b_out;        // (d, D), (d), (D, d), (D); NULL where the kernel does not read them
    const long long *idx_in;                         // decode
    float *out;                                      // forward / decode: z_q; backward: grad_z.  May be NULL (forward, backward)
    long long *idx;                                  // forward
    int *hist;                                       // forward, may be NULL; zero on entry
    double *partials;                                // backward: one record of fsq_partial_count() doubles per workgroup, or NULL
    long long N;
    int D, HW, d, K;
    int L[kFsqMaxLevels], hw[kFsqMaxLevels], basis[kFsqMaxLevels];
    double half_l[kFsqMaxLevels], shift[kFsqMaxLevels], offset[kFsqMaxLevels];
};

// one workgroup's record of parameter-gradient partials: [W_out (D, d)] [b_out (D)] [W_in (d, D)] [b_in (d)]
__device__ __forceinline__ int fsq_partial_count(int D, int d) { return 2 * D * d + D + d; }

// ---- the weights in LDS: [W_in d D] [b_in 8] [W_out D d] [b_out D]; uniform reads are broadcasts --------------------------------
struct FsqLdsW { const float *w_in, *b_in, *w_out, *b_out; };

__device__ __forceinline__ FsqLdsW fsq_stage_weights(const FsqArgs &a, float *w) {
    const int dD = a.d * a.D;
    float *wi = w, *bi = w + dD, *wo = bi + kFsqMaxLevels, *bo = wo + dD;
    for (int i = threadIdx.x; i < dD; i += kFsqBlockRows) {
        if (a.w_in) wi[i] = a.w_in[i];
        if (a.w_out) wo[i] = a.w_out[i];
    }
    if (a.b_in)
        for (int i = threadIdx.x; i < a.d; i += kFsqBlockRows) bi[i] = a.b_in[i];
    if (a.b_out)
        for (int i = threadIdx.x; i < a.D; i += kFsqBlockRows) bo[i] = a.b_out[i];
    __syncthreads();
    return {wi, bi, wo, bo};
}

// ---- the per-row operations, one IEEE operation each -----------------------------------------------------------------------------

// channel c of a row joins the d sums `acc` through row c of a (D, d)-shaped view: w[j * sj + c * sc]
__device__ __forceinline__ void fsq_project(double *acc, const float *w, int sj, int sc, int c, int d, float x) {
#pragma unroll
    for (int j = 0; j < kFsqMaxLevels; ++j)
        if (j < d) acc[j] = acc[j] + (double)w[j * sj + c * sc] * (double)x;
}

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

// an index -> codes; outside [0, K): NaN codes, nothing read
__device__ __forceinline__ void fsq_codes_of_index(const FsqArgs &a, long long idx, float *chat) {
    const bool ok = idx >= 0 && idx < (long long)a.K;
    const unsigned u = ok ? (unsigned)idx : 0u;
#pragma unroll
    for (int j = 0; j < kFsqMaxLevels; ++j)
        if (j < a.d) {
            const int q = (int)((u / (unsigned)a.basis[j]) % (unsigned)a.L[j]) - a.hw[j];
            chat[j] = ok ? (float)((double)q / (double)a.hw[j]) : __builtin_nanf("");
        }
}

// z_q of channel c from the codes
__device__ __forceinline__ float fsq_zq(const FsqLdsW &w, int c, int d, const float *chat) {
    double s = (double)w.b_out[c];
#pragma unroll
    for (int j = 0; j < kFsqMaxLevels; ++j)
        if (j < d) s = s + (double)w.w_out[c * d + j] * (double)chat[j];
    return (float)s;
}

// grad_z of channel c from gy (fp64, unrounded)
__device__ __forceinline__ float fsq_gz(const FsqLdsW &w, int c, int D, int d, const double *gy) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < kFsqMaxLevels; ++j)
        if (j < d) s = s + (double)w.w_in[j * D + c] * gy[j];
    return (float)s;
}

__device__ __forceinline__ void fsq_gy(const FsqArgs &a, const double *gc, const double *t, double *gy) {
#pragma unroll
    for (int j = 0; j < kFsqMaxLevels; ++j)
        if (j < a.d) gy[j] = gc[j] / (double)a.hw[j] * a.half_l[j] * (1.0 - t[j] * t[j]);
}

// ---- forward and decode ----------------------------------------------------------------------------------------------------------

// NCHW maps: a lane owns one pixel; every channel is one coalesced access of the wave
template <bool DECODE>
__device__ __forceinline__ void fsq_fwd_nchw_body(const FsqArgs &a, float *wl) {
    const FsqLdsW w = fsq_stage_weights(a, wl);
    const long long row = (long long)blockIdx.x * kFsqBlockRows + threadIdx.x;
    if (row >= a.N) return;                                                   // (no barrier below)
    const int D = a.D, d = a.d;
    const long long b = row / a.HW;
    const size_t base = (size_t)b * D * a.HW + (size_t)(row - b * a.HW), stride = (size_t)a.HW;
    float chat[kFsqMaxLevels];
    if constexpr (DECODE) {
        fsq_codes_of_index(a, a.idx_in[row], chat);
    } else {
        double acc[kFsqMaxLevels], t[kFsqMaxLevels];
#pragma unroll
        for (int j = 0; j < kFsqMaxLevels; ++j) acc[j] = j < d ? (double)w.b_in[j] : 0.0;
#pragma unroll 8
        for (int c = 0; c < D; ++c) fsq_project(acc, w.w_in, D, 1, c, d, a.z[base + c * stride]);
        const long long idx = fsq_quantize(a, acc, chat, t);
        a.idx[row] = idx;
        if (a.hist) atomicAdd(a.hist + idx, 1);
        if (!a.out) return;
    }
#pragma unroll 4
    for (int c = 0; c < D; ++c) a.out[base + c * stride] = fsq_zq(w, c, d, chat);
}

// row-major rows: a wave owns 64 consecutive rows and stages 64 channels of them at a time through its LDS tile (vq_cosine.h)
template <bool DECODE, int V>
__device__ __forceinline__ void fsq_fwd_rows_body(const FsqArgs &a, float *tiles, float *wl) {
    const FsqLdsW w = fsq_stage_weights(a, wl);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float *tx = tiles + wave * kL2TileFloats, *mx = tx + lane * kL2Stride;
    const long long r0 = ((long long)blockIdx.x * kL2Waves + wave) * 64, left = a.N - r0;
    const int nr = left <= 0 ? 0 : (left < 64 ? (int)left : 64);              // a wave without rows still meets every barrier
    const int D = a.D, d = a.d, nch = (D + kL2Chunk - 1) / kL2Chunk;
    const bool mine = lane < nr;
    float chat[kFsqMaxLevels];
    if constexpr (DECODE) {
        fsq_codes_of_index(a, mine ? a.idx_in[r0 + lane] : 0, chat);
    } else {
        double acc[kFsqMaxLevels], t[kFsqMaxLevels];
#pragma unroll
        for (int j = 0; j < kFsqMaxLevels; ++j) acc[j] = j < d ? (double)w.b_in[j] : 0.0;
        for (int ch = 0; ch < nch; ++ch) {
            const int c0 = ch * kL2Chunk, cw = D - c0 < kL2Chunk ? D - c0 : kL2Chunk;
            l2n_copy<V, true>(const_cast<float *>(a.z), tx, r0, nr, D, c0, cw, lane);
            __syncthreads();
            if (mine)
                for (int c = 0; c < cw; c += 4) {
                    float xv[4];
                    l2n_load<4>(mx, (size_t)c, xv);
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (c + k < cw) fsq_project(acc, w.w_in, D, 1, c0 + c + k, d, xv[k]);
                }
            __syncthreads();
        }
        const long long idx = fsq_quantize(a, acc, chat, t);
        if (mine) {
            a.idx[r0 + lane] = idx;
            if (a.hist) atomicAdd(a.hist + idx, 1);
        }
        if (!a.out) return;                                                   // (uniform: every thread leaves)
    }
    for (int ch = 0; ch < nch; ++ch) {
        const int c0 = ch * kL2Chunk, cw = D - c0 < kL2Chunk ? D - c0 : kL2Chunk;
        if (mine)
            for (int c = 0; c < cw; c += 4) {
                float o[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] = c + k < cw ? fsq_zq(w, c0 + c + k, d, chat) : 0.0f;
                l2n_store<4>(mx, (size_t)c, o);                               // (slots past cw belong to the row's padding)
            }
        __syncthreads();
        l2n_copy<V, false>(a.out, tx, r0, nr, D, c0, cw, lane);
        __syncthreads();
    }
}

// ---- backward --------------------------------------------------------------------------------------------------------------------
// The row-local part runs as the forward does.  The parameter gradients are sums over rows: every workgroup owns the SAME 256
// consecutive rows in either layout, leaves their codes c^ (fp32) and gy (fp64) in LDS, brings 64 channels of g, then of z, into a
// tile, and thread o of the workgroup adds the 256 terms of output o one row after the other, in ascending row order, into an fp64
// partial of the workgroup's record.  fsq_param_finalize_body adds the records in ascending workgroup order.  `tile` is addressed
// as tile[row * RS + channel * CS]: the four waves' row-major tiles are one (256, 68) image (RS = 68, CS = 1); the NCHW kernel
// writes a lane's pixel at RS = 1, CS = 257, so that stores (lanes = rows) and reads (lanes = channels) both miss bank conflicts.

template <int RS, int CS>
__device__ __forceinline__ void fsq_reduce_w_out(const FsqArgs &a, const float *tile, const float *chat_l, int c0, int cw, int nrb,
                                                 double *part) {
    const int d = a.d;
    for (int o = threadIdx.x; o < cw * d + cw; o += kFsqBlockRows) {
        double s = 0.0;
        if (o < cw * d) {
            const int j = o / cw, c = o - j * cw;
#pragma unroll 8
            for (int r = 0; r < nrb; ++r) s = s + (double)tile[r * RS + c * CS] * (double)chat_l[r * kFsqMaxLevels + j];
            part[(c0 + c) * d + j] = s;
        } else {
            const int c = o - cw * d;
#pragma unroll 8
            for (int r = 0; r < nrb; ++r) s = s + (double)tile[r * RS + c * CS];
            part[a.D * d + c0 + c] = s;
        }
    }
}

template <int RS, int CS>
__device__ __forceinline__ void fsq_reduce_w_in(const FsqArgs &a, const float *tile, const double *gy_l, int c0, int cw, int nrb,
                                                double *part) {
    const int d = a.d, D = a.D;
    double *p_w = part + D * d + D, *p_b = p_w + d * D;
    for (int o = threadIdx.x; o < cw * d + (c0 == 0 ? d : 0); o += kFsqBlockRows) {
        double s = 0.0;
        if (o < cw * d) {
            const int j = o / cw, c = o - j * cw;
#pragma unroll 8
            for (int r = 0; r < nrb; ++r) s = s + gy_l[r * kFsqMaxLevels + j] * (double)tile[r * RS + c * CS];
            p_w[j * D + c0 + c] = s;
        } else {
            const int j = o - cw * d;
#pragma unroll 8
            for (int r = 0; r < nrb; ++r) s = s + gy_l[r * kFsqMaxLevels + j];
            p_b[j] = s;
        }
    }
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

template <bool PARAMS>
__device__ __forceinline__ void fsq_bwd_nchw_body(const FsqArgs &a, float *tile, float *wl, float *chat_l, double *gy_l) {
    const FsqLdsW w = fsq_stage_weights(a, wl);
    const long long row0 = (long long)blockIdx.x * kFsqBlockRows, row = row0 + threadIdx.x, left = a.N - row0;
    const int nrb = left < kFsqBlockRows ? (int)left : kFsqBlockRows;
    const bool mine = row < a.N;
    const int D = a.D, d = a.d;
    const long long b = mine ? row / a.HW : 0;
    const size_t base = (size_t)b * D * a.HW + (size_t)(mine ? row - b * a.HW : 0), stride = (size_t)a.HW;
    double acc_y[kFsqMaxLevels], acc_g[kFsqMaxLevels], gy[kFsqMaxLevels];
#pragma unroll
    for (int j = 0; j < kFsqMaxLevels; ++j) {
        acc_y[j] = j < d ? (double)w.b_in[j] : 0.0;
        acc_g[j] = 0.0;
    }
    if (mine) {
#pragma unroll 4
        for (int c = 0; c < D; ++c) {
            fsq_project(acc_y, w.w_in, D, 1, c, d, a.z[base + c * stride]);
            fsq_project(acc_g, w.w_out, 1, d, c, d, a.g[base + c * stride]);
        }
    }
    fsq_bwd_row(a, acc_y, acc_g, PARAMS, mine, chat_l, gy_l, gy);
    if (a.out && mine) {
#pragma unroll 4
        for (int c = 0; c < D; ++c) a.out[base + c * stride] = fsq_gz(w, c, D, d, gy);
    }
    if constexpr (PARAMS) {
        double *part = a.partials + (size_t)blockIdx.x * fsq_partial_count(D, d);
        for (int c0 = 0; c0 < D; c0 += kL2Chunk) {
            const int cw = D - c0 < kL2Chunk ? D - c0 : kL2Chunk;
            __syncthreads();                                                  // chat_l / gy_l written; the tile's last readers are done
            if (mine)
                for (int c = 0; c < cw; ++c) tile[c * kFsqNchwStride + threadIdx.x] = a.g[base + (c0 + c) * stride];
            __syncthreads();
            fsq_reduce_w_out<1, kFsqNchwStride>(a, tile, chat_l, c0, cw, nrb, part);
            __syncthreads();
            if (mine)
                for (int c = 0; c < cw; ++c) tile[c * kFsqNchwStride + threadIdx.x] = a.z[base + (c0 + c) * stride];
            __syncthreads();
            fsq_reduce_w_in<1, kFsqNchwStride>(a, tile, gy_l, c0, cw, nrb, part);
        }
    }
}

template <bool PARAMS, int V>
__device__ __forceinline__ void fsq_bwd_rows_body(const FsqArgs &a, float *tiles, float *wl, float *chat_l, double *gy_l) {
    const FsqLdsW w = fsq_stage_weights(a, wl);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float *tx = tiles + wave * kL2TileFloats, *mx = tx + lane * kL2Stride;
    const long long row0 = (long long)blockIdx.x * kFsqBlockRows, r0 = row0 + wave * 64, left = a.N - r0, leftb = a.N - row0;
    const int nr = left <= 0 ? 0 : (left < 64 ? (int)left : 64);
    const int nrb = leftb < kFsqBlockRows ? (int)leftb : kFsqBlockRows;
    const int D = a.D, d = a.d, nch = (D + kL2Chunk - 1) / kL2Chunk;
    const bool mine = lane < nr;
    double acc_y[kFsqMaxLevels], acc_g[kFsqMaxLevels], gy[kFsqMaxLevels];
#pragma unroll
    for (int j = 0; j < kFsqMaxLevels; ++j) {
        acc_y[j] = j < d ? (double)w.b_in[j] : 0.0;
        acc_g[j] = 0.0;
    }
    // the lane walks the chunk of its row that lies in the tile: into the y sums (G = false) or the gc sums
    auto walk = [&](bool G, int c0, int cw) {
        if (mine)
            for (int c = 0; c < cw; c += 4) {
                float xv[4];
                l2n_load<4>(mx, (size_t)c, xv);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (c + k < cw) {
                        if (G) fsq_project(acc_g, w.w_out, 1, d, c0 + c + k, d, xv[k]);
                        else fsq_project(acc_y, w.w_in, D, 1, c0 + c + k, d, xv[k]);
                    }
            }
    };
    for (int ch = 0; ch < nch; ++ch) {
        const int c0 = ch * kL2Chunk, cw = D - c0 < kL2Chunk ? D - c0 : kL2Chunk;
        l2n_copy<V, true>(const_cast<float *>(a.z), tx, r0, nr, D, c0, cw, lane);
        __syncthreads();
        walk(false, c0, cw);
        __syncthreads();
        l2n_copy<V, true>(const_cast<float *>(a.g), tx, r0, nr, D, c0, cw, lane);
        __syncthreads();
        walk(true, c0, cw);
        __syncthreads();
    }
    fsq_bwd_row(a, acc_y, acc_g, PARAMS, mine, chat_l, gy_l, gy);
    double *part = PARAMS ? a.partials + (size_t)blockIdx.x * fsq_partial_count(D, d) : nullptr;
    for (int ch = 0; ch < nch; ++ch) {
        const int c0 = ch * kL2Chunk, cw = D - c0 < kL2Chunk ? D - c0 : kL2Chunk;
        if constexpr (PARAMS) {
            l2n_copy<V, true>(const_cast<float *>(a.g), tx, r0, nr, D, c0, cw, lane);
            __syncthreads();                                                  // (and chat_l / gy_l are written)
            fsq_reduce_w_out<kL2Stride, 1>(a, tiles, chat_l, c0, cw, nrb, part);
            __syncthreads();
            l2n_copy<V, true>(const_cast<float *>(a.z), tx, r0, nr, D, c0, cw, lane);
            __syncthreads();
            fsq_reduce_w_in<kL2Stride, 1>(a, tiles, gy_l, c0, cw, nrb, part);
            __syncthreads();
        }
        if (a.out) {
            if (mine)
                for (int c = 0; c < cw; c += 4) {
                    float o[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) o[k] = c + k < cw ? fsq_gz(w, c0 + c + k, D, d, gy) : 0.0f;
                    l2n_store<4>(mx, (size_t)c, o);
                }
            __syncthreads();
            l2n_copy<V, false>(a.out, tx, r0, nr, D, c0, cw, lane);
            __syncthreads();
        }
    }
}

// the second launch: output o = the workgroups' partials of o in ascending workgroup order, rounded once.  A NULL gradient is skipped.
__device__ __forceinline__ void fsq_param_finalize_body(const double *partials, long long nblocks, int D, int d, float *g_w_in,
                                                        float *g_b_in, float *g_w_out, float *g_b_out) {
    const int P = fsq_partial_count(D, d), o = blockIdx.x * kFsqBlockRows + threadIdx.x;
    if (o >= P) return;
    float *dst;
    int at;
    if (o < D * d) { dst = g_w_out; at = o; }
    else if (o < D * d + D) { dst = g_b_out; at = o - D * d; }
    else if (o < 2 * D * d + D) { dst = g_w_in; at = o - D * d - D; }
    else { dst = g_b_in; at = o - 2 * D * d - D; }
    if (!dst) return;
    double s = 0.0;
#pragma unroll 8
    for (long long b = 0; b < nblocks; ++b) s = s + partials[(size_t)b * P + o];
    dst[at] = (float)s;
}

#ifdef __HIPCC__
// vq_fsq.hip: pick the access width (alignment, D % 4) and the weight capacity, and launch
void launch_fsq_forward(const FsqArgs &a, bool rowmajor, hipStream_t st);
void launch_fsq_decode(const FsqArgs &a, bool rowmajor, hipStream_t st);
void launch_fsq_backward(const FsqArgs &a, bool rowmajor, hipStream_t st);
#endif

}  // namespace vqvae
