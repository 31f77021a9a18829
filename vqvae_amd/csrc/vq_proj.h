// The kernel skeleton of the quantizers that project a latent row to d channels, quantize the d sums and project the codes back:
// finite scalar quantization (vq_fsq.h, MAXD = 8) and lookup-free quantization (vq_lfq.h, MAXD = 16).  Everything here is the same
// text for both: the arguments they share, the weights in LDS, the per-row projections, the whole forward / decode bodies, the
// parameter-gradient reductions, where a thread stands in the backward, and the second launch of the parameter gradients.  What a
// quantizer does with the finished sums of a row comes in as a small static policy type P:
//     P::Args                          the kernel's argument struct, a ProjArgs
//     P::kMaxD, P::kNchwUnroll         the code width the registers and LDS are sized for; the unroll factor of the NCHW projection loop
//     P::codes_of_index(a, idx, code)  an index -> codes; outside [0, K): NaN codes, nothing read
//     P::quantize_row(a, acc, row, mine, code, side)
//                                      the d sums (b_in included) -> codes; where `mine`, the row's index, histogram count and
//                                      whatever else the quantizer keeps of the row are stored.  Every lane runs it: only stores are masked
//     P::Side                          an array type for what quantize_row computes beside the codes (FSQ's t, LFQ's y).  The bodies
//                                      declare it next to the sums: declared inside quantize_row, LFQ's NCHW forward took 91 VGPRs for 78
//     P::bwd_nchw_body, P::bwd_rows_body   the backward bodies (vq_proj_kernels.h launches them).  They are the quantizer's own from head
//                                      to tail and share the reductions below: with the tails (grad_z write-out, the chunk loop around
//                                      the reductions) as functions of this file the compiler made other, slower backward kernels
// Plain C++ over `__device__ __forceinline__`, so that tests/host/fsq_harness.cpp and lfq_harness.cpp compile THIS text for the host
// (tests/host/device_shim.h supplies blockIdx / threadIdx, f32x4, __syncthreads and atomicAdd).  The LDS tile, its 16-byte / element
// copies and the lane-walks-its-own-row scheme are vq_cosine.h's.
#pragma once

#include "vq_cosine.h"

namespace vqvae {

constexpr int kProjBlockRows = 64 * kL2Waves;                         // rows of one workgroup, in either layout: 256
constexpr int kProjNchwStride = kProjBlockRows + 1;                   // dwords between two channels of the backward's NCHW tile
constexpr int kProjSmallD = 64;                                       // up to this D the small weight capacity serves: the tile's workgroup fits a CU twice
constexpr int kProjMaxD = 256;

// floats of W_in, b_in (maxd slots), W_out, b_out in LDS at width D; the two capacities the kernels are instantiated with
constexpr int proj_weight_floats(int maxd, int D) { return 2 * maxd * D + maxd + D; }
constexpr int proj_weight_floats_small(int maxd) { return proj_weight_floats(maxd, kProjSmallD); }
constexpr int proj_weight_floats_max(int maxd) { return proj_weight_floats(maxd, kProjMaxD); }

struct ProjArgs {
    const float *z;                                  // forward / backward: z_e.  (N, D) rows or (B, D, HW) maps
    const float *g;                                  // backward: grad_zq, z's layout; LFQ: or NULL (zero)
    const float *w_in, *b_in, *w_out, *b_out;        // (d, D), (d), (D, d), (D); NULL where the kernel does not read them
    const long long *idx_in;                         // decode
    float *out;                                      // forward / decode: z_q; backward: grad_z.  May be NULL (forward, backward)
    long long *idx;                                  // forward; LFQ: may be NULL (the backward's y pass)
    int *hist;                                       // forward, may be NULL; zero on entry
    double *partials;                                // backward: one record of proj_partial_count() doubles per workgroup, or NULL
    long long N;
    int D, HW, d, K;
};

// one workgroup's record of parameter-gradient partials: [W_out (D, d)] [b_out (D)] [W_in (d, D)] [b_in (d)]
constexpr int proj_partial_count(int D, int d) { return 2 * D * d + D + d; }

// ---- the weights in LDS: [W_in d D] [b_in MAXD] [W_out D d] [b_out D]; uniform reads are broadcasts ------------------------------
struct ProjLdsW { const float *w_in, *b_in, *w_out, *b_out; };

template <int MAXD>
__device__ __forceinline__ ProjLdsW proj_stage_weights(const ProjArgs &a, float *w) {
    const int dD = a.d * a.D;
    float *wi = w, *bi = w + dD, *wo = bi + MAXD, *bo = wo + dD;
    for (int i = threadIdx.x; i < dD; i += kProjBlockRows) {
        if (a.w_in) wi[i] = a.w_in[i];
        if (a.w_out) wo[i] = a.w_out[i];
    }
    if (a.b_in)
        for (int i = threadIdx.x; i < a.d; i += kProjBlockRows) bi[i] = a.b_in[i];
    if (a.b_out)
        for (int i = threadIdx.x; i < a.D; i += kProjBlockRows) bo[i] = a.b_out[i];
    __syncthreads();
    return {wi, bi, wo, bo};
}

// ---- the per-row operations, one IEEE operation each -----------------------------------------------------------------------------

// channel c of a row joins the d sums `acc` through row c of a (D, d)-shaped view: w[j * sj + c * sc]
template <int MAXD>
__device__ __forceinline__ void proj_project(double *acc, const float *w, int sj, int sc, int c, int d, float x) {
#pragma unroll
    for (int j = 0; j < MAXD; ++j)
        if (j < d) acc[j] = acc[j] + (double)w[j * sj + c * sc] * (double)x;
}

// z_q of channel c from the codes
template <int MAXD>
__device__ __forceinline__ float proj_zq(const ProjLdsW &w, int c, int d, const float *code) {
    double s = (double)w.b_out[c];
#pragma unroll
    for (int j = 0; j < MAXD; ++j)
        if (j < d) s = s + (double)w.w_out[c * d + j] * (double)code[j];
    return (float)s;
}

// grad_z of channel c from gy (fp64, unrounded)
template <int MAXD>
__device__ __forceinline__ float proj_gz(const ProjLdsW &w, int c, int D, int d, const double *gy) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < MAXD; ++j)
        if (j < d) s = s + (double)w.w_in[j * D + c] * gy[j];
    return (float)s;
}

// ---- where a thread stands ----------------------------------------------------------------------------------------------------------

// row-major rows: a wave owns 64 consecutive rows (nr of them exist; a wave without rows still meets every barrier) and its LDS tile
// tx; the lane's row of the tile is mx.  nrb: the rows of the workgroup.
struct ProjRowsPos {
    float *tx, *mx;
    long long r0;
    int lane, nr, nrb;
    bool mine;
};

__device__ __forceinline__ ProjRowsPos proj_rows_pos(const ProjArgs &a, float *tiles) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float *tx = tiles + wave * kL2TileFloats;
    const long long row0 = (long long)blockIdx.x * kProjBlockRows, r0 = row0 + wave * 64, left = a.N - r0, leftb = a.N - row0;
    const int nr = left <= 0 ? 0 : (left < 64 ? (int)left : 64);
    const int nrb = leftb < kProjBlockRows ? (int)leftb : kProjBlockRows;
    return {tx, tx + lane * kL2Stride, r0, lane, nr, nrb, lane < nr};
}

// NCHW maps in the backward: a lane owns one pixel, channel c of it lies at base + c * stride; a lane past the last row stands on 0
struct ProjNchwPos {
    long long row;
    size_t base, stride;
    int nrb;
    bool mine;
};

__device__ __forceinline__ ProjNchwPos proj_nchw_pos(const ProjArgs &a) {
    const long long row0 = (long long)blockIdx.x * kProjBlockRows, row = row0 + threadIdx.x, left = a.N - row0;
    const int nrb = left < kProjBlockRows ? (int)left : kProjBlockRows;
    const bool mine = row < a.N;
    const long long b = mine ? row / a.HW : 0;
    return {row, (size_t)b * a.D * a.HW + (size_t)(mine ? row - b * a.HW : 0), (size_t)a.HW, nrb, mine};
}

// ---- forward and decode ----------------------------------------------------------------------------------------------------------

// NCHW maps: a lane owns one pixel; every channel is one coalesced access of the wave
template <typename P, bool DECODE>
__device__ __forceinline__ void proj_fwd_nchw_body(const typename P::Args &a, float *wl) {
    constexpr int MAXD = P::kMaxD;
    const ProjLdsW w = proj_stage_weights<MAXD>(a, wl);
    const long long row = (long long)blockIdx.x * kProjBlockRows + threadIdx.x;
    if (row >= a.N) return;                                                   // (no barrier below)
    const int D = a.D, d = a.d;
    const long long b = row / a.HW;
    const size_t base = (size_t)b * D * a.HW + (size_t)(row - b * a.HW), stride = (size_t)a.HW;
    float code[MAXD];
    if constexpr (DECODE) {
        P::codes_of_index(a, a.idx_in[row], code);
    } else {
        double acc[MAXD];
        typename P::Side side;
#pragma unroll
        for (int j = 0; j < MAXD; ++j) acc[j] = j < d ? (double)w.b_in[j] : 0.0;
#pragma unroll P::kNchwUnroll
        for (int c = 0; c < D; ++c) proj_project<MAXD>(acc, w.w_in, D, 1, c, d, a.z[base + c * stride]);
        P::quantize_row(a, acc, row, true, code, side);
        if (!a.out) return;
    }
#pragma unroll 4
    for (int c = 0; c < D; ++c) a.out[base + c * stride] = proj_zq<MAXD>(w, c, d, code);
}

// row-major rows: a wave stages 64 channels of its 64 rows at a time through its LDS tile (vq_cosine.h)
template <typename P, bool DECODE, int V>
__device__ __forceinline__ void proj_fwd_rows_body(const typename P::Args &a, float *tiles, float *wl) {
    constexpr int MAXD = P::kMaxD;
    const ProjLdsW w = proj_stage_weights<MAXD>(a, wl);
    const ProjRowsPos p = proj_rows_pos(a, tiles);
    const int D = a.D, d = a.d, nch = (D + kL2Chunk - 1) / kL2Chunk;
    float code[MAXD];
    if constexpr (DECODE) {
        P::codes_of_index(a, p.mine ? a.idx_in[p.r0 + p.lane] : 0, code);
    } else {
        double acc[MAXD];
        typename P::Side side;
#pragma unroll
        for (int j = 0; j < MAXD; ++j) acc[j] = j < d ? (double)w.b_in[j] : 0.0;
        for (int ch = 0; ch < nch; ++ch) {
            const int c0 = ch * kL2Chunk, cw = D - c0 < kL2Chunk ? D - c0 : kL2Chunk;
            l2n_copy<V, true>(const_cast<float *>(a.z), p.tx, p.r0, p.nr, D, c0, cw, p.lane);
            __syncthreads();
            if (p.mine)
                for (int c = 0; c < cw; c += 4) {
                    float xv[4];
                    l2n_load<4>(p.mx, (size_t)c, xv);
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (c + k < cw) proj_project<MAXD>(acc, w.w_in, D, 1, c0 + c + k, d, xv[k]);
                }
            __syncthreads();
        }
        P::quantize_row(a, acc, p.r0 + p.lane, p.mine, code, side);
        if (!a.out) return;                                                   // (uniform: every thread leaves)
    }
    for (int ch = 0; ch < nch; ++ch) {
        const int c0 = ch * kL2Chunk, cw = D - c0 < kL2Chunk ? D - c0 : kL2Chunk;
        if (p.mine)
            for (int c = 0; c < cw; c += 4) {
                float o[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] = c + k < cw ? proj_zq<MAXD>(w, c0 + c + k, d, code) : 0.0f;
                l2n_store<4>(p.mx, (size_t)c, o);                             // (slots past cw belong to the row's padding)
            }
        __syncthreads();
        l2n_copy<V, false>(a.out, p.tx, p.r0, p.nr, D, c0, cw, p.lane);
        __syncthreads();
    }
}

// ---- backward --------------------------------------------------------------------------------------------------------------------
// The row-local part runs as the forward does and is the quantizer's own (P::bwd_*_body): it ends with the row's gy (fp64) in
// registers and, for the parameter gradients, the codes (fp32) and gy of the workgroup's rows in LDS.  The parameter gradients are
// sums over rows: every workgroup owns the SAME 256 consecutive rows in either layout, brings 64 channels of g, then of z, into a
// tile, and thread o of the workgroup adds the 256 terms of output o one row after the other, in ascending row order, into an fp64
// partial of the workgroup's record.  proj_param_finalize_body adds the records in ascending workgroup order.  `tile` is addressed
// as tile[row * RS + channel * CS]: the four waves' row-major tiles are one (256, 68) image (RS = 68, CS = 1); the NCHW kernel
// writes a lane's pixel at RS = 1, CS = 257, so that stores (lanes = rows) and reads (lanes = channels) both miss bank conflicts.

// NULL_G: the quantizer's backward takes g == NULL for "no upstream gradient" (LFQ), and the sums are then 0.0
template <int MAXD, int RS, int CS, bool NULL_G>
__device__ __forceinline__ void proj_reduce_w_out(const ProjArgs &a, const float *tile, const float *code_l, int c0, int cw, int nrb,
                                                  double *part) {
    const int d = a.d;
    const bool have = !NULL_G || a.g != nullptr;
    for (int o = threadIdx.x; o < cw * d + cw; o += kProjBlockRows) {
        double s = 0.0;
        if (o < cw * d) {
            const int j = o / cw, c = o - j * cw;
            if (have) {
#pragma unroll 8
                for (int r = 0; r < nrb; ++r) s = s + (double)tile[r * RS + c * CS] * (double)code_l[r * MAXD + j];
            }
            part[(c0 + c) * d + j] = s;
        } else {
            const int c = o - cw * d;
            if (have) {
#pragma unroll 8
                for (int r = 0; r < nrb; ++r) s = s + (double)tile[r * RS + c * CS];
            }
            part[a.D * d + c0 + c] = s;
        }
    }
}

template <int MAXD, int RS, int CS>
__device__ __forceinline__ void proj_reduce_w_in(const ProjArgs &a, const float *tile, const double *gy_l, int c0, int cw, int nrb,
                                                 double *part) {
    const int d = a.d, D = a.D;
    double *p_w = part + D * d + D, *p_b = p_w + d * D;
    for (int o = threadIdx.x; o < cw * d + (c0 == 0 ? d : 0); o += kProjBlockRows) {
        double s = 0.0;
        if (o < cw * d) {
            const int j = o / cw, c = o - j * cw;
#pragma unroll 8
            for (int r = 0; r < nrb; ++r) s = s + gy_l[r * MAXD + j] * (double)tile[r * RS + c * CS];
            p_w[j * D + c0 + c] = s;
        } else {
            const int j = o - cw * d;
#pragma unroll 8
            for (int r = 0; r < nrb; ++r) s = s + gy_l[r * MAXD + j];
            p_b[j] = s;
        }
    }
}

// the last launch: output o = the workgroups' partials of o in ascending workgroup order, rounded once.  A NULL gradient is skipped.
__device__ __forceinline__ void proj_param_finalize_body(const double *partials, long long nblocks, int D, int d, float *g_w_in,
                                                         float *g_b_in, float *g_w_out, float *g_b_out) {
    const int P = proj_partial_count(D, d), o = blockIdx.x * kProjBlockRows + threadIdx.x;
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

}  // namespace vqvae
