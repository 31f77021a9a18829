// Lookup-free quantization (vq_lfq.hip, whose header states the arithmetic): what LFQ does with the finished sums of a row -- the sign
// code -- every loss kernel, and its backward bodies, which read the y and e the earlier launches left.  The kernel skeleton around
// them (the weights in LDS, the projections, the forward / decode bodies, the parameter-gradient reductions and their second launch)
// is vq_proj.h's, the same text FSQ's row kernels compile; it takes `Lfq` below as its policy.  Plain C++ over
// `__device__ __forceinline__`, so that tests/host/lfq_harness.cpp compiles THIS text for the host and runs it under the sanitizers.
#pragma once

#include "vq_proj.h"

namespace vqvae {

constexpr int kLfqMaxBits = 16;
constexpr int kLfqChunkRows = 64;                                     // rows whose probabilities the avg kernel stages at a time
constexpr int kLfqTileCodes = 4 * 256;                                // codes of one workgroup of the avg kernel: 4 per thread
constexpr int kLfqLdsLogK = 4096;                                     // log avg lies in LDS up to this K (padded: kLfqLogLdsDoubles)
constexpr int kLfqLogLdsDoubles = 64 * 65;                            // K = 4096: 64 rows of 64 + 1
constexpr int kLfqLogLdsDoublesSmall = 32 * 33;                       // K <= 1024: more workgroups fit a CU
constexpr int kLfqGradThreads = 64;                                  // one wave per row in the entropy-gradient kernel
constexpr int kLfqScalarSlots = 2 * kLfqMaxBits;                      // per partition: [P sums of the d channels] [C sums]

struct LfqArgs : ProjArgs {
    float *y;                                        // forward: (N, d) out, may be NULL.  backward: (N, d) in
    const double *e;                                 // backward: (N, d) d loss / d y without grad_loss, or NULL (no loss gradient)
    const float *gl;                                 // backward: grad_loss (device scalar), NULL = 1
};

// what the loss kernels share
struct LfqLossArgs {
    const float *y;                                  // (N, d)
    long long N, rows_per_part;
    int d, K, P, nwg;                                // P partitions of rows_per_part rows; nwg workgroups of the gradient kernel
    double s, beta, we, gamma;                       // s = 4 / temperature
    double *avg_part, *sc_part;                      // (P, K) and (P, kLfqScalarSlots)
    const double *avg;                               // backward: (K)
    double *avg_out;                                 // forward: (K)
    float *losses;                                   // forward: (loss, C, P, H)
    double *logavg;                                  // backward: (K), log 0 = 0
    double *e;                                       // backward: (N, d)
};

// ---- the per-row operations, one IEEE operation each -----------------------------------------------------------------------------

// the code of one y: +1 above zero, -1 at and below it, NaN for a NaN
__device__ __forceinline__ float lfq_code(float y) { return y != y ? __builtin_nanf("") : (y > 0.0f ? 1.0f : -1.0f); }

// acc (the d sums, b_in included) -> y, codes c (fp32) and the row's index.  A NaN y_j: bit 0, c_j NaN.
__device__ __forceinline__ long long lfq_quantize(int d, const double *acc, float *y, float *code) {
    long long idx = 0;
#pragma unroll
    for (int j = 0; j < kLfqMaxBits; ++j)
        if (j < d) {
            y[j] = (float)acc[j];
            code[j] = lfq_code(y[j]);
            idx += y[j] > 0.0f ? (1LL << j) : 0LL;
        }
    return idx;
}

// p+ = sigma(a), p- = sigma(-a), each computed directly from e = exp(-|a|); small = sigma(-|a|)
__device__ __forceinline__ void lfq_sigmoid(double a, double &pp, double &pm, double &e, double &small) {
    const double m = fabs(a);
    e = exp(-m);
    const double den = 1.0 + e, big = 1.0 / den;
    small = e / den;
    const bool pos = a >= 0.0;
    pp = pos ? big : small;
    pm = pos ? small : big;
}

// sum of one fp64 value per thread of a 256-thread workgroup through red[256], by a fixed tree (common.h's block_sum_f64)
__device__ __forceinline__ void lfq_block_sum(double *red, int tid, double v) {
    red[tid] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] += red[tid + o];
        __syncthreads();
    }
}

// what the forward keeps of a row
__device__ __forceinline__ void lfq_row_out(const LfqArgs &a, long long row, long long idx, const float *y) {
    if (a.idx) a.idx[row] = idx;
    if (a.hist) atomicAdd(a.hist + idx, 1);
    if (a.y) {
#pragma unroll
        for (int j = 0; j < kLfqMaxBits; ++j)
            if (j < a.d) a.y[(size_t)row * a.d + j] = y[j];
    }
}

// ---- the losses ------------------------------------------------------------------------------------------------------------------
// lfq_avg_body: workgroup (x = partition, y = tile of 1024 codes).  The partition's rows are staged 64 at a time as p-, p+ of every
// channel (LDS, fp64); thread t then takes the rows one after the other, in ascending order, and adds
//     p_n(k) = ((..(1 * p_0) * p_1 ..) * p_{d-1}),  p_j = p+ where bit j of k is set, p- where not,
// to its code k = tile * 1024 + i * 256 + t, i = 0 .. 3 (bits 0 .. 7 of k are t's: that part of the product is shared).  In tile 0
// thread j < d also adds channel j's entropy h and commitment term (y - c)^2 of the rows in the same order.
__device__ __forceinline__ void lfq_avg_body(const LfqLossArgs &a, double *pp, double *hh, double *cc) {
    const int part = blockIdx.x, tile = blockIdx.y, t = threadIdx.x, d = a.d;
    const long long r_begin = (long long)part * a.rows_per_part;
    const long long r_end = a.N - r_begin < a.rows_per_part ? a.N : r_begin + a.rows_per_part;
    const int dlo = d < 8 ? d : 8;
    double acc[4] = {0.0, 0.0, 0.0, 0.0}, acc_p = 0.0, acc_c = 0.0;
    int k[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) k[i] = tile * kLfqTileCodes + i * 256 + t;
    for (long long r0 = r_begin; r0 < r_end; r0 += kLfqChunkRows) {
        const int nr = r_end - r0 < kLfqChunkRows ? (int)(r_end - r0) : kLfqChunkRows;
        __syncthreads();                                                      // the last chunk's readers are done
        for (int it = t; it < nr * d; it += 256) {
            const float y = a.y[(size_t)r0 * d + it];
            double p1, p0, e, small;
            lfq_sigmoid(a.s * (double)y, p1, p0, e, small);
            pp[2 * it] = p0;
            pp[2 * it + 1] = p1;
            if (tile == 0) {
                const double m = fabs(a.s * (double)y), c = y > 0.0f ? 1.0 : -1.0, df = (double)y - c;
                hh[it] = log1p(e) + m * small;
                cc[it] = df * df;
            }
        }
        __syncthreads();
#pragma unroll 4
        for (int r = 0; r < nr; ++r) {
            const double *p = pp + 2 * r * d;
            double lo = 1.0;
            for (int j = 0; j < dlo; ++j) lo = lo * p[2 * j + ((t >> j) & 1)];
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (k[i] < a.K) {
                    double v = lo;
                    for (int j = 8; j < d; ++j) v = v * p[2 * j + ((k[i] >> j) & 1)];
                    acc[i] = acc[i] + v;
                }
            if (tile == 0 && t < d) {
                acc_p = acc_p + hh[r * d + t];
                acc_c = acc_c + cc[r * d + t];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (k[i] < a.K) a.avg_part[(size_t)part * a.K + k[i]] = acc[i];
    if (tile == 0 && t < d) {
        a.sc_part[part * kLfqScalarSlots + t] = acc_p;
        a.sc_part[part * kLfqScalarSlots + kLfqMaxBits + t] = acc_c;
    }
}

// avg[k] = (partitions in ascending order, from 0.0) / N: one thread per code
__device__ __forceinline__ void lfq_avg_reduce_body(const LfqLossArgs &a) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= a.K) return;
    double s = 0.0;
#pragma unroll 8
    for (int p = 0; p < a.P; ++p) s = s + a.avg_part[(size_t)p * a.K + k];
    a.avg_out[k] = s / (double)a.N;
}

// one workgroup: H: thread t adds avg log avg of k = t, t + 256, .. in ascending order, the 256 sums meet in the fixed tree;
// P and C: per channel the partitions in order, then the channels in order
__device__ __forceinline__ void lfq_loss_finalize_body(const LfqLossArgs &a, double *red, double *ch) {
    const int t = threadIdx.x;
    double hs = 0.0;
    for (int k = t; k < a.K; k += 256) {
        const double av = a.avg_out[k];
        hs = hs + (av == 0.0 ? 0.0 : av * log(av));
    }
    lfq_block_sum(red, t, hs);
    if (t < a.d) {
        double sp = 0.0, sc = 0.0;
        for (int p = 0; p < a.P; ++p) {
            sp = sp + a.sc_part[p * kLfqScalarSlots + t];
            sc = sc + a.sc_part[p * kLfqScalarSlots + kLfqMaxBits + t];
        }
        ch[t] = sp;
        ch[kLfqMaxBits + t] = sc;
    }
    __syncthreads();
    if (t == 0) {
        double sp = 0.0, sc = 0.0;
        for (int j = 0; j < a.d; ++j) {
            sp = sp + ch[j];
            sc = sc + ch[kLfqMaxBits + j];
        }
        const double H = -red[0], P = sp / (double)a.N, C = sc / ((double)a.N * (double)a.d);
        const double loss = a.beta * C + a.we * (P - a.gamma * H);
        a.losses[0] = (float)loss;
        a.losses[1] = (float)C;
        a.losses[2] = (float)P;
        a.losses[3] = (float)H;
    }
}

__device__ __forceinline__ void lfq_logavg_body(const LfqLossArgs &a) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= a.K) return;
    const double av = a.avg[k];
    a.logavg[k] = av == 0.0 ? 0.0 : log(av);
}

// bit b put in at position j of m
__device__ __forceinline__ int lfq_insert_bit(int m, int j, int b) { return ((m >> j) << (j + 1)) | (b << j) | (m & ((1 << j) - 1)); }

// lfq_entgrad_body: one wave per row, rows blockIdx.x, + nwg, ..: e[n][j] = d loss / d y_nj without grad_loss.  The bits are split
// into dl = ceil(d / 2) low and dh = d - dl high ones; A[lo], B[hi] are the products over each half (ascending j, from 1.0);
// u[lo] = sum_hi L[hi][lo] B[hi], v[hi] = sum_lo L[hi][lo] A[lo] (ascending, from 0.0), L = log avg;
// T_j^b = sum over the half's entries q with bit j = b, ascending, of u[q] (or v[q]) * the product of the half's other channels.
// L lies in LDS with rows 2^dl + 1 apart (both walks miss bank conflicts) up to K = 4096, above that it is read from memory.
__device__ __forceinline__ void lfq_entgrad_body(const LfqLossArgs &a, double *l_lds, double *pb, double *A, double *B, double *u,
                                                 double *v, double *T) {
    const int t = threadIdx.x, d = a.d, dl = (d + 1) / 2, dh = d - dl, nlo = 1 << dl, nhi = 1 << dh;
    const double *L = a.logavg;
    int ls = nlo;
    if (a.K <= kLfqLdsLogK) {
        ls = nlo + 1;
        for (int k = t; k < a.K; k += kLfqGradThreads) l_lds[(k >> dl) * ls + (k & (nlo - 1))] = a.logavg[k];
        L = l_lds;
    }
    const double n = (double)a.N;
    for (long long row = blockIdx.x; row < a.N; row += a.nwg) {
        __syncthreads();
        float y = 0.0f;
        double p1 = 0.0, p0 = 0.0;
        if (t < d) {
            double e, small;
            y = a.y[(size_t)row * d + t];
            lfq_sigmoid(a.s * (double)y, p1, p0, e, small);
            pb[2 * t] = p0;
            pb[2 * t + 1] = p1;
        }
        __syncthreads();
        for (int q = t; q < nlo; q += kLfqGradThreads) {
            double s = 1.0;
            for (int j = 0; j < dl; ++j) s = s * pb[2 * j + ((q >> j) & 1)];
            A[q] = s;
        }
        for (int q = t; q < nhi; q += kLfqGradThreads) {
            double s = 1.0;
            for (int j = 0; j < dh; ++j) s = s * pb[2 * (dl + j) + ((q >> j) & 1)];
            B[q] = s;
        }
        __syncthreads();
        for (int q = t; q < nlo; q += kLfqGradThreads) {
            double s = 0.0;
#pragma unroll 8
            for (int hi = 0; hi < nhi; ++hi) s = s + L[hi * ls + q] * B[hi];
            u[q] = s;
        }
        for (int q = t; q < nhi; q += kLfqGradThreads) {
            double s = 0.0;
#pragma unroll 8
            for (int lo = 0; lo < nlo; ++lo) s = s + L[q * ls + lo] * A[lo];
            v[q] = s;
        }
        __syncthreads();
        if (t < 2 * d) {
            const int j = t >> 1, b = t & 1, low = j < dl, jj = low ? j : j - dl, nb = low ? dl : dh, j0 = low ? 0 : dl;
            const double *w = low ? u : v;
            double s = 0.0;
#pragma unroll 4
            for (int m = 0; m < (1 << (nb - 1)); ++m) {
                const int q = lfq_insert_bit(m, jj, b);
                double f = w[q];
                for (int i = 0; i < nb; ++i)
                    if (i != jj) f = f * pb[2 * (j0 + i) + ((q >> i) & 1)];
                s = s + f;
            }
            T[t] = s;
        }
        __syncthreads();
        if (t < d) {
            const double c = y > 0.0f ? 1.0 : -1.0, pq = p1 * p0, yd = (double)y;
            const double t1 = a.beta * 2.0 * (yd - c) / (n * (double)d);
            const double t2 = a.we * (a.s * a.s / n) * yd * pq;
            const double t3 = a.we * a.gamma * (a.s / n) * pq * (T[2 * t + 1] - T[2 * t]);
            a.e[(size_t)row * d + t] = t1 - t2 + t3;
        }
    }
}

// ---- backward --------------------------------------------------------------------------------------------------------------------

// gy of a row from its gc sums: gy_j = gc_j + g * e_j (two operations; without e: gc_j); codes and gy to LDS for the reductions
__device__ __forceinline__ void lfq_bwd_row(const LfqArgs &a, long long row, const double *acc_g, bool params, bool mine, float *code_l,
                                            double *gy_l, double *gy) {
    const double gl = a.gl ? (double)*a.gl : 1.0;
#pragma unroll
    for (int j = 0; j < kLfqMaxBits; ++j)
        if (j < a.d) {
            gy[j] = acc_g[j];
            if (mine) {
                if (a.e) gy[j] = acc_g[j] + gl * a.e[(size_t)row * a.d + j];
                if (params) {
                    code_l[threadIdx.x * kLfqMaxBits + j] = lfq_code(a.y[(size_t)row * a.d + j]);
                    gy_l[threadIdx.x * kLfqMaxBits + j] = gy[j];
                }
            }
        }
}

// ---- vq_proj.h's policy ------------------------------------------------------------------------------------------------------------
struct Lfq {
    using Args = LfqArgs;
    static constexpr int kMaxD = kLfqMaxBits, kNchwUnroll = 4;
    using Side = float[kLfqMaxBits];                 // y

    // an index -> codes; outside [0, K): NaN codes
    static __device__ __forceinline__ void codes_of_index(const LfqArgs &a, long long idx, float *code) {
        const bool ok = idx >= 0 && idx < (long long)a.K;
        const unsigned u = ok ? (unsigned)idx : 0u;
#pragma unroll
        for (int j = 0; j < kLfqMaxBits; ++j)
            if (j < a.d) code[j] = ok ? (((u >> j) & 1u) ? 1.0f : -1.0f) : __builtin_nanf("");
    }

    static __device__ __forceinline__ void quantize_row(const LfqArgs &a, const double *acc, long long row, bool mine, float *code,
                                                        float *y) {
        const long long idx = lfq_quantize(a.d, acc, y, code);
        if (mine) lfq_row_out(a, row, idx, y);
    }

    // the backward: the row-local part runs from the y the first launch left; only gc is projected, and only where g is given
    template <bool PARAMS>
    static __device__ __forceinline__ void bwd_nchw_body(const LfqArgs &a, float *tile, float *wl, float *code_l, double *gy_l) {
        const ProjLdsW w = proj_stage_weights<kMaxD>(a, wl);
        const ProjNchwPos p = proj_nchw_pos(a);
        const int D = a.D, d = a.d;
        double acc_g[kMaxD], gy[kMaxD];
#pragma unroll
        for (int j = 0; j < kMaxD; ++j) acc_g[j] = 0.0;
        if (p.mine && a.g) {
#pragma unroll 4
            for (int c = 0; c < D; ++c) proj_project<kMaxD>(acc_g, w.w_out, 1, d, c, d, a.g[p.base + c * p.stride]);
        }
        lfq_bwd_row(a, p.row, acc_g, PARAMS, p.mine, code_l, gy_l, gy);
        if (a.out && p.mine) {
#pragma unroll 4
            for (int c = 0; c < D; ++c) a.out[p.base + c * p.stride] = proj_gz<kMaxD>(w, c, D, d, gy);
        }
        if constexpr (PARAMS) {
            double *part = a.partials + (size_t)blockIdx.x * proj_partial_count(D, d);
            for (int c0 = 0; c0 < D; c0 += kL2Chunk) {
                const int cw = D - c0 < kL2Chunk ? D - c0 : kL2Chunk;
                __syncthreads();                                              // code_l / gy_l written; the tile's last readers are done
                if (p.mine && a.g)
                    for (int c = 0; c < cw; ++c) tile[c * kProjNchwStride + threadIdx.x] = a.g[p.base + (c0 + c) * p.stride];
                __syncthreads();
                proj_reduce_w_out<kMaxD, 1, kProjNchwStride, true>(a, tile, code_l, c0, cw, p.nrb, part);
                __syncthreads();
                if (p.mine)
                    for (int c = 0; c < cw; ++c) tile[c * kProjNchwStride + threadIdx.x] = a.z[p.base + (c0 + c) * p.stride];
                __syncthreads();
                proj_reduce_w_in<kMaxD, 1, kProjNchwStride>(a, tile, gy_l, c0, cw, p.nrb, part);
            }
        }
    }

    template <bool PARAMS, int V>
    static __device__ __forceinline__ void bwd_rows_body(const LfqArgs &a, float *tiles, float *wl, float *code_l, double *gy_l) {
        const ProjLdsW w = proj_stage_weights<kMaxD>(a, wl);
        const ProjRowsPos p = proj_rows_pos(a, tiles);
        const int D = a.D, d = a.d, nch = (D + kL2Chunk - 1) / kL2Chunk;
        double acc_g[kMaxD], gy[kMaxD];
#pragma unroll
        for (int j = 0; j < kMaxD; ++j) acc_g[j] = 0.0;
        if (a.g)                                                                  // (uniform)
            for (int ch = 0; ch < nch; ++ch) {
                const int c0 = ch * kL2Chunk, cw = D - c0 < kL2Chunk ? D - c0 : kL2Chunk;
                l2n_copy<V, true>(const_cast<float *>(a.g), p.tx, p.r0, p.nr, D, c0, cw, p.lane);
                __syncthreads();
                if (p.mine)
                    for (int c = 0; c < cw; c += 4) {
                        float xv[4];
                        l2n_load<4>(p.mx, (size_t)c, xv);
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (c + k < cw) proj_project<kMaxD>(acc_g, w.w_out, 1, d, c0 + c + k, d, xv[k]);
                    }
                __syncthreads();
            }
        lfq_bwd_row(a, p.r0 + p.lane, acc_g, PARAMS, p.mine, code_l, gy_l, gy);
        double *part = PARAMS ? a.partials + (size_t)blockIdx.x * proj_partial_count(D, d) : nullptr;
        for (int ch = 0; ch < nch; ++ch) {
            const int c0 = ch * kL2Chunk, cw = D - c0 < kL2Chunk ? D - c0 : kL2Chunk;
            if constexpr (PARAMS) {
                if (a.g) l2n_copy<V, true>(const_cast<float *>(a.g), p.tx, p.r0, p.nr, D, c0, cw, p.lane);
                __syncthreads();                                              // (and code_l / gy_l are written)
                proj_reduce_w_out<kMaxD, kL2Stride, 1, true>(a, tiles, code_l, c0, cw, p.nrb, part);
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

// the partition of the rows for the sums of the losses: whole blocks of 256 rows, at most max(16, min(1024, 2^20 / K)) partitions,
// so that the (P, K) partials take at most 8 MiB.  A function of (N, K) alone.
inline void lfq_partition(long long N, int K, long long &rows_per_part, int &P) {
    long long pmax = (1LL << 20) / K;
    pmax = pmax < 16 ? 16 : (pmax > 1024 ? 1024 : pmax);
    const long long blocks = (N + kProjBlockRows - 1) / kProjBlockRows, bpp = (blocks + pmax - 1) / pmax;
    rows_per_part = bpp * kProjBlockRows;
    P = (int)((blocks + bpp - 1) / bpp);
}

}  // namespace vqvae
