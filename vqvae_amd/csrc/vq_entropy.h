// The code-entropy loss of a learned codebook (vq_entropy.hip, whose header states the arithmetic): the whole bodies of the kernels.
// Plain C++ over `__device__ __forceinline__`, so that tests/host/entropy_harness.cpp compiles THIS text for the host (blockIdx /
// threadIdx and __syncthreads supplied by the harness) and runs it under the sanitizers.
//
// Everything is built from two tile routines on a workgroup of 256 threads, laid out as 16 x 16 (tx = t % 16, ty = t / 16):
//   ent_dots       the 64 x 64 tile dot[i][k] = sum_c a_ic b_kc of two fp32 sources, staged kEntChunk channels at a time as doubles
//                  (channel-major, kEntStride doubles apart) -- thread (tx, ty) keeps the 4 x 4 entries of rows 4 ty .. 4 ty + 3 and
//                  codes 4 tx .. 4 tx + 3 as sixteen independent fp64 chains, channels in ascending order
//   ent_contract2  acc[o][c] += sum_i w[i][o] x_ic for the 64 i of a tile, w an LDS tile of doubles, x a source staged kEntSub rows at
//                  a time over all DT channels -- thread (tx, ty) keeps outputs o = 4 ty .. 4 ty + 3 and channels 64 q + 4 tx .. + 3
// A source (EntSrc) is (n, D) rows, or (B, D, HW) maps read one pixel per lane; what is staged is the same doubles in both layouts,
// and everything after staging is layout-free.  Rows past n and channels past D are staged as 0.0 and add fma(0, 0, s) = s.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <cmath>

namespace vqvae {

constexpr int kEntThreads = 256;
constexpr int kEntTile = 64;                                 // rows and codes of one tile
constexpr int kEntChunk = 16;                                // channels staged per step of ent_dots
constexpr int kEntStride = kEntTile + 2;                     // doubles between the channels of a staged chunk, the rows of a w tile
constexpr int kEntSub = 8;                                   // rows of x staged per step of ent_contract2
constexpr int kEntMaxK = 16384, kEntMaxD = 256;
constexpr int kEntBlockRows = 256;                           // the contract's block of rows
constexpr int kEntBufDoubles = 2 * kEntChunk * kEntStride;   // the staging buffer: two chunks | kEntSub x 256 of x | 64 x 16 of red
constexpr int kEntWDoubles = kEntTile * kEntStride;          // the w tile
static_assert(kEntSub * kEntMaxD <= kEntBufDoubles && kEntTile * 16 <= kEntBufDoubles, "the staging buffer takes its three uses");

struct EntSrc {
    const float *p;
    long long n;                                             // rows
    int D, HW, rm;                                           // rm: (n, D) rows; else (B, D, HW) maps
};

struct EntArgs {
    EntSrc z, e;                                             // the rows (either layout) and the codebook (K, D)
    long long N, rows_per_part;                              // of the launch's partition scheme (avg's or grad_E's)
    int K, D, P;
    double s, gamma;
    const float *gl;                                         // backward: grad_loss, NULL = 1
    double *zz, *ee;                                         // (N), (K): squared norms
    double *rs;                                              // (N, 2): log-sum-exp and H_n (the forward writes, the backward reads)
    double *rs_out;                                          // forward: the caller's rowstat or NULL
    double *avg_part, *sc_part;                              // forward: (P, K), (P)
    double *avg;                                             // forward: out (K); backward: in
    float *losses;                                           // forward: (term, P, H)
    double *logavg, *m;                                      // backward: (K), (N)
    double *ge_part, *as_part;                               // backward: (P, K, D), (P, K)
    float *grad_z, *grad_e;
};

__device__ __forceinline__ size_t ent_index(const EntSrc &s, long long i, int c) {
    if (s.rm) return (size_t)i * s.D + c;
    const long long b = i / s.HW;
    return ((size_t)b * s.D + c) * s.HW + (size_t)(i - b * s.HW);
}

// squared norms: one thread per row, c ascending from 0.0 (each square is exact in fp64)
__device__ __forceinline__ void ent_sqnorm_body(const EntSrc &s, double *out) {
    const long long i = (long long)blockIdx.x * kEntThreads + threadIdx.x;
    if (i >= s.n) return;
    const size_t base = ent_index(s, i, 0), step = s.rm ? 1 : (size_t)s.HW;
    double a = 0.0;
    for (int c = 0; c < s.D; ++c) {
        const double x = (double)s.p[base + c * step];
        a = __builtin_fma(x, x, a);
    }
    out[i] = a;
}

// rows i0 .. i0 + 63, channels c0 .. c0 + kEntChunk - 1 of a source: each thread's four elements, 0 outside the source.  ent_fetch
// loads them into registers, ent_put writes them to dst[c][r] as doubles: ent_dots issues the next chunk's loads in front of the
// current chunk's arithmetic, so that the loads' latency is not waited for at every step.
__device__ __forceinline__ void ent_fetch(const EntSrc &s, long long i0, int c0, float (&v)[4]) {
    const int t = (int)threadIdx.x;
    if (s.rm) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = t + q * kEntThreads, c = e % kEntChunk, r = e / kEntChunk;
            const bool in = i0 + r < s.n && c0 + c < s.D;
            v[q] = in ? s.p[(size_t)(i0 + r) * s.D + c0 + c] : 0.f;
        }
    } else {
        const int r = t % kEntTile;
        const long long i = i0 + r;
        const bool row = i < s.n;
        const size_t base = row ? ent_index(s, i, 0) : 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c = t / kEntTile + q * (kEntThreads / kEntTile);
            const bool in = row && c0 + c < s.D;
            v[q] = in ? s.p[base + (size_t)(c0 + c) * s.HW] : 0.f;
        }
    }
}

__device__ __forceinline__ void ent_put(const EntSrc &s, const float (&v)[4], double *dst) {
    const int t = (int)threadIdx.x;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int e = t + q * kEntThreads;
        const int c = s.rm ? e % kEntChunk : t / kEntTile + q * (kEntThreads / kEntTile), r = s.rm ? e / kEntChunk : t % kEntTile;
        dst[c * kEntStride + r] = (double)v[q];
    }
}
static_assert(kEntTile * kEntChunk == 4 * kEntThreads, "four elements of a chunk per thread");

// dot[i][j] = sum_c a(i0 + 4 ty + i, c) b(k0 + 4 tx + j, c), c ascending from 0.0; buf: kEntBufDoubles
__device__ __forceinline__ void ent_dots(const EntSrc &a, long long i0, const EntSrc &b, long long k0, double *buf,
                                         double (&dot)[4][4]) {
    const int tx = (int)threadIdx.x & 15, ty = (int)threadIdx.x >> 4;
    double *al = buf, *bl = buf + kEntChunk * kEntStride;
    float fa[4], fb[4];
    ent_fetch(a, i0, 0, fa);
    ent_fetch(b, k0, 0, fb);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) dot[i][j] = 0.0;
    for (int c0 = 0; c0 < a.D; c0 += kEntChunk) {
        __syncthreads();                                                      // the buffer's last readers are done
        ent_put(a, fa, al);
        ent_put(b, fb, bl);
        __syncthreads();
        if (c0 + kEntChunk < a.D) {                                           // (uniform) the next chunk's loads, used after this one's sums
            ent_fetch(a, i0, c0 + kEntChunk, fa);
            ent_fetch(b, k0, c0 + kEntChunk, fb);
        }
#pragma unroll 4
        for (int c = 0; c < kEntChunk; ++c) {
            double av[4], bv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) av[i] = al[c * kEntStride + 4 * ty + i];
#pragma unroll
            for (int j = 0; j < 4; ++j) bv[j] = bl[c * kEntStride + 4 * tx + j];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) dot[i][j] = __builtin_fma(av[i], bv[j], dot[i][j]);
        }
    }
}

// rows i0 .. i0 + kEntSub - 1 of x over DT channels: each thread's DT / 32 elements, 0 outside the source (ent_fetch's scheme)
template <int DT>
__device__ __forceinline__ void ent_fetch2(const EntSrc &x, long long i0, float (&v)[DT / 32]) {
    const int t = (int)threadIdx.x;
    if (x.rm) {
#pragma unroll
        for (int q = 0; q < DT / 32; ++q) {
            const int e = t + q * kEntThreads, c = e % DT, r = e / DT;
            const bool in = i0 + r < x.n && c < x.D;
            v[q] = in ? x.p[(size_t)(i0 + r) * x.D + c] : 0.f;
        }
    } else {
        const int r = t % kEntSub;
        const long long i = i0 + r;
        const bool row = i < x.n;
        const size_t base = row ? ent_index(x, i, 0) : 0;
#pragma unroll
        for (int q = 0; q < DT / 32; ++q) {
            const int c = t / kEntSub + q * (kEntThreads / kEntSub);
            const bool in = row && c < x.D;
            v[q] = in ? x.p[base + (size_t)c * x.HW] : 0.f;
        }
    }
}

template <int DT>
__device__ __forceinline__ void ent_put2(const EntSrc &x, const float (&v)[DT / 32], double *buf) {
    const int t = (int)threadIdx.x;
#pragma unroll
    for (int q = 0; q < DT / 32; ++q) {
        const int e = t + q * kEntThreads;
        const int c = x.rm ? e % DT : t / kEntSub + q * (kEntThreads / kEntSub), r = x.rm ? e / DT : t % kEntSub;
        buf[r * DT + c] = (double)v[q];
    }
}

// acc[o][4 q + e] += sum_{i < 64} w[i][4 ty + o] x(i0 + i, 64 q + 4 tx + e), i ascending; buf: kEntSub x DT doubles
template <int DT>
__device__ __forceinline__ void ent_contract2(const double *w, const EntSrc &x, long long i0, double *buf, double (&acc)[4][DT / 16]) {
    const int t = (int)threadIdx.x, tx = t & 15, ty = t >> 4;
    float xf[DT / 32];
    ent_fetch2<DT>(x, i0, xf);
    for (int sub = 0; sub < kEntTile; sub += kEntSub) {
        __syncthreads();                                                      // the buffer's last readers are done; w is written
        ent_put2<DT>(x, xf, buf);
        __syncthreads();
        if (sub + kEntSub < kEntTile) ent_fetch2<DT>(x, i0 + sub + kEntSub, xf);      // the next rows' loads, used after these sums
#pragma unroll 2
        for (int r = 0; r < kEntSub; ++r) {
            double wv[4];
#pragma unroll
            for (int o = 0; o < 4; ++o) wv[o] = w[(sub + r) * kEntStride + 4 * ty + o];
#pragma unroll
            for (int q = 0; q < DT / 64; ++q) {
                double xv[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) xv[e] = buf[r * DT + 64 * q + 4 * tx + e];
#pragma unroll
                for (int o = 0; o < 4; ++o)
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[o][4 * q + e] = __builtin_fma(wv[o], xv[e], acc[o][4 * q + e]);
            }
        }
    }
}

// v[i] of the 16 threads of a row group -> every thread gets the sum (ascending tx, from 0.0) or the maximum; red: 64 x 16 doubles
template <bool MAX>
__device__ __forceinline__ void ent_across_tx(double *red, double (&v)[4]) {
    const int tx = (int)threadIdx.x & 15, ty = (int)threadIdx.x >> 4;
    __syncthreads();                                                          // red's region is free
#pragma unroll
    for (int i = 0; i < 4; ++i) red[(4 * ty + i) * 16 + tx] = v[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        double s = MAX ? -INFINITY : 0.0;
        for (int q = 0; q < 16; ++q) {
            const double x = red[(4 * ty + i) * 16 + q];
            s = MAX ? fmax(s, x) : s + x;
        }
        v[i] = s;
    }
    __syncthreads();
}

// the thread's rows and codes of a tile: what the logits need
struct EntTileCtx {
    double zz[4], ee[4];
    bool row[4], code[4];
};

__device__ __forceinline__ void ent_rows_ctx(const EntArgs &a, long long r0, long long r_end, EntTileCtx &x) {
    const int ty = (int)threadIdx.x >> 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long long r = r0 + 4 * ty + i;
        x.row[i] = r < r_end;
        x.zz[i] = x.row[i] ? a.zz[r] : 0.0;
    }
}

__device__ __forceinline__ void ent_codes_ctx(const EntArgs &a, int k0, EntTileCtx &x) {
    const int tx = (int)threadIdx.x & 15;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int k = k0 + 4 * tx + j;
        x.code[j] = k < a.K;
        x.ee[j] = x.code[j] ? a.ee[k] : 0.0;
    }
}

// l = -s ((zz + ee) - 2 dot)
__device__ __forceinline__ double ent_logit(const EntArgs &a, double zz, double ee, double dot) {
    const double d = (zz + ee) - 2.0 * dot;
    return -a.s * d;
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------

// workgroup = 64 rows; pass 1: the row maximum; pass 2: S = sum e^x, T = sum e^x x, x = l - max; lse = max + log S, H_n = log S - T / S
__device__ __forceinline__ void ent_row_fwd_body(const EntArgs &a, double *buf) {
    const int tx = (int)threadIdx.x & 15, ty = (int)threadIdx.x >> 4;
    const long long r0 = (long long)blockIdx.x * kEntTile;
    EntTileCtx x;
    ent_rows_ctx(a, r0, a.N, x);
    double dot[4][4], mx[4], S[4], T[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        mx[i] = -INFINITY;
        S[i] = 0.0;
        T[i] = 0.0;
    }
    for (int k0 = 0; k0 < a.K; k0 += kEntTile) {
        ent_dots(a.z, r0, a.e, k0, buf, dot);
        ent_codes_ctx(a, k0, x);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x.code[j]) mx[i] = fmax(mx[i], ent_logit(a, x.zz[i], x.ee[j], dot[i][j]));
    }
    ent_across_tx<true>(buf, mx);
    for (int k0 = 0; k0 < a.K; k0 += kEntTile) {
        ent_dots(a.z, r0, a.e, k0, buf, dot);
        ent_codes_ctx(a, k0, x);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (x.code[j]) {
                    const double v = ent_logit(a, x.zz[i], x.ee[j], dot[i][j]) - mx[i], e = exp(v);
                    S[i] = S[i] + e;
                    T[i] = T[i] + (e == 0.0 ? 0.0 : e * v);
                }
    }
    ent_across_tx<false>(buf, S);
    ent_across_tx<false>(buf, T);
    if (tx == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (x.row[i]) {
                const long long r = r0 + 4 * ty + i;
                const double ls = log(S[i]), lse = mx[i] + ls, h = ls - T[i] / S[i];
                a.rs[2 * r] = lse;
                a.rs[2 * r + 1] = h;
                if (a.rs_out) {
                    a.rs_out[2 * r] = lse;
                    a.rs_out[2 * r + 1] = h;
                }
            }
    }
}

// the 16 row classes' sums of a code, v[j] of thread (tx, ty) -> out[code] for the 64 codes, ascending ty from 0.0; red: 16 x 64
__device__ __forceinline__ void ent_across_ty(double *red, const double (&v)[4], double *out, int k0, int K) {
    const int t = (int)threadIdx.x, tx = t & 15, ty = t >> 4;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) red[ty * kEntTile + 4 * tx + j] = v[j];
    __syncthreads();
    if (t < kEntTile && k0 + t < K) {
        double s = 0.0;
        for (int q = 0; q < 16; ++q) s = s + red[q * kEntTile + t];
        out[k0 + t] = s;
    }
    __syncthreads();
}

// workgroup (x = partition, y = tile of 64 codes): avg's partial sums; in code tile 0 also the partition's sum of H_n
__device__ __forceinline__ void ent_avg_body(const EntArgs &a, double *buf) {
    const int t = (int)threadIdx.x, part = (int)blockIdx.x, k0 = (int)blockIdx.y * kEntTile;
    const long long r_begin = (long long)part * a.rows_per_part;
    const long long r_end = a.N - r_begin < a.rows_per_part ? a.N : r_begin + a.rows_per_part;
    EntTileCtx x;
    ent_codes_ctx(a, k0, x);
    double dot[4][4], acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (long long r0 = r_begin; r0 < r_end; r0 += kEntTile) {
        ent_dots(a.z, r0, a.e, k0, buf, dot);
        ent_rows_ctx(a, r0, r_end, x);
        const int ty = t >> 4;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (x.row[i]) {
                const double lse = a.rs[2 * (r0 + 4 * ty + i)];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (x.code[j]) {
                        acc[j] = acc[j] + exp(ent_logit(a, x.zz[i], x.ee[j], dot[i][j]) - lse);
                        }
            }
    }
    ent_across_ty(buf, acc, a.avg_part + (size_t)part * a.K, k0, a.K);
    if (blockIdx.y == 0) {                                                    // (uniform)
        double h = 0.0;
        for (long long r = r_begin + t; r < r_end; r += kEntThreads) h = h + a.rs[2 * r + 1];
        buf[t] = h;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (t < o) buf[t] += buf[t + o];
            __syncthreads();
        }
        if (t == 0) a.sc_part[part] = buf[0];
    }
}

// avg[k] = (partitions in ascending order, from 0.0) / N
__device__ __forceinline__ void ent_avg_reduce_body(const EntArgs &a) {
    const int k = (int)blockIdx.x * kEntThreads + (int)threadIdx.x;
    if (k >= a.K) return;
    double s = 0.0;
    for (int p = 0; p < a.P; ++p) s = s + a.avg_part[(size_t)p * a.K + k];
    a.avg[k] = s / (double)a.N;
}

// one workgroup: H (thread t: k = t, t + 256, ..; the fixed tree), P (the partitions in order), the three scalars
__device__ __forceinline__ void ent_finalize_body(const EntArgs &a, double *red) {
    const int t = (int)threadIdx.x;
    double hs = 0.0;
    for (int k = t; k < a.K; k += kEntThreads) {
        const double av = a.avg[k];
        hs = hs + (av == 0.0 ? 0.0 : av * log(av));
    }
    red[t] = hs;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    if (t == 0) {
        double sp = 0.0;
        for (int p = 0; p < a.P; ++p) sp = sp + a.sc_part[p];
        const double H = -red[0], P = sp / (double)a.N;
        a.losses[0] = (float)(P - a.gamma * H);
        a.losses[1] = (float)P;
        a.losses[2] = (float)H;
    }
}

// ---- backward --------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ void ent_logavg_body(const EntArgs &a) {
    const int k = (int)blockIdx.x * kEntThreads + (int)threadIdx.x;
    if (k >= a.K) return;
    const double av = a.avg[k];
    a.logavg[k] = av == 0.0 ? 0.0 : log(av);
}

// a_nk = (g / N) p [-(log p + H_n) + gamma (L_k - M_n)], log p = l - lse
__device__ __forceinline__ double ent_a(const EntArgs &a, double gn, double l, double lse, double hn, double L, double M) {
    const double lp = l - lse, p = exp(lp);
    const double br = -(lp + hn) + a.gamma * (L - M);
    return (gn * p) * br;
}

// workgroup = 64 rows.  Pass A: M_n = sum_k p_nk L_k.  Pass B (WANT_Z): per code tile the a_nk go to the w tile (code-major), their
// row sums A_n to registers, and G_nc = sum_k a_nk e_kc to the second contraction; grad_z_nc = float(-2 s (z_nc A_n - G_nc)).
template <int DT, bool WANT_Z>
__device__ __forceinline__ void ent_row_bwd_body(const EntArgs &a, double *buf, double *w) {
    const int tx = (int)threadIdx.x & 15, ty = (int)threadIdx.x >> 4;
    const long long r0 = (long long)blockIdx.x * kEntTile;
    EntTileCtx x;
    ent_rows_ctx(a, r0, a.N, x);
    double dot[4][4], lse[4], hn[4], M[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const long long r = r0 + 4 * ty + i;
        lse[i] = x.row[i] ? a.rs[2 * r] : 0.0;
        hn[i] = x.row[i] ? a.rs[2 * r + 1] : 0.0;
        M[i] = 0.0;
    }
    for (int k0 = 0; k0 < a.K; k0 += kEntTile) {
        ent_dots(a.z, r0, a.e, k0, buf, dot);
        ent_codes_ctx(a, k0, x);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (x.code[j]) {
                const double L = a.logavg[k0 + 4 * tx + j];
#pragma unroll
                for (int i = 0; i < 4; ++i) M[i] = M[i] + exp(ent_logit(a, x.zz[i], x.ee[j], dot[i][j]) - lse[i]) * L;
            }
    }
    ent_across_tx<false>(buf, M);
    if (tx == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (x.row[i]) a.m[r0 + 4 * ty + i] = M[i];
    }
    if (!WANT_Z) return;
    const double gn = (a.gl ? (double)*a.gl : 1.0) / (double)a.N;
    double A[4] = {0.0, 0.0, 0.0, 0.0}, acc[4][DT / 16];
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
        for (int c = 0; c < DT / 16; ++c) acc[o][c] = 0.0;
    for (int k0 = 0; k0 < a.K; k0 += kEntTile) {
        ent_dots(a.z, r0, a.e, k0, buf, dot);
        ent_codes_ctx(a, k0, x);
        __syncthreads();                                                      // the last contraction has read w
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double L = x.code[j] ? a.logavg[k0 + 4 * tx + j] : 0.0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                double v = 0.0;
                if (x.code[j] && x.row[i]) v = ent_a(a, gn, ent_logit(a, x.zz[i], x.ee[j], dot[i][j]), lse[i], hn[i], L, M[i]);
                A[i] = A[i] + v;
                w[(4 * tx + j) * kEntStride + 4 * ty + i] = v;
            }
        }
        ent_contract2<DT>(w, a.e, k0, buf, acc);
    }
    ent_across_tx<false>(buf, A);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (!x.row[i]) continue;
        const long long r = r0 + 4 * ty + i;
#pragma unroll
        for (int q = 0; q < DT / 64; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int c = 64 * q + 4 * tx + e;
                if (c < a.D) {
                    const size_t at = ent_index(a.z, r, c);
                    const double zc = (double)a.z.p[at];
                    a.grad_z[at] = (float)((-2.0 * a.s) * (zc * A[i] - acc[i][4 * q + e]));
                }
            }
    }
}

// workgroup (x = partition, y = tile of 64 codes): the partials of sum_n a_nk z_nc (P, K, D) and of sum_n a_nk (P, K)
template <int DT>
__device__ __forceinline__ void ent_grad_e_body(const EntArgs &a, double *buf, double *w) {
    const int t = (int)threadIdx.x, tx = t & 15, ty = t >> 4, part = (int)blockIdx.x, k0 = (int)blockIdx.y * kEntTile;
    const long long r_begin = (long long)part * a.rows_per_part;
    const long long r_end = a.N - r_begin < a.rows_per_part ? a.N : r_begin + a.rows_per_part;
    const double gn = (a.gl ? (double)*a.gl : 1.0) / (double)a.N;
    EntTileCtx x;
    ent_codes_ctx(a, k0, x);
    double L[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) L[j] = x.code[j] ? a.logavg[k0 + 4 * tx + j] : 0.0;
    double dot[4][4], As[4] = {0.0, 0.0, 0.0, 0.0}, acc[4][DT / 16];
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
        for (int c = 0; c < DT / 16; ++c) acc[o][c] = 0.0;
    EntSrc zr = a.z;
    zr.n = r_end;                                                             // rows past the partition are staged as 0.0
    for (long long r0 = r_begin; r0 < r_end; r0 += kEntTile) {
        ent_dots(zr, r0, a.e, k0, buf, dot);
        ent_rows_ctx(a, r0, r_end, x);
        __syncthreads();                                                      // the last contraction has read w
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long long r = r0 + 4 * ty + i;
            const double lse = x.row[i] ? a.rs[2 * r] : 0.0, hn = x.row[i] ? a.rs[2 * r + 1] : 0.0, M = x.row[i] ? a.m[r] : 0.0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                double v = 0.0;
                if (x.code[j] && x.row[i]) v = ent_a(a, gn, ent_logit(a, x.zz[i], x.ee[j], dot[i][j]), lse, hn, L[j], M);
                As[j] = As[j] + v;
                w[(4 * ty + i) * kEntStride + 4 * tx + j] = v;
            }
        }
        ent_contract2<DT>(w, zr, r0, buf, acc);
    }
    ent_across_ty(buf, As, a.as_part + (size_t)part * a.K, k0, a.K);
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const int k = k0 + 4 * ty + o;
        if (k >= a.K) continue;
#pragma unroll
        for (int q = 0; q < DT / 64; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int c = 64 * q + 4 * tx + e;
                if (c < a.D) a.ge_part[((size_t)part * a.K + k) * a.D + c] = acc[o][4 * q + e];
            }
    }
}

// grad_E_kc = float(2 s (sum_p part_kc - e_kc sum_p as_k)), the partitions in ascending order from 0.0: one thread per element
__device__ __forceinline__ void ent_grad_e_reduce_body(const EntArgs &a) {
    const long long q = (long long)blockIdx.x * kEntThreads + threadIdx.x, n = (long long)a.K * a.D;
    if (q >= n) return;
    const int k = (int)(q / a.D);
    double s = 0.0, as = 0.0;
    for (int p = 0; p < a.P; ++p) {
        s = s + a.ge_part[(size_t)p * n + q];
        as = as + a.as_part[(size_t)p * a.K + k];
    }
    a.grad_e[q] = (float)((2.0 * a.s) * (s - (double)a.e.p[q] * as));
}

// ---- the partitions of the rows: whole blocks of 256 rows, at most `pmax` partitions.  Functions of (N, K, D) alone ----------------

inline void ent_partition(long long N, long long pmax, long long &rows_per_part, int &P) {
    const long long blocks = (N + kEntBlockRows - 1) / kEntBlockRows, bpp = (blocks + pmax - 1) / pmax;
    rows_per_part = bpp * kEntBlockRows;
    P = (int)((blocks + bpp - 1) / bpp);
}

// avg: at most max(16, min(256, 2^20 / K)) partitions: the (P, K) partials take at most 8 MiB (LFQ's rule with a lower cap: the
// second launch adds a code's partitions one after the other)
inline void ent_partition_avg(long long N, int K, long long &rows_per_part, int &P) {
    long long pmax = (1LL << 20) / K;
    pmax = pmax < 16 ? 16 : (pmax > 256 ? 256 : pmax);
    ent_partition(N, pmax, rows_per_part, P);
}

// grad_E: at most max(1, min(1024, 2^22 / (K D))) partitions: the (P, K, D) partials take at most 32 MiB
inline void ent_partition_grad(long long N, int K, int D, long long &rows_per_part, int &P) {
    long long pmax = (1LL << 22) / ((long long)K * D);
    pmax = pmax < 1 ? 1 : (pmax > 1024 ? 1024 : pmax);
    ent_partition(N, pmax, rows_per_part, P);
}

}  // namespace vqvae
