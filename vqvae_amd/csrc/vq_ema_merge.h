// The split EMA codebook update (vq_ema_merge.hip, whose header states the arithmetic): the whole bodies of the pack kernel and of
// the two apply kernels.  Plain C++ over `__device__ __forceinline__`, so that tests/host/ema_merge_harness.cpp compiles THIS text
// for the host (blockIdx / threadIdx and __syncthreads supplied by the harness) and compares it with the restatement bit for bit
// under the sanitizers.  The per-code sum of the shard's rows is formed by the caller (segsum_key_sum, train_reduce.h) and handed
// to the pack body as a value: the body owns the record's layout, the counts and the candidate gather.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

namespace vqvae {

constexpr int kEmaMergeThreads = 256;          // threads of the pack and of the update kernel
constexpr int kEmaCountThreads = 1024;         // threads of the one workgroup that forms N_k and n (vqe_counts_kernel's shape)
constexpr int kEmaMergeMaxR = 1024;            // shards one apply takes

// floor(u * n) clamped into [0, n - 1]: the restart row of a shard of n rows, the shard of R shards
__device__ __forceinline__ long long ema_pick(float u, long long n) {
    long long r = (long long)floor((double)u * (double)n);
    return r < 0 ? 0 : (r > n - 1 ? n - 1 : r);
}

// which field of a record column c is: 0 the count, 1 a sum (channel c - 1), 2 a candidate (channel c - D - 1)
__device__ __forceinline__ int ema_stats_field(int c, int D) { return c == 0 ? 0 : (c <= D ? 1 : 2); }

// stats[k][c] of one shard, one thread per element e = k C + c (c across the lanes: the stores coalesce, and so do the reads of the
// units' partials in front of this body).  `sum`: segsum_key_sum of (k, c - 1) for a sum column, unused otherwise.
__device__ __forceinline__ void ema_pack_body(long long e, double sum, const int *offsets, const float *z, const float *row_uniforms,
                                              long long N, int K, int D, int C, int HW, int rowmajor, double *stats) {
    if (e >= (long long)K * C) return;
    const int k = (int)(e / C), c = (int)(e - (long long)k * C);
    const int field = ema_stats_field(c, D);
    double v;
    if (field == 0) {
        v = (double)(offsets[k + 1] - offsets[k]);
    } else if (field == 1) {
        v = sum;
    } else {
        const long long r = ema_pick(row_uniforms[k], N);
        const int ch = c - D - 1;
        if (rowmajor) {
            v = (double)z[(size_t)r * D + ch];
        } else {
            const long long bb = r / HW;
            const int hw = (int)(r - bb * HW);
            v = (double)z[((size_t)bb * D + ch) * HW + hw];
        }
    }
    stats[e] = v;
}

// c_k = sum over the shards of their counts (exact integers: any order gives the same double), N_k <- decay N_k + (1 - decay) c_k
// kept unrounded in nk[], n = sum_k N_k in vqe_counts_kernel's order (contiguous codes per thread, then its tree over part[1024]).
// One workgroup of kEmaCountThreads threads: K <= 16384.
__device__ __forceinline__ void ema_count_body(const double *stats, int R, int K, int C, const float *cluster_size, double decay,
                                               double *nk, double *n_total, double *part) {
    const int tid = (int)threadIdx.x;
    const int per = (K + kEmaCountThreads - 1) / kEmaCountThreads;
    double local = 0.0;
    for (int j = 0; j < per; ++j) {
        const int k = tid * per + j;
        if (k < K) {
            double cnt = stats[(size_t)k * C];
            for (int s = 1; s < R; ++s) cnt += stats[((size_t)s * K + k) * C];
            const double v = decay * (double)cluster_size[k] + (1.0 - decay) * cnt;
            nk[k] = v;
            local += v;
        }
    }
    part[tid] = local;
    __syncthreads();
    for (int o = kEmaCountThreads / 2; o > 0; o >>= 1) {
        if (tid < o) part[tid] += part[tid + o];
        __syncthreads();
    }
    if (tid == 0) *n_total = part[0];
}

// One thread per (k, c), c across the lanes so that the R reads of stats[s][k][1 + c] coalesce: S = ((s_0 + s_1) + ...) in shard
// order from shard 0's value itself, m <- decay m + (1 - decay) S, then e_k = m / ((N_k + eps) / (n + K eps) n), or, with restart on
// and N_k < threshold, the candidate of shard j_k = ema_pick(v_k, R).  vqe_update_kernel's operations in its order, in fp64, one
// rounding per store.  Reads only stats / nk / n_total / ema_w: codebook may be any buffer of K x D floats apart from them.
__device__ __forceinline__ void ema_apply_body(long long e, const double *stats, int R, int K, int D, int C, const double *nk,
                                               const double *n_total, const float *shard_uniforms, double decay, double eps,
                                               double threshold, float *cluster_size, float *ema_w, float *codebook) {
    if (e >= (long long)K * D) return;
    const int k = (int)(e / D), c = (int)(e - (long long)k * D);
    const size_t shard = (size_t)K * C, at = (size_t)k * C + 1 + c;
    double s = stats[at];
    for (int j = 1; j < R; ++j) s += stats[(size_t)j * shard + at];
    const double m = decay * (double)ema_w[e] + (1.0 - decay) * s;
    const double Nk = nk[k];
    double ek;
    if (shard_uniforms && Nk < threshold) {
        const long long j = ema_pick(shard_uniforms[k], R);
        ek = stats[(size_t)j * shard + at + D];
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
