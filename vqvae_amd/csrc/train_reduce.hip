// What the training translation units share (train_reduce.h), gfx950: the sorted segmented sum, the second stage of the weight
// and bias gradients, and vqvae_train_reduction_plan.  No floating-point atomics: every sum has a fixed order.
#include <hipcub/hipcub.hpp>

#include "train_reduce.h"

namespace vqvae {

SegsumPlan segsum_plan(long long n, int nkeys, int C) {
    SegsumPlan p;
    p.key_bits = 1;
    while ((1LL << p.key_bits) < nkeys) ++p.key_bits;
    p.off_keys = 0;
    p.off_keys_out = align_up(p.off_keys + (size_t)n * 4, 256);
    p.off_vals = align_up(p.off_keys_out + (size_t)n * 4, 256);
    p.off_vals_out = align_up(p.off_vals + (size_t)n * 4, 256);
    p.off_offsets = align_up(p.off_vals_out + (size_t)n * 4, 256);
    p.off_units = align_up(p.off_offsets + (size_t)(nkeys + 1) * 4, 256);
    p.max_units = n / kSegChunk + nkeys;                   // sum_k ceil(count_k / chunk) <= n / chunk + nkeys
    p.off_partials = align_up(p.off_units + (size_t)(nkeys + 1) * 4, 256);
    p.off_sort = align_up(p.off_partials + (size_t)p.max_units * C * sizeof(double), 256);
    size_t sb = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, sb, (const unsigned *)nullptr, (unsigned *)nullptr,
                                             (const int *)nullptr, (int *)nullptr, (int)n, 0, p.key_bits, 0);
    p.sort_bytes = sb;
    p.total = align_up(p.off_sort + sb, 256);
    return p;
}

// keys = the index of each row, clamped into [0, nkeys) (as gather_rows_kernel clamps in the forward); vals = the row itself
__global__ __launch_bounds__(256) void segsum_keys_kernel(const long long *__restrict__ idx, long long n, int nkeys,
                                                          unsigned *__restrict__ keys, int *__restrict__ vals) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const long long k = idx[i];
        keys[i] = (unsigned)(k < 0 ? 0 : (k >= nkeys ? nkeys - 1 : k));
        vals[i] = (int)i;
    }
}

// offsets[k] = first sorted position whose key is >= k (k = 0 .. nkeys): one binary search per key
__global__ __launch_bounds__(256) void segsum_offsets_kernel(const unsigned *__restrict__ keys, long long n, int nkeys,
                                                             int *__restrict__ offsets) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k > nkeys) return;
    long long lo = 0, hi = n;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (keys[mid] < (unsigned)k) lo = mid + 1; else hi = mid;
    }
    offsets[k] = (int)lo;
}

// unit_start[k] = number of units (chunks of kSegChunk sorted rows) owned by keys < k; one block scans nkeys + 1
__global__ __launch_bounds__(1024) void segsum_units_kernel(const int *__restrict__ offsets, int nkeys, int *__restrict__ unit_start) {
    __shared__ int part[1024];
    const int tid = threadIdx.x;
    const int per = (nkeys + 1023) / 1024;
    int local = 0;
    for (int j = 0; j < per; ++j) {
        const int k = tid * per + j;
        if (k < nkeys) local += (offsets[k + 1] - offsets[k] + kSegChunk - 1) / kSegChunk;
    }
    part[tid] = local;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {                    // inclusive scan
        const int v = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int run = part[tid] - local;                             // exclusive prefix of this thread's keys
    for (int j = 0; j < per; ++j) {
        const int k = tid * per + j;
        if (k < nkeys) {
            unit_start[k] = run;
            run += (offsets[k + 1] - offsets[k] + kSegChunk - 1) / kSegChunk;
        }
    }
    if (tid == 1023) unit_start[nkeys] = part[1023];
}

// partial[unit][c] = sum over the unit's (<= kSegChunk, ascending) rows of src[row][c]   (fp64, fixed order).
// C <= 256: threads [0, G C) are G = 256 / C row groups, group g adds rows a + g, a + g + G, ... and the groups are combined in
// group order; wider rows: one group, channels in 256-wide passes.  Four rows' (index, value) loads in flight either way.
__global__ __launch_bounds__(256) void segsum_kernel(const float *__restrict__ src, const int *__restrict__ rows,
                                                     const int *__restrict__ offsets, const int *__restrict__ unit_start,
                                                     int nkeys, int C, int HW, int rowmajor, double *__restrict__ partial) {
    __shared__ double red[256];
    const int unit = blockIdx.x, tid = threadIdx.x;
    if (unit >= unit_start[nkeys]) return;
    int lo_k = 0, hi_k = nkeys;                              // last k with unit_start[k] <= unit
    while (hi_k - lo_k > 1) {
        const int mid = (lo_k + hi_k) >> 1;
        if (unit_start[mid] <= unit) lo_k = mid; else hi_k = mid;
    }
    const int k = lo_k;
    const int a = offsets[k] + (unit - unit_start[k]) * kSegChunk;
    const int b = a + kSegChunk < offsets[k + 1] ? a + kSegChunk : offsets[k + 1];
    // rows j0, j0 + step, ... < b of channel c, in that order
    auto sum_rows = [&](int j0, int step, int c) {
        auto at = [&](long long r) {
            if (rowmajor) return src[(size_t)r * C + c];
            const long long bb = r / HW;
            const int hw = (int)(r - bb * HW);
            return src[((size_t)bb * C + c) * HW + hw];
        };
        double acc = 0.0;
        int j = j0;
        for (; j + 3 * step < b; j += 4 * step) {
            long long r[4];
            float v[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) r[q] = rows[j + q * step];
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = at(r[q]);
#pragma unroll
            for (int q = 0; q < 4; ++q) acc += (double)v[q];
        }
        for (; j < b; j += step) acc += (double)at(rows[j]);
        return acc;
    };
    if (C > 256) {
        for (int c = tid; c < C; c += 256) partial[(size_t)unit * C + c] = sum_rows(a, 1, c);
        return;
    }
    const int G = 256 / C;
    const int g = tid / C, c = tid - g * C;
    red[tid] = g < G ? sum_rows(a + g, G, c) : 0.0;
    __syncthreads();
    if (tid < C) {
        double t = 0.0;
        for (int q = 0; q < G; ++q) t += red[q * C + tid];
        partial[(size_t)unit * C + tid] = t;
    }
}

hipError_t launch_segsum(const SegsumPlan &p, const float *src, const long long *idx, long long n, int nkeys, int C, int HW,
                         int rowmajor, char *ws, hipStream_t st) {
    unsigned *keys = reinterpret_cast<unsigned *>(ws + p.off_keys);
    unsigned *keys_out = reinterpret_cast<unsigned *>(ws + p.off_keys_out);
    int *vals = reinterpret_cast<int *>(ws + p.off_vals);
    int *vals_out = reinterpret_cast<int *>(ws + p.off_vals_out);
    int *offsets = reinterpret_cast<int *>(ws + p.off_offsets);
    int *unit_start = reinterpret_cast<int *>(ws + p.off_units);
    double *partial = reinterpret_cast<double *>(ws + p.off_partials);
    hipLaunchKernelGGL(segsum_keys_kernel, dim3(grid_of(n, 4096)), dim3(256), 0, st, idx, n, nkeys, keys, vals);
    size_t sb = p.sort_bytes;
    hipError_t e = hipcub::DeviceRadixSort::SortPairs(ws + p.off_sort, sb, keys, keys_out, vals, vals_out, (int)n, 0,
                                                      p.key_bits, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(segsum_offsets_kernel, dim3((unsigned)((nkeys + 1 + 255) / 256)), dim3(256), 0, st, keys_out, n, nkeys, offsets);
    hipLaunchKernelGGL(segsum_units_kernel, dim3(1), dim3(1024), 0, st, offsets, nkeys, unit_start);
    hipLaunchKernelGGL(segsum_kernel, dim3((unsigned)p.max_units), dim3(256), 0, st, src, vals_out, offsets, unit_start, nkeys, C,
                       HW, rowmajor, partial);
    return hipSuccess;
}

// dW[ca][cb][tap] = sum_split partial[split][tap][ca][cb]   (fixed order)
__global__ __launch_bounds__(256) void split_reduce_kernel(const float *__restrict__ partial, int nsplit, int ntap, int CA, int CB,
                                                           float *__restrict__ dw) {
    const long long total = (long long)ntap * CA * CB;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        // eight interleaved running sums (loads in flight instead of one dependent add per load), combined in a fixed order
        float s8[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        int sp = 0;
        for (; sp + 8 <= nsplit; sp += 8)
#pragma unroll
            for (int j = 0; j < 8; ++j) s8[j] += partial[(size_t)(sp + j) * total + e];
        for (int j = 0; sp < nsplit; ++sp, ++j) s8[j] += partial[(size_t)sp * total + e];
        const float s = ((s8[0] + s8[1]) + (s8[2] + s8[3])) + ((s8[4] + s8[5]) + (s8[6] + s8[7]));
        const int tap = (int)(e / ((long long)CA * CB));
        const long long rem = e - (long long)tap * CA * CB;          // ca * CB + cb
        dw[rem * ntap + tap] = s;
    }
}

void launch_split_reduce(const float *partial, int nsplit, int ntap, int CA, int CB, float *dw, hipStream_t st) {
    hipLaunchKernelGGL(split_reduce_kernel, dim3(grid_of((long long)ntap * CA * CB, 4096)), dim3(256), 0, st, partial, nsplit, ntap,
                       CA, CB, dw);
}

// one workgroup per channel: strided sums over the block partials, then a fixed tree
__global__ __launch_bounds__(256) void colsum_final_kernel(const double *__restrict__ partial, int nblocks, int C,
                                                           float *__restrict__ db) {
    __shared__ double red[256];
    const int c = blockIdx.x, tid = threadIdx.x;
    double s = 0.0;
    for (int b = tid; b < nblocks; b += 256) s += partial[(size_t)b * C + c];
    block_sum_f64(red, tid, s);
    if (tid == 0) db[c] = (float)red[0];
}

void launch_colsum_final(const double *partial, int nblocks, int C, float *db, hipStream_t st) {
    hipLaunchKernelGGL(colsum_final_kernel, dim3((unsigned)C), dim3(256), 0, st, partial, nblocks, C, db);
}

}  // namespace vqvae

using namespace vqvae;

extern "C" int vqvae_train_reduction_plan(int what, const int64_t *dims, int ndims, int64_t *out) {
    if (!dims || !out) return VQVAE_ERR_NULL;
    for (int i = 0; i < ndims; ++i)
        if (dims[i] < INT32_MIN || dims[i] > INT32_MAX) return VQVAE_ERR_OVERFLOW;
    const auto d = [&](int i) { return (int)dims[i]; };
    const auto positive = [&](int n) {                       // dims[0 .. n) exist and are >= 1
        for (int i = 0; i < n; ++i)
            if (i >= ndims || dims[i] < 1) return false;
        return true;
    };
    ReducePlan p;
    if (what == VQVAE_TRAIN_PLAN_CONV_WGRAD) {
        if (ndims != 12 || !positive(9) || d(9) < 0) return VQVAE_ERR_SHAPE;
        if (d(7) > 4 || (d(11) & ~VQVAE_CONV_EXACT_FP32)) return VQVAE_ERR_UNSUPPORTED;
        p = conv_wgrad_plan(d(0), d(1), d(2), d(3), d(4), d(5), d(6), d(7), d(8), d(9), d(10), d(11));
    } else if (what == VQVAE_TRAIN_PLAN_CONV_TAPS_WGRAD) {
        if (!positive(6) || d(5) > 32 || ndims != 6 + 2 * d(5)) return VQVAE_ERR_SHAPE;
        if (d(3) % 4 || d(4) % 4) return VQVAE_ERR_UNSUPPORTED;
        int8_t dy[32], dx[32];
        for (int i = 0; i < d(5); ++i) {
            const int y = d(6 + i), x = d(6 + d(5) + i);
            if (y < -7 || y > 7 || x < -7 || x > 7) return VQVAE_ERR_UNSUPPORTED;
            dy[i] = (int8_t)y;
            dx[i] = (int8_t)x;
        }
        const int rc = conv_taps_wgrad_plan(d(0), d(1), d(2), d(3), d(4), d(5), dy, dx, p);
        if (rc != VQVAE_OK) return rc;
    } else if (what == VQVAE_TRAIN_PLAN_BIAS_GRAD || what == VQVAE_TRAIN_PLAN_BIAS_GRAD_WIDE) {
        if (ndims != 2 || !positive(2)) return VQVAE_ERR_SHAPE;
        const bool wide = what == VQVAE_TRAIN_PLAN_BIAS_GRAD_WIDE;
        if (!wide && d(1) > 256) return VQVAE_ERR_UNSUPPORTED;
        p = wide ? bias_grad_wide_plan(d(0)) : bias_grad_plan(d(0));
    } else if (what == VQVAE_TRAIN_PLAN_SEGSUM) {
        if (ndims != 3 || !positive(3)) return VQVAE_ERR_SHAPE;
        if (d(1) > (1 << 24)) return VQVAE_ERR_OVERFLOW;
        p = segsum_reduce_plan(segsum_plan(d(0), d(1), d(2)), d(0));
    } else {
        return VQVAE_ERR_UNSUPPORTED;
    }
    const long long v[8] = {p.kernel, p.items, p.splits, p.per_split, p.last(), p.want, p.aux0, p.aux1};
    for (int i = 0; i < 8; ++i) out[i] = v[i];
    return VQVAE_OK;
}
