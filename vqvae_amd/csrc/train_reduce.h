// What the training translation units (backward.hip, train.hip, pixelcnn_backward.hip) share: the plan every batch-dependent
// reduction is launched from, and the launchers of the kernels that exist once, in train_reduce.hip.
#pragma once

#include "common.h"

namespace vqvae {

// ---- one plan per reduction: read by the launcher, by the *_workspace_bytes query and by vqvae_train_reduction_plan -------------
// A reduction cuts `items` (images, 32-pixel blocks, rows) into `splits` ranges of `per_split` items, one partial sum each.
struct ReducePlan {
    int kernel = 0;                   // VQVAE_TRAIN_KERNEL_*: which kernel runs
    long long items = 0;              // what is split: images (map / image-operand kernels), 32-pixel blocks, rows
    long long want = 0;               // the split count the rule asks for before its clamps to a cap and to the items
    long long splits = 0, per_split = 0;
    int aux0 = 0, aux1 = 0;           // map8: waves along (ca, cb); taps map: tap groups, taps per group; segmented sum: chunk, max units
    long long last() const {          // items of the last split (0: an empty one, conv_wgrad_kernel's plan only)
        const long long before = (splits - 1) * per_split;
        return items - (before < items ? before : items);
    }
};

// ranges of ceil(items / want') items, want' = want clamped into [1, cap]; the split count follows from the range
inline void plan_ranges(ReducePlan &p, long long cap) {
    long long ns = p.want < cap ? p.want : cap;
    if (ns < 1) ns = 1;
    p.per_split = (p.items + ns - 1) / ns;
    p.splits = (p.items + p.per_split - 1) / p.per_split;
}

// backward.hip: vqvae_conv_wgrad_ex_f32
ReducePlan conv_wgrad_plan(long long B, int HA, int WA, int CA, int HB, int WB, int CB, int k, int stride, int pad, int bt_nchw,
                           int flags);
// pixelcnn_backward.hip: vqvae_conv_taps_wgrad_f32 (VQVAE_ERR_* when the taps are out of range)
int conv_taps_wgrad_plan(long long B, int H, int W, int Cin, int Cout, int ntaps, const int8_t *dy, const int8_t *dx, ReducePlan &p);

// column sums (vqvae_bias_grad_f32: at least 1024 rows per block; vqvae_bias_grad_wide_f32: 64), never more than kColsumBlocks blocks
constexpr int kColsumBlocks = 512;
inline ReducePlan colsum_plan(long long P, int min_rows, int kernel) {
    ReducePlan p;
    p.kernel = kernel;
    p.items = P;
    p.want = (P + min_rows - 1) / min_rows;
    plan_ranges(p, kColsumBlocks);
    return p;
}
inline ReducePlan bias_grad_plan(long long P) { return colsum_plan(P, 1024, VQVAE_TRAIN_KERNEL_BIAS_GRAD); }
inline ReducePlan bias_grad_wide_plan(long long P) { return colsum_plan(P, 64, VQVAE_TRAIN_KERNEL_BIAS_GRAD_WIDE); }

// ---- sorted segmented sum --------------------------------------------------------------------------------------------------------
// partial[unit][c] = sum over the unit's rows of src[row][c] in fp64: rows are sorted by key (keys clamped into [0, nkeys); stable
// radix sort, so ascending inside a key), a key owns ceil(count / kSegChunk) units of consecutive sorted rows, and a unit is added
// in a fixed order.  No floating-point atomics; the work follows the rows however skewed the histogram.  The callers combine a
// key's units themselves (unit_start[k] .. unit_start[k + 1]), each in its own order.
constexpr int kSegChunk = 512;

struct SegsumPlan {
    size_t off_keys, off_keys_out, off_vals, off_vals_out, off_offsets, off_units, off_partials, off_sort, sort_bytes, total;
    long long max_units;              // n / kSegChunk + nkeys >= sum_k ceil(count_k / kSegChunk): the grid and the partials' size
    int key_bits;
};
SegsumPlan segsum_plan(long long n, int nkeys, int C);
inline ReducePlan segsum_reduce_plan(const SegsumPlan &s, long long n) {     // the launch in the terms of the other reductions
    ReducePlan p;
    p.kernel = VQVAE_TRAIN_KERNEL_SEGSUM;
    p.items = n;
    p.want = p.splits = s.max_units;
    p.per_split = p.aux0 = kSegChunk;
    p.aux1 = (int)s.max_units;
    return p;
}
// src: n rows of C floats, row-major, or NCHW images of HW pixels (rowmajor == 0: row r is pixel r % HW of image r / HW)
hipError_t launch_segsum(const SegsumPlan &p, const float *src, const long long *idx, long long n, int nkeys, int C, int HW,
                         int rowmajor, char *ws, hipStream_t st);

// A key's sum of channel c from its units' partials, in the ONE order every caller combines them (part of their numeric contracts:
// vqvae_vq_backward_f32, vqvae_vq_ema_update_f32, vqvae_vq_kmeans_update_f32, vqvae_vq_residual_backward_f32): four interleaved
// running sums over the units (a key that owns many rows has many units: their loads are in flight together instead of one
// dependent add per load), then (s0 + s1) + (s2 + s3).
__device__ __forceinline__ double segsum_key_sum(const int *__restrict__ unit_start, const double *__restrict__ partial, int k, int c,
                                                 int C) {
    double z4[4] = {0.0, 0.0, 0.0, 0.0};
    int u = unit_start[k];
    const int u1 = unit_start[k + 1];
    for (; u + 4 <= u1; u += 4)
#pragma unroll
        for (int j = 0; j < 4; ++j) z4[j] += partial[(size_t)(u + j) * C + c];
    for (int j = 0; u < u1; ++u, ++j) z4[j] += partial[(size_t)u * C + c];
    return (z4[0] + z4[1]) + (z4[2] + z4[3]);
}

// ---- the second stage of the split reductions -------------------------------------------------------------------------------------
// dw[ca][cb][tap] = sum_split partial[split][tap][ca][cb], eight interleaved sums combined in a fixed order
void launch_split_reduce(const float *partial, int nsplit, int ntap, int CA, int CB, float *dw, hipStream_t st);
// db[c] = sum_block partial[block][c]: one workgroup per channel, strided fp64 sums and a fixed tree
void launch_colsum_final(const double *partial, int nblocks, int C, float *db, hipStream_t st);

}  // namespace vqvae
