// The orthogonal regularization loss of a codebook (vq_orthogonal.hip, whose header states the arithmetic): the whole bodies of the
// kernels.  Plain C++ over `__device__ __forceinline__`, so that tests/host/orthogonal_harness.cpp compiles THIS text for the host
// (blockIdx / threadIdx, f32x4 and __syncthreads supplied by the harness) and compares it with the restatement bit for bit under
// the sanitizers.
//
// The main kernel: a workgroup of 256 threads owns kOrthRows = 16 rows i and walks the codebook in tiles of kOrthTile = 32 codes j,
// in ascending order.  Per tile: the tile's rows are staged in LDS as they lie in memory (fp32, rows DT + 4 dwords apart, columns
// D .. Dp - 1 of a width that is no multiple of 4 filled with zeros); the 16 x 32 Gram entries are formed cooperatively, two per
// thread, each one fp64 chain over the columns in ascending order, and left in LDS; then every thread adds the tile's selected codes,
// in ascending j, to the RI x 4 slice of V and the RI row sums it keeps in registers.  The order per (i, c) is "ascending j"
// whatever the block height, so the height is a launch choice.  Zero columns add fma(0, 0, s) = s to a sum that is never -0.0
// (it starts from +0.0, and x + (-x) = +0.0): the padding leaves every bit as it is.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace vqvae {

constexpr int kOrthThreads = 256;                            // threads of every kernel here
constexpr int kOrthRows = 16;                                // rows i of one workgroup of the main kernel
constexpr int kOrthTile = 32;                                // codes j staged per step
constexpr int kOrthSumBlock = 256;                           // the contract's block of the total: 256 consecutive codes
constexpr int kOrthMaxK = 16384;
constexpr int kOrthMaxD = 256;
constexpr int kOrthSumBlocks = kOrthMaxK / kOrthSumBlock;    // 64: one thread of the last kernel each

struct OrthArgs {
    const float *rows;                                       // (K, D)
    const int32_t *selected;                                 // (K) 0 / 1, written by the launch before
    double *r;                                               // (K): R_i, 0.0 for an unselected row
    double *v;                                               // (K, D): V, 0.0 in unselected rows; or NULL
    int K, D;
};

// selected[k]: a candidate (hist NULL or hist[k] > 0) that, under a cap, has fewer than max_codes candidates in front of it in the
// order (u ascending, then k ascending).  With no more candidates than the cap every rank is below it: one rule for both cases.
__device__ __forceinline__ void orth_select_body(const int32_t *hist, const float *u, int max_codes, int K, int32_t *selected) {
    const int k = (int)blockIdx.x * kOrthThreads + (int)threadIdx.x;
    if (k >= K) return;
    const bool cand = !hist || hist[k] > 0;
    int s = cand ? 1 : 0;
    if (cand && u && max_codes > 0) {
        const float uk = u[k];
        int rank = 0;
        for (int j = 0; j < K; ++j) {
            const bool cj = !hist || hist[j] > 0;
            const float uj = u[j];
            rank += (cj && (uj < uk || (uj == uk && j < k))) ? 1 : 0;
        }
        s = rank < max_codes ? 1 : 0;
    }
    selected[k] = s;
}

// rows r0 .. r0 + nr - 1 -> tile (S dwords between rows), zeros for a row past K and for columns D .. Dp - 1; a wave takes every
// fourth row, 16 bytes per lane where the rows allow it (vec: D % 4 == 0 and a 16-byte aligned pointer), else one element
template <int S>
__device__ __forceinline__ void orth_stage(const OrthArgs &a, int Dp, bool vec, int r0, int nr, float *tile) {
    const int lane = (int)threadIdx.x & 63;
    for (int r = (int)threadIdx.x >> 6; r < nr; r += kOrthThreads / 64) {
        const int k = r0 + r;
        const bool in = k < a.K;
        const float *src = a.rows + (size_t)(in ? k : 0) * a.D;
        if (vec) {
            for (int c = 4 * lane; c < a.D; c += 256) {
                f32x4 x = {0.f, 0.f, 0.f, 0.f};
                if (in) x = *reinterpret_cast<const f32x4 *>(src + c);
                *reinterpret_cast<f32x4 *>(tile + r * S + c) = x;
            }
        } else {
            for (int c = lane; c < Dp; c += 64) tile[r * S + c] = (in && c < a.D) ? src[c] : 0.f;
        }
    }
}

// DT: the width class (64, 128 or 256 >= D).  CT threads side by side own four columns each, RT thread rows own RI rows each.
template <int DT, bool WANT_V>
__device__ __forceinline__ void orth_main_body(const OrthArgs &a, float *ni, float *nj, double *g, int *selj) {
    constexpr int CT = DT / 4, RT = kOrthThreads / CT, RI = kOrthRows / RT, S = DT + 4;
    static_assert(RI >= 1 && RI * RT == kOrthRows, "the thread grid covers the block's rows");
    const int t = (int)threadIdx.x, i0 = (int)blockIdx.x * kOrthRows;
    const int Dp = (a.D + 3) & ~3;
    const bool vec = !(a.D & 3) && !(reinterpret_cast<uintptr_t>(a.rows) & 15);
    const int cg = t % CT, rg = t / CT;
    const bool active = 4 * cg < Dp;                                          // the thread's columns exist

    bool any = false;                                                         // uniform: a block without a selected row only clears
    for (int r = 0; r < kOrthRows; ++r) any = any || (i0 + r < a.K && a.selected[i0 + r] != 0);
    bool seli[RI];
    double racc[RI], vacc[RI][4];
#pragma unroll
    for (int r = 0; r < RI; ++r) {
        const int i = i0 + rg * RI + r;
        seli[r] = i < a.K && a.selected[i] != 0;
        racc[r] = 0.0;
#pragma unroll
        for (int e = 0; e < 4; ++e) vacc[r][e] = 0.0;
    }

    if (any) {
        orth_stage<S>(a, Dp, vec, i0, kOrthRows, ni);
        for (int j0 = 0; j0 < a.K; j0 += kOrthTile) {
            __syncthreads();                                                  // the step before has read its tile, flags and G
            if (t < kOrthTile) selj[t] = (j0 + t < a.K && a.selected[j0 + t] != 0) ? 1 : 0;
            orth_stage<S>(a, Dp, vec, j0, kOrthTile, nj);
            __syncthreads();
            // the tile's flags as bits: no LDS read, and hence no LDS latency, in front of a step of the sums below
            unsigned mask = 0;
#pragma unroll
            for (int q = 0; q < kOrthTile; ++q) mask |= (unsigned)selj[q] << q;
            if (!mask) continue;                                              // (uniform) nothing of this tile is added
            {   // G_ij for i = ih and ih + 8, j = t % 32: c ascending; the products are exact, so the fma is the contract's two steps
                const int j = t & (kOrthTile - 1), ih = t / kOrthTile;
                const float *pj = nj + j * S, *p0 = ni + ih * S, *p1 = ni + (ih + kOrthRows / 2) * S;
                double g0 = 0.0, g1 = 0.0;
#pragma unroll 4                     // (the LDS reads of four steps in flight; the order of the sums stays)
                for (int c = 0; c < Dp; c += 4) {
                    const f32x4 x = *reinterpret_cast<const f32x4 *>(pj + c);
                    const f32x4 y0 = *reinterpret_cast<const f32x4 *>(p0 + c), y1 = *reinterpret_cast<const f32x4 *>(p1 + c);
                    const double x0 = (double)x.x, x1 = (double)x.y, x2 = (double)x.z, x3 = (double)x.w;
                    g0 = __builtin_fma((double)y0.x, x0, g0);
                    g1 = __builtin_fma((double)y1.x, x0, g1);
                    g0 = __builtin_fma((double)y0.y, x1, g0);
                    g1 = __builtin_fma((double)y1.y, x1, g1);
                    g0 = __builtin_fma((double)y0.z, x2, g0);
                    g1 = __builtin_fma((double)y1.z, x2, g1);
                    g0 = __builtin_fma((double)y0.w, x3, g0);
                    g1 = __builtin_fma((double)y1.w, x3, g1);
                }
                g[ih * kOrthTile + j] = g0;
                g[(ih + kOrthRows / 2) * kOrthTile + j] = g1;
            }
            __syncthreads();
            auto add = [&](int q) {                                           // code j0 + q joins the thread's sums
                double gq[RI];
#pragma unroll
                for (int r = 0; r < RI; ++r) {
                    gq[r] = g[(rg * RI + r) * kOrthTile + q];
                    const double p = gq[r] * gq[r];                           // the product rounded, then the add
                    racc[r] = racc[r] + p;
                }
                if (WANT_V && active) {
                    const f32x4 x = *reinterpret_cast<const f32x4 *>(nj + q * S + 4 * cg);
                    const double xd[4] = {(double)x.x, (double)x.y, (double)x.z, (double)x.w};
#pragma unroll
                    for (int r = 0; r < RI; ++r)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const double p = gq[r] * xd[e];
                            vacc[r][e] = vacc[r][e] + p;
                        }
                }
            };
            if (mask == 0xffffffffu) {       // the whole tile: no branch between the steps, so later steps' LDS reads are issued early
#pragma unroll 8
                for (int q = 0; q < kOrthTile; ++q) add(q);
            } else {                                                          // ascending j; an unselected code adds nothing
                for (int q = 0; q < kOrthTile; ++q)
                    if (mask >> q & 1) add(q);
            }
        }
    }

#pragma unroll
    for (int r = 0; r < RI; ++r) {
        const int i = i0 + rg * RI + r;
        if (i >= a.K) continue;
        if (cg == 0) a.r[i] = seli[r] ? racc[r] : 0.0;
        if (WANT_V && active)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (4 * cg + e < a.D) a.v[(size_t)i * a.D + 4 * cg + e] = seli[r] ? vacc[r][e] : 0.0;
    }
}

// One workgroup: M, the total in the contract's order, the loss.  part: kOrthSumBlocks doubles, cnt: kOrthThreads ints.
__device__ __forceinline__ void orth_finalize_body(const double *r, const int32_t *selected, int K, float *loss, int32_t *count,
                                                   double *part, int *cnt) {
    const int t = (int)threadIdx.x;
    int c = 0;
    for (int k = t; k < K; k += kOrthThreads) c += selected[k] != 0 ? 1 : 0;
    cnt[t] = c;
    if (t < kOrthSumBlocks && t * kOrthSumBlock < K) {
        const int end = (t + 1) * kOrthSumBlock < K ? (t + 1) * kOrthSumBlock : K;
        double s = 0.0;
#pragma unroll 8
        for (int k = t * kOrthSumBlock; k < end; ++k) s = s + r[k];
        part[t] = s;
    }
    __syncthreads();
    if (t != 0) return;
    int M = 0;
#pragma unroll 1
    for (int q = 0; q < kOrthThreads; ++q) M += cnt[q];
    double T = 0.0;
#pragma unroll 1
    for (int b = 0; b * kOrthSumBlock < K; ++b) T = T + part[b];
    *count = M;
    if (M == 0) {
        *loss = 0.f;
        return;
    }
    const double m = (double)M, mm = m * m;
    const double mean = T / mm, diag = 1.0 / m;
    *loss = (float)(mean - diag);
}

// grad_rows[i][c] = float((double(g) (4 / M^2)) V_ic) in selected rows, +0.0 elsewhere; a grid-stride loop over the elements
__device__ __forceinline__ void orth_backward_body(const double *saved, const int32_t *selected, const int32_t *count,
                                                   const float *grad_loss, int K, int D, float *grad_rows, unsigned nblocks) {
    const double gl = grad_loss ? (double)*grad_loss : 1.0;
    const double m = (double)*count, mm = m * m;
    const double q = 4.0 / mm;
    const double s = gl * q;
    const size_t n = (size_t)K * D, step = (size_t)nblocks * kOrthThreads;
    for (size_t e = (size_t)blockIdx.x * kOrthThreads + threadIdx.x; e < n; e += step) {
        const size_t i = e / (size_t)D;
        float o = 0.f;
        if (selected[i] != 0) {
            const double p = s * saved[e];
            o = (float)p;
        }
        grad_rows[e] = o;
    }
}

}  // namespace vqvae
