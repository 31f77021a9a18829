// The per-row linear map of latent rows (vq_linear.hip, whose header states the arithmetic): the whole bodies of the kernels.  Plain C++
// over `__device__ __forceinline__`, so that tests/host/linear_harness.cpp compiles THIS text for the host (blockIdx / threadIdx,
// f32x4 and __syncthreads supplied by the harness) and compares it with the restatement bit for bit under the sanitizers.  The
// 16-byte / element accesses and the parameter kernel's row-major tile are vq_cosine.h's.
//
// Forward and grad_x are one operation on two views of w: out[n][o] = float(first[o] + sum_i W(o, i) in[n][i]), i ascending, with
// W(o, i) = w[o * ws_o + i * ws_i] -- (Cin, 1) for y, (1, Cin) for grad_x -- and first = b or 0.0.  A workgroup converts the weights of
// R output channels to fp64 once and keeps them in LDS as wl[i * R + r]; a lane owns P rows and P R sums in registers: P R independent
// fp64 chains, and every weight -- one broadcast read -- serves P rows.  Wider outputs take several passes over the rows (the tiling
// is over the OUTPUT channels: the order over i is the contract).
#pragma once

#include "vq_cosine.h"

namespace vqvae {

constexpr int kLinBlockRows = 64 * kL2Waves;                 // threads of the NCHW and parameter kernels, and the contract's block: 256
constexpr int kLinWeightsSmall = 64 * 16;                    // fp64 weights of one pass in LDS: NI * R <= this (8 KiB) ...
constexpr int kLinWeightsMax = 256 * 16;                     // ... or this (32 KiB): 256 inputs x 16 outputs
constexpr int kLinNchwStride = kLinBlockRows + 1;            // dwords between two channels of the parameter kernel's NCHW tile
constexpr int kLinBChunk = 16;                               // channels of the parameter kernel's register side per pass
constexpr int kLinBStride = kLinBChunk + 4;                  // dwords between two rows of its tile (16-byte aligned)

struct LinArgs {
    const float *x;                                          // the rows that are read: NI channels, (N, NI) or (B, NI, HW)
    const float *w;                                          // (Cout, Cin); the view's element (o, i) is w[o * ws_o + i * ws_i]
    const float *b;                                          // (NO): the first term of every sum, or NULL: 0.0
    float *out;                                              // NO channels, x's layout
    long long N;
    int NI, NO, HW, ws_o, ws_i;
};

// the weights of outputs o0 .. o0 + R - 1, all NI inputs, as doubles; an output past NO gets zeros (its sums are not stored)
template <int R, int NT>
__device__ __forceinline__ void lin_stage_weights(const LinArgs &a, int o0, double *wl) {
    const int n = a.NI * R;
    for (int e = threadIdx.x; e < n; e += NT) {
        const int i = e / R, o = o0 + (e - i * R);
        wl[e] = o < a.NO ? (double)a.w[(size_t)o * a.ws_o + (size_t)i * a.ws_i] : 0.0;
    }
}

template <int R, int P>
__device__ __forceinline__ void lin_first(const LinArgs &a, int o0, double (*acc)[R]) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const double f = (a.b && o0 + r < a.NO) ? (double)a.b[o0 + r] : 0.0;
#pragma unroll
        for (int p = 0; p < P; ++p) acc[p][r] = f;
    }
}

// input i of the lane's P rows joins their R sums each (call in ascending i): every weight is read once for the P rows.  The
// product of two fp32 values is exact in fp64, so the fused multiply-add rounds exactly as the multiplication and the addition of
// the contract do.
template <int R, int P>
__device__ __forceinline__ void lin_join(double (*acc)[R], const double *wi, const float *x) {
    double xd[P];
#pragma unroll
    for (int p = 0; p < P; ++p) xd[p] = (double)x[p];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const double w = wi[r];
#pragma unroll
        for (int p = 0; p < P; ++p) acc[p][r] = __builtin_fma(w, xd[p], acc[p][r]);
    }
}

// ---- NCHW maps: a lane owns P neighbouring pixels of one image (P = 4 needs HW % 4 == 0 and 16-byte aligned maps), so every channel
// is one coalesced access of the wave, 16 bytes per lane with P = 4, and every weight read from LDS serves P rows ------------------
template <int R, int P>
__device__ __forceinline__ void lin_nchw_body(const LinArgs &a, double *wl) {
    const long long row = ((long long)blockIdx.x * kLinBlockRows + threadIdx.x) * P;
    const bool mine = row < a.N;                                              // (P = 4: N % 4 == 0, the four are inside)
    const long long b = mine ? row / a.HW : 0;
    const size_t pix = (size_t)(mine ? row - b * a.HW : 0), stride = (size_t)a.HW;
    const size_t bin = (size_t)b * a.NI * a.HW + pix, bout = (size_t)b * a.NO * a.HW + pix;
    for (int o0 = 0; o0 < a.NO; o0 += R) {
        if (o0) __syncthreads();                                              // the pass before has read its weights
        lin_stage_weights<R, kLinBlockRows>(a, o0, wl);
        __syncthreads();
        if (!mine) continue;                                                  // (meets the next pass's barriers all the same)
        double acc[P][R];
        lin_first<R, P>(a, o0, acc);
#pragma unroll 2
        for (int i = 0; i < a.NI; ++i) {                                      // (unrolled by 8: measured 15 % slower at D = 64 -> 8)
            float xv[P];
            l2n_load<P>(a.x, bin + i * stride, xv);
            lin_join<R, P>(acc, wl + i * R, xv);
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (o0 + r < a.NO) {
                float o[P];
#pragma unroll
                for (int p = 0; p < P; ++p) o[p] = (float)acc[p][r];
                l2n_store<P>(a.out, bout + (o0 + r) * stride, o);
            }
    }
}

// ---- row-major rows: a wave owns 256 consecutive rows and stages 16 input channels of them at a time through its LDS tile in
// coalesced accesses (16 bytes per lane with V = 4, one element with V = 1; the scheme of vq_cosine.h with a narrower, longer tile),
// the next chunk's loads in flight while this one is walked; lane l walks rows l, l + 64, l + 128 and l + 192 of the tile, 16 bytes
// at a time -- rows are kLinStride = 20 dwords apart, so the lanes of every access group hit different banks -- and every weight
// read from LDS serves its four rows.  (Two rows per lane with R = 16 keep the sums out of the AGPRs and measured 9 - 16 % slower.)
// Rows of at most one chunk stay in the tile for every pass.  A lane stores its outputs itself: 16 bytes at a time with V = 4
// (NO % 4 == 0).
constexpr int kLinRowsPerLane = 4;
constexpr int kLinChunk = 16;                                // channels staged per pass
constexpr int kLinStride = kLinChunk + 4;                    // dwords between two rows of the tile
constexpr int kLinWaveRows = 64 * kLinRowsPerLane;           // rows of one wave: 256
constexpr int kLinTileFloats = kLinWaveRows * kLinStride;    // one wave's tile: 20 KiB
constexpr int kLinRowsWaves = 2;                             // waves (tiles) per workgroup of the row-major kernels

// `cw` channels from c0 on of rows r0 .. r0 + nr - 1: memory -> the lane's registers (FETCH), or registers -> tile.  Two
// steps, so that the next chunk's loads are in flight while the lanes walk this one.
template <int V, int P, bool FETCH>
__device__ __forceinline__ void lin_move(const float *mem, float *tile, long long r0, int nr, int C, int c0, int cw, int lane, float *pre) {
    const int per = cw / V, n = nr * per;                // accesses per row, and of the tile
#pragma unroll
    for (int u = 0; u < P * kLinChunk / V; ++u) {            // (a lane brings P * 16 floats per chunk)
        const int j = lane + 64 * u;
        if (j < n) {
            const int row = per == 4 ? (j >> 2) : (per == 16 ? (j >> 4) : j / per), q = j - row * per;
            if constexpr (FETCH) l2n_load<V>(mem + (size_t)(r0 + row) * C + c0, (size_t)q * V, pre + u * V);
            else l2n_store<V>(tile + row * kLinStride, (size_t)q * V, pre + u * V);
        }
    }
}

template <int R, int V>
__device__ __forceinline__ void lin_rows_body(const LinArgs &a, float *tiles, double *wl) {
    constexpr int P = kLinRowsPerLane;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float *tx = tiles + wave * kLinTileFloats;
    const long long r0 = ((long long)blockIdx.x * kLinRowsWaves + wave) * kLinWaveRows, left = a.N - r0;
    const int nr = left <= 0 ? 0 : (left < kLinWaveRows ? (int)left : kLinWaveRows);   // a wave without rows still meets every barrier
    const int NI = a.NI, NO = a.NO, nch = (NI + kLinChunk - 1) / kLinChunk;
    for (int o0 = 0; o0 < NO; o0 += R) {
        if (o0) __syncthreads();                                              // the pass before has read its weights and the tile
        lin_stage_weights<R, 64 * kLinRowsWaves>(a, o0, wl);
        double acc[P][R];
        lin_first<R, P>(a, o0, acc);
        const bool restage = nch > 1 || o0 == 0;                              // (one chunk: the tile is kept for every pass)
        float pre[P * kLinChunk];
        if (restage) lin_move<V, P, true>(a.x, tx, r0, nr, NI, 0, NI < kLinChunk ? NI : kLinChunk, lane, pre);
        for (int ch = 0; ch < nch; ++ch) {
            const int c0 = ch * kLinChunk, cw = NI - c0 < kLinChunk ? NI - c0 : kLinChunk;
            if (restage) {
                if (ch) __syncthreads();                                      // the chunk before is walked
                lin_move<V, P, false>(a.x, tx, r0, nr, NI, c0, cw, lane, pre);
            }
            __syncthreads();                                                  // the tile and the weights are in place
            if (restage && ch + 1 < nch)                                      // the next chunk's loads fly while this one is walked
                lin_move<V, P, true>(a.x, tx, r0, nr, NI, c0 + kLinChunk, NI - c0 - kLinChunk < kLinChunk ? NI - c0 - kLinChunk : kLinChunk,
                                  lane, pre);
            if (lane < nr)                                                    // (rows past nr: stale tile values, never stored)
                for (int c = 0; c < cw; c += 4) {
                    float xv[P][4];
#pragma unroll
                    for (int p = 0; p < P; ++p) l2n_load<4>(tx + (lane + 64 * p) * kLinStride, (size_t)c, xv[p]);
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (c + k < cw) {
                            float xk[P];
#pragma unroll
                            for (int p = 0; p < P; ++p) xk[p] = xv[p][k];
                            lin_join<R, P>(acc, wl + (c0 + c + k) * R, xk);
                        }
                }
        }
#pragma unroll
        for (int p = 0; p < P; ++p) {
            if (lane + 64 * p >= nr) continue;
            float *orow = a.out + (size_t)(r0 + lane + 64 * p) * NO + o0;
            if constexpr (V == 4) {
#pragma unroll
                for (int r = 0; r < R; r += 4)
                    if (o0 + r < NO) {                                        // (NO % 4 == 0: the four are inside the row)
                        const float o[4] = {(float)acc[p][r], (float)acc[p][r + 1], (float)acc[p][r + 2], (float)acc[p][r + 3]};
                        l2n_store<4>(orow, (size_t)r, o);
                    }
            } else {
#pragma unroll
                for (int r = 0; r < R; ++r)
                    if (o0 + r < NO) orow[r] = (float)acc[p][r];
            }
        }
    }
}

// ---- the parameter gradients: grad_w[j][c] = sum_n gy[n][j] x[n][c], grad_b[j] = sum_n gy[n][j] ----------------------------------
// Every workgroup owns the SAME 256 consecutive rows in either layout and adds their terms in fp64 one row after the other, in
// ascending row order from 0.0, into its record of partials; lin_param_finalize_body adds the records in ascending workgroup order.
// The wider of the two operands lies across the lanes, 64 channels at a time (the `A` side, in the 256-row tile: the four waves'
// row-major tiles as one (256, 68) image, or the NCHW kernel's tile[channel * 257 + row]); 16 channels of the other lie in the
// small tile `bt`, and a thread keeps 4 of them in registers: four independent chains per thread, one conflict-free read and one
// broadcast 16-byte read per row.  Wave 0 adds the bias sums on the side, one channel per lane.
struct LinParamArgs {
    const float *x, *g;                                      // rows of Cin / of Cout channels
    double *partials;                                        // per workgroup: [grad_w (Cout, Cin)] [grad_b (Cout)]
    long long N;
    int Cin, Cout, HW;
};

__device__ __forceinline__ int lin_partial_count(int Cin, int Cout) { return Cout * Cin + Cout; }

template <bool ROWMAJOR, int V>
__device__ __forceinline__ void lin_params_body(const LinParamArgs &a, float *tiles, float *bt) {
    constexpr int RS = ROWMAJOR ? kL2Stride : 1, CS = ROWMAJOR ? 1 : kLinNchwStride;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const long long row0 = (long long)blockIdx.x * kLinBlockRows, leftb = a.N - row0;
    const int nrb = leftb < kLinBlockRows ? (int)leftb : kLinBlockRows;
    const int Cin = a.Cin, Cout = a.Cout;
    const bool swap = Cout > Cin;                                             // gy across the lanes, x in the registers
    const float *src_a = swap ? a.g : a.x, *src_b = swap ? a.x : a.g;
    const int LA = swap ? Cout : Cin, LB = swap ? Cin : Cout;
    const bool mine = t < nrb;                                                // (NCHW staging: thread t brings row t)
    const long long row = row0 + t, img = mine ? row / a.HW : 0;
    const size_t pix = (size_t)(mine ? row - img * a.HW : 0), stride = (size_t)a.HW;
    const size_t base_a = (size_t)img * LA * a.HW + pix, base_b = (size_t)img * LB * a.HW + pix;
    const int nrw = nrb - wave * 64 <= 0 ? 0 : (nrb - wave * 64 < 64 ? nrb - wave * 64 : 64);
    double *part = a.partials + (size_t)blockIdx.x * lin_partial_count(Cin, Cout);
    bool first = true;
    for (int a0 = 0; a0 < LA; a0 += kL2Chunk) {
        const int aw = LA - a0 < kL2Chunk ? LA - a0 : kL2Chunk;
        for (int b0 = 0; b0 < LB; b0 += kLinBChunk) {
            const int bw = LB - b0 < kLinBChunk ? LB - b0 : kLinBChunk;
            if (!first) __syncthreads();                                      // the tiles' last readers are done
            first = false;
            if (b0 == 0) {
                if constexpr (ROWMAJOR) {
                    l2n_copy<V, true>(const_cast<float *>(src_a), tiles + wave * kL2TileFloats, row0 + wave * 64, nrw, LA, a0, aw, lane);
                } else if (mine) {
                    for (int c = 0; c < aw; ++c) tiles[c * kLinNchwStride + t] = src_a[base_a + (a0 + c) * stride];
                }
            }
            if constexpr (ROWMAJOR) {
                for (int e = t; e < nrb * bw; e += kLinBlockRows) {
                    const int r = e / bw, q = e - r * bw;
                    bt[r * kLinBStride + q] = src_b[(size_t)(row0 + r) * LB + b0 + q];
                }
            } else if (mine) {
                for (int q = 0; q < bw; ++q) bt[t * kLinBStride + q] = src_b[base_b + (b0 + q) * stride];
            }
            __syncthreads();
            const int bq = wave * 4;
            if (bq >= bw) continue;                                           // (wave-uniform; wave 0 always has work)
            const bool la_ok = lane < aw;
            const int la = la_ok ? lane : 0, lb = lane < bw ? lane : 0;
            const bool bias_a = swap && b0 == 0 && wave == 0, bias_b = !swap && a0 == 0 && wave == 0;
            double s[4] = {0.0, 0.0, 0.0, 0.0}, sb = 0.0;
#pragma unroll 4
            for (int r = 0; r < nrb; ++r) {
                const double av = (double)tiles[r * RS + la * CS];
                float bv[4];
                l2n_load<4>(bt, (size_t)(r * kLinBStride + bq), bv);
#pragma unroll
                for (int k = 0; k < 4; ++k) s[k] = __builtin_fma(av, (double)bv[k], s[k]);
                if (bias_a) sb = sb + av;
                else if (bias_b) sb = sb + (double)bt[r * kLinBStride + lb];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (la_ok && bq + k < bw) {
                    const int j = swap ? a0 + lane : b0 + bq + k, c = swap ? b0 + bq + k : a0 + lane;
                    part[j * Cin + c] = s[k];
                }
            if (bias_a && la_ok) part[Cout * Cin + a0 + lane] = sb;
            if (bias_b && lane < bw) part[Cout * Cin + b0 + lane] = sb;
        }
    }
}

// the second launch: output o = the workgroups' partials of o in ascending workgroup order from 0.0, rounded once.  A NULL gradient
// is skipped.
__device__ __forceinline__ void lin_param_finalize_body(const double *partials, long long nblocks, int Cin, int Cout, float *grad_w,
                                                        float *grad_b) {
    const int P = lin_partial_count(Cin, Cout), o = blockIdx.x * kLinBlockRows + threadIdx.x;
    if (o >= P) return;
    float *dst = o < Cout * Cin ? grad_w : grad_b;
    if (!dst) return;
    double s = 0.0;
#pragma unroll 8
    for (long long b = 0; b < nblocks; ++b) s = s + partials[(size_t)b * P + o];
    dst[o < Cout * Cin ? o : o - Cout * Cin] = (float)s;
}

#ifdef __HIPCC__
// vq_linear.hip: pick the access width (alignment, channels % 4), the sums per lane and the weight capacity, and launch
void launch_linear_rows(const LinArgs &a, bool rowmajor, hipStream_t st);
void launch_linear_params(const LinParamArgs &a, bool rowmajor, float *grad_w, float *grad_b, hipStream_t st);
#endif

}  // namespace vqvae
