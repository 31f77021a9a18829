// l2-normalisation of rows, forward and backward (vq_cosine.hip, whose header states the arithmetic): the per-row operations and the
// whole bodies of the kernels.  Plain C++ over `__device__ __forceinline__`, so that tests/host/cosine_harness.cpp compiles THIS text
// for the host (blockIdx / threadIdx, f32x4 and __syncthreads supplied by the harness) and compares it with a scalar loop, bit for
// bit and under the sanitizers.
#pragma once

namespace vqvae {

constexpr int kL2Chunk = 64;                        // channels of a row-major row staged through LDS per pass
constexpr int kL2Stride = kL2Chunk + 4;             // dwords between two rows of a tile: 16-byte accesses of 64 lanes hit 64 banks
constexpr int kL2TileFloats = 64 * kL2Stride;       // one wave's tile: 64 rows
constexpr int kL2Waves = 4;                         // waves (tiles) per workgroup of the row-major kernels

struct L2nArgs {
    const float *x;                                 // forward: x; backward: y.  (N, D) rows or (B, D, HW) maps
    const float *g;                                 // backward: grad_y, x's layout (forward: unused)
    const float *denom_in;                          // backward: the forward's denom (N)
    float *out;                                     // forward: y; backward: grad_x
    float *denom_out;                               // forward: (N)
    long long N;
    int D, HW;
    float eps;
};

// channel c of a row joins its sum (call in ascending c: the order is the contract).  The product of two fp32 values is exact in
// fp64; the addition rounds.
__device__ __forceinline__ void l2n_add(double &s, float a, float b) { s = s + (double)a * (double)b; }

// the row's divisor from its sum of squares.  The comparison is written out: a NaN norm stays NaN (fmaxf would return eps).
__device__ __forceinline__ float l2n_denom(double s, float eps) {
    const double n = __builtin_sqrt(s);
    const float d = (float)n;
    return (d < eps) ? eps : d;
}

__device__ __forceinline__ float l2n_fwd_out(float x, float d) { return x / d; }

// grad_x of one element from t = sum_c y_c g_c: three fp64 operations and one rounding off the clamp, g / eps on it
__device__ __forceinline__ float l2n_bwd_out(float y, float g, double t, float d, float eps) {
    if (d > eps) return (float)(((double)g - (double)y * t) / (double)d);
    return (float)((double)g / (double)eps);
}

// V consecutive elements from element offset `o` on (V = 4: one 16-byte access; the launch has checked alignment and divisibility)
template <int V>
__device__ __forceinline__ void l2n_load(const float *p, size_t o, float *v) {
    if constexpr (V == 4) {
        const f32x4 t = *reinterpret_cast<const f32x4 *>(p + o);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = p[o];
    }
}
template <int V>
__device__ __forceinline__ void l2n_store(float *p, size_t o, const float *v) {
    if constexpr (V == 4) {
        f32x4 t;
        t.x = v[0]; t.y = v[1]; t.z = v[2]; t.w = v[3];
        *reinterpret_cast<f32x4 *>(p + o) = t;
    } else {
        p[o] = v[0];
    }
}

// ---- NCHW maps: a lane owns V neighbouring pixels of one image (V = 4 needs HW % 4 == 0), so every channel is one coalesced access
// of the wave and the lane adds its rows' sums in ascending channel order.  DREG > 0 (D <= DREG): the rows stay in registers between
// the sums and the output; DREG = 0: the second pass reads them again (the lane's own lines, just used).  One item per thread: the
// grid covers all rows, there is no stride loop.
template <bool BWD, int DREG, int V>
__device__ __forceinline__ void l2n_nchw_body(const L2nArgs &a) {
    const long long row0 = ((long long)blockIdx.x * 256 + threadIdx.x) * V;
    if (row0 >= a.N) return;
    const int D = a.D;
    const long long b = row0 / a.HW;
    const size_t base = (size_t)b * D * a.HW + (size_t)(row0 - b * a.HW), stride = (size_t)a.HW;
    constexpr int R = DREG > 0 ? DREG : 1;
    float xr[R][V], gr[BWD ? R : 1][V];
    double s[V];
#pragma unroll
    for (int j = 0; j < V; ++j) s[j] = 0.0;
    auto sums = [&](int c, float *xv, float *gv) {
        l2n_load<V>(a.x, base + c * stride, xv);
        if constexpr (BWD) l2n_load<V>(a.g, base + c * stride, gv);
#pragma unroll
        for (int j = 0; j < V; ++j) l2n_add(s[j], xv[j], BWD ? gv[j] : xv[j]);
    };
    if constexpr (DREG > 0) {
#pragma unroll
        for (int c = 0; c < DREG; ++c)
            if (c < D) sums(c, xr[c], gr[BWD ? c : 0]);
    } else {
        for (int c = 0; c < D; ++c) sums(c, xr[0], gr[0]);
    }
    float d[V];
    if constexpr (BWD) {
        l2n_load<V>(a.denom_in, (size_t)row0, d);
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) d[j] = l2n_denom(s[j], a.eps);
        l2n_store<V>(a.denom_out, (size_t)row0, d);
    }
    auto emit = [&](int c, const float *xv, const float *gv) {
        float o[V];
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = BWD ? l2n_bwd_out(xv[j], gv[j], s[j], d[j], a.eps) : l2n_fwd_out(xv[j], d[j]);
        l2n_store<V>(a.out, base + c * stride, o);
    };
    if constexpr (DREG > 0) {
#pragma unroll
        for (int c = 0; c < DREG; ++c)
            if (c < D) emit(c, xr[c], gr[BWD ? c : 0]);
    } else {
        for (int c = 0; c < D; ++c) {
            l2n_load<V>(a.x, base + c * stride, xr[0]);
            if constexpr (BWD) l2n_load<V>(a.g, base + c * stride, gr[0]);
            emit(c, xr[0], gr[0]);
        }
    }
}

// ---- row-major rows: a wave owns 64 consecutive rows, which lie in memory as one run of 64 D floats.  One lane per row straight
// from memory would touch 64 lines per access; instead the wave copies `cw` <= 64 channels of its rows into an LDS tile in coalesced
// accesses (16 bytes per lane with V = 4, one element with V = 1), and each lane then walks its own row of the tile, 16 bytes at a
// time -- rows are kL2Stride = 68 dwords apart, so the lanes of every access group hit different banks.  Rows wider than one chunk
// carry the running sum from chunk to chunk (the ascending order holds) and are staged a second time for the output (they are still
// in L2); rows of at most one chunk stay in the tile between the sum and the output.  The output goes back through the tile, so the
// stores are coalesced like the loads.

// `cw` channels from c0 on of rows r0 .. r0 + nr - 1: memory -> tile (TO_TILE) or tile -> memory
template <int V, bool TO_TILE>
__device__ __forceinline__ void l2n_copy(float *mem, float *tile, long long r0, int nr, int D, int c0, int cw, int lane) {
    const int per = cw / V, n = nr * per;                // accesses per row, and of the tile
#pragma unroll 4
    for (int j = lane; j < n; j += 64) {
        const int row = per == 16 ? (j >> 4) : j / per, q = j - row * per;
        float v[V];
        float *m = mem + (size_t)(r0 + row) * D + c0, *t = tile + row * kL2Stride;
        if constexpr (TO_TILE) {
            l2n_load<V>(m, (size_t)q * V, v);
            l2n_store<V>(t, (size_t)q * V, v);
        } else {
            l2n_load<V>(t, (size_t)q * V, v);
            l2n_store<V>(m, (size_t)q * V, v);
        }
    }
}

template <bool BWD, int V>
__device__ __forceinline__ void l2n_rows_body(const L2nArgs &a, float *lds) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float *tx = lds + wave * (BWD ? 2 : 1) * kL2TileFloats, *tg = tx + (BWD ? kL2TileFloats : 0);
    const long long r0 = ((long long)blockIdx.x * kL2Waves + wave) * 64, left = a.N - r0;
    const int nr = left <= 0 ? 0 : (left < 64 ? (int)left : 64);           // a wave without rows still meets every barrier
    const int D = a.D, nch = (D + kL2Chunk - 1) / kL2Chunk;
    const bool mine = lane < nr;
    float *mx = tx + lane * kL2Stride, *mg = tg + lane * kL2Stride;         // the lane's row of the tile(s)
    auto stage = [&](int c0, int cw) {
        l2n_copy<V, true>(const_cast<float *>(a.x), tx, r0, nr, D, c0, cw, lane);
        if constexpr (BWD) l2n_copy<V, true>(const_cast<float *>(a.g), tg, r0, nr, D, c0, cw, lane);
    };
    double s = 0.0;
    for (int ch = 0; ch < nch; ++ch) {
        const int c0 = ch * kL2Chunk, cw = D - c0 < kL2Chunk ? D - c0 : kL2Chunk;
        stage(c0, cw);
        __syncthreads();
        if (mine)
            for (int c = 0; c < cw; c += 4) {
                float xv[4], gv[4];
                l2n_load<4>(mx, (size_t)c, xv);
                if constexpr (BWD) l2n_load<4>(mg, (size_t)c, gv);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (c + j < cw) l2n_add(s, xv[j], BWD ? gv[j] : xv[j]);
            }
        if (nch > 1) __syncthreads();                                       // (one chunk: the tile is kept for the output)
    }
    float d = 1.0f;
    if constexpr (BWD) {
        if (mine) d = a.denom_in[r0 + lane];
    } else {
        d = l2n_denom(s, a.eps);
        if (mine) a.denom_out[r0 + lane] = d;
    }
    for (int ch = 0; ch < nch; ++ch) {
        const int c0 = ch * kL2Chunk, cw = D - c0 < kL2Chunk ? D - c0 : kL2Chunk;
        if (nch > 1) {
            stage(c0, cw);
            __syncthreads();
        }
        if (mine)
            for (int c = 0; c < cw; c += 4) {
                float xv[4], gv[4], o[4];
                l2n_load<4>(mx, (size_t)c, xv);
                if constexpr (BWD) l2n_load<4>(mg, (size_t)c, gv);
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = BWD ? l2n_bwd_out(xv[j], gv[j], s, d, a.eps) : l2n_fwd_out(xv[j], d);
                l2n_store<4>(mx, (size_t)c, o);                             // (slots past cw belong to the row's padding)
            }
        __syncthreads();
        l2n_copy<V, false>(a.out, tx, r0, nr, D, c0, cw, lane);
        if (nch > 1) __syncthreads();
    }
}

#ifdef __HIPCC__
// vq_cosine.hip: pick the access width (alignment, HW % 4 or D % 4) and the register form, and launch
void launch_l2norm(const L2nArgs &a, bool backward, bool rowmajor, hipStream_t st);
#endif

}  // namespace vqvae
