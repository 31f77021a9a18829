// The element-wise arithmetic of grouped (product) quantization (vq_grouped.hip, whose header states the contract): the whole bodies
// of the split, finish / decode and grad_z kernels.  Plain C++ over `__device__ __forceinline__`, so that
// tests/host/grouped_harness.cpp compiles THIS text for the host (blockIdx / threadIdx / gridDim and f32x4 supplied by the harness)
// and compares it with scalar loops, bit for bit and under the sanitizers.
#pragma once

namespace vqvae {

constexpr int kGrpMaxGroups = 16;

struct GrpBooks {                         // kernel argument: the groups' codebooks, each (K, d)
    const float *cb[kGrpMaxGroups];
};

enum { kGrpFinish = 0, kGrpGradz = 1 };

struct GrpArgs {
    const float *z;                       // the whole rows; finish: NULL = decode
    const long long *idx;                 // (G, N), group-major
    long long N, total;                   // rows; elements the launch walks: N D, or N d (g1 - g0) for the split
    int D, d, HW, K, rowmajor, G;
    int g0, g1;                           // split: groups [g0, g1), slab g0 first in `out`
    float *out;                           // split: the slabs; finish: z_q; gradz: grad_z
    float *out2;                          // split: a second copy of the slabs, or NULL
    const float *g_zq, *g_loss;           // gradz
    float scale;                          // gradz: fp32(2 / (N d)), or fp32(2 beta / (N d)) for the commitment-only form
    const float *loss_group;              // finish: the G group losses and where their mean goes (both or neither)
    float *loss;
};

template <int V>
__device__ __forceinline__ void grp_load(const float *p, float (&v)[V]) {
    if constexpr (V == 4) {
        const f32x4 t = *reinterpret_cast<const f32x4 *>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = p[0];
    }
}

template <int V>
__device__ __forceinline__ void grp_store(float *p, const float (&v)[V]) {
    if constexpr (V == 4) {
        f32x4 t;
        t.x = v[0]; t.y = v[1]; t.z = v[2]; t.w = v[3];
        *reinterpret_cast<f32x4 *>(p) = t;
    } else {
        p[0] = v[0];
    }
}

// Every kernel body takes the type I of its element arithmetic: unsigned where the launch has checked N D < 2^32 (every index, unit
// count and grid-stride sum then fits, and the divisions by d, D and H W are 32-bit ones), long long otherwise.  The results are
// the same integers either way.

// ---- split: slab g = the channels [g d, (g + 1) d) of every row, in the layout of the input -------------------------------------
// V elements of the slabs from element o on (o counts from slab g0's first element): V channels of one row of one group
// (row-major), or one channel of V consecutive rows (NCHW).  The writes are dense; the reads come in runs of d channels (row-major)
// or whole planes (NCHW).  V = 4 only where the launch has checked divisibility and alignment.
template <int V, typename I>
__device__ __forceinline__ void grp_split_unit(const GrpArgs &a, I o) {
    const I d = (I)a.d, D = (I)a.D, HW = (I)a.HW;
    const I slab = (I)a.N * d;
    const I gi = o / slab, rem = o - gi * slab;
    const I c0 = ((I)a.g0 + gi) * d;                      // the group's first channel
    I src;
    if (a.rowmajor) {
        const I row = rem / d;
        src = row * D + c0 + (rem - row * d);
    } else {
        const I plane = rem / HW;                         // b d + cc
        const I hw = rem - plane * HW;
        const I b = plane / d;
        src = (b * D + c0 + (plane - b * d)) * HW + hw;
    }
    float v[V];
    grp_load<V>(a.z + src, v);
    grp_store<V>(a.out + o, v);
    if (a.out2) grp_store<V>(a.out2 + o, v);
}

template <int V, typename I>
__device__ __forceinline__ void grp_split_body(const GrpArgs &a) {
    const I units = (I)(a.total / V);                     // (V = 4: the launch has checked total % 4 == 0)
    for (I u = (I)blockIdx.x * 256 + (I)threadIdx.x; u < units; u += (I)gridDim.x * 256)
        grp_split_unit<V, I>(a, u * V);
}

// ---- finish / decode / grad_z: one pass over the whole rows in their own layout --------------------------------------------------
// V elements from element e on; the group of channel c is c / d, its code row E_g[idx_g[row]] (an index outside [0, K): NaN, no read)
template <int V, int MODE, typename I>
__device__ __forceinline__ void grp_unit(const GrpArgs &a, const GrpBooks &books, I e, float gs) {
    const I D = (I)a.D, HW = (I)a.HW;
    I row;
    int c;
    if (a.rowmajor) {
        row = e / D;
        c = (int)(e - row * D);
    } else {
        const I plane = e / HW;                           // b D + c
        const I hw = e - plane * HW;
        const I b = plane / D;
        c = (int)(plane - b * D);
        row = b * HW + hw;
    }
    const int g = c / a.d, cc = c - g * a.d;              // (V = 4 on rows: d % 4 == 0, the four channels are one group's)
    const float *cb = books.cb[g];
    const long long *ig = a.idx + (size_t)g * a.N;
    float ev[V];
    if (a.rowmajor) {
        const long long k = ig[(size_t)row];
        if (k >= 0 && k < a.K) {
            grp_load<V>(cb + (size_t)k * a.d + cc, ev);
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) ev[j] = __builtin_nanf("");
        }
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const long long k = ig[(size_t)row + j];
            ev[j] = (k >= 0 && k < a.K) ? cb[(size_t)k * a.d + cc] : __builtin_nanf("");
        }
    }
    float zv[V], o[V];
    if (a.z) grp_load<V>(a.z + e, zv);
    if (MODE == kGrpFinish) {
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = a.z ? zv[j] + (ev[j] - zv[j]) : ev[j];
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = gs * (zv[j] - ev[j]);
        if (a.g_zq) {
            float gv[V];
            grp_load<V>(a.g_zq + e, gv);
#pragma unroll
            for (int j = 0; j < V; ++j) o[j] = gv[j] + o[j];
        }
    }
    grp_store<V>(a.out + e, o);
}

template <int V, int MODE, typename I>
__device__ __forceinline__ void grp_walk(const GrpArgs &a, const GrpBooks &books, float gs) {
    const I units = (I)(a.total / V);
    for (I u = (I)blockIdx.x * 256 + (I)threadIdx.x; u < units; u += (I)gridDim.x * 256)
        grp_unit<V, MODE, I>(a, books, u * V, gs);
}

// z_q = z + (e - z) (z == NULL: z_q = e); the first thread also takes the mean of the group losses:
// loss = ((loss_0 + loss_1) + ...) / (float)G, group order, one division.  total = 0: the loss alone.
template <int V, typename I>
__device__ __forceinline__ void grp_finish_body(const GrpArgs &a, const GrpBooks &books) {
    if (a.loss && blockIdx.x == 0 && threadIdx.x == 0) {
        float l = a.loss_group[0];
        for (int g = 1; g < a.G; ++g) l = l + a.loss_group[g];
        a.loss[0] = l / (float)a.G;
    }
    grp_walk<V, kGrpFinish, I>(a, books, 0.0f);
}

// grad_z = grad_zq + gs * (z - e), gs = (g / (float)G) * scale: vqvae_vq_backward_f32's grad_z of every group with the upstream
// loss gradient g / G, written into the group's channels
template <int V, typename I>
__device__ __forceinline__ void grp_gradz_body(const GrpArgs &a, const GrpBooks &books) {
    const float gq = (a.g_loss ? a.g_loss[0] : 1.0f) / (float)a.G;
    grp_walk<V, kGrpGradz, I>(a, books, gq * a.scale);
}

}  // namespace vqvae
