// The element-wise arithmetic of residual quantization (vq_residual.hip, whose header states the operation order): the whole bodies
// of the advance, finish and grad_z kernels.  Plain C++ over `__device__ __forceinline__`, so that
// tests/host/rvq_harness.cpp compiles THIS text for the host (blockIdx / threadIdx / gridDim and f32x4 supplied by the harness)
// and compares it with a scalar loop, bit for bit and under the sanitizers.
#pragma once

namespace vqvae {

constexpr int kRvqMaxStages = 16;

struct RvqBooks {                         // kernel argument: the stages' codebooks (shared: all the same pointer)
    const float *cb[kRvqMaxStages];
};

enum { kRvqAdvance = 0, kRvqFinish = 1, kRvqGradz = 2 };

struct RvqArgs {
    const float *z;                       // r_{q0}: z itself, or the workspace's residual (advance, in place); NULL: decode
    const long long *idx;                 // (Q, N), stage-major
    long long N, total;                   // rows; elements N D
    int D, HW, K, rowmajor;
    int q0, q1;                           // stages [q0, q1)
    float *out;                           // advance: r_{q1}; finish: z_q (may be NULL); gradz: grad_z
    float *out_r;                         // finish: r_Q, or NULL
    const float *g_zq, *g_loss;           // gradz
    float scale;                          // gradz: fp32(2 / (N D))
    const float *loss_stage;              // finish: the Q stage losses and where their sum goes (both or neither)
    float *loss;
    int Q;
};

// V elements from element e on: V channels of one row (row-major), or one channel of V consecutive rows (NCHW).  V = 4 only where
// the launch has checked divisibility and alignment.
template <int V, int MODE>
__device__ __forceinline__ void rvq_unit(const RvqArgs &a, const RvqBooks &books, long long e, float gs) {
    long long row;
    int c;
    if (a.rowmajor) {
        row = e / a.D;
        c = (int)(e - row * a.D);
    } else {
        const long long plane = e / a.HW;                 // b D + c
        const int hw = (int)(e - plane * a.HW);
        const long long b = plane / a.D;
        c = (int)(plane - b * a.D);
        row = b * a.HW + hw;
    }
    float zv[V], r[V], s[V], acc[V];                      // zv: z, loaded once (the finish kernel needs it again for z_q)
    if (a.z) {
        if constexpr (V == 4) {
            const f32x4 v = *reinterpret_cast<const f32x4 *>(a.z + e);
            zv[0] = v.x; zv[1] = v.y; zv[2] = v.z; zv[3] = v.w;
        } else {
            zv[0] = a.z[e];
        }
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) zv[j] = 0.0f;
    }
#pragma unroll
    for (int j = 0; j < V; ++j) {
        r[j] = zv[j];
        s[j] = acc[j] = 0.0f;
    }
    for (int q = a.q0; q < a.q1; ++q) {
        const float *cb = books.cb[q];
        const long long *iq = a.idx + (size_t)q * a.N;
        float ev[V];
        if (a.rowmajor) {
            const long long k = iq[row];
            const bool ok = k >= 0 && k < a.K;
            if constexpr (V == 4) {
                f32x4 v;
                if (ok) v = *reinterpret_cast<const f32x4 *>(cb + (size_t)k * a.D + c);
                else v.x = v.y = v.z = v.w = __builtin_nanf("");
                ev[0] = v.x; ev[1] = v.y; ev[2] = v.z; ev[3] = v.w;
            } else {
                ev[0] = ok ? cb[(size_t)k * a.D + c] : __builtin_nanf("");
            }
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const long long k = iq[row + j];
                ev[j] = (k >= 0 && k < a.K) ? cb[(size_t)k * a.D + c] : __builtin_nanf("");
            }
        }
        const bool first = q == a.q0;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            if (MODE == kRvqFinish) s[j] = first ? ev[j] : s[j] + ev[j];
            r[j] = r[j] - ev[j];
            if (MODE == kRvqGradz) acc[j] = first ? r[j] : acc[j] + r[j];
        }
    }
    float o[V];
    if (MODE == kRvqAdvance) {
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = r[j];
    } else if (MODE == kRvqFinish) {
        if (a.out_r) {
            if constexpr (V == 4) {
                f32x4 v;
                v.x = r[0]; v.y = r[1]; v.z = r[2]; v.w = r[3];
                *reinterpret_cast<f32x4 *>(a.out_r + e) = v;
            } else {
                a.out_r[e] = r[0];
            }
        }
        if (!a.out) return;
        if (a.z) {
#pragma unroll
            for (int j = 0; j < V; ++j) o[j] = zv[j] + (s[j] - zv[j]);
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) o[j] = s[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = gs * acc[j];
        if (a.g_zq) {
            if constexpr (V == 4) {
                const f32x4 v = *reinterpret_cast<const f32x4 *>(a.g_zq + e);
                o[0] = v.x + o[0]; o[1] = v.y + o[1]; o[2] = v.z + o[2]; o[3] = v.w + o[3];
            } else {
                o[0] = a.g_zq[e] + o[0];
            }
        }
    }
    if constexpr (V == 4) {
        f32x4 v;
        v.x = o[0]; v.y = o[1]; v.z = o[2]; v.w = o[3];
        *reinterpret_cast<f32x4 *>(a.out + e) = v;
    } else {
        a.out[e] = o[0];
    }
}

template <int V, int MODE>
__device__ __forceinline__ void rvq_walk(const RvqArgs &a, const RvqBooks &books) {
    const float gs = MODE == kRvqGradz ? (a.g_loss ? a.g_loss[0] : 1.0f) * a.scale : 0.0f;
    const long long units = a.total / V;                  // (V = 4: the launch has checked total % 4 == 0)
    for (long long u = (long long)blockIdx.x * 256 + threadIdx.x; u < units; u += (long long)gridDim.x * 256)
        rvq_unit<V, MODE>(a, books, u * V, gs);
}

// ---- the bodies of the three kernels (vq_residual.hip wraps each in a __global__ function and nothing else) ----------------------

// r_{q+1} = r_q - E_q[idx_q]: stage q0 only (q1 = q0 + 1).  z -> out for stage 0, in place (z == out) afterwards: a thread reads
// and writes its own elements only.
template <int V>
__device__ __forceinline__ void rvq_advance_body(const RvqArgs &a, const RvqBooks &books) {
    rvq_walk<V, kRvqAdvance>(a, books);
}

// S, z_q = z + (S - z) (z == NULL: z_q = S), on request r_Q; the first thread also adds the stage losses:
// loss = ((loss_0 + loss_1) + ...) in stage order.
template <int V>
__device__ __forceinline__ void rvq_finish_body(const RvqArgs &a, const RvqBooks &books) {
    if (a.loss && blockIdx.x == 0 && threadIdx.x == 0) {
        float l = a.loss_stage[0];
        for (int q = 1; q < a.Q; ++q) l = l + a.loss_stage[q];
        a.loss[0] = l;
    }
    rvq_walk<V, kRvqFinish>(a, books);
}

// grad_z = grad_zq + gs * ((r_1 + r_2) + ... + r_Q), the chain re-run in registers from z and the Q indices
template <int V>
__device__ __forceinline__ void rvq_gradz_body(const RvqArgs &a, const RvqBooks &books) {
    rvq_walk<V, kRvqGradz>(a, books);
}

}  // namespace vqvae
