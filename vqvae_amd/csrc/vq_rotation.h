// The rotation-trick z gradient (vq_rotation.hip, whose header states the arithmetic): the per-row coefficients from the five sums,
// and the whole body of the kernel -- one lane owns one row, so there is no cross-lane step.  Plain C++ over
// `__device__ __forceinline__`, so that tests/host/rotation_harness.cpp compiles THIS text for the host (blockIdx / threadIdx /
// gridDim and f32x4 supplied by the harness) and compares it with a scalar loop, bit for bit and under the sanitizers.
#pragma once

namespace vqvae {

constexpr double kRotMinNs2 = 0x1p-20;    // below this ||e^ + q^||^2 the reflection axis is taken as undefined: straight-through

struct RotCoef {
    bool rotate;                          // false: the row keeps grad_zq (zero row, zero code, non-finite norm, antipodal)
    double ce, cq, lam;                   // rot_c = lam * ((g_c + ce * e_c) + cq * q_c)
};

// The five fp64 sums of a row -> its coefficients.  Every operation is one IEEE fp64 operation (the library and the harness are
// compiled with -ffp-contract=off; sqrt and the divisions are correctly rounded).
__device__ __forceinline__ RotCoef rot_coef(double ee, double qq, double eq, double eg, double qg) {
    const double inf = __builtin_huge_val();
    const double ne = __builtin_sqrt(ee), nq = __builtin_sqrt(qq), p = ne * nq;
    const double ns2 = 2.0 + 2.0 * (eq / p);
    RotCoef r;
    r.rotate = ee > 0.0 && qq > 0.0 && ee < inf && qq < inf && ns2 >= kRotMinNs2;      // (a NaN fails every comparison)
    const double a = (eg / ne + qg / nq) / ns2;
    r.ce = (2.0 * qg) / p - (2.0 * a) / ne;
    r.cq = -((2.0 * a) / nq);
    r.lam = nq / ne;
    return r;
}

struct RotSums {
    double ee = 0.0, qq = 0.0, eq = 0.0, eg = 0.0, qg = 0.0;
};

// channel c of a row joins its five sums (call in ascending c: the order is the contract)
__device__ __forceinline__ void rot_add(RotSums &s, float z, float q, float g) {
    const double e_ = (double)z, q_ = (double)q, g_ = (double)g;
    s.ee = s.ee + e_ * e_;
    s.qq = s.qq + q_ * q_;
    s.eq = s.eq + e_ * q_;
    s.eg = s.eg + e_ * g_;
    s.qg = s.qg + q_ * g_;
}

// grad_z of one element: rot_c, rounded to fp32 once (g_c itself where the row is not rotated), plus the loss term in fp32 as
// vqb_gradz_kernel forms it
__device__ __forceinline__ float rot_out(const RotCoef &co, float z, float q, float g, float gs) {
    const double t = co.lam * (((double)g + co.ce * (double)z) + co.cq * (double)q);
    const float rot = co.rotate ? (float)t : g;
    const float d = z - q;
    const float s = gs * d;
    return rot + s;
}

struct RotArgs {
    const float *z, *cb;                  // z: (N, D) rows or (B, D, HW) maps; cb: (K, D)
    const long long *idx;                 // (N)
    const float *g_zq, *g_loss;           // g_zq: z's layout, never NULL here; g_loss: device scalar or NULL (= 1)
    long long N;
    int D, HW, K, rowmajor;
    float scale;                          // fp32(2 / (N D)), or fp32(2 beta / (N D)) for the commitment-only loss
    float *out;                           // grad_z
};

// V consecutive channels of a row from element offset `o` on (V = 4: one 16-byte access; the launch has checked alignment, D % 4 == 0
// and the row-major layout, where a row's channels are adjacent)
template <int V>
__device__ __forceinline__ void rot_load(const float *p, size_t o, float *v) {
    if constexpr (V == 4) {
        const f32x4 t = *reinterpret_cast<const f32x4 *>(p + o);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = p[o];
    }
}

// One row.  Pass 1 adds the five sums channel by channel in ascending order; pass 2 writes the gradient.  DREG > 0 (D <= DREG): z and
// g stay in registers between the passes, so they are read once; DREG = 0: pass 2 reads them again (the lane's own lines, just
// used).  The code row is read in both passes: it comes through L2 either way.  An index outside [0, K) never reads the codebook:
// its code is NaN, so the row is not rotated and its gradient is NaN, as the code term of the straight-through form would be.
template <int DREG, int V>
__device__ __forceinline__ void rot_row(const RotArgs &a, long long row, float gs) {
    const int D = a.D;
    size_t base, stride;
    if (a.rowmajor) {
        base = (size_t)row * D;
        stride = 1;
    } else {
        const long long b = row / a.HW;
        base = (size_t)b * D * a.HW + (size_t)(row - b * a.HW);
        stride = (size_t)a.HW;
    }
    const long long k = a.idx[row];
    const bool ok = k >= 0 && k < a.K;
    const float *q = a.cb + (ok ? (size_t)k * D : 0);
    constexpr int R = DREG > 0 ? DREG : V;
    float zr[R], gr[R];
    RotSums sm;
    auto sums = [&](const float *zv, const float *gv, const float *qv) {
#pragma unroll
        for (int j = 0; j < V; ++j) rot_add(sm, zv[j], qv[j], gv[j]);
    };
    auto code = [&](int c, float *qv) {
        if (ok) {
            rot_load<V>(q, (size_t)c, qv);
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) qv[j] = __builtin_nanf("");
        }
    };
    if constexpr (DREG > 0) {
#pragma unroll
        for (int c = 0; c < DREG; c += V)
            if (c < D) {
                rot_load<V>(a.z, base + c * stride, zr + c);
                rot_load<V>(a.g_zq, base + c * stride, gr + c);
            }
#pragma unroll
        for (int c = 0; c < DREG; c += V)
            if (c < D) {
                float qv[V];
                code(c, qv);
                sums(zr + c, gr + c, qv);
            }
    } else {
        for (int c = 0; c < D; c += V) {
            float qv[V];
            rot_load<V>(a.z, base + c * stride, zr);
            rot_load<V>(a.g_zq, base + c * stride, gr);
            code(c, qv);
            sums(zr, gr, qv);
        }
    }
    const RotCoef co = rot_coef(sm.ee, sm.qq, sm.eq, sm.eg, sm.qg);
    auto emit = [&](int c, const float *zv, const float *gv, const float *qv) {
        float o[V];
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = rot_out(co, zv[j], qv[j], gv[j], gs);
        if constexpr (V == 4) {
            f32x4 t;
            t.x = o[0]; t.y = o[1]; t.z = o[2]; t.w = o[3];
            *reinterpret_cast<f32x4 *>(a.out + base + c * stride) = t;
        } else {
            a.out[base + c * stride] = o[0];
        }
    };
    if constexpr (DREG > 0) {
#pragma unroll
        for (int c = 0; c < DREG; c += V)
            if (c < D) {
                float qv[V];
                code(c, qv);
                emit(c, zr + c, gr + c, qv);
            }
    } else {
        for (int c = 0; c < D; c += V) {
            float qv[V];
            rot_load<V>(a.z, base + c * stride, zr);
            rot_load<V>(a.g_zq, base + c * stride, gr);
            code(c, qv);
            emit(c, zr, gr, qv);
        }
    }
}

// ---- the body of the kernel (vq_rotation.hip wraps it in a __global__ function and nothing else) --------------------------------
template <int DREG, int V>
__device__ __forceinline__ void rot_gradz_body(const RotArgs &a) {
    const float gs = (a.g_loss ? a.g_loss[0] : 1.0f) * a.scale;
    for (long long row = (long long)blockIdx.x * 256 + threadIdx.x; row < a.N; row += (long long)gridDim.x * 256)
        rot_row<DREG, V>(a, row, gs);
}

#ifdef __HIPCC__
// vq_rotation.hip: picks the access width (alignment, D % 4, layout) and the register form (D <= 16, D <= 64, wider) and launches
void launch_vq_rotation_gradz(const RotArgs &a, hipStream_t st);
#endif

}  // namespace vqvae
