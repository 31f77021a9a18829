// Host-side check of the rotation-trick gradient kernels: compiles vqvae_amd/csrc/vq_rotation.h -- the text the HIP kernels compile
// -- for the host and runs it thread by thread over a small grid in both layouts, both access widths and all three register
// forms.  Every output is compared bit for bit with a scalar loop in the order of vq_rotation.hip's header.  Zero rows, zero codes, antipodal rows, NaNs
// in g and in z and out-of-range indices are among the rows.  tests/test_vq_rotation_cpu.py builds it with the sanitizers on (and
// -ffp-contract=off, as the library).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define __device__
#define __forceinline__ inline
struct alignas(16) f32x4 { float x, y, z, w; };
struct Dim3 { unsigned x; };
static Dim3 blockIdx, gridDim, threadIdx;
#include "../../vqvae_amd/csrc/vq_rotation.h"
using namespace vqvae;

template <int DREG, int V> static void kernel(RotArgs a) { rot_gradz_body<DREG, V>(a); }

// a grid of at most 3 workgroups of 256 threads, one thread after the other: the grid-stride loop takes several steps
template <typename Kfn> static void run(Kfn k, RotArgs a) {
    long long g = (a.N + 255) / 256;
    g = g > 3 ? 3 : (g < 1 ? 1 : g);
    gridDim.x = (unsigned)g;
    for (unsigned bx = 0; bx < g; ++bx)
        for (unsigned t = 0; t < 256; ++t) { blockIdx.x = bx; threadIdx.x = t; k(a); }
}
static size_t pos(long long row, int c, int D, int HW, int rm) {
    if (rm) return (size_t)(row * D + c);
    const long long b = row / HW;
    return (size_t)((b * D + c) * HW + row % HW);
}

int main() {
    int bad = 0;
    struct Case { int B, HW, D, K; } cases[] = {{1, 1, 1, 1}, {3, 35, 1, 4}, {3, 15, 3, 7}, {3, 35, 64, 64}, {20, 64, 64, 96}, {2, 64, 48, 96},
                                                {2, 16, 256, 32}, {5, 12, 16, 9}, {5, 12, 20, 9}, {4, 9, 68, 5},
                                                {7, 55, 4, 6}, {3, 43, 60, 10}, {1, 9, 12, 4}, {9, 64, 8, 5}};
    for (auto cs : cases) for (int rm = 0; rm < 2; ++rm) for (int V : {1, 4}) for (int form = 0; form < 2; ++form) {
        const int D = cs.D, K = cs.K, HW = cs.HW;
        const long long N = (long long)cs.B * HW, total = N * D;
        if (V == 4 && (!rm || D % 4)) continue;
        const int dreg = form ? 0 : (D <= 16 ? 16 : (D <= 64 ? 64 : 0));          // form 1: the re-reading kernel at every width
        if (form && dreg == 0 && D > 64) continue;
        std::vector<float> z(total), g(total), cb((size_t)K * D), out(total, -7.f), want(total);
        std::vector<long long> idx(N);
        const float sc = (cs.K & 1) ? 0.05f : 1.0f;
        for (auto &v : z) v = sc * ((float)(rand() % 8192) / 4096.0f - 1.0f);
        for (auto &v : g) v = (float)(rand() % 8192) / 4096.0f - 1.0f;
        for (auto &v : cb) v = sc * ((float)(rand() % 8192) / 4096.0f - 1.0f);
        for (auto &i : idx) i = rand() % K;
        if (N >= 8) {
            for (int c = 0; c < D; ++c) z[pos(0, c, D, HW, rm)] = 0.f;                                    // a zero row of z
            for (int c = 0; c < D; ++c) cb[(size_t)(K - 1) * D + c] = 0.f;                                // a zero code
            idx[1] = K - 1;
            if (K >= 2) { for (int c = 0; c < D; ++c) cb[(size_t)(K - 2) * D + c] = -z[pos(2, c, D, HW, rm)]; idx[2] = K - 2; }   // antipodal
            g[pos(3, D / 2, D, HW, rm)] = NAN;
            z[pos(4, D - 1, D, HW, rm)] = NAN;
            idx[5] = K; idx[6] = -1;                                                                       // out of range: NaN, no read
            z[pos(7, 0, D, HW, rm)] = INFINITY;
        }
        const float gl = 0.7f, scale = (float)(2.0 / ((double)N * D)), gs = gl * scale;
        // the contract, one scalar at a time
        for (long long row = 0; row < N; ++row) {
            const long long k = idx[row];
            const bool ok = k >= 0 && k < K;
            double ee = 0, qq = 0, eq = 0, eg = 0, qg = 0;
            for (int c = 0; c < D; ++c) {
                const double e_ = z[pos(row, c, D, HW, rm)], q_ = ok ? cb[(size_t)k * D + c] : NAN, g_ = g[pos(row, c, D, HW, rm)];
                ee = ee + e_ * e_; qq = qq + q_ * q_; eq = eq + e_ * q_; eg = eg + e_ * g_; qg = qg + q_ * g_;
            }
            const double ne = std::sqrt(ee), nq = std::sqrt(qq), p = ne * nq, ns2 = 2.0 + 2.0 * (eq / p);
            const bool rotate = ee > 0 && qq > 0 && std::isfinite(ee) && std::isfinite(qq) && ns2 >= std::ldexp(1.0, -20);
            const double a = (eg / ne + qg / nq) / ns2, ce = (2.0 * qg) / p - (2.0 * a) / ne, cq = -((2.0 * a) / nq), lam = nq / ne;
            for (int c = 0; c < D; ++c) {
                const float zf = z[pos(row, c, D, HW, rm)], qf = ok ? cb[(size_t)k * D + c] : NAN, gf = g[pos(row, c, D, HW, rm)];
                const float rot = rotate ? (float)(lam * (((double)gf + ce * (double)zf) + cq * (double)qf)) : gf;
                const float d = zf - qf, s = gs * d;
                want[pos(row, c, D, HW, rm)] = rot + s;
            }
            if (N >= 8 && row < 3 && rotate) { printf("row %lld of D=%d rm=%d must not rotate\n", row, D, rm); ++bad; }
        }
        RotArgs a = {};
        a.z = z.data(); a.cb = cb.data(); a.idx = idx.data(); a.g_zq = g.data(); a.g_loss = &gl; a.N = N; a.D = D; a.HW = HW; a.K = K;
        a.rowmajor = rm; a.scale = scale; a.out = out.data();
        if (V == 4) { if (dreg == 16) run(kernel<16, 4>, a); else if (dreg == 64) run(kernel<64, 4>, a); else run(kernel<0, 4>, a); }
        else { if (dreg == 16) run(kernel<16, 1>, a); else if (dreg == 64) run(kernel<64, 1>, a); else run(kernel<0, 1>, a); }
        long long nans = 0;
        for (long long i = 0; i < total; ++i) {
            if (std::isnan(out[i]) && std::isnan(want[i])) { ++nans; continue; }
            if (memcmp(&out[i], &want[i], 4)) {
                printf("MISMATCH B=%d HW=%d D=%d rm=%d V=%d dreg=%d at %lld: %a %a\n", cs.B, HW, D, rm, V, dreg, i, out[i], want[i]); ++bad; break; }
        }
        // a NaN stays in its row: rows 3 (g), 4 (z: not rotated, one element), 5, 6 (bad index), 7 (inf) and nothing else
        if (N >= 8) {
            for (long long row = 8; row < N; ++row) for (int c = 0; c < D; ++c)
                if (std::isnan(out[pos(row, c, D, HW, rm)])) { printf("NaN escaped to row %lld (D=%d rm=%d)\n", row, D, rm); ++bad; row = N; break; }
            for (long long row = 0; row < 3; ++row) for (int c = 0; c < D; ++c)
                if (std::isnan(out[pos(row, c, D, HW, rm)])) { printf("NaN in fallback row %lld (D=%d rm=%d)\n", row, D, rm); ++bad; row = 3; break; }
        }
        (void)nans;
    }
    printf(bad ? "FAILED %d\n" : "emulation ok\n", bad);
    return bad != 0;
}
