// Host-side check of the residual quantizer's element-wise kernels: compiles vqvae_amd/csrc/vq_residual.h -- the text the HIP
// kernels compile -- for the host, runs it thread by thread over a small grid in both layouts and both access widths, out of place
// and in place, with out-of-range indices among the rows, and compares every output bit for bit with a scalar loop in the order of
// vq_residual.hip's header.  tests/test_vq_residual_cpu.py builds it with the sanitizers on.
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
#include "../../vqvae_amd/csrc/vq_residual.h"
using namespace vqvae;

// the three kernels: vq_residual.hip wraps exactly these bodies
template <int V> static void rvq_advance_kernel(RvqArgs a, RvqBooks books) { rvq_advance_body<V>(a, books); }
template <int V> static void rvq_finish_kernel(RvqArgs a, RvqBooks books) { rvq_finish_body<V>(a, books); }
template <int V> static void rvq_gradz_kernel(RvqArgs a, RvqBooks books) { rvq_gradz_body<V>(a, books); }

// a grid of at most 7 workgroups of 256 threads, one thread after the other: the grid-stride loops take several steps
template <typename Kfn> static void run(Kfn k, RvqArgs a, RvqBooks b, int V) {
    long long units = a.total / V, g = (units + 255) / 256;
    g = g > 7 ? 7 : (g < 1 ? 1 : g);
    gridDim.x = (unsigned)g;
    for (unsigned bx = 0; bx < g; ++bx)
        for (unsigned t = 0; t < 256; ++t) { blockIdx.x = bx; threadIdx.x = t; k(a, b); }
}
// element c of row `row`: row-major rows, or NCHW images of HW pixels
static size_t pos(long long row, int c, int D, int HW, int rm) {
    if (rm) return (size_t)(row * D + c);
    const long long b = row / HW;
    return (size_t)((b * D + c) * HW + row % HW);
}
static float at(const std::vector<float> &z, long long row, int c, int D, int HW, int rm) { return z[pos(row, c, D, HW, rm)]; }
static float &at(std::vector<float> &z, long long row, int c, int D, int HW, int rm) { return z[pos(row, c, D, HW, rm)]; }
int main() {
    int bad = 0;
    struct Case { int B, HW, D, K, Q; } cases[] = {{3, 64, 64, 96, 3}, {2, 15, 48, 64, 4}, {5, 32, 3, 5, 2}, {40, 64, 8, 7, 16}, {2, 15, 4, 9, 1}};
    for (auto cs : cases) for (int rm = 0; rm < 2; ++rm) for (int V : {1, 4}) {
        long long N = (long long)cs.B * cs.HW, total = N * cs.D;
        if (V == 4 && (rm ? cs.D % 4 : cs.HW % 4)) continue;
        std::vector<float> z(total), gzq(total); std::vector<std::vector<float>> cb(cs.Q, std::vector<float>((size_t)cs.K * cs.D));
        std::vector<long long> idx((size_t)cs.Q * N);
        for (auto &v : z) v = (float)(rand() % 4096) / 4096.0f - 0.5f;
        for (auto &v : gzq) v = (float)(rand() % 4096) / 4096.0f;
        for (auto &c : cb) for (auto &v : c) v = (float)(rand() % 4096) / 4096.0f - 0.5f;
        for (auto &i : idx) i = rand() % cs.K;
        idx[5] = cs.K; idx[N > 9 ? 9 : 0] = -1;                       // out of range: NaN, no read
        RvqBooks books; for (int q = 0; q < 16; ++q) books.cb[q] = q < cs.Q ? cb[q].data() : nullptr;
        RvqArgs a = {}; a.idx = idx.data(); a.N = N; a.total = total; a.D = cs.D; a.HW = cs.HW; a.K = cs.K; a.rowmajor = rm; a.Q = cs.Q;
        // reference
        std::vector<float> r = z, S(total), A(total), zq(total), gz(total);
        float gl = 0.7f, scale = (float)(2.0 / ((double)N * cs.D)), gs = gl * scale;
        for (long long row = 0; row < N; ++row) for (int c = 0; c < cs.D; ++c) {
            float rr = at(z, row, c, cs.D, cs.HW, rm), s = 0, acc = 0;
            for (int q = 0; q < cs.Q; ++q) { long long k = idx[(size_t)q * N + row]; float e = (k >= 0 && k < cs.K) ? cb[q][k * cs.D + c] : NAN;
                s = q ? s + e : e; rr = rr - e; acc = q ? acc + rr : rr; }
            float zz = at(z, row, c, cs.D, cs.HW, rm);
            at(r, row, c, cs.D, cs.HW, rm) = rr; at(S, row, c, cs.D, cs.HW, rm) = s; at(zq, row, c, cs.D, cs.HW, rm) = zz + (s - zz);
            at(gz, row, c, cs.D, cs.HW, rm) = at(gzq, row, c, cs.D, cs.HW, rm) + gs * acc; }
        auto same = [&](const std::vector<float>& x, const std::vector<float>& y, const char *what) {
            for (long long i = 0; i < total; ++i) if (memcmp(&x[i], &y[i], 4) && !(std::isnan(x[i]) && std::isnan(y[i]))) {
                printf("MISMATCH %s B=%d HW=%d D=%d rm=%d V=%d at %lld: %g %g\n", what, cs.B, cs.HW, cs.D, rm, V, i, x[i], y[i]); ++bad; return; } };
        // advance chain (stage 0 out of place, then in place)
        std::vector<float> res(total, -7.f);
        for (int q = 0; q < cs.Q; ++q) { RvqArgs b = a; b.z = q ? res.data() : z.data(); b.out = res.data(); b.q0 = q; b.q1 = q + 1;
            if (V == 4) run(rvq_advance_kernel<4>, b, books, 4); else run(rvq_advance_kernel<1>, b, books, 1); }
        same(res, r, "advance");
        // finish
        std::vector<float> ozq(total, -7.f), orr(total, -7.f), ls(cs.Q, 0.25f); float loss = -1;
        { RvqArgs b = a; b.z = z.data(); b.q0 = 0; b.q1 = cs.Q; b.out = ozq.data(); b.out_r = orr.data(); b.loss_stage = ls.data(); b.loss = &loss;
          if (V == 4) run(rvq_finish_kernel<4>, b, books, 4); else run(rvq_finish_kernel<1>, b, books, 1); }
        same(ozq, zq, "z_q"); same(orr, r, "r_Q"); if (loss != 0.25f * cs.Q) { printf("loss %g\n", loss); ++bad; }
        { RvqArgs b = a; b.z = nullptr; b.q0 = 0; b.q1 = cs.Q; b.out = ozq.data();
          if (V == 4) run(rvq_finish_kernel<4>, b, books, 4); else run(rvq_finish_kernel<1>, b, books, 1); }
        same(ozq, S, "decode");
        { RvqArgs b = a; b.z = z.data(); b.q0 = 0; b.q1 = cs.Q; b.out = nullptr; b.out_r = nullptr; b.loss_stage = ls.data(); b.loss = &loss; b.total = 0;
          run(rvq_finish_kernel<1>, b, books, 1); }
        // gradz
        std::vector<float> ogz(total, -7.f);
        { RvqArgs b = a; b.z = z.data(); b.q0 = 0; b.q1 = cs.Q; b.out = ogz.data(); b.g_zq = gzq.data(); b.g_loss = &gl; b.scale = scale;
          if (V == 4) run(rvq_gradz_kernel<4>, b, books, 4); else run(rvq_gradz_kernel<1>, b, books, 1); }
        same(ogz, gz, "grad_z");
    }
    printf(bad ? "FAILED %d\n" : "emulation ok\n", bad);
    return bad != 0;
}
