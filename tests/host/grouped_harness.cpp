// Host-side check of the grouped quantizer's element-wise kernels: compiles vqvae_amd/csrc/vq_grouped.h -- the text the HIP kernels
// compile -- for the host, runs it thread by thread over a small grid in both layouts and both access widths, with G up to 16,
// d = 1 and out-of-range indices among the rows, and compares every output bit for bit with scalar loops in the order of
// vq_grouped.hip's header, with both types of element arithmetic.  tests/test_vq_grouped_cpu.py builds it with the sanitizers on:
// every buffer has its exact size.
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
#include "../../vqvae_amd/csrc/vq_grouped.h"
using namespace vqvae;

// the kernels: vq_grouped.hip wraps exactly these bodies
template <int V, typename I> static void grp_split_kernel(GrpArgs a, GrpBooks) { grp_split_body<V, I>(a); }
template <int V, typename I> static void grp_finish_kernel(GrpArgs a, GrpBooks books) { grp_finish_body<V, I>(a, books); }
template <int V, typename I> static void grp_gradz_kernel(GrpArgs a, GrpBooks books) { grp_gradz_body<V, I>(a, books); }

// a grid of at most 7 workgroups of 256 threads, one thread after the other: the grid-stride loops take several steps
template <typename Kfn> static void run(Kfn k, GrpArgs a, GrpBooks b, int V) {
    long long units = a.total / V, g = (units + 255) / 256;
    g = g > 7 ? 7 : (g < 1 ? 1 : g);
    gridDim.x = (unsigned)g;
    for (unsigned bx = 0; bx < g; ++bx)
        for (unsigned t = 0; t < 256; ++t) { blockIdx.x = bx; threadIdx.x = t; k(a, b); }
}
// (wide: the long long element arithmetic of launches with N D >= 2^32; else the unsigned one)
static bool wide = false;
#define RUN(KERNEL, A, BOOKS, V)                                                                                      \
    do {                                                                                                              \
        if (wide) { if ((V) == 4) run(KERNEL<4, long long>, A, BOOKS, 4); else run(KERNEL<1, long long>, A, BOOKS, 1); } \
        else { if ((V) == 4) run(KERNEL<4, unsigned>, A, BOOKS, 4); else run(KERNEL<1, unsigned>, A, BOOKS, 1); }        \
    } while (0)

// element c of row `row` of a map with C channels: row-major rows, or NCHW images of HW pixels
static size_t pos(long long row, int c, int C, int HW, int rm) {
    if (rm) return (size_t)(row * C + c);
    const long long b = row / HW;
    return (size_t)((b * C + c) * HW + row % HW);
}

static int bad = 0;
static void same(const std::vector<float> &x, const std::vector<float> &y, const char *what, int B, int HW, int D, int G, int rm, int V) {
    if (x.size() != y.size()) { printf("SIZE %s\n", what); ++bad; return; }
    for (size_t i = 0; i < x.size(); ++i)
        if (memcmp(&x[i], &y[i], 4) && !(std::isnan(x[i]) && std::isnan(y[i]))) {
            printf("MISMATCH %s B=%d HW=%d D=%d G=%d rm=%d V=%d at %zu: %g %g\n", what, B, HW, D, G, rm, V, i, x[i], y[i]);
            ++bad;
            return;
        }
}

int main() {
    struct Case { int B, HW, D, K, G; } cases[] = {{3, 64, 64, 96, 2}, {2, 15, 48, 64, 3}, {5, 32, 3, 5, 3}, {4, 8, 64, 7, 16},
                                                   {2, 15, 16, 9, 16}, {3, 16, 6, 5, 3}, {2, 12, 8, 9, 1}, {40, 64, 32, 11, 4}};
    for (auto cs : cases) for (int rm = 0; rm < 2; ++rm) for (int V : {1, 4}) for (int w = 0; w < 2; ++w) {
        wide = w != 0;
        const int d = cs.D / cs.G;
        const long long N = (long long)cs.B * cs.HW, total = N * cs.D, slab = N * d;
        if (V == 4 && (rm ? d % 4 : cs.HW % 4)) continue;
        std::vector<float> z(total), gzq(total);
        std::vector<std::vector<float>> cb(cs.G, std::vector<float>((size_t)cs.K * d));
        std::vector<long long> idx((size_t)cs.G * N);
        for (auto &v : z) v = (float)(rand() % 4096) / 4096.0f - 0.5f;
        z[3] = -0.0f; z[7] = INFINITY; z[11] = NAN;
        for (auto &v : gzq) v = (float)(rand() % 4096) / 4096.0f;
        for (auto &c : cb) for (auto &v : c) v = (float)(rand() % 4096) / 4096.0f - 0.5f;
        for (auto &i : idx) i = rand() % cs.K;
        idx[5] = cs.K;                                                    // group 0, row 5: out of range -> NaN, no read
        idx[(size_t)(cs.G - 1) * N + (N > 9 ? 9 : 0)] = -1;               // the last group, row 9
        GrpBooks books; for (int g = 0; g < kGrpMaxGroups; ++g) books.cb[g] = g < cs.G ? cb[g].data() : nullptr;
        GrpArgs a = {}; a.idx = idx.data(); a.N = N; a.total = total; a.D = cs.D; a.d = d; a.HW = cs.HW; a.K = cs.K; a.rowmajor = rm;
        a.G = cs.G; a.g0 = 0; a.g1 = cs.G;
        // reference: scalar loops
        const float gl = 0.7f, scale = (float)(2.0 / ((double)N * d)), gq = gl / (float)cs.G, gs = gq * scale;
        std::vector<float> slabs(total), zq(total), dec(total), gz(total), gz0(total);
        for (long long row = 0; row < N; ++row) for (int c = 0; c < cs.D; ++c) {
            const int g = c / d, cc = c % d;
            const size_t p = pos(row, c, cs.D, cs.HW, rm);
            const long long k = idx[(size_t)g * N + row];
            const float e = (k >= 0 && k < cs.K) ? cb[g][(size_t)k * d + cc] : NAN, zz = z[p];
            slabs[(size_t)g * slab + pos(row, cc, d, cs.HW, rm)] = zz;
            zq[p] = zz + (e - zz);
            dec[p] = e;
            const float t = gs * (zz - e);
            gz0[p] = t;
            gz[p] = gzq[p] + t;
        }
        // split: every group at once with a second copy, then each group alone
        std::vector<float> os(total, -7.f), os2(total, -7.f);
        { GrpArgs b = a; b.z = z.data(); b.out = os.data(); b.out2 = os2.data(); RUN(grp_split_kernel, b, books, V); }
        same(os, slabs, "split", cs.B, cs.HW, cs.D, cs.G, rm, V); same(os2, slabs, "split copy", cs.B, cs.HW, cs.D, cs.G, rm, V);
        for (int g = 0; g < cs.G; ++g) {
            std::vector<float> one(slab, -7.f), want(slabs.begin() + (size_t)g * slab, slabs.begin() + (size_t)(g + 1) * slab);
            GrpArgs b = a; b.z = z.data(); b.out = one.data(); b.g0 = g; b.g1 = g + 1; b.total = slab;
            RUN(grp_split_kernel, b, books, V);
            same(one, want, "split one", cs.B, cs.HW, cs.D, cs.G, rm, V);
        }
        // finish: z_q and the mean of the group losses; decode; the loss alone
        std::vector<float> ozq(total, -7.f), lg(cs.G);
        float loss = -1, want_loss = 0;
        for (int g = 0; g < cs.G; ++g) { lg[g] = 0.1f * (float)(g + 1) + 0.013f; want_loss = g ? want_loss + lg[g] : lg[g]; }
        want_loss = want_loss / (float)cs.G;
        { GrpArgs b = a; b.z = z.data(); b.out = ozq.data(); b.loss_group = lg.data(); b.loss = &loss; RUN(grp_finish_kernel, b, books, V); }
        same(ozq, zq, "z_q", cs.B, cs.HW, cs.D, cs.G, rm, V);
        if (memcmp(&loss, &want_loss, 4)) { printf("loss %g %g\n", loss, want_loss); ++bad; }
        { GrpArgs b = a; b.z = nullptr; b.out = ozq.data(); RUN(grp_finish_kernel, b, books, V); }
        same(ozq, dec, "decode", cs.B, cs.HW, cs.D, cs.G, rm, V);
        loss = -1;
        { GrpArgs b = a; b.z = z.data(); b.out = nullptr; b.loss_group = lg.data(); b.loss = &loss; b.total = 0; RUN(grp_finish_kernel, b, books, 1); }
        if (memcmp(&loss, &want_loss, 4)) { printf("loss alone %g %g\n", loss, want_loss); ++bad; }
        // grad_z with and without an upstream gradient of z_q
        std::vector<float> ogz(total, -7.f);
        { GrpArgs b = a; b.z = z.data(); b.out = ogz.data(); b.g_zq = gzq.data(); b.g_loss = &gl; b.scale = scale; RUN(grp_gradz_kernel, b, books, V); }
        same(ogz, gz, "grad_z", cs.B, cs.HW, cs.D, cs.G, rm, V);
        { GrpArgs b = a; b.z = z.data(); b.out = ogz.data(); b.g_loss = &gl; b.scale = scale; RUN(grp_gradz_kernel, b, books, V); }
        same(ogz, gz0, "grad_z alone", cs.B, cs.HW, cs.D, cs.G, rm, V);
    }
    printf(bad ? "FAILED %d\n" : "emulation ok\n", bad);
    return bad != 0;
}
