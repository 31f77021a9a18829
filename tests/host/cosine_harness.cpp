// Host-side check of the l2-normalisation kernels: compiles vqvae_amd/csrc/vq_cosine.h -- the text the HIP kernels compile -- for the
// host and runs it over small grids, forward and backward, in both layouts, both access widths, the register forms, the re-reading
// form and the LDS forms (one chunk kept in the tile; wide rows staged twice).  The NCHW bodies run thread by thread; a workgroup of
// the row-major bodies runs as 256 host threads that meet at a barrier where the kernel has __syncthreads().  Every output is compared
// bit for bit with a scalar loop in the order of vq_cosine.hip's header.  Zero rows, rows below eps, NaN and Inf rows are among the
// rows.  tests/test_vq_cosine_cpu.py builds it with the sanitizers on (and -ffp-contract=off, as the library).
#include "device_shim.h"
#include "../../vqvae_amd/csrc/vq_cosine.h"
using namespace vqvae;

template <bool BWD, int DREG, int V> static void nchw_kernel(L2nArgs a) { l2n_nchw_body<BWD, DREG, V>(a); }

template <typename Kfn> static void run_nchw(Kfn k, L2nArgs a, int V) {
    const long long g = (a.N / V + 255) / 256;
    for (long long bx = 0; bx < (g < 1 ? 1 : g); ++bx)
        for (unsigned t = 0; t < 256; ++t) { blockIdx.x = (unsigned)bx; threadIdx.x = t; k(a); }
}

alignas(16) static float g_lds[kL2Waves * 2 * kL2TileFloats];

template <bool BWD, int V> static void run_rows(L2nArgs a) {
    run_grid((a.N + 64 * kL2Waves - 1) / (64 * kL2Waves), 1, 256, [] { for (auto &v : g_lds) v = 0.f; }, [=] { l2n_rows_body<BWD, V>(a, g_lds); });
}

static size_t pos(long long row, int c, int D, int HW, int rm) {
    if (rm) return (size_t)(row * D + c);
    const long long b = row / HW;
    return (size_t)((b * D + c) * HW + row % HW);
}

int main() {
    int bad = 0;
    struct Case { int B, HW, D; } cases[] = {{1, 1, 1}, {3, 35, 1}, {3, 15, 3}, {3, 35, 64}, {5, 64, 64}, {2, 64, 48}, {2, 16, 256}, {5, 12, 16},
                                             {5, 12, 20}, {4, 9, 68}, {9, 36, 130}, {3, 43, 60}, {1, 300, 5}, {7, 44, 256}};
    const float eps = 1e-12f;
    for (auto cs : cases) for (int rm = 0; rm < 2; ++rm) for (int V : {1, 4}) for (int form = 0; form < 2; ++form) {
        const int D = cs.D, HW = cs.HW;
        const long long N = (long long)cs.B * HW, total = N * D;
        if (V == 4 && (rm ? D % 4 : HW % 4)) continue;
        // NCHW: form 0 = the register form the launch picks, form 1 = the re-reading kernel at every width; row-major has one form
        const int dreg = form ? 0 : (D <= 16 ? 16 : (D <= 64 && V == 1 ? 64 : 0));
        if (rm && form) continue;
        if (!rm && form && dreg == 0 && (D > 64 || (V == 4 && D > 16))) continue;
        std::vector<float> x(total), g(total), y(total, -7.f), den(N, -7.f), gx(total, -7.f), wy(total), wden(N), wgx(total);
        const float sc = (cs.B & 1) ? 0.05f : 1.0f;
        for (auto &v : x) v = sc * ((float)(rand() % 8192) / 4096.0f - 1.0f);
        for (auto &v : g) v = (float)(rand() % 8192) / 4096.0f - 1.0f;
        if (N >= 8) {
            for (int c = 0; c < D; ++c) x[pos(0, c, D, HW, rm)] = 0.f;                                     // a zero row
            for (int c = 0; c < D; ++c) x[pos(1, c, D, HW, rm)] = (c & 1) ? 1e-20f : -1e-21f;              // a norm below eps
            x[pos(3, D / 2, D, HW, rm)] = NAN;
            x[pos(4, D - 1, D, HW, rm)] = INFINITY;
            g[pos(5, 0, D, HW, rm)] = NAN;
            for (int c = 0; c < D; ++c) x[pos(6, c, D, HW, rm)] = 3e18f;                                    // the fp32 sum would overflow
        }
        // the contract, one scalar at a time
        for (long long row = 0; row < N; ++row) {
            double s = 0.0;
            for (int c = 0; c < D; ++c) { const double v = x[pos(row, c, D, HW, rm)]; s = s + v * v; }
            float d = (float)std::sqrt(s);
            d = (d < eps) ? eps : d;
            wden[row] = d;
            for (int c = 0; c < D; ++c) wy[pos(row, c, D, HW, rm)] = x[pos(row, c, D, HW, rm)] / d;
            double t = 0.0;
            for (int c = 0; c < D; ++c) t = t + (double)wy[pos(row, c, D, HW, rm)] * (double)g[pos(row, c, D, HW, rm)];
            for (int c = 0; c < D; ++c) {
                const float yf = wy[pos(row, c, D, HW, rm)], gf = g[pos(row, c, D, HW, rm)];
                wgx[pos(row, c, D, HW, rm)] = d > eps ? (float)(((double)gf - (double)yf * t) / (double)d) : (float)((double)gf / (double)eps);
            }
        }
        L2nArgs f = {};
        f.x = x.data(); f.out = y.data(); f.denom_out = den.data(); f.N = N; f.D = D; f.HW = HW; f.eps = eps;
        L2nArgs b = {};
        b.x = wy.data(); b.g = g.data(); b.denom_in = wden.data(); b.out = gx.data(); b.N = N; b.D = D; b.HW = HW; b.eps = eps;
        if (rm) {
            if (V == 4) { run_rows<false, 4>(f); run_rows<true, 4>(b); }
            else { run_rows<false, 1>(f); run_rows<true, 1>(b); }
        } else if (V == 4) {
            if (dreg == 16) { run_nchw(nchw_kernel<false, 16, 4>, f, 4); run_nchw(nchw_kernel<true, 16, 4>, b, 4); }
            else { run_nchw(nchw_kernel<false, 0, 4>, f, 4); run_nchw(nchw_kernel<true, 0, 4>, b, 4); }
        } else {
            if (dreg == 16) { run_nchw(nchw_kernel<false, 16, 1>, f, 1); run_nchw(nchw_kernel<true, 16, 1>, b, 1); }
            else if (dreg == 64) { run_nchw(nchw_kernel<false, 64, 1>, f, 1); run_nchw(nchw_kernel<true, 64, 1>, b, 1); }
            else { run_nchw(nchw_kernel<false, 0, 1>, f, 1); run_nchw(nchw_kernel<true, 0, 1>, b, 1); }
        }
        for (long long i = 0; i < total; ++i)
            if (!same(y[i], wy[i]) || !same(gx[i], wgx[i])) {
                printf("MISMATCH B=%d HW=%d D=%d rm=%d V=%d dreg=%d at %lld: y %a %a  gx %a %a\n", cs.B, HW, D, rm, V, dreg, i, y[i], wy[i],
                       gx[i], wgx[i]);
                ++bad;
                break;
            }
        for (long long i = 0; i < N; ++i)
            if (!same(den[i], wden[i])) { printf("DENOM B=%d HW=%d D=%d rm=%d V=%d at %lld: %a %a\n", cs.B, HW, D, rm, V, i, den[i], wden[i]); ++bad; break; }
        if (N >= 8) {
            // the clamp rows: y = x / eps (zero stays zero), grad_x = g / eps; the NaN / Inf rows keep them; nothing escapes
            if (den[0] != eps || den[1] != eps) { printf("clamp rows: denom %a %a (D=%d rm=%d)\n", den[0], den[1], D, rm); ++bad; }
            for (int c = 0; c < D; ++c) {
                if (y[pos(0, c, D, HW, rm)] != 0.f) { printf("zero row: y != 0 (D=%d rm=%d)\n", D, rm); ++bad; break; }
                if (gx[pos(0, c, D, HW, rm)] != (float)((double)g[pos(0, c, D, HW, rm)] / (double)eps)) { printf("zero row: gx (D=%d rm=%d)\n", D, rm); ++bad; break; }
            }
            if (!std::isnan(den[3]) || !std::isinf(den[4])) { printf("NaN / Inf rows: denom %a %a\n", den[3], den[4]); ++bad; }
            if (!std::isfinite(den[6])) { printf("row 6 overflowed in fp64?\n"); ++bad; }
            for (long long row = 0; row < N; ++row) for (int c = 0; c < D; ++c) {
                const bool nan_ok = row == 3 || row == 4 || row == 5;
                if (!nan_ok && (std::isnan(y[pos(row, c, D, HW, rm)]) || std::isnan(gx[pos(row, c, D, HW, rm)]))) {
                    printf("NaN escaped to row %lld (D=%d rm=%d V=%d)\n", row, D, rm, V); ++bad; row = N; break; }
            }
        }
    }
    printf(bad ? "FAILED %d\n" : "emulation ok\n", bad);
    return bad != 0;
}
