// Host-side check of the per-row linear map's kernels: compiles vqvae_amd/csrc/vq_linear.h -- the text the HIP kernels compile -- for
// the host and runs the forward, grad_x, the parameter gradients' block kernel and their second launch over the GPU test's shapes, in
// both layouts and on both access paths (16 bytes or one element per lane), with 8 and with 16 sums per row.  A workgroup runs as host
// threads that meet at a barrier where the kernel has __syncthreads().  Every output is compared bit for bit with the values
// tests/test_vq_linear_cpu.py computed with tests/vq_linear_ref.py and wrote into the file named on the command line.  Built with
// the sanitizers on and -ffp-contract=off, as the library.
#include "device_shim.h"
#include "../../vqvae_amd/csrc/vq_linear.h"
using namespace vqvae;

alignas(16) static float g_tiles[kL2Waves * kL2TileFloats > kLinRowsWaves * kLinTileFloats ? kL2Waves * kL2TileFloats : kLinRowsWaves * kLinTileFloats];
alignas(16) static float g_bt[kLinBlockRows * kLinBStride];
static double g_wl[kLinWeightsMax];

// one grid of workgroups of `threads` threads, one after the other
template <typename Body> static void run_grid(long long blocks, Body body, unsigned threads = kLinBlockRows) {
    run_grid(blocks, 1, threads, [] {
        for (auto &v : g_tiles) v = -3.f;
        for (auto &v : g_bt) v = -3.f;
        for (auto &v : g_wl) v = -3.0;
    }, body);
}

static int g_bad = 0;
static void cmp(const char *what, const std::vector<float> &got, const std::vector<float> &want, int rm, int V, int R, int cs) {
    for (size_t i = 0; i < want.size(); ++i)
        if (!same(got[i], want[i])) {
            printf("MISMATCH case %d %s rm=%d V=%d R=%d at %zu: %a want %a\n", cs, what, rm, V, R, i, got[i], want[i]);
            ++g_bad;
            return;
        }
}

// V = 4: the 16-byte path -- four pixels per lane of an NCHW map, 16-byte copies of row-major rows
template <int R> static void apply(const LinArgs &a, int rm, int V) {
    const long long per = rm ? kLinRowsWaves * kLinWaveRows : V * kLinBlockRows, blocks = (a.N + per - 1) / per;
    if (!rm && V == 4) run_grid(blocks, [=] { lin_nchw_body<R, 4>(a, g_wl); });
    else if (!rm) run_grid(blocks, [=] { lin_nchw_body<R, 1>(a, g_wl); });
    else if (V == 4) run_grid(blocks, [=] { lin_rows_body<R, 4>(a, g_tiles, g_wl); }, 64 * kLinRowsWaves);
    else run_grid(blocks, [=] { lin_rows_body<R, 1>(a, g_tiles, g_wl); }, 64 * kLinRowsWaves);
}

int main(int argc, char **argv) {
    if (argc < 2) { printf("usage: linear_harness cases.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    const int ncases = take<int>(f, 1)[0];
    for (int cs = 0; cs < ncases; ++cs) {
        const std::vector<int> h = take<int>(f, 4);                                // B, HW, Cin, Cout
        const int B = h[0], HW = h[1], Cin = h[2], Cout = h[3];
        const long long N = (long long)B * HW;
        const std::vector<float> x = take<float>(f, N * Cin), gy = take<float>(f, N * Cout), w = take<float>(f, (size_t)Cout * Cin),
                                 b = take<float>(f, Cout), w_y = take<float>(f, N * Cout), w_gx = take<float>(f, N * Cin),
                                 w_gw = take<float>(f, (size_t)Cout * Cin), w_gb = take<float>(f, Cout);
        const long long blocks = (N + kLinBlockRows - 1) / kLinBlockRows;
        const int P = Cout * Cin + Cout;
        for (int rm = 0; rm < 2; ++rm) for (int V : {1, 4}) {
            const std::vector<float> xl = lay(x, N, Cin, HW, rm), gl = lay(gy, N, Cout, HW, rm);
            if (V == 1 || (rm ? ((Cin | Cout) & 3) == 0 : (HW & 3) == 0))
                for (int R : {8, 16}) {
                    std::vector<float> y(N * Cout, -7.f), gx(N * Cin, -7.f);
                    LinArgs a = {};
                    a.x = xl.data(); a.w = w.data(); a.b = b.data(); a.out = y.data(); a.N = N; a.HW = HW;
                    a.NI = Cin; a.NO = Cout; a.ws_o = Cin; a.ws_i = 1;
                    if (R == 8) apply<8>(a, rm, V); else apply<16>(a, rm, V);
                    cmp("y", y, lay(w_y, N, Cout, HW, rm), rm, V, R, cs);
                    a.x = gl.data(); a.b = nullptr; a.out = gx.data();
                    a.NI = Cout; a.NO = Cin; a.ws_o = 1; a.ws_i = Cin;
                    if (R == 8) apply<8>(a, rm, V); else apply<16>(a, rm, V);
                    cmp("grad_x", gx, lay(w_gx, N, Cin, HW, rm), rm, V, R, cs);
                }
            if (V == 4 && (!rm || ((Cout > Cin ? Cout : Cin) & 3))) continue;
            std::vector<double> part((size_t)blocks * P, -7.0);
            LinParamArgs p = {};
            p.x = xl.data(); p.g = gl.data(); p.partials = part.data(); p.N = N; p.Cin = Cin; p.Cout = Cout; p.HW = HW;
            if (!rm) run_grid(blocks, [=] { lin_params_body<false, 1>(p, g_tiles, g_bt); });
            else if (V == 4) run_grid(blocks, [=] { lin_params_body<true, 4>(p, g_tiles, g_bt); });
            else run_grid(blocks, [=] { lin_params_body<true, 1>(p, g_tiles, g_bt); });
            std::vector<float> gw((size_t)Cout * Cin, -7.f), gb(Cout, -7.f);
            const double *pp = part.data();
            float *p_w = gw.data(), *p_b = gb.data();
            run_grid((P + kLinBlockRows - 1) / kLinBlockRows, [=] { lin_param_finalize_body(pp, blocks, Cin, Cout, p_w, p_b); });
            cmp("grad_w", gw, w_gw, rm, V, 0, cs);
            cmp("grad_b", gb, w_gb, rm, V, 0, cs);
            // a NULL gradient is skipped: nothing is written through the other's slots either
            std::vector<float> only(Cout, -7.f);
            float *p_only = only.data();
            run_grid((P + kLinBlockRows - 1) / kLinBlockRows, [=] { lin_param_finalize_body(pp, blocks, Cin, Cout, nullptr, p_only); });
            cmp("grad_b alone", only, w_gb, rm, V, 0, cs);
        }
    }
    fclose(f);
    printf(g_bad ? "FAILED %d\n" : "emulation ok\n", g_bad);
    return g_bad != 0;
}
