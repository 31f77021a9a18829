// Host-side check of the finite-scalar-quantization kernels: compiles vqvae_amd/csrc/vq_fsq.h and, through it, the skeleton it shares
// with LFQ, vq_proj.h -- the text the HIP kernels compile -- for the host and runs the forward, the decode, the backward (with and
// without the parameter gradients) and the second launch of the parameter gradients over small grids, in both layouts and on both access paths of the row-major kernels.  A workgroup runs as 256
// host threads that meet at a barrier where the kernel has __syncthreads().  Every output is compared bit for bit with the values
// tests/test_vq_fsq_cpu.py computed with tests/vq_fsq_ref.py and wrote into the file named on the command line (the same libm serves
// both).  Built with the sanitizers on and -ffp-contract=off, as the library.
#include "device_shim.h"
#include "../../vqvae_amd/csrc/vq_fsq.h"
using namespace vqvae;

alignas(16) static float g_tiles[kL2Waves * kL2TileFloats];
static float g_wl[proj_weight_floats_max(kFsqMaxLevels)];
static float g_chat[kProjBlockRows * kFsqMaxLevels];
static double g_gy[kProjBlockRows * kFsqMaxLevels];

// one grid of 256-thread workgroups, one after the other
template <typename Body> static void run_grid(long long blocks, Body body) {
    run_grid(blocks, 1, kProjBlockRows, [] {
        for (auto &v : g_tiles) v = -3.f;
        for (auto &v : g_wl) v = -3.f;
    }, body);
}

static int g_bad = 0;
static void cmp(const char *what, const std::vector<float> &got_laid, const std::vector<float> &want_rows, long long N, int D, int HW,
                int rm, int V, int cs) {
    const std::vector<float> want = lay(want_rows, N, D, HW, rm);
    for (size_t i = 0; i < want.size(); ++i)
        if (!same(got_laid[i], want[i])) {
            printf("MISMATCH case %d %s rm=%d V=%d at %zu: %a want %a\n", cs, what, rm, V, i, got_laid[i], want[i]);
            ++g_bad;
            return;
        }
}
static void cmp_flat(const char *what, const float *got, const std::vector<float> &want, int rm, int V, int cs) {
    for (size_t i = 0; i < want.size(); ++i)
        if (!same(got[i], want[i])) {
            printf("MISMATCH case %d %s rm=%d V=%d at %zu: %a want %a\n", cs, what, rm, V, i, got[i], want[i]);
            ++g_bad;
            return;
        }
}

int main(int argc, char **argv) {
    if (argc < 2) { printf("usage: fsq_harness cases.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    const int ncases = take<int>(f, 1)[0];
    for (int cs = 0; cs < ncases; ++cs) {
        const std::vector<int> h = take<int>(f, 5 + 3 * kFsqMaxLevels);            // B, HW, D, d, K, L[8], hw[8], basis[8]
        const int B = h[0], HW = h[1], D = h[2], d = h[3], K = h[4];
        const long long N = (long long)B * HW, ND = N * D;
        const std::vector<double> cst = take<double>(f, 3 * kFsqMaxLevels);        // half_l[8], shift[8], offset[8]
        FsqArgs base = {};
        base.N = N; base.D = D; base.HW = HW; base.d = d; base.K = K;
        for (int j = 0; j < kFsqMaxLevels; ++j) {
            base.L[j] = h[5 + j]; base.hw[j] = h[13 + j]; base.basis[j] = h[21 + j];
            base.half_l[j] = cst[j]; base.shift[j] = cst[8 + j]; base.offset[j] = cst[16 + j];
        }
        const std::vector<float> z = take<float>(f, ND), g = take<float>(f, ND), w_in = take<float>(f, (size_t)d * D), b_in = take<float>(f, d),
                                 w_out = take<float>(f, (size_t)D * d), b_out = take<float>(f, D);
        const std::vector<long long> w_idx = take<long long>(f, N);
        const std::vector<int> w_hist = take<int>(f, K);
        const std::vector<float> w_zq = take<float>(f, ND);
        const std::vector<long long> dec_idx = take<long long>(f, N);
        const std::vector<float> w_dec = take<float>(f, ND), w_gz = take<float>(f, ND), w_gwo = take<float>(f, (size_t)D * d),
                                 w_gbo = take<float>(f, D), w_gwi = take<float>(f, (size_t)d * D), w_gbi = take<float>(f, d);
        const long long blocks = (N + kProjBlockRows - 1) / kProjBlockRows;
        const int P = 2 * D * d + D + d;
        for (int rm = 0; rm < 2; ++rm) for (int V : {1, 4}) {
            if (V == 4 && (!rm || D % 4)) continue;
            const std::vector<float> zl = lay(z, N, D, HW, rm), gl = lay(g, N, D, HW, rm);
            // forward, with and without z_q
            for (int with_zq = 0; with_zq < 2; ++with_zq) {
                std::vector<float> zq(ND, -7.f);
                std::vector<long long> idx(N, -7);
                std::vector<int> hist(K, 0);
                FsqArgs a = base;
                a.z = zl.data(); a.w_in = w_in.data(); a.b_in = b_in.data();
                a.w_out = with_zq ? w_out.data() : nullptr; a.b_out = with_zq ? b_out.data() : nullptr;
                a.out = with_zq ? zq.data() : nullptr; a.idx = idx.data(); a.hist = hist.data();
                if (!rm) run_grid(blocks, [=] { proj_fwd_nchw_body<Fsq, false>(a, g_wl); });
                else if (V == 4) run_grid(blocks, [=] { proj_fwd_rows_body<Fsq, false, 4>(a, g_tiles, g_wl); });
                else run_grid(blocks, [=] { proj_fwd_rows_body<Fsq, false, 1>(a, g_tiles, g_wl); });
                if (idx != w_idx) { printf("MISMATCH case %d idx rm=%d V=%d\n", cs, rm, V); ++g_bad; }
                if (hist != w_hist) { printf("MISMATCH case %d hist rm=%d V=%d\n", cs, rm, V); ++g_bad; }
                if (with_zq) cmp("z_q", zq, w_zq, N, D, HW, rm, V, cs);
                for (long long i = 0; i < N; ++i)
                    if (idx[i] < 0 || idx[i] >= K) { printf("case %d: idx out of range\n", cs); ++g_bad; break; }
            }
            {   // decode (some indices are out of range: NaN rows)
                std::vector<float> zq(ND, -7.f);
                FsqArgs a = base;
                a.idx_in = dec_idx.data(); a.w_out = w_out.data(); a.b_out = b_out.data(); a.out = zq.data();
                if (!rm) run_grid(blocks, [=] { proj_fwd_nchw_body<Fsq, true>(a, g_wl); });
                else if (V == 4) run_grid(blocks, [=] { proj_fwd_rows_body<Fsq, true, 4>(a, g_tiles, g_wl); });
                else run_grid(blocks, [=] { proj_fwd_rows_body<Fsq, true, 1>(a, g_tiles, g_wl); });
                cmp("decode", zq, w_dec, N, D, HW, rm, V, cs);
            }
            // backward: grad_z alone, then everything
            for (int params = 0; params < 2; ++params) {
                std::vector<float> gz(ND, -7.f);
                std::vector<double> part((size_t)blocks * P, -7.0);
                FsqArgs a = base;
                a.z = zl.data(); a.g = gl.data(); a.w_in = w_in.data(); a.b_in = b_in.data(); a.w_out = w_out.data();
                a.out = gz.data(); a.partials = params ? part.data() : nullptr;
                if (!rm) {
                    if (params) run_grid(blocks, [=] { Fsq::bwd_nchw_body<true>(a, g_tiles, g_wl, g_chat, g_gy); });
                    else run_grid(blocks, [=] { Fsq::bwd_nchw_body<false>(a, g_tiles, g_wl, g_chat, g_gy); });
                } else if (V == 4) {
                    if (params) run_grid(blocks, [=] { Fsq::bwd_rows_body<true, 4>(a, g_tiles, g_wl, g_chat, g_gy); });
                    else run_grid(blocks, [=] { Fsq::bwd_rows_body<false, 4>(a, g_tiles, g_wl, g_chat, g_gy); });
                } else {
                    if (params) run_grid(blocks, [=] { Fsq::bwd_rows_body<true, 1>(a, g_tiles, g_wl, g_chat, g_gy); });
                    else run_grid(blocks, [=] { Fsq::bwd_rows_body<false, 1>(a, g_tiles, g_wl, g_chat, g_gy); });
                }
                cmp("grad_z", gz, w_gz, N, D, HW, rm, V, cs);
                if (!params) continue;
                std::vector<float> gwi((size_t)d * D, -7.f), gbi(d, -7.f), gwo((size_t)D * d, -7.f), gbo(D, -7.f);
                const double *pp = part.data();
                float *p_wi = gwi.data(), *p_bi = gbi.data(), *p_wo = gwo.data(), *p_bo = gbo.data();
                run_grid((P + kProjBlockRows - 1) / kProjBlockRows, [=] { proj_param_finalize_body(pp, blocks, D, d, p_wi, p_bi, p_wo, p_bo); });
                cmp_flat("grad_w_out", gwo.data(), w_gwo, rm, V, cs);
                cmp_flat("grad_b_out", gbo.data(), w_gbo, rm, V, cs);
                cmp_flat("grad_w_in", gwi.data(), w_gwi, rm, V, cs);
                cmp_flat("grad_b_in", gbi.data(), w_gbi, rm, V, cs);
                // a NULL gradient is skipped: nothing is written through the others' slots either
                std::vector<float> only(D, -7.f);
                float *p_only = only.data();
                run_grid((P + kProjBlockRows - 1) / kProjBlockRows, [=] { proj_param_finalize_body(pp, blocks, D, d, nullptr, nullptr, nullptr, p_only); });
                cmp_flat("grad_b_out alone", only.data(), w_gbo, rm, V, cs);
            }
        }
    }
    fclose(f);
    printf(g_bad ? "FAILED %d\n" : "emulation ok\n", g_bad);
    return g_bad != 0;
}
