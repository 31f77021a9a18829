// Host-side check of the lookup-free-quantization kernels: compiles vqvae_amd/csrc/vq_lfq.h and, through it, the skeleton it shares
// with FSQ, vq_proj.h -- the text the HIP kernels compile -- for the host and runs both launch chains of vq_lfq.hip over small
// grids, in both layouts and on both access paths of the row-major kernels: forward (row kernel, avg partials, avg, loss finalize), decode, backward (y pass, log avg, entropy gradient, row kernel with
// and without the parameter gradients, parameter finalize), with and without a loss gradient.  A workgroup runs as host threads that
// meet at a barrier where the kernel has __syncthreads().  z_q, idx, hist, y, decode and the straight-through gradients are compared
// bit for bit with the values tests/test_vq_lfq_cpu.py computed with tests/vq_lfq_ref.py and wrote into the file named on the
// command line; the losses, avg and the loss's gradients within the bounds written there (their sums run in another order than
// numpy's).  Built with the sanitizers on and -ffp-contract=off, as the library.
#include "device_shim.h"
#include "../../vqvae_amd/csrc/vq_lfq.h"
using namespace vqvae;

alignas(16) static float g_tiles[kL2Waves * kL2TileFloats];
static float g_nchw[kL2Chunk * kProjNchwStride];
static float g_wl[proj_weight_floats_max(kLfqMaxBits)];
static float g_code[kProjBlockRows * kLfqMaxBits];
static double g_gy[kProjBlockRows * kLfqMaxBits];
static double g_pp[2 * kLfqChunkRows * kLfqMaxBits], g_hh[kLfqChunkRows * kLfqMaxBits], g_cc[kLfqChunkRows * kLfqMaxBits];
static double g_red[256], g_ch[kLfqScalarSlots];
static double g_llds[kLfqLogLdsDoubles], g_pb[2 * kLfqMaxBits], g_A[256], g_B[256], g_u[256], g_v[256], g_T[2 * kLfqMaxBits];

// one grid of workgroups of `nthreads` threads, one after the other
template <typename Body> static void run_grid(long long bx_n, int by_n, int nthreads, Body body) {
    run_grid(bx_n, by_n, (unsigned)nthreads, [] {
        for (auto &v : g_tiles) v = -3.f;
        for (auto &v : g_wl) v = -3.f;
        for (auto &v : g_llds) v = -3.0;
    }, body);
}

// a grid whose kernel has no barrier: the threads of a workgroup one after the other on this thread
template <typename Body> static void run_grid_serial(long long bx_n, int nthreads, Body body) {
    for (long long bx = 0; bx < bx_n; ++bx) {
        blockIdx.x = (unsigned)bx;
        blockIdx.y = 0;
        for (unsigned t = 0; t < (unsigned)nthreads; ++t) {
            threadIdx.x = t;
            body();
        }
    }
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
// |got - want| <= bound (a NaN bound passes: the reference itself is NaN there)
template <typename T>
static void cmp_tol(const char *what, const T *got, const std::vector<double> &want, const std::vector<double> &bound, int rm, int V, int cs) {
    for (size_t i = 0; i < want.size(); ++i) {
        if (std::isnan(bound[i]) || std::isnan(want[i])) continue;
        if (!(std::fabs((double)got[i] - want[i]) <= bound[i])) {
            printf("OUT OF BOUND case %d %s rm=%d V=%d at %zu: %.17g want %.17g +- %.3g\n", cs, what, rm, V, i, (double)got[i], want[i], bound[i]);
            ++g_bad;
            return;
        }
    }
}

int main(int argc, char **argv) {
    if (argc < 2) { printf("usage: lfq_harness cases.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    const int ncases = take<int>(f, 1)[0];
    for (int cs = 0; cs < ncases; ++cs) {
        const std::vector<int> h = take<int>(f, 6);                                // B, HW, D, d, clean (losses compared), nwg
        const int B = h[0], HW = h[1], D = h[2], d = h[3], clean = h[4], nwg = h[5], K = 1 << d;
        const long long N = (long long)B * HW, ND = N * D, Nd = N * d;
        const std::vector<double> sc = take<double>(f, 5);                         // beta, w_e, gamma, inv_temperature, grad_loss
        const float gl_f = (float)sc[4];
        const std::vector<float> z = take<float>(f, ND), g = take<float>(f, ND), w_in = take<float>(f, (size_t)d * D), b_in = take<float>(f, d),
                                 w_out = take<float>(f, (size_t)D * d), b_out = take<float>(f, D);
        const std::vector<long long> w_idx = take<long long>(f, N);
        const std::vector<int> w_hist = take<int>(f, K);
        const std::vector<float> w_zq = take<float>(f, ND), w_y = take<float>(f, Nd);
        const std::vector<long long> dec_idx = take<long long>(f, N);
        const std::vector<float> w_dec = take<float>(f, ND);
        const std::vector<double> w_loss = take<double>(f, 4), b_loss = take<double>(f, 4), w_avg = take<double>(f, K), b_avg = take<double>(f, K);
        // the straight-through backward (no loss gradient): exact
        const std::vector<float> st_gz = take<float>(f, ND), st_gwo = take<float>(f, (size_t)D * d), st_gbo = take<float>(f, D),
                                 st_gwi = take<float>(f, (size_t)d * D), st_gbi = take<float>(f, d);
        // with the loss: e, grad_z, grad_w_in, grad_b_in within bounds (grad_w_out, grad_b_out are the straight-through ones)
        const std::vector<double> w_e = take<double>(f, Nd), b_e = take<double>(f, Nd), w_gz = take<double>(f, ND), b_gz = take<double>(f, ND),
                                  w_gwi = take<double>(f, (size_t)d * D), b_gwi = take<double>(f, (size_t)d * D), w_gbi = take<double>(f, d),
                                  b_gbi = take<double>(f, d);
        const long long blocks = (N + kProjBlockRows - 1) / kProjBlockRows;
        const int PC = 2 * D * d + D + d;
        LfqArgs base = {};
        base.N = N; base.D = D; base.HW = HW; base.d = d; base.K = K;
        LfqLossArgs lbase = {};
        lbase.N = N; lbase.d = d; lbase.K = K; lbase.nwg = nwg;
        lbase.s = 4.0 * (double)(float)sc[3]; lbase.beta = (double)(float)sc[0]; lbase.we = (double)(float)sc[1]; lbase.gamma = (double)(float)sc[2];
        lfq_partition(N, K, lbase.rows_per_part, lbase.P);
        for (int rm = 0; rm < 2; ++rm) for (int V : {1, 4}) {
            if (V == 4 && (!rm || D % 4)) continue;
            const std::vector<float> zl = lay(z, N, D, HW, rm), gl = lay(g, N, D, HW, rm);
            auto fwd = [&](const LfqArgs &a) {
                if (!rm) run_grid(blocks, 1, 256, [=] { proj_fwd_nchw_body<Lfq, false>(a, g_wl); });
                else if (V == 4) run_grid(blocks, 1, 256, [=] { proj_fwd_rows_body<Lfq, false, 4>(a, g_tiles, g_wl); });
                else run_grid(blocks, 1, 256, [=] { proj_fwd_rows_body<Lfq, false, 1>(a, g_tiles, g_wl); });
            };
            std::vector<double> avg(K, -7.0);
            // forward, with z_q and the losses, then without either
            for (int full = 1; full >= 0; --full) {
                std::vector<float> zq(ND, -7.f), y(Nd, -7.f), losses(4, -7.f);
                std::vector<long long> idx(N, -7);
                std::vector<int> hist(K, 0);
                LfqArgs a = base;
                a.z = zl.data(); a.w_in = w_in.data(); a.b_in = b_in.data();
                a.w_out = full ? w_out.data() : nullptr; a.b_out = full ? b_out.data() : nullptr;
                a.out = full ? zq.data() : nullptr; a.idx = idx.data(); a.hist = hist.data(); a.y = full ? y.data() : nullptr;
                fwd(a);
                if (idx != w_idx) { printf("MISMATCH case %d idx rm=%d V=%d\n", cs, rm, V); ++g_bad; }
                if (hist != w_hist) { printf("MISMATCH case %d hist rm=%d V=%d\n", cs, rm, V); ++g_bad; }
                if (!full) continue;
                cmp("z_q", zq, w_zq, N, D, HW, rm, V, cs);
                cmp_flat("y", y.data(), w_y, rm, V, cs);
                std::vector<double> avg_part((size_t)lbase.P * K, -7.0), sc_part((size_t)lbase.P * kLfqScalarSlots, -7.0);
                LfqLossArgs l = lbase;
                l.y = y.data(); l.avg_part = avg_part.data(); l.sc_part = sc_part.data(); l.avg_out = avg.data(); l.losses = losses.data();
                run_grid(l.P, (K + kLfqTileCodes - 1) / kLfqTileCodes, 256, [=] { lfq_avg_body(l, g_pp, g_hh, g_cc); });
                run_grid_serial((K + 255) / 256, 256, [=] { lfq_avg_reduce_body(l); });
                run_grid(1, 1, 256, [=] { lfq_loss_finalize_body(l, g_red, g_ch); });
                if (clean) {
                    cmp_tol("avg", avg.data(), w_avg, b_avg, rm, V, cs);
                    cmp_tol("losses", losses.data(), w_loss, b_loss, rm, V, cs);
                }
            }
            {   // decode (some indices are out of range: NaN rows)
                std::vector<float> zq(ND, -7.f);
                LfqArgs a = base;
                a.idx_in = dec_idx.data(); a.w_out = w_out.data(); a.b_out = b_out.data(); a.out = zq.data();
                if (!rm) run_grid(blocks, 1, 256, [=] { proj_fwd_nchw_body<Lfq, true>(a, g_wl); });
                else if (V == 4) run_grid(blocks, 1, 256, [=] { proj_fwd_rows_body<Lfq, true, 4>(a, g_tiles, g_wl); });
                else run_grid(blocks, 1, 256, [=] { proj_fwd_rows_body<Lfq, true, 1>(a, g_tiles, g_wl); });
                cmp("decode", zq, w_dec, N, D, HW, rm, V, cs);
            }
            // backward: without the loss gradient (exact), then with it; grad_z alone, then everything
            for (int with_loss = 0; with_loss < 2; ++with_loss) {
                std::vector<float> y(Nd, -7.f);
                LfqArgs fa = base;
                fa.z = zl.data(); fa.w_in = w_in.data(); fa.b_in = b_in.data(); fa.y = y.data();
                fwd(fa);
                cmp_flat("y (backward)", y.data(), w_y, rm, V, cs);
                std::vector<double> logavg(K, -7.0), e(Nd, -7.0);
                if (with_loss) {
                    LfqLossArgs l = lbase;
                    l.y = y.data(); l.avg = w_avg.data(); l.logavg = logavg.data(); l.e = e.data();
                    run_grid_serial((K + 255) / 256, 256, [=] { lfq_logavg_body(l); });
                    run_grid(nwg, 1, kLfqGradThreads, [=] { lfq_entgrad_body(l, g_llds, g_pb, g_A, g_B, g_u, g_v, g_T); });
                    if (clean) cmp_tol("e", e.data(), w_e, b_e, rm, V, cs);
                }
                for (int params = 0; params < 2; ++params) {
                    std::vector<float> gz(ND, -7.f);
                    std::vector<double> part((size_t)blocks * PC, -7.0);
                    LfqArgs a = base;
                    a.z = zl.data(); a.g = gl.data(); a.w_in = w_in.data(); a.w_out = w_out.data(); a.y = y.data();
                    a.e = with_loss ? e.data() : nullptr; a.gl = &gl_f;
                    a.out = gz.data(); a.partials = params ? part.data() : nullptr;
                    if (!rm) {
                        if (params) run_grid(blocks, 1, 256, [=] { Lfq::bwd_nchw_body<true>(a, g_nchw, g_wl, g_code, g_gy); });
                        else run_grid(blocks, 1, 256, [=] { Lfq::bwd_nchw_body<false>(a, g_nchw, g_wl, g_code, g_gy); });
                    } else if (V == 4) {
                        if (params) run_grid(blocks, 1, 256, [=] { Lfq::bwd_rows_body<true, 4>(a, g_tiles, g_wl, g_code, g_gy); });
                        else run_grid(blocks, 1, 256, [=] { Lfq::bwd_rows_body<false, 4>(a, g_tiles, g_wl, g_code, g_gy); });
                    } else {
                        if (params) run_grid(blocks, 1, 256, [=] { Lfq::bwd_rows_body<true, 1>(a, g_tiles, g_wl, g_code, g_gy); });
                        else run_grid(blocks, 1, 256, [=] { Lfq::bwd_rows_body<false, 1>(a, g_tiles, g_wl, g_code, g_gy); });
                    }
                    if (!with_loss) cmp("grad_z (straight-through)", gz, st_gz, N, D, HW, rm, V, cs);
                    else if (clean) {
                        const std::vector<double> wl_ = lay(w_gz, N, D, HW, rm), bl_ = lay(b_gz, N, D, HW, rm);
                        cmp_tol("grad_z", gz.data(), wl_, bl_, rm, V, cs);
                    }
                    if (!params) continue;
                    std::vector<float> gwi((size_t)d * D, -7.f), gbi(d, -7.f), gwo((size_t)D * d, -7.f), gbo(D, -7.f);
                    const double *pp = part.data();
                    float *p_wi = gwi.data(), *p_bi = gbi.data(), *p_wo = gwo.data(), *p_bo = gbo.data();
                    run_grid((PC + kProjBlockRows - 1) / kProjBlockRows, 1, 256, [=] { proj_param_finalize_body(pp, blocks, D, d, p_wi, p_bi, p_wo, p_bo); });
                    cmp_flat("grad_w_out", gwo.data(), st_gwo, rm, V, cs);
                    cmp_flat("grad_b_out", gbo.data(), st_gbo, rm, V, cs);
                    if (!with_loss) {
                        cmp_flat("grad_w_in (straight-through)", gwi.data(), st_gwi, rm, V, cs);
                        cmp_flat("grad_b_in (straight-through)", gbi.data(), st_gbi, rm, V, cs);
                    } else if (clean) {
                        cmp_tol("grad_w_in", gwi.data(), w_gwi, b_gwi, rm, V, cs);
                        cmp_tol("grad_b_in", gbi.data(), w_gbi, b_gbi, rm, V, cs);
                    }
                    // a NULL gradient is skipped: nothing is written through the others' slots either
                    std::vector<float> only(D, -7.f);
                    float *p_only = only.data();
                    run_grid((PC + kProjBlockRows - 1) / kProjBlockRows, 1, 256, [=] { proj_param_finalize_body(pp, blocks, D, d, nullptr, nullptr, nullptr, p_only); });
                    cmp_flat("grad_b_out alone", only.data(), st_gbo, rm, V, cs);
                }
            }
            {   // no upstream gradient of z_q: grad_w_out and grad_b_out are zeros, nothing of g is read
                std::vector<float> y(w_y), gz(ND, -7.f), gwo((size_t)D * d, -7.f), gbo(D, -7.f);
                std::vector<double> part((size_t)blocks * PC, -7.0);
                LfqArgs a = base;
                a.z = zl.data(); a.w_in = w_in.data(); a.w_out = w_out.data(); a.y = y.data(); a.out = gz.data(); a.partials = part.data();
                if (!rm) run_grid(blocks, 1, 256, [=] { Lfq::bwd_nchw_body<true>(a, g_nchw, g_wl, g_code, g_gy); });
                else if (V == 4) run_grid(blocks, 1, 256, [=] { Lfq::bwd_rows_body<true, 4>(a, g_tiles, g_wl, g_code, g_gy); });
                else run_grid(blocks, 1, 256, [=] { Lfq::bwd_rows_body<true, 1>(a, g_tiles, g_wl, g_code, g_gy); });
                const double *pp = part.data();
                float *p_wo = gwo.data(), *p_bo = gbo.data();
                run_grid((PC + kProjBlockRows - 1) / kProjBlockRows, 1, 256, [=] { proj_param_finalize_body(pp, blocks, D, d, nullptr, nullptr, p_wo, p_bo); });
                for (float v : gz) if (v != 0.0f) { printf("case %d: grad_z without any upstream gradient is not zero\n", cs); ++g_bad; break; }
                for (float v : gwo) if (v != 0.0f) { printf("case %d: grad_w_out without grad_zq is not zero\n", cs); ++g_bad; break; }
                for (float v : gbo) if (v != 0.0f) { printf("case %d: grad_b_out without grad_zq is not zero\n", cs); ++g_bad; break; }
            }
        }
    }
    fclose(f);
    printf(g_bad ? "FAILED %d\n" : "emulation ok\n", g_bad);
    return g_bad != 0;
}
