// Host-side check of the code-entropy kernels: compiles vqvae_amd/csrc/vq_entropy.h -- the text the HIP kernels compile -- for the
// host and runs both launch chains (squared norms, row kernel, avg partials, avg, finalize; log avg, backward row kernel, grad_E
// partials, grad_E) in both layouts, the first case also 4 bytes off a 16-byte boundary.  A workgroup runs as host threads that meet
// at a barrier where the kernel has __syncthreads().  Every output is compared with the values and the bounds that
// tests/test_vq_entropy_cpu.py computed with tests/vq_entropy_ref.py and wrote into the file named on the command line (the host's
// exp and log are not the restatement's either: the comparison is the GPU test's, by bound), and the two layouts bit for bit.  Built
// with the sanitizers on and -ffp-contract=off, as the library.
#include "device_shim.h"
#include "../../vqvae_amd/csrc/vq_entropy.h"
using namespace vqvae;

alignas(16) static double g_buf[kEntBufDoubles], g_w[kEntWDoubles];

template <typename Body> static void grid(long long bx, int by, Body body) {
    run_grid(bx, by, kEntThreads, [] {
        for (auto &v : g_buf) v = -3.0;
        for (auto &v : g_w) v = -3.0;
    }, body);
}

static int g_bad = 0;
template <typename T>
static void within(const char *what, const T *got, const double *want, const double *bound, size_t n, int cs, int rm) {
    for (size_t i = 0; i < n; ++i)
        if (!(std::fabs((double)got[i] - want[i]) <= bound[i])) {
            printf("OUTSIDE case %d %s rowmajor=%d at %zu: %a want %a bound %a\n", cs, what, rm, i, (double)got[i], want[i], bound[i]);
            ++g_bad;
            return;
        }
}

template <typename T> static void bits(const char *what, const std::vector<T> &a, const std::vector<T> &b, int cs) {
    if (a.size() != b.size() || memcmp(a.data(), b.data(), a.size() * sizeof(T))) {
        printf("MISMATCH case %d %s between the runs\n", cs, what);
        ++g_bad;
    }
}

struct Out {
    std::vector<float> losses, gz, ge;
    std::vector<double> avg, rs;
};

template <int DT> static void backward(EntArgs a) {
    const long long tiles = (a.N + kEntTile - 1) / kEntTile;
    grid(tiles, 1, [=] { ent_row_bwd_body<DT, true>(a, g_buf, g_w); });
    ent_partition_grad(a.N, a.K, a.D, a.rows_per_part, a.P);
    std::vector<double> gp((size_t)a.P * a.K * a.D, -7.0), ap((size_t)a.P * a.K, -7.0);
    a.ge_part = gp.data();
    a.as_part = ap.data();
    grid(a.P, (a.K + kEntTile - 1) / kEntTile, [=] { ent_grad_e_body<DT>(a, g_buf, g_w); });
    grid(((long long)a.K * a.D + kEntThreads - 1) / kEntThreads, 1, [=] { ent_grad_e_reduce_body(a); });
}

// rows: (N, D) in row order.  gz comes back in row order too.
static Out run(const std::vector<float> &rows, const std::vector<float> &E, long long N, int D, int K, int HW, int rm, int off, double s,
               double gamma, const float *gl, const std::vector<double> &avg_in, const std::vector<double> &rs_in) {
    const std::vector<float> laid = lay(rows, N, D, HW, rm);
    std::vector<float> zb(laid.size() + 8), eb(E.size() + 8), gzb(laid.size() + 8, -7.f);
    float *z = zb.data(), *e = eb.data(), *gz = gzb.data();
    while (reinterpret_cast<uintptr_t>(z) & 15) ++z;
    while (reinterpret_cast<uintptr_t>(e) & 15) ++e;
    z += off; e += off; gz += off;
    memcpy(z, laid.data(), laid.size() * 4);
    memcpy(e, E.data(), E.size() * 4);
    Out o;
    o.losses.assign(3, -7.f); o.avg.assign(K, -7.0); o.rs.assign(2 * N, -7.0); o.ge.assign((size_t)K * D, -7.f);
    std::vector<double> zz(N, -7.0), ee(K, -7.0), rs(2 * N, -7.0), logavg(K, -7.0), m(N, -7.0);
    EntArgs a = {};
    a.z = EntSrc{z, N, D, HW, rm};
    a.e = EntSrc{e, K, D, 1, 1};
    a.N = N; a.K = K; a.D = D; a.s = s; a.gamma = gamma;
    a.zz = zz.data(); a.ee = ee.data(); a.rs = rs.data(); a.rs_out = o.rs.data(); a.avg = o.avg.data(); a.losses = o.losses.data();
    ent_partition_avg(N, K, a.rows_per_part, a.P);
    std::vector<double> avg_part((size_t)a.P * K, -7.0), sc_part(a.P, -7.0);
    a.avg_part = avg_part.data(); a.sc_part = sc_part.data();
    const EntSrc zs = a.z, es = a.e;
    double *pzz = zz.data(), *pee = ee.data();
    grid((N + kEntThreads - 1) / kEntThreads, 1, [=] { ent_sqnorm_body(zs, pzz); });
    grid((K + kEntThreads - 1) / kEntThreads, 1, [=] { ent_sqnorm_body(es, pee); });
    grid((N + kEntTile - 1) / kEntTile, 1, [=] { ent_row_fwd_body(a, g_buf); });
    grid(a.P, (K + kEntTile - 1) / kEntTile, [=] { ent_avg_body(a, g_buf); });
    grid((K + kEntThreads - 1) / kEntThreads, 1, [=] { ent_avg_reduce_body(a); });
    grid(1, 1, [=] { ent_finalize_body(a, g_buf); });
    // the backward reads the restatement's avg and rowstat, as the GPU test's does
    EntArgs b = a;
    b.rs = const_cast<double *>(rs_in.data()); b.avg = const_cast<double *>(avg_in.data());
    b.gl = gl; b.logavg = logavg.data(); b.m = m.data(); b.grad_z = gz; b.grad_e = o.ge.data();
    grid((K + kEntThreads - 1) / kEntThreads, 1, [=] { ent_logavg_body(b); });
    if (D <= 64) backward<64>(b); else if (D <= 128) backward<128>(b); else backward<256>(b);
    o.gz.assign((size_t)N * D, 0.f);
    for (long long r = 0; r < N; ++r)
        for (int c = 0; c < D; ++c) o.gz[(size_t)r * D + c] = gz[ent_index(a.z, r, c)];
    return o;
}

int main(int argc, char **argv) {
    if (argc < 2) { printf("usage: entropy_harness cases.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    const int ncases = take<int>(f, 1)[0];
    for (int cs = 0; cs < ncases; ++cs) {
        const std::vector<int> h = take<int>(f, 5);                                // N, D, K, HW, grad_loss?
        const long long N = h[0];
        const int D = h[1], K = h[2], HW = h[3];
        const std::vector<double> sc = take<double>(f, 2);                         // s, gamma
        const float gl = take<float>(f, 1)[0];
        const std::vector<float> rows = take<float>(f, (size_t)N * D), E = take<float>(f, (size_t)K * D);
        const std::vector<double> w_l = take<double>(f, 3), b_l = take<double>(f, 3), w_avg = take<double>(f, K), b_avg = take<double>(f, K);
        const std::vector<double> w_rs = take<double>(f, 2 * N), b_rs = take<double>(f, 2 * N);
        const std::vector<double> w_gz = take<double>(f, (size_t)N * D), b_gz = take<double>(f, (size_t)N * D);
        const std::vector<double> w_ge = take<double>(f, (size_t)K * D), b_ge = take<double>(f, (size_t)K * D);
        Out first;
        int nrun = 0;
        for (int rm : {1, 0})
            for (int off : {0, 1}) {
                if (off && cs != 0) continue;
                const Out o = run(rows, E, N, D, K, HW, rm, off, sc[0], sc[1], h[4] ? &gl : nullptr, w_avg, w_rs);
                within("losses", o.losses.data(), w_l.data(), b_l.data(), 3, cs, rm);
                within("avg", o.avg.data(), w_avg.data(), b_avg.data(), K, cs, rm);
                within("rowstat", o.rs.data(), w_rs.data(), b_rs.data(), 2 * N, cs, rm);
                within("grad_z", o.gz.data(), w_gz.data(), b_gz.data(), (size_t)N * D, cs, rm);
                within("grad_codebook", o.ge.data(), w_ge.data(), b_ge.data(), (size_t)K * D, cs, rm);
                if (nrun++ == 0) { first = o; continue; }
                bits("losses", o.losses, first.losses, cs);
                bits("avg", o.avg, first.avg, cs);
                bits("rowstat", o.rs, first.rs, cs);
                bits("grad_z", o.gz, first.gz, cs);
                bits("grad_codebook", o.ge, first.ge, cs);
            }
    }
    fclose(f);
    printf(g_bad ? "FAILED %d\n" : "emulation ok\n", g_bad);
    return g_bad != 0;
}
