// Host-side check of the split EMA codebook update: compiles vqvae_amd/csrc/vq_ema_merge.h -- the text the HIP kernels compile -- for
// the host and runs the pack body, the count body and the apply body over the cases tests/test_vq_ema_merge_cpu.py wrote into the
// file named on the command line.  The pack and the apply body have no barrier: their threads are walked one after the other, a
// few past the last element too; the count body runs as one workgroup of 1024 host threads that meet at a barrier where the kernel
// has __syncthreads().  Every output is compared bit for bit with the values the test computed from tests/vq_ema_merge_ref.py's
// formulas in the kernels' order.  Built with the sanitizers on and -ffp-contract=off, as the library.
#include "device_shim.h"
#include "../../vqvae_amd/csrc/vq_ema_merge.h"
using namespace vqvae;

static double g_part[kEmaCountThreads];

static int g_bad = 0;
template <typename T> static void cmp(const char *what, const T *got, const T *want, size_t n, int cs) {
    for (size_t i = 0; i < n; ++i)
        if (!(std::isnan((double)got[i]) && std::isnan((double)want[i])) && memcmp(&got[i], &want[i], sizeof(T))) {
            printf("MISMATCH case %d %s at %zu: %a want %a\n", cs, what, i, (double)got[i], (double)want[i]);
            ++g_bad;
            return;
        }
}

int main(int argc, char **argv) {
    if (argc < 2) { printf("usage: ema_merge_harness cases.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    const int ncases = take<int>(f, 1)[0];
    for (int cs = 0; cs < ncases; ++cs) {
        const std::vector<int> h = take<int>(f, 6);                                // N, K, D, HW, row_uniforms?, R (0: a pack case)
        const int N = h[0], K = h[1], D = h[2], HW = h[3], has_u = h[4], R = h[5];
        const int C = has_u ? 2 * D + 1 : D + 1;
        if (R == 0) {
            // ---- pack: the record of one shard, in both layouts
            const std::vector<float> rows = take<float>(f, (size_t)N * D);
            const std::vector<int32_t> offsets = take<int32_t>(f, (size_t)K + 1);
            const std::vector<double> sums = take<double>(f, (size_t)K * D);       // what segsum_key_sum hands to the body
            const std::vector<float> u = take<float>(f, has_u ? K : 0);
            const std::vector<double> want = take<double>(f, (size_t)K * C);
            for (int rm : {1, 0}) {
                const std::vector<float> z = lay(rows, N, D, HW, rm);
                std::vector<double> stats((size_t)K * C, -7.0);
                for (long long e = 0; e < (long long)K * C + 70; ++e) {
                    const int k = (int)(e / C), c = (int)(e - (long long)k * C);
                    const double sum = (e < (long long)K * C && ema_stats_field(c, D) == 1) ? sums[(size_t)k * D + c - 1] : -3.0;
                    ema_pack_body(e, sum, offsets.data(), z.data(), has_u ? u.data() : nullptr, N, K, D, C, HW, rm, stats.data());
                }
                cmp(rm ? "stats (rows)" : "stats (maps)", stats.data(), want.data(), stats.size(), cs);
            }
            continue;
        }
        // ---- apply: R records -> N_k, n, then m and the codebook
        const std::vector<double> par = take<double>(f, 3);                        // decay, eps, threshold (< 0: no restart)
        const std::vector<double> stats = take<double>(f, (size_t)R * K * C);
        const std::vector<float> v = take<float>(f, has_u ? K : 0);
        std::vector<float> cluster = take<float>(f, K), ema_w = take<float>(f, (size_t)K * D);
        const std::vector<double> w_nk = take<double>(f, K), w_n = take<double>(f, 1);
        const std::vector<float> w_cluster = take<float>(f, K), w_m = take<float>(f, (size_t)K * D), w_e = take<float>(f, (size_t)K * D);
        std::vector<double> nk(K, -7.0);
        double n_total = -7.0;
        {
            const double *ps = stats.data();
            const float *pc = cluster.data();
            double *pn = nk.data(), *pt = &n_total;
            const double decay = par[0];
            run_grid(1, 1, kEmaCountThreads, [] { for (auto &p : g_part) p = -3.0; },
                     [=] { ema_count_body(ps, R, K, C, pc, decay, pn, pt, g_part); });
        }
        cmp("N_k", nk.data(), w_nk.data(), (size_t)K, cs);
        cmp("n", &n_total, w_n.data(), 1, cs);
        const bool restart = has_u && par[2] >= 0.0;
        std::vector<float> cb((size_t)K * D, -7.f);
        for (long long e = 0; e < (long long)K * D + 70; ++e)
            ema_apply_body(e, stats.data(), R, K, D, C, nk.data(), &n_total, restart ? v.data() : nullptr, par[0], par[1],
                           restart ? par[2] : 0.0, cluster.data(), ema_w.data(), cb.data());
        cmp("ema_cluster_size", cluster.data(), w_cluster.data(), (size_t)K, cs);
        cmp("ema_w", ema_w.data(), w_m.data(), (size_t)K * D, cs);
        cmp("codebook", cb.data(), w_e.data(), (size_t)K * D, cs);
    }
    fclose(f);
    printf(g_bad ? "FAILED %d\n" : "emulation ok\n", g_bad);
    return g_bad != 0;
}
