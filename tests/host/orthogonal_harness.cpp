// Host-side check of the orthogonal regularization kernels: compiles vqvae_amd/csrc/vq_orthogonal.h -- the text the HIP kernels
// compile -- for the host and runs the selection, the main kernel, the total and the backward over the GPU test's shapes and calls:
// with the rows 16-byte aligned and 4 bytes off, and every fourth call in every width class that takes the shape, with and without
// V.  A workgroup runs as host threads that meet at a barrier where the kernel has __syncthreads().  Every output is compared bit for bit with the values
// tests/test_vq_orthogonal_cpu.py computed with tests/vq_orthogonal_ref.py and wrote into the file named on the command line.  Built
// with the sanitizers on and -ffp-contract=off, as the library.
#include "device_shim.h"
#include "../../vqvae_amd/csrc/vq_orthogonal.h"
using namespace vqvae;

alignas(16) static float g_ni[kOrthRows * (kOrthMaxD + 4)];
alignas(16) static float g_nj[kOrthTile * (kOrthMaxD + 4)];
static double g_g[kOrthRows * kOrthTile], g_part[kOrthSumBlocks];
static int g_selj[kOrthTile], g_cnt[kOrthThreads];

// one grid of workgroups of 256 threads, one after the other; the "LDS" holds other values at every start
template <typename Body> static void run_grid(long long blocks, Body body) {
    run_grid(blocks, 1, kOrthThreads, [] {
        for (auto &v : g_ni) v = -3.f;
        for (auto &v : g_nj) v = -3.f;
        for (auto &v : g_g) v = -3.0;
        for (auto &v : g_part) v = -3.0;
        for (auto &v : g_selj) v = 1;
        for (auto &v : g_cnt) v = 9;
    }, body);
}

static int g_bad = 0;
template <typename T> static void cmp(const char *what, const T *got, const T *want, size_t n, int cs, int DT, int off) {
    for (size_t i = 0; i < n; ++i)
        if (!(std::isnan((double)got[i]) && std::isnan((double)want[i])) && memcmp(&got[i], &want[i], sizeof(T))) {
            printf("MISMATCH case %d %s DT=%d offset=%d at %zu: %a want %a\n", cs, what, DT, off, i, (double)got[i], (double)want[i]);
            ++g_bad;
            return;
        }
}

template <int DT> static void main_kernel(const OrthArgs &a) {
    const long long blocks = (a.K + kOrthRows - 1) / kOrthRows;
    if (a.v) run_grid(blocks, [=] { orth_main_body<DT, true>(a, g_ni, g_nj, g_g, g_selj); });
    else run_grid(blocks, [=] { orth_main_body<DT, false>(a, g_ni, g_nj, g_g, g_selj); });
}

int main(int argc, char **argv) {
    if (argc < 2) { printf("usage: orthogonal_harness cases.bin\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { printf("cannot open %s\n", argv[1]); return 2; }
    const int ncases = take<int>(f, 1)[0];
    for (int cs = 0; cs < ncases; ++cs) {
        const std::vector<int> h = take<int>(f, 6);                                // K, D, hist?, uniforms?, max_codes, grad_loss?
        const int K = h[0], D = h[1], max_codes = h[4];
        const size_t n = (size_t)K * D;
        const float gl = take<float>(f, 1)[0];
        const std::vector<float> rows = take<float>(f, n);
        const std::vector<int32_t> hist = take<int32_t>(f, h[2] ? K : 0);
        const std::vector<float> u = take<float>(f, h[3] ? K : 0);
        const float w_loss = take<float>(f, 1)[0];
        const int32_t w_M = take<int32_t>(f, 1)[0];
        const std::vector<int32_t> w_sel = take<int32_t>(f, K);
        const std::vector<double> w_V = take<double>(f, n);
        const std::vector<float> w_g = take<float>(f, n);

        std::vector<int32_t> sel(K, -7);
        {
            const int32_t *ph = h[2] ? hist.data() : nullptr;
            const float *pu = h[3] ? u.data() : nullptr;
            int32_t *ps = sel.data();
            run_grid((K + kOrthThreads - 1) / kOrthThreads, [=] { orth_select_body(ph, pu, max_codes, K, ps); });
        }
        cmp("selected", sel.data(), w_sel.data(), (size_t)K, cs, 0, 0);

        std::vector<float> buf(n + 8);
        for (int off : {0, 1}) {                                                   // 16-byte aligned rows, and 4 bytes off
            float *base = buf.data();
            while (reinterpret_cast<uintptr_t>(base) & 15) ++base;
            float *r = base + off;
            memcpy(r, rows.data(), n * sizeof(float));
            const int DT0 = D <= 64 ? 64 : (D <= 128 ? 128 : 256);                  // the class the library launches
            const bool more = cs % 4 == 0 && off == 0;                             // every fourth case: the wider classes, and no V
            for (int DT : {64, 128, 256}) {
                if (DT < DT0 || (DT > DT0 && !more)) continue;
                for (int want_v = more ? 0 : 1; want_v < 2; ++want_v) {
                    std::vector<double> R(K, -7.0), V(n, -7.0);
                    OrthArgs a = {};
                    a.rows = r; a.selected = sel.data(); a.r = R.data(); a.v = want_v ? V.data() : nullptr; a.K = K; a.D = D;
                    if (DT == 64) main_kernel<64>(a); else if (DT == 128) main_kernel<128>(a); else main_kernel<256>(a);
                    float loss = -7.f;
                    int32_t M = -7;
                    const double *pr = R.data();
                    const int32_t *ps = sel.data();
                    float *pl = &loss;
                    int32_t *pm = &M;
                    run_grid(1, [=] { orth_finalize_body(pr, ps, K, pl, pm, g_part, g_cnt); });
                    cmp("loss", &loss, &w_loss, 1, cs, DT, off);
                    cmp("count", &M, &w_M, 1, cs, DT, off);
                    if (!want_v) continue;
                    cmp("saved", V.data(), w_V.data(), n, cs, DT, off);
                    std::vector<float> g(n, -7.f);
                    const double *pv = V.data();
                    const float *pg = h[5] ? &gl : nullptr;
                    float *po = g.data();
                    const unsigned nb = DT == 64 ? 1 : 3;                          // (the grid of a grid-stride loop is free)
                    run_grid(nb, [=] { orth_backward_body(pv, ps, pm, pg, K, D, po, nb); });
                    cmp("grad_rows", g.data(), w_g.data(), n, cs, DT, off);
                }
            }
        }
    }
    fclose(f);
    printf(g_bad ? "FAILED %d\n" : "emulation ok\n", g_bad);
    return g_bad != 0;
}
