// Micro-benchmark: the sustained v_fma_f64 rate of independent fp64 chains per lane -- the ceiling of csrc/vq_linear.hip's arithmetic --
// at 1, 2, 4 and 8 waves per SIMD and 8, 16, 32 and 64 chains per lane, with the shader clock it runs at.
// Build: hipcc -O3 --offload-arch=gfx950 fma_f64_rate.hip -o fma_f64_rate
#include <hip/hip_runtime.h>
#include <stdio.h>

template <int NACC>
__global__ __launch_bounds__(256) void fma_loop(double *out, int iters, double w, unsigned long long *cyc, unsigned long long *wall) {
    double acc[NACC];
    for (int a = 0; a < NACC; ++a) acc[a] = 1e-3 * (threadIdx.x + a);
    const double x = 0.5 + 1e-6 * blockIdx.x;
    unsigned long long c0 = __builtin_readcyclecounter(), w0 = wall_clock64();
    for (int i = 0; i < iters; ++i) {
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int a = 0; a < NACC; ++a) acc[a] = __builtin_fma(acc[a], w, x);
    }
    unsigned long long c1 = __builtin_readcyclecounter(), w1 = wall_clock64();
    double s = 0;
    for (int a = 0; a < NACC; ++a) s += acc[a];
    out[blockIdx.x * 256 + threadIdx.x] = s;
    if (blockIdx.x == 0 && threadIdx.x == 0) { *cyc = c1 - c0; *wall = w1 - w0; }
}

template <int NACC>
void run(int cus, int waves_per_simd, int iters) {
    int blocks = cus * waves_per_simd;    // 256 threads = 4 waves = 1 per SIMD per block
    double *out; unsigned long long *cyc, *wall;
    hipMalloc(&out, (size_t)blocks * 256 * 8); hipMalloc(&cyc, 8); hipMalloc(&wall, 8);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    fma_loop<NACC><<<blocks, 256>>>(out, 10, 0.999, cyc, wall);
    hipDeviceSynchronize();
    hipEventRecord(e0);
    fma_loop<NACC><<<blocks, 256>>>(out, iters, 0.999, cyc, wall);
    hipEventRecord(e1); hipDeviceSynchronize();
    float ms; hipEventElapsedTime(&ms, e0, e1);
    unsigned long long hc, hw; hipMemcpy(&hc, cyc, 8, hipMemcpyDeviceToHost); hipMemcpy(&hw, wall, 8, hipMemcpyDeviceToHost);
    double fma = (double)blocks * 256 * iters * 4 * NACC;
    printf("chains/lane=%d waves/simd=%d iters=%d: %.3f ms  %.2f T fma/s  cycles per v_fma_f64 (one wave)=%.2f  shader clock=%.3f GHz\n",
           NACC, waves_per_simd, iters, ms, fma / ms / 1e9, (double)hc / ((double)iters * 4 * NACC), (double)hc / ((double)hw * 10.0));
    hipFree(out); hipFree(cyc); hipFree(wall);
}

int main() {
    hipDeviceProp_t p; hipGetDeviceProperties(&p, 0);
    int cus = p.multiProcessorCount;
    printf("%s, %d CUs\n", p.gcnArchName, cus);
    run<8>(cus, 1, 8000); run<16>(cus, 1, 4000); run<32>(cus, 1, 2000); run<64>(cus, 1, 1000);
    run<16>(cus, 2, 4000); run<16>(cus, 4, 4000); run<16>(cus, 8, 4000); run<64>(cus, 2, 1000);
    return 0;
}
