// What the host harnesses of this directory put in front of a kernel header (vqvae_amd/csrc/vq_*.h) so that g++ compiles the kernels'
// own text: the device qualifiers, f32x4, blockIdx / threadIdx, __syncthreads and atomicAdd; then what they all repeat around it:
// run_grid, take, same and lay.  A workgroup runs as host threads, each with its own threadIdx, that meet at a pthread barrier where
// the kernel has __syncthreads(); outside run_grid (a harness that walks the threads of a barrier-free kernel one after the other on
// the calling thread) __syncthreads() does nothing.
#pragma once

#include <pthread.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#define __device__
#define __forceinline__ inline
struct alignas(16) f32x4 { float x, y, z, w; };
struct Dim3 { unsigned x, y; };
static Dim3 blockIdx;
static thread_local Dim3 threadIdx;
static pthread_barrier_t g_barrier;
static bool g_in_grid = false;
static void __syncthreads() { if (g_in_grid) pthread_barrier_wait(&g_barrier); }
static int atomicAdd(int *p, int v) { return __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }

// one grid of (bx_n, by_n) workgroups of `nthreads` threads, one workgroup after the other; `reset` runs in front of each (the harness
// poisons what stands for the workgroup's LDS)
template <typename Reset, typename Body> static void run_grid(long long bx_n, int by_n, unsigned nthreads, Reset reset, Body body) {
    g_in_grid = true;
    for (int by = 0; by < by_n; ++by)
        for (long long bx = 0; bx < bx_n; ++bx) {
            blockIdx.x = (unsigned)bx;
            blockIdx.y = (unsigned)by;
            reset();
            pthread_barrier_init(&g_barrier, nullptr, nthreads);
            std::vector<std::thread> th;
            for (unsigned t = 0; t < nthreads; ++t) th.emplace_back([=] { threadIdx.x = t; threadIdx.y = 0; body(); });
            for (auto &t : th) t.join();
            pthread_barrier_destroy(&g_barrier);
        }
    g_in_grid = false;
}

template <typename T> static std::vector<T> take(FILE *f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { printf("short input file\n"); exit(2); }
    return v;
}

static bool same(float a, float b) { return (std::isnan(a) && std::isnan(b)) || !memcmp(&a, &b, 4); }

// (N, C) rows -> the layout under test: as they are (rm), or (B, C, HW) maps
template <typename T> static std::vector<T> lay(const std::vector<T> &rows, long long N, int C, int HW, int rm) {
    if (rm) return rows;
    std::vector<T> m(rows.size());
    for (long long r = 0; r < N; ++r)
        for (int c = 0; c < C; ++c) m[(size_t)((r / HW * C + c) * HW + r % HW)] = rows[(size_t)(r * C + c)];
    return m;
}
