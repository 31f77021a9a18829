// Cached ancestral sampler of the GatedPixelCNN prior (pixelcnn/models.py:129-142), gfx950.
//
// GatedPixelCNN.generate runs one full forward per position and keeps one pixel's logits.  The prior is causal: every value at
// pixel (y, x), in every layer, reads only input pixels strictly before (y, x) in raster order, so writing a pixel changes nothing
// computed earlier.  This kernel keeps each layer's state and computes only what the next pixel needs (notation of
// include/vqvae_hip.h: hv_L the vertical stack's pre-gate output, V_L = out_v, Hs_L = out_h of layer L):
//   per row y      hv_L(y, .), V_L(y, .) = gate(hv_L + cond_L) and v2h_L(y, .) = vert_to_horiz(hv_L) for every layer and column:
//                  hv_0 reads embedded input rows y-3 .. y-1 (make_causal zeroes the dy = 0 taps), hv_L (L >= 1) reads V_{L-1}
//                  at rows y-1 and y -- all of it input rows above y
//   per (y, x)     Hs_L(y, x) for L = 0 .. n-1 from Hs_{L-1} at (y, x-1) and (y, x) (layer 0: the embedded input at
//                  (y, x-3 .. x-1)) and v2h_L(y, x); the 512-wide head; the draw; the drawn code becomes layer 0's input
// One workgroup per image loops over every row and position with __syncthreads only: no cross-workgroup communication.
// Products are fp32 fmaf chains; a dot product is split over 16 lanes (16-byte loads along the input channels) and the lanes'
// partial sums are combined by a fixed xor butterfly, so an image's bits do not depend on the batch around it.
// The gate is gated_activation_kernel's expression, with the reference's order of sums (:75-79).
#include "common.h"

namespace vqvae {

constexpr int kPsThreads = 512;                       // 256 VGPRs per lane: no scratch
constexpr int kPsLanes = 16;                          // lanes per dot product
constexpr int kPsGroups = kPsThreads / kPsLanes;      // dot products in flight per step
constexpr int kPsWaves = kPsThreads / kWave;
constexpr int kPsHidden = 512;                        // output_conv's hidden width (models.py:111-115)
constexpr int kPsMaxDim = 256, kPsMaxK = 8192, kPsMaxSide = 128;
constexpr int kPsTapsV0 = 21, kPsTapsV = 6, kPsTapsH0 = 3, kPsTapsH = 2;   // causal taps that are read (layer 0 / others)
static_assert(kPsThreads % kWave == 0 && kPsMaxDim <= kPsThreads, "one thread per channel in the copies of Hs");

// ---- sampler image: floats, every tensor at a multiple of 4 floats (dim % 4 == 0) -------------------------------------------
//   embedding (K, dim)
//   per layer: class embedding (ncls, 2 dim); vert_stack (2 dim, Tv, dim) + bias; vert_to_horiz (2 dim, 2 dim) + bias;
//              horiz_stack (2 dim, Th, dim) + bias; horiz_resid (dim, dim) + bias           [tap lists of the read taps only]
//   head: output_conv.0 (512, dim) + bias; output_conv.2 (K, 512) + bias
struct PsLayer {
    const float *cond, *vs, *vs_b, *vh, *vh_b, *hs, *hs_b, *hr, *hr_b;
};

__host__ __device__ inline size_t ps_layer_floats(int L, int dim, int ncls) {
    const size_t d = dim, tv = L == 0 ? kPsTapsV0 : kPsTapsV, th = L == 0 ? kPsTapsH0 : kPsTapsH;
    return (size_t)ncls * 2 * d + 2 * d * tv * d + 2 * d + 4 * d * d + 2 * d + 2 * d * th * d + 2 * d + d * d + d;
}

__host__ __device__ inline size_t ps_layer_offset(int L, int K, int dim, int ncls) {
    size_t off = (size_t)K * dim;
    if (L > 0) off += ps_layer_floats(0, dim, ncls) + (size_t)(L - 1) * ps_layer_floats(1, dim, ncls);
    return off;
}

__host__ __device__ inline size_t ps_head_offset(int K, int dim, int nl, int ncls) { return ps_layer_offset(nl, K, dim, ncls); }

__host__ __device__ inline size_t ps_image_floats(int K, int dim, int nl, int ncls) {
    return ps_head_offset(K, dim, nl, ncls) + (size_t)kPsHidden * dim + kPsHidden + (size_t)K * kPsHidden + K;
}

__device__ inline PsLayer ps_layer(const float *img, int L, int K, int dim, int ncls) {
    const size_t d = dim, tv = L == 0 ? kPsTapsV0 : kPsTapsV, th = L == 0 ? kPsTapsH0 : kPsTapsH;
    PsLayer p;
    p.cond = img + ps_layer_offset(L, K, dim, ncls);
    p.vs = p.cond + (size_t)ncls * 2 * d;
    p.vs_b = p.vs + 2 * d * tv * d;
    p.vh = p.vs_b + 2 * d;
    p.vh_b = p.vh + 4 * d * d;
    p.hs = p.vh_b + 2 * d;
    p.hs_b = p.hs + 2 * d * th * d;
    p.hr = p.hs_b + 2 * d;
    p.hr_b = p.hr + d * d;
    return p;
}

// ---- workspace per image (floats): V rows of every layer (two rows, y & 1), v2h of the current row, hv of the current row (two
// buffers, layer & 1), and Hs_L(y, x-1) of layers 0 .. n-2 ------------------------------------------------------------------------
__host__ __device__ inline size_t ps_ws_floats(int S, int dim, int nl) {
    return 2 * (size_t)nl * S * dim + (size_t)nl * S * 2 * dim + 2 * (size_t)S * 2 * dim + (size_t)(nl - 1) * dim;
}

struct PsArgs {
    const float *img;
    const long long *label;
    const float *u;
    long long *out;
    float *logits;
    int *status;
    float *ws;
    size_t ws_per_image;
    int S, dim, K, nl, ncls;
    // the filtered instantiations only (pixelcnn_sample_kernel<true, .>)
    float temperature, top_p;            // top_p >= 1: off
    int top_k;                           // 0: off
    const long long *given;              // (B, S, S), < 0: draw; may be NULL
};

__device__ __forceinline__ float fma4(f32x4 w, f32x4 v, float acc) {
    acc = fmaf(w.x, v.x, acc);
    acc = fmaf(w.y, v.y, acc);
    acc = fmaf(w.z, v.z, acc);
    return fmaf(w.w, v.w, acc);
}

__device__ __forceinline__ float group_sum(float v) {        // 16 lanes; a + b == b + a, so every lane ends with the same bits
#pragma unroll
    for (int m = kPsLanes / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, kPsLanes);
    return v;
}

__device__ __forceinline__ f32x4 ld4(const float *p) { return *reinterpret_cast<const f32x4 *>(p); }

__device__ __forceinline__ float gate(float a, float g) { return tanhf(a) * (1.0f / (1.0f + expf(-g))); }

// R rows o, o + step, .. of w (row length 4 n4) against the vector v (LDS), lanes over the inputs; group-reduced sums in s[]
template <int R>
__device__ __forceinline__ void dot_rows(const float *__restrict__ w, int o, int step, const float *v, int n4, int l, float *s) {
    float acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = 0.0f;
    for (int q = l; q < n4; q += kPsLanes) {
        const f32x4 x = ld4(v + 4 * q);
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = fma4(ld4(w + (size_t)(o + r * step) * 4 * n4 + 4 * q), x, acc[r]);
    }
#pragma unroll
    for (int r = 0; r < R; ++r) s[r] = group_sum(acc[r]);
}

// out[o] = act(bias[o] + w[o] . v) for o < O, lanes over the inputs (n4 float4s), four rows per group while they last
template <bool kRelu>
__device__ __forceinline__ void matvec(const float *__restrict__ w, const float *__restrict__ bias, const float *v, int n4, int O,
                                       float *out, int g, int l) {
    int o = g;
    for (; o + 3 * kPsGroups < O; o += 4 * kPsGroups) {
        float s[4];
        dot_rows<4>(w, o, kPsGroups, v, n4, l, s);
        if (l == 0)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float t = s[r] + bias[o + r * kPsGroups];
                out[o + r * kPsGroups] = kRelu ? (t < 0.0f ? 0.0f : t) : t;      // NaN passes, as torch's relu lets it
            }
    }
    for (; o < O; o += kPsGroups) {
        float s[1];
        dot_rows<1>(w, o, 0, v, n4, l, s);
        if (l == 0) {
            const float t = s[0] + bias[o];
            out[o] = kRelu ? (t < 0.0f ? 0.0f : t) : t;
        }
    }
}

// ---- the filtered draw (pixelcnn_sample_kernel<true, .>): top-k, temperature, top-p -----------------------------------------------
// Both truncations are a threshold on the codes ranked by (logit descending, index ascending).  The threshold is found by bisection
// on an order-preserving integer key of the fp32 logit, two key bits per step: each step takes the block's count (top-k) or mass
// (top-p) above three candidate keys.  Counts are integers; masses are fp32 sums in one fixed tree (a thread's codes in ascending
// order, an xor butterfly over the wave, the waves in sequence), so they depend on K and the logits alone.  Every operation of that
// tree is monotone in its operands and a dropped code adds an exact zero, so the mass above a key never grows with the key: the
// bisection is exact for the sums it uses.  Ties at a threshold are cut by index in a second, short step.
constexpr int kPsCand = 3;                            // candidate thresholds per bisection step: two bits per block reduction

// a > b <=> ps_key(a) > ps_key(b) for finite a, b; -0 ranks as +0
__device__ __forceinline__ unsigned ps_key(float v) {
    const unsigned b = __float_as_uint(v + 0.0f);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}

// v[i] <- the block's sum of v[i], the same bits in every thread.  red: kPsWaves * N words; consecutive calls alternate between two
// such buffers, so a call needs one barrier: a wave that runs ahead writes the other buffer
template <typename T, int N>
__device__ __forceinline__ void block_sums(T (&v)[N], T *red, int lane, int wave) {
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
        for (int sh = kWave / 2; sh >= 1; sh >>= 1) v[i] = v[i] + __shfl_xor(v[i], sh);
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < N; ++i) red[wave * N + i] = v[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) {
        T s = red[i];
        for (int w = 1; w < kPsWaves; ++w) s = s + red[w * N + i];
        v[i] = s;
    }
}

// the smallest v in [0, 2^kBits) with pred(v), for a monotone pred (false .. false true .. true) that holds at 2^kBits - 1.
// eval(t, ok) sets ok[i] = pred(t[i]) for the tops t[i] of the first three of the four buckets that the next two bits select
template <int kBits, typename F>
__device__ __forceinline__ unsigned ps_bisect(F eval) {
    static_assert(kBits % 2 == 0, "two bits per step");
    unsigned lo = 0;
    for (int sh = kBits - 2; sh >= 0; sh -= 2) {
        unsigned t[kPsCand];
        bool ok[kPsCand];
#pragma unroll
        for (int i = 0; i < kPsCand; ++i) t[i] = lo | ((unsigned)i << sh) | ((1u << sh) - 1u);
        eval(t, ok);
        int d = 0;
#pragma unroll
        for (int i = 0; i < kPsCand; ++i) d += !ok[i];
        lo |= (unsigned)d << sh;
    }
    return lo;
}

// kFilter = false: the plain draw (temperature 1, every code, every position drawn).  kFilter = true adds the filtered draw and the
// given codes; it is a separate instantiation so that the plain one keeps its registers, LDS and barriers.
// Two workgroups share a CU once B exceeds the CU count.  The plain kernel fits twice (126 VGPRs, 43 KiB of LDS); the filtered one
// (75 KiB of LDS) takes 141 VGPRs, one workgroup per CU and 1.8 x the time at B = 1024.  kTwoPerCu holds it to 128 VGPRs, which costs
// four spilled dwords and 5 % at small B: the launch picks it for B above the CU count only.  Same arithmetic, same bits
template <bool kFilter, bool kTwoPerCu>
__global__ __launch_bounds__(kPsThreads, kTwoPerCu ? 4 : 1) void pixelcnn_sample_kernel(PsArgs a) {
    __shared__ int idx_ring[4 * kPsMaxSide];                       // sampled codes of rows y-3 .. y (row r at r & 3)
    __shared__ __attribute__((aligned(16))) float vin[kPsTapsH0 * kPsMaxDim];   // the horizontal stack's tap vector
    __shared__ __attribute__((aligned(16))) float gout[kPsMaxDim];              // gate output of the horizontal stack
    __shared__ __attribute__((aligned(16))) float hs[kPsMaxDim];                // Hs_L(y, x)
    __shared__ __attribute__((aligned(16))) float hidden[kPsHidden];
    __shared__ __attribute__((aligned(16))) float lg[kPsMaxK];                  // the position's logits
    __shared__ float part[kPsThreads];
    __shared__ float red_f[kPsWaves];
    __shared__ int red_i[kPsWaves], red_j[kPsWaves];
    __shared__ float total_s;
    __shared__ int status_s;

    const int tid = threadIdx.x, g = tid >> 4, l = tid & (kPsLanes - 1), lane = tid & (kWave - 1), wave = tid >> 6;
    const int S = a.S, dim = a.dim, K = a.K, nl = a.nl, d4 = dim >> 2;
    const long long b = blockIdx.x;
    long long lab = a.label[b];
    lab = lab < 0 ? 0 : (lab >= a.ncls ? a.ncls - 1 : lab);           // clamped like vqvae_gather_rows_f32
    float *ws = a.ws + (size_t)b * a.ws_per_image;
    float *vring = ws;                                                // [y & 1][L][x][dim]
    float *v2h = vring + 2 * (size_t)nl * S * dim;                    // [L][x][2 dim]
    float *hvb = v2h + (size_t)nl * S * 2 * dim;                      // [L & 1][x][2 dim]
    float *hsp = hvb + 2 * (size_t)S * 2 * dim;                       // [L - 1][dim]: Hs_{L-1}(y, x-1)
    const float *emb = a.img;
    const size_t head = ps_head_offset(K, dim, nl, a.ncls);
    const float *w0 = a.img + head, *b0 = w0 + (size_t)kPsHidden * dim, *w2 = b0 + kPsHidden, *b2 = w2 + (size_t)K * kPsHidden;
    const int ck = (K + kPsThreads - 1) / kPsThreads;                 // logits per thread in the draw
    const int k_lo = tid * ck < K ? tid * ck : K, k_hi = k_lo + ck < K ? k_lo + ck : K;
    const int owner = (K - 1) / ck;                                   // the thread holding the last code
    if (tid == 0) status_s = 0;
    float *ev = nullptr;                                              // e_k after the filters (this thread touches k_lo .. k_hi only)
    unsigned *sel_red = nullptr;                                      // block_sums' two buffers
    int ph = 0;
    if constexpr (kFilter) {
        __shared__ float ev_s[kPsMaxK];
        __shared__ unsigned sel_red_s[2 * kPsWaves * kPsCand];
        ev = ev_s;
        sel_red = sel_red_s;
    }
    auto red_next = [&]() { ph ^= 1; return sel_red + ph * kPsWaves * kPsCand; };
    (void)red_next;

    for (int y = 0; y < S; ++y) {
        // ------------------------------------------------------------------ row pass: hv_L, V_L, v2h_L of row y, every layer
        for (int L = 0; L < nl; ++L) {
            const PsLayer P = ps_layer(a.img, L, K, dim, a.ncls);
            const float *cond = P.cond + (size_t)lab * 2 * dim;
            const int T = L == 0 ? kPsTapsV0 : kPsTapsV;
            float *hv = hvb + (size_t)(L & 1) * S * 2 * dim;
            for (int j = g; j < S * dim; j += kPsGroups) {
                const int x = j / dim, c = j - x * dim;
                const float *wa = P.vs + (size_t)c * T * dim, *wg = P.vs + (size_t)(dim + c) * T * dim;
                float sa = 0.0f, sg = 0.0f;
                for (int t = 0; t < T; ++t) {
                    // layer 0: (dy, dx) = (t / 7 - 3, t % 7 - 3); others: (t / 3 - 1, t % 3 - 1)
                    const int yy = L == 0 ? y + t / 7 - 3 : y + t / 3 - 1, xx = L == 0 ? x + t % 7 - 3 : x + t % 3 - 1;
                    if (yy < 0 || xx < 0 || xx >= S) continue;             // zero padding (yy <= y always)
                    const float *src = L == 0 ? emb + (size_t)idx_ring[(yy & 3) * kPsMaxSide + xx] * dim
                                              : vring + (((size_t)(yy & 1) * nl + (L - 1)) * S + xx) * dim;
                    for (int q = l; q < d4; q += kPsLanes) {
                        const f32x4 v = ld4(src + 4 * q);
                        sa = fma4(ld4(wa + (size_t)t * dim + 4 * q), v, sa);
                        sg = fma4(ld4(wg + (size_t)t * dim + 4 * q), v, sg);
                    }
                }
                sa = group_sum(sa);
                sg = group_sum(sg);
                if (l == 0) {
                    const float ha = sa + P.vs_b[c], hg = sg + P.vs_b[dim + c];
                    hv[(size_t)x * 2 * dim + c] = ha;
                    hv[(size_t)x * 2 * dim + dim + c] = hg;
                    vring[(((size_t)(y & 1) * nl + L) * S + x) * dim + c] = gate(ha + cond[c], hg + cond[dim + c]);   // :71
                }
            }
            __syncthreads();
            // v2h_L(y, x) = vert_to_horiz(hv_L(y, x)), read back by the position pass; hv is double-buffered over L, so the next
            // layer's writes need no barrier behind this loop
            for (int j = g; j < S * 2 * dim; j += kPsGroups) {
                const int x = j / (2 * dim), o = j - x * 2 * dim;
                const float *w = P.vh + (size_t)o * 2 * dim, *src = hv + (size_t)x * 2 * dim;
                float s = 0.0f;
                for (int q = l; q < 2 * d4; q += kPsLanes) s = fma4(ld4(w + 4 * q), ld4(src + 4 * q), s);
                s = group_sum(s);
                if (l == 0) v2h[((size_t)L * S + x) * 2 * dim + o] = s + P.vh_b[o];
            }
        }
        __syncthreads();

        // ------------------------------------------------------------------ position pass
        for (int x = 0; x < S; ++x) {
            for (int L = 0; L < nl; ++L) {
                const PsLayer P = ps_layer(a.img, L, K, dim, a.ncls);
                const float *cond = P.cond + (size_t)lab * 2 * dim;
                const int T = L == 0 ? kPsTapsH0 : kPsTapsH;
                // the horizontal stack's taps: layer 0 the embedded input at (y, x-3 .. x-1); others Hs_{L-1} at (y, x-1), (y, x)
                for (int e = tid; e < T * dim; e += kPsThreads) {
                    const int t = e / dim, c = e - t * dim;
                    float v;
                    if (L == 0) {
                        const int xx = x + t - 3;
                        v = xx >= 0 ? emb[(size_t)idx_ring[(y & 3) * kPsMaxSide + xx] * dim + c] : 0.0f;
                    } else {
                        v = t == 0 ? (x > 0 ? hsp[(size_t)(L - 1) * dim + c] : 0.0f) : hs[c];
                    }
                    vin[e] = v;
                }
                __syncthreads();
                if (L > 0 && tid < dim) hsp[(size_t)(L - 1) * dim + tid] = vin[dim + tid];   // Hs_{L-1}(y, x) for column x + 1
                for (int c = g; c < dim; c += kPsGroups) {
                    float s[2];
                    dot_rows<2>(P.hs, c, dim, vin, T * d4, l, s);
                    if (l == 0) {
                        const float *vh = v2h + ((size_t)L * S + x) * 2 * dim;
                        const float ha = (vh[c] + (s[0] + P.hs_b[c])) + cond[c];                     // :77 (v2h + h_horiz) + h
                        const float hg = (vh[dim + c] + (s[1] + P.hs_b[dim + c])) + cond[dim + c];
                        gout[c] = gate(ha, hg);
                    }
                }
                __syncthreads();
                for (int c = g; c < dim; c += kPsGroups) {                                            // :78-81
                    float s[1];
                    dot_rows<1>(P.hr, c, 0, gout, d4, l, s);
                    if (l == 0) {
                        const float r = s[0] + P.hr_b[c];
                        hs[c] = L > 0 ? r + vin[dim + c] : r;
                    }
                }
                __syncthreads();
            }
            const size_t pos = ((size_t)b * S + y) * S + x;
            long long gv = -1;                                           // >= 0: the code of (y, x) is given, nothing is drawn
            if constexpr (kFilter)
                if (a.given) gv = a.given[pos];
            if (gv >= 0) {
                // the head only where its logits are asked for; the state of the layers is already that of this position
                if (a.logits) {
                    matvec<true>(w0, b0, hs, d4, kPsHidden, hidden, g, l);
                    __syncthreads();
                    matvec<false>(w2, b2, hidden, kPsHidden / 4, K, lg, g, l);
                    __syncthreads();
                    for (int k = tid; k < K; k += kPsThreads) a.logits[(((size_t)b * K + k) * S + y) * S + x] = lg[k];
                }
                if (tid == 0) {
                    if (gv >= K) status_s |= VQVAE_SAMPLE_GIVEN_RANGE;
                    const int k = status_s ? 0 : (int)gv;
                    idx_ring[(y & 3) * kPsMaxSide + x] = k;
                    a.out[pos] = k;
                }
                __syncthreads();
                continue;
            }
            // output_conv (:111-115)
            matvec<true>(w0, b0, hs, d4, kPsHidden, hidden, g, l);
            __syncthreads();
            matvec<false>(w2, b2, hidden, kPsHidden / 4, K, lg, g, l);
            __syncthreads();

            // ---- the draw: m = max l, e_k = exp(l_k - m), C_k running sums in ascending k; the smallest k with u S < C_k
            float m = -INFINITY;
            int bad = 0;
            for (int k = k_lo; k < k_hi; ++k) {
                const float v = lg[k];
                bad |= !isfinite(v);
                m = fmaxf(m, v);
            }
#pragma unroll
            for (int sh = kWave / 2; sh >= 1; sh >>= 1) {
                m = fmaxf(m, __shfl_xor(m, sh));
                bad |= __shfl_xor(bad, sh);
            }
            if (lane == 0) { red_f[wave] = m; red_i[wave] = bad; }
            __syncthreads();
            m = red_f[0];
            bad = red_i[0];
            for (int w = 1; w < kPsWaves; ++w) { m = fmaxf(m, red_f[w]); bad |= red_i[w]; }
            if constexpr (kFilter) {
                // a. top-k: vk the top_k-th largest key, i.e. the smallest key with fewer than top_k codes above it; the codes above
                // it stay, and of those at it the first top_k - (codes above) by index
                const bool tk = a.top_k >= 1 && a.top_k < K;
                unsigned vk = 0;
                int rank = 0, need = 0;
                if (tk) {
                    vk = ps_bisect<32>([&](const unsigned *t, bool *ok) {
                        int c[kPsCand] = {0, 0, 0};
                        for (int k = k_lo; k < k_hi; ++k) {
                            const unsigned key = ps_key(lg[k]);
#pragma unroll
                            for (int i = 0; i < kPsCand; ++i) c[i] += key > t[i];
                        }
                        block_sums(c, reinterpret_cast<int *>(red_next()), lane, wave);
#pragma unroll
                        for (int i = 0; i < kPsCand; ++i) ok[i] = c[i] < a.top_k;
                    });
                    int above = 0, ties = 0;
                    for (int k = k_lo; k < k_hi; ++k) {
                        const unsigned key = ps_key(lg[k]);
                        above += key > vk;
                        ties += key == vk;
                    }
                    int inc = ties;                                      // ties before this thread's codes: a scan over the threads
#pragma unroll
                    for (int sh = 1; sh < kWave; sh <<= 1) {
                        const int o = __shfl_up(inc, sh);
                        if (lane >= sh) inc += o;
                    }
#pragma unroll
                    for (int sh = kWave / 2; sh >= 1; sh >>= 1) above += __shfl_xor(above, sh);
                    int *sc = reinterpret_cast<int *>(red_next());
                    if (lane == kWave - 1) sc[wave] = inc;
                    if (lane == 0) sc[kPsWaves + wave] = above;
                    __syncthreads();
                    rank = inc - ties;
                    need = a.top_k;
                    for (int w = 0; w < kPsWaves; ++w) {
                        if (w < wave) rank += sc[w];
                        need -= sc[kPsWaves + w];
                    }
                }
                // b. temperature: a correctly rounded divide, exact at temperature 1
                for (int k = k_lo; k < k_hi; ++k) {
                    const float v = lg[k];
                    bool keep = true;
                    if (tk) {
                        const unsigned key = ps_key(v);
                        keep = key > vk || (key == vk && rank++ < need);
                    }
                    ev[k] = keep ? expf((v - m) / a.temperature) : 0.0f;
                }
                // c. top-p: v0 the smallest key with a mass of less than top_p S above it.  The codes above it stay, as does the
                // first code at it; the codes below it have at least top_p S before them.  Of several codes at v0, those below
                // the smallest index J with a mass of at least top_p S before it stay
                if (a.top_p < 1.0f) {
                    float tot[1] = {0.0f};
                    for (int k = k_lo; k < k_hi; ++k) tot[0] = tot[0] + ev[k];
                    block_sums(tot, reinterpret_cast<float *>(red_next()), lane, wave);
                    const float P = a.top_p * tot[0];
                    const unsigned v0 = ps_bisect<32>([&](const unsigned *t, bool *ok) {
                        float f[kPsCand] = {0.0f, 0.0f, 0.0f};
                        for (int k = k_lo; k < k_hi; ++k) {
                            const unsigned key = ps_key(lg[k]);
                            const float e = ev[k];
#pragma unroll
                            for (int i = 0; i < kPsCand; ++i) f[i] = f[i] + (key > t[i] ? e : 0.0f);
                        }
                        block_sums(f, reinterpret_cast<float *>(red_next()), lane, wave);
#pragma unroll
                        for (int i = 0; i < kPsCand; ++i) ok[i] = f[i] < P;
                    });
                    int nt[1] = {0};
                    for (int k = k_lo; k < k_hi; ++k) nt[0] += ps_key(lg[k]) == v0;
                    block_sums(nt, reinterpret_cast<int *>(red_next()), lane, wave);
                    unsigned J = (unsigned)K;
                    if (nt[0] > 1)
                        J = ps_bisect<14>([&](const unsigned *t, bool *ok) {          // 2^14 > kPsMaxK
                            float f[kPsCand] = {0.0f, 0.0f, 0.0f};
                            for (int k = k_lo; k < k_hi; ++k) {
                                const unsigned key = ps_key(lg[k]);
                                const float e = ev[k];
#pragma unroll
                                for (int i = 0; i < kPsCand; ++i)
                                    f[i] = f[i] + (key > v0 || (key == v0 && (unsigned)k < t[i]) ? e : 0.0f);
                            }
                            block_sums(f, reinterpret_cast<float *>(red_next()), lane, wave);
#pragma unroll
                            for (int i = 0; i < kPsCand; ++i) ok[i] = t[i] >= (unsigned)K || f[i] >= P;
                        });
                    for (int k = k_lo; k < k_hi; ++k) {
                        const unsigned key = ps_key(lg[k]);
                        if (key < v0 || (key == v0 && (unsigned)k >= J)) ev[k] = 0.0f;
                    }
                }
            }
            // d. the draw over e_k: the filtered ones in ev, or exp(l_k - m)
            auto ek = [&](int k) {
                if constexpr (kFilter) return ev[k];
                else return expf(lg[k] - m);
            };
            float r = 0.0f;                                              // this thread's sum of e_k, ascending k
            for (int k = k_lo; k < k_hi; ++k) r = r + ek(k);
            part[tid] = r;
            __syncthreads();
            if (tid < kWave) {                                           // exclusive prefix of the thread sums, fixed order:
                constexpr int kPer = kPsThreads / kWave;                 // blocks of kPer in sequence, a scan over the 64 blocks
                float blk = 0.0f;
                for (int i = 0; i < kPer; ++i) blk = blk + part[kPer * tid + i];
                float inc = blk;
#pragma unroll
                for (int sh = 1; sh < kWave; sh <<= 1) {
                    const float o = __shfl_up(inc, sh);
                    if (lane >= sh) inc = o + inc;
                }
                float pre = __shfl_up(inc, 1);
                if (lane == 0) pre = 0.0f;
                for (int i = 0; i < kPer; ++i) {
                    const float p = part[kPer * tid + i];
                    part[kPer * tid + i] = pre;
                    pre = pre + p;
                }
            }
            __syncthreads();
            const float base = part[tid];
            if (tid == owner) total_s = base + r;                        // S = C_{K-1}
            __syncthreads();
            const float thr = a.u[((size_t)b * S + y) * S + x] * total_s;
            int first = K, last = -1;
            float run = 0.0f;
            for (int k = k_lo; k < k_hi; ++k) {
                const float e = ek(k);
                run = run + e;
                if (first == K && thr < base + run) first = k;
                if (e > 0.0f) last = k;
            }
#pragma unroll
            for (int sh = kWave / 2; sh >= 1; sh >>= 1) {
                first = min(first, __shfl_xor(first, sh));
                last = max(last, __shfl_xor(last, sh));
            }
            if (lane == 0) { red_i[wave] = first; red_j[wave] = last; }
            __syncthreads();
            if (tid == 0) {
                for (int w = 0; w < kPsWaves; ++w) { first = min(first, red_i[w]); last = max(last, red_j[w]); }
                if (bad) status_s |= VQVAE_SAMPLE_NONFINITE;
                int k = first < K ? first : (last >= 0 ? last : 0);      // rounding left no C_k above u S: the last e_k > 0
                if (status_s) k = 0;
                idx_ring[(y & 3) * kPsMaxSide + x] = k;
                a.out[((size_t)b * S + y) * S + x] = k;
            }
            if (a.logits)
                for (int k = tid; k < K; k += kPsThreads) a.logits[(((size_t)b * K + k) * S + y) * S + x] = lg[k];
            __syncthreads();
        }
    }
    if (tid == 0) a.status[b] = status_s;
}

struct PsPack {
    const float *src;
    float *dst;
    int O, Cin, Tsrc, T;
    signed char tmap[32];
};

// dst (O, T, Cin) = src (O, Cin, Tsrc) at the taps tmap[0 .. T): a conv weight to the sampler's tap-major rows; T = Tsrc = 1 copies
__global__ __launch_bounds__(256) void pixelcnn_sample_pack_kernel(PsPack p) {
    const long long total = (long long)p.O * p.T * p.Cin;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int ci = (int)(e % p.Cin);
        const long long r = e / p.Cin;
        const int t = (int)(r % p.T);
        const long long o = r / p.T;
        p.dst[e] = p.src[(o * p.Cin + ci) * p.Tsrc + p.tmap[t]];
    }
}

static bool ps_supported(int K, int dim, int nl, int ncls) {
    return dim % 4 == 0 && dim <= kPsMaxDim && K >= 2 && K <= kPsMaxK && nl >= 1 && ncls >= 1;
}

}  // namespace vqvae

using namespace vqvae;

extern "C" {

size_t vqvae_pixelcnn_sample_packed_bytes(int K, int dim, int n_layers, int n_classes) {
    if (K < 1 || dim < 1 || n_layers < 1 || n_classes < 1 || !ps_supported(K, dim, n_layers, n_classes)) return 0;
    return ps_image_floats(K, dim, n_layers, n_classes) * sizeof(float);
}

int vqvae_pixelcnn_sample_pack_f32(const float *const *params, int n_params, int K, int dim, int n_layers, int n_classes,
                                   void *packed, size_t packed_bytes, vqvae_stream_t stream) {
    if (!params || !packed) return VQVAE_ERR_NULL;
    if (K < 1 || dim < 1 || n_layers < 1 || n_classes < 1 || n_params != 9 * n_layers + 5) return VQVAE_ERR_SHAPE;
    for (int i = 0; i < n_params; ++i)
        if (!params[i]) return VQVAE_ERR_NULL;
    if (!ps_supported(K, dim, n_layers, n_classes) || (reinterpret_cast<uintptr_t>(packed) & 15)) return VQVAE_ERR_UNSUPPORTED;
    if (packed_bytes < vqvae_pixelcnn_sample_packed_bytes(K, dim, n_layers, n_classes)) return VQVAE_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *dst = static_cast<float *>(packed);
    auto copy = [&](const float *src, int O, int Cin, int Tsrc, int T, const signed char *tmap) -> int {
        PsPack p;
        p.src = src;
        p.dst = dst;
        p.O = O; p.Cin = Cin; p.Tsrc = Tsrc; p.T = T;
        for (int i = 0; i < 32; ++i) p.tmap[i] = i < T ? tmap[i] : 0;
        const long long total = (long long)O * T * Cin;
        long long grid = (total + 255) / 256;
        grid = grid > 4096 ? 4096 : grid;
        hipLaunchKernelGGL(pixelcnn_sample_pack_kernel, dim3((unsigned)grid), dim3(256), 0, st, p);
        dst += total;
        return (int)hipGetLastError();
    };
    const signed char id[1] = {0};
    signed char v0[kPsTapsV0], h0[kPsTapsH0], v[kPsTapsV], h[kPsTapsH];
    for (int t = 0; t < kPsTapsV0; ++t) v0[t] = (signed char)t;      // rows ky = 0 .. 2 of the 4 x 7 stack (ky = 3 is masked)
    for (int t = 0; t < kPsTapsH0; ++t) h0[t] = (signed char)t;      // columns kx = 0 .. 2 of the 1 x 4 stack (kx = 3 is masked)
    for (int t = 0; t < kPsTapsV; ++t) v[t] = (signed char)t;
    for (int t = 0; t < kPsTapsH; ++t) h[t] = (signed char)t;
    const int d = dim;
    int rc = copy(params[0], K, d, 1, 1, id);                                          // embedding
    for (int L = 0; L < n_layers && rc == 0; ++L) {
        const float *const *q = params + 1 + 9 * L;
        const bool a = L == 0;
        if ((rc = copy(q[0], n_classes, 2 * d, 1, 1, id))) break;                        // class_cond_embedding
        if ((rc = copy(q[1], 2 * d, d, a ? 28 : 6, a ? kPsTapsV0 : kPsTapsV, a ? v0 : v))) break;   // vert_stack
        if ((rc = copy(q[2], 1, 2 * d, 1, 1, id))) break;
        if ((rc = copy(q[3], 2 * d, 2 * d, 1, 1, id))) break;                            // vert_to_horiz
        if ((rc = copy(q[4], 1, 2 * d, 1, 1, id))) break;
        if ((rc = copy(q[5], 2 * d, d, a ? 4 : 2, a ? kPsTapsH0 : kPsTapsH, a ? h0 : h))) break;    // horiz_stack
        if ((rc = copy(q[6], 1, 2 * d, 1, 1, id))) break;
        if ((rc = copy(q[7], d, d, 1, 1, id))) break;                                    // horiz_resid
        rc = copy(q[8], 1, d, 1, 1, id);
    }
    const float *const *q = params + 1 + 9 * n_layers;
    if (rc == 0) rc = copy(q[0], kPsHidden, d, 1, 1, id);                              // output_conv.0
    if (rc == 0) rc = copy(q[1], 1, kPsHidden, 1, 1, id);
    if (rc == 0) rc = copy(q[2], K, kPsHidden, 1, 1, id);                              // output_conv.2
    if (rc == 0) rc = copy(q[3], 1, K, 1, 1, id);
    return rc;
}

size_t vqvae_pixelcnn_sample_workspace_bytes(int64_t B, int H, int W, int dim, int n_layers) {
    if (B < 1 || H < 1 || W < 1 || dim < 1 || n_layers < 1) return 0;
    if (H != W || H > kPsMaxSide || dim % 4 || dim > kPsMaxDim || B > 0x7fffffff) return 0;
    const size_t per = ps_ws_floats(H, dim, n_layers) * sizeof(float);
    if ((size_t)B > SIZE_MAX / per) return 0;
    return (size_t)B * per;
}

int vqvae_pixelcnn_sample_f32(const void *packed, size_t packed_bytes, const int64_t *label, const float *uniforms, int64_t B, int H,
                              int W, int K, int dim, int n_layers, int n_classes, int64_t *samples, float *logits, int32_t *status,
                              void *workspace, size_t workspace_bytes, vqvae_stream_t stream) {
    return vqvae_pixelcnn_sample_ex_f32(packed, packed_bytes, label, uniforms, B, H, W, K, dim, n_layers, n_classes, 1.0f, 0, 1.0f,
                                        nullptr, samples, logits, status, workspace, workspace_bytes, stream);
}

int vqvae_pixelcnn_sample_ex_f32(const void *packed, size_t packed_bytes, const int64_t *label, const float *uniforms, int64_t B,
                                 int H, int W, int K, int dim, int n_layers, int n_classes, float temperature, int top_k,
                                 float top_p, const int64_t *given, int64_t *samples, float *logits, int32_t *status,
                                 void *workspace, size_t workspace_bytes, vqvae_stream_t stream) {
    if (!packed || !label || !uniforms || !samples || !status || !workspace) return VQVAE_ERR_NULL;
    if (B < 1 || H < 1 || W < 1 || K < 1 || dim < 1 || n_layers < 1 || n_classes < 1) return VQVAE_ERR_SHAPE;
    if (!std::isfinite(temperature) || !(temperature > 0.0f) || top_k < 0 || !(top_p > 0.0f && top_p <= 1.0f)) return VQVAE_ERR_SHAPE;
    if (H != W || H > kPsMaxSide || !ps_supported(K, dim, n_layers, n_classes)) return VQVAE_ERR_UNSUPPORTED;
    if (B > 0x7fffffff) return VQVAE_ERR_OVERFLOW;
    if ((reinterpret_cast<uintptr_t>(packed) | reinterpret_cast<uintptr_t>(workspace)) & 15) return VQVAE_ERR_UNSUPPORTED;
    if (packed_bytes < vqvae_pixelcnn_sample_packed_bytes(K, dim, n_layers, n_classes)) return VQVAE_ERR_WORKSPACE;
    if (workspace_bytes < vqvae_pixelcnn_sample_workspace_bytes(B, H, W, dim, n_layers)) return VQVAE_ERR_WORKSPACE;
    PsArgs a;
    a.img = static_cast<const float *>(packed);
    a.label = reinterpret_cast<const long long *>(label);
    a.u = uniforms;
    a.out = reinterpret_cast<long long *>(samples);
    a.logits = logits;
    a.status = status;
    a.ws = static_cast<float *>(workspace);
    a.ws_per_image = ps_ws_floats(H, dim, n_layers);
    a.S = H; a.dim = dim; a.K = K; a.nl = n_layers; a.ncls = n_classes;
    a.temperature = temperature;
    a.top_k = top_k >= K ? 0 : top_k;
    a.top_p = top_p;
    a.given = reinterpret_cast<const long long *>(given);
    // the plain draw is its own instantiation: no option costs it a register, a byte of LDS or a barrier; the filtered one has a
    // form for batches that put two workgroups on a CU (see the kernel)
    const bool filtered = temperature != 1.0f || a.top_k != 0 || top_p < 1.0f || given;
    const dim3 grid((unsigned)B), block(kPsThreads);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (!filtered)
        hipLaunchKernelGGL((pixelcnn_sample_kernel<false, false>), grid, block, 0, st, a);
    else if (B <= num_cus())
        hipLaunchKernelGGL((pixelcnn_sample_kernel<true, false>), grid, block, 0, st, a);
    else
        hipLaunchKernelGGL((pixelcnn_sample_kernel<true, true>), grid, block, 0, st, a);
    return (int)hipGetLastError();
}

}  // extern "C"
