// Backward of the GatedPixelCNN prior (pixelcnn/models.py), gfx950.  Row-major (B,H,W,C) activations throughout.
//
//   vqvae_conv_taps_wgrad_f32        grad_w[co][ci][t] = sum_{b,y,x} gy[b,y,x,co] * x[b, y+dy_t, x+dx_t, ci]   (0 outside the map)
//                                    the weight gradient of a tap-list (masked) convolution, in the weight's own (Cout, Cin, kh, kw)
//                                    layout.  Exact fp32 products on v_mfma_f32_32x32x2_f32 with the PIXEL as the reduction index;
//                                    maps of at most 8 x 8 with 32-channel multiples (the prior's latent maps): both maps of an
//                                    image staged once in LDS -- the x map inside a zero frame wide enough for every tap -- and
//                                    every tap served from that staging (taps_wgrad_map_kernel); other shapes: 32-pixel blocks per
//                                    tap (taps_wgrad_blk_kernel).  Per-range partial sums, combined in a fixed order.
//   vqvae_conv_taps_pack_dgrad_f32   packs the data gradient of a tap-list conv: the forward's tap kernels with the taps negated,
//                                    Cin and Cout swapped and the per-tap transposed weight (vqvae_conv_taps_pack_f32's scheme)
//   vqvae_gated_activation_backward_f32   da = go sigma(g) (1 - tanh^2 a), dg = go tanh(a) sigma(g) (1 - sigma(g)), recomputing
//                                    (a|g) in the forward's order, plus the per-image sum of (da|dg) for the class embedding
//   vqvae_gather_rows_backward_f32   grad_table[k] = sum_{i: idx_i = k} grad_out[i]: stable radix sort by row, fixed-order fp64 sums
//   vqvae_cross_entropy_f32 / _backward_f32   mean softmax cross-entropy over rows (max-subtracted log-sum-exp), fixed-order mean
//   vqvae_bias_grad_wide_f32         per-channel column sums of any width (the 512-wide hidden layer and the K logits)
// No floating-point atomics anywhere: every result is bit-reproducible run to run.
#include "train_reduce.h"

namespace vqvae {

// ------------------------------------------------------------------------------------------------ tap-list weight gradient
constexpr int kTwBlkMaxSplit = 64;      // pixel-range splits of the per-tap kernel
constexpr int kTwMapWgs = 256;          // workgroups the map-resident kernel aims for (one per CU: its LDS staging is large)
constexpr int kTwTapsPerGroup = 8;      // taps one wave accumulates at once (8 x 16 accumulators)
constexpr int kTwLd = 68;               // LDS row: 64 channels + 4 (16-byte aligned rows, staggered banks)

struct TapsWgGeom {
    int B, H, W, CA, CB;                // A = gy (B,H,W,CA = Cout), Bt = x (B,H,W,CB = Cin)
    int ntaps;
    signed char dy[32], dx[32];
    // map-resident kernel: zero frame of the x map and taps as offsets into it
    int ylo, xlo, PH, PW, per_group;
    int toff[32];
    long long rows_per_split;           // pixel blocks (per-tap kernel) or images (map kernel) per split
};

// Per tap: a workgroup owns a 64 x 64 (ca, cb) tile of one tap and a range of 32-pixel blocks; the blocks' gy rows and
// tap-shifted x rows are staged in LDS (double-buffered), wave w multiplies pixels [8w, 8w + 8), and the four waves' tiles are
// added in wave order.  Channel counts are multiples of 4 (16-byte loads).
__global__ __launch_bounds__(256, 2) void taps_wgrad_blk_kernel(const float *__restrict__ A, const float *__restrict__ Bt,
                                                                float *__restrict__ partial, TapsWgGeom g) {
    constexpr int MT = 2, NT = 2, PB = 32, LD = kTwLd;
    __shared__ __attribute__((aligned(16))) float smem[2 * 2 * PB * LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int tiles_b = (g.CB + 63) / 64, tiles_a = (g.CA + 63) / 64;
    int t = blockIdx.x;
    const int tb = t % tiles_b; t /= tiles_b;
    const int ta = t % tiles_a; t /= tiles_a;
    const int tap = t;
    const int dy = g.dy[tap], dx = g.dx[tap];
    const unsigned npix = (unsigned)g.B * g.H * g.W, img_px = (unsigned)g.H * g.W;
    const unsigned nblk = (npix + PB - 1) / PB;
    const unsigned blk_lo = (unsigned)(blockIdx.y * g.rows_per_split);
    unsigned blk_hi = blk_lo + (unsigned)g.rows_per_split;
    if (blk_hi > nblk) blk_hi = nblk;

    f32x16 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mt][nt][r] = 0.0f;

    const int pi = tid >> 3, cg = tid & 7;
    const int ca0 = ta * 64 + 8 * cg, cb0 = tb * 64 + 8 * cg;
    f32x4 ra[2], rb[2];
    auto fetch = [&](unsigned blk) {
        const unsigned p = blk * PB + pi;
        const f32x4 z4 = {0.0f, 0.0f, 0.0f, 0.0f};
        ra[0] = ra[1] = rb[0] = rb[1] = z4;
        if (p >= npix) return;
        const unsigned b = p / img_px, rem = p - b * img_px;
        const int y = (int)(rem / (unsigned)g.W), x = (int)(rem - (unsigned)y * g.W);
        const float *ap = A + (size_t)p * g.CA;
#pragma unroll
        for (int q = 0; q < 2; ++q)
            if (ca0 + 4 * q < g.CA) ra[q] = *reinterpret_cast<const f32x4 *>(ap + ca0 + 4 * q);
        const int yB = y + dy, xB = x + dx;
        if (yB < 0 || yB >= g.H || xB < 0 || xB >= g.W) return;
        const float *bp = Bt + (((size_t)b * g.H + yB) * g.W + xB) * g.CB;
#pragma unroll
        for (int q = 0; q < 2; ++q)
            if (cb0 + 4 * q < g.CB) rb[q] = *reinterpret_cast<const f32x4 *>(bp + cb0 + 4 * q);
    };
    auto park = [&](int buf) {
        float *as = smem + (buf * 2 + 0) * PB * LD + pi * LD + 8 * cg;
        float *bs = smem + (buf * 2 + 1) * PB * LD + pi * LD + 8 * cg;
        *reinterpret_cast<f32x4 *>(as) = ra[0]; *reinterpret_cast<f32x4 *>(as + 4) = ra[1];
        *reinterpret_cast<f32x4 *>(bs) = rb[0]; *reinterpret_cast<f32x4 *>(bs + 4) = rb[1];
    };

    if (blk_lo < blk_hi) {
        fetch(blk_lo);
        park(0);
    }
    __syncthreads();
    for (unsigned blk = blk_lo; blk < blk_hi; ++blk) {
        const int buf = (blk - blk_lo) & 1;
        if (blk + 1 < blk_hi) fetch(blk + 1);
        const float *as = smem + (buf * 2 + 0) * PB * LD + (8 * wave + h) * LD + l31;
        const float *bs = smem + (buf * 2 + 1) * PB * LD + (8 * wave + h) * LD + l31;
#pragma unroll
        for (int q = 0; q < 4; ++q) {                       // k-step q: pixels 8 wave + 2q + h
            float av[MT], bv[NT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) av[mt] = as[2 * q * LD + 32 * mt];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) bv[nt] = bs[2 * q * LD + 32 * nt];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[mt], bv[nt], acc[mt][nt], 0, 0, 0);
        }
        if (blk + 1 < blk_hi) park(buf ^ 1);
        __syncthreads();
    }
    float *red = smem;                                       // 4096 floats
    for (int w = 3; w >= 1; --w) {
        __syncthreads();
        if (wave == w) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) red[((mt * NT + nt) * 16 + r) * 64 + lane] = acc[mt][nt][r];
        }
        __syncthreads();
        if (wave == w - 1) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[mt][nt][r] += red[((mt * NT + nt) * 16 + r) * 64 + lane];
        }
    }
    if (wave == 0) {
        float *dst = partial + ((size_t)blockIdx.y * g.ntaps + tap) * g.CA * g.CB;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int a = ta * 64 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    const int c = tb * 64 + nt * 32 + l31;
                    if (a < g.CA && c < g.CB) dst[(size_t)a * g.CB + c] = acc[mt][nt][r];
                }
    }
}

// Map-resident form for maps of at most 8 x 8 pixels and 32-channel multiples.  A workgroup owns a 64 x 64 (ca, cb) tile, a group
// of up to 8 taps and a range of images; per image it stages gy (64 pixel rows, zero beyond H*W) and x inside its zero frame
// ((H + ylo..yhi) x (W + xlo..xhi) rows, the frame zeroed once and never written again) in LDS.  Wave w owns the 32 x 32 sub-tile
// (w & 1, w >> 1) for all taps of the group: per pixel pair one read of gy and, per tap, one read of x at the pixel's frame
// offset plus the tap's constant offset.  Its accumulators are final for its range: no reduction across waves.
__global__ __launch_bounds__(256, 1) void taps_wgrad_map_kernel(const float *__restrict__ A, const float *__restrict__ Bt,
                                                                float *__restrict__ partial, TapsWgGeom g) {
    constexpr int LD = kTwLd, NTW = kTwTapsPerGroup;
    extern __shared__ __attribute__((aligned(16))) float dsm[];
    float *As = dsm;                                         // [64][LD]
    float *Bs = dsm + 64 * LD;                               // [PH * PW][LD]
    __shared__ int boff[64];
    const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, h = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int qa = wave & 1, qb = wave >> 1;
    const int tiles_b = (g.CB + 63) / 64, tiles_a = (g.CA + 63) / 64;
    int t = blockIdx.x;
    const int tb = t % tiles_b; t /= tiles_b;
    const int ta = t % tiles_a; t /= tiles_a;
    const int grp = t;
    const int t0 = grp * g.per_group;
    const int ntw = (g.ntaps - t0) < g.per_group ? (g.ntaps - t0) : g.per_group;
    const int ca0 = ta * 64, cb0 = tb * 64;
    const bool active = ca0 + 32 * qa < g.CA && cb0 + 32 * qb < g.CB;      // uniform per wave (32-channel multiples)
    const int HW = g.H * g.W, nframe = g.PH * g.PW;
    const long long b_lo = (long long)blockIdx.y * g.rows_per_split;
    long long b_hi = b_lo + g.rows_per_split;
    if (b_hi > g.B) b_hi = g.B;

    for (int i = tid; i < (64 + nframe) * LD / 4; i += 256) reinterpret_cast<f32x4 *>(dsm)[i] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    if (tid < 64) {
        // pixel slots beyond the map read gy = 0 and the frame position of pixel (0, 0): in bounds for every tap
        const int p = tid < HW ? tid : 0;
        const int y = p / g.W, x = p - (p / g.W) * g.W;
        boff[tid] = (y - g.ylo) * g.PW + (x - g.xlo);
    }
    f32x16 acc[NTW];
#pragma unroll
    for (int j = 0; j < NTW; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.0f;
    int toff[NTW];
#pragma unroll
    for (int j = 0; j < NTW; ++j) toff[j] = j < ntw ? g.toff[t0 + j] : 0;

    for (long long b = b_lo; b < b_hi; ++b) {
        __syncthreads();                                    // the previous image has been read (first: the zero fill)
        // gy: HW rows x 16 float4 of the tile's 64 channels; x: HW rows into the frame
        for (int e = tid; e < HW * 16; e += 256) {
            const int p = e >> 4, c = (e & 15) * 4;
            if (ca0 + c < g.CA)
                *reinterpret_cast<f32x4 *>(As + p * LD + c) =
                    *reinterpret_cast<const f32x4 *>(A + ((size_t)b * HW + p) * g.CA + ca0 + c);
            if (cb0 + c < g.CB) {
                const int y = p / g.W, x = p - y * g.W;
                *reinterpret_cast<f32x4 *>(Bs + ((y - g.ylo) * g.PW + (x - g.xlo)) * LD + c) =
                    *reinterpret_cast<const f32x4 *>(Bt + ((size_t)b * HW + p) * g.CB + cb0 + c);
            }
        }
        __syncthreads();
        if (active) {
            const float *ar = As + h * LD + 32 * qa + l31;
            const float *br = Bs + 32 * qb + l31;
#pragma unroll 4
            for (int q = 0; q < 32; ++q) {
                const float av = ar[2 * q * LD];
                const int bo = boff[2 * q + h];
#pragma unroll
                for (int j = 0; j < NTW; ++j)
                    if (j < ntw) {
                        const float bv = br[(bo + toff[j]) * LD];
                        acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[j], 0, 0, 0);
                    }
            }
        }
    }
    if (!active) return;
    float *dst = partial + (size_t)blockIdx.y * g.ntaps * g.CA * g.CB;
#pragma unroll
    for (int j = 0; j < NTW; ++j)
        if (j < ntw) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int a = ca0 + 32 * qa + (r & 3) + 8 * (r >> 2) + 4 * h;
                dst[((size_t)(t0 + j) * g.CA + a) * g.CB + cb0 + 32 * qb + l31] = acc[j][r];
            }
        }
}

static int taps_groups(int ntaps) { return (ntaps + kTwTapsPerGroup - 1) / kTwTapsPerGroup; }

static int taps_fill(TapsWgGeom &g, int ntaps, const int8_t *dy, const int8_t *dx) {
    g.ntaps = ntaps;
    int ylo = 0, yhi = 0, xlo = 0, xhi = 0;
    for (int i = 0; i < 32; ++i) {
        const int a = i < ntaps ? dy[i] : 0, b = i < ntaps ? dx[i] : 0;
        if (a < -7 || a > 7 || b < -7 || b > 7) return VQVAE_ERR_UNSUPPORTED;
        g.dy[i] = (signed char)a; g.dx[i] = (signed char)b;
        ylo = a < ylo ? a : ylo; yhi = a > yhi ? a : yhi;
        xlo = b < xlo ? b : xlo; xhi = b > xhi ? b : xhi;
    }
    g.ylo = ylo; g.xlo = xlo;
    g.PH = g.H + yhi - ylo; g.PW = g.W + xhi - xlo;
    for (int i = 0; i < 32; ++i) g.toff[i] = g.dy[i] * g.PW + g.dx[i];
    const int ngroups = taps_groups(ntaps);
    g.per_group = (ntaps + ngroups - 1) / ngroups;
    return VQVAE_OK;
}

static size_t taps_map_lds(const TapsWgGeom &g) { return (size_t)(64 + g.PH * g.PW) * kTwLd * sizeof(float); }

static bool taps_map_ok(const TapsWgGeom &g) {
    return g.H <= 8 && g.W <= 8 && g.CA % 32 == 0 && g.CB % 32 == 0 && taps_map_lds(g) <= 96 * 1024;
}

static long long taps_tiles(int CA, int CB) { return (long long)((CA + 63) / 64) * ((CB + 63) / 64); }

// image ranges the map-resident kernel asks for: kTwMapWgs workgroups over its (ca, cb) tiles and tap groups
static long long taps_map_splits(int ntaps, int CA, int CB) {
    const long long wgs = taps_tiles(CA, CB) * taps_groups(ntaps);
    return (kTwMapWgs + wgs - 1) / wgs;
}

// What vqvae_conv_taps_wgrad_f32 launches for a filled geometry: the map-resident kernel over ranges of images, or the per-tap
// kernel over ranges of 32-pixel blocks (enough workgroups for eight per CU of 256, at least 8 blocks each, at most kTwBlkMaxSplit)
static ReducePlan taps_plan(const TapsWgGeom &g) {
    ReducePlan p;
    if (taps_map_ok(g)) {
        p.kernel = VQVAE_TRAIN_KERNEL_CONV_TAPS_WGRAD_MAP;
        p.items = g.B;
        p.want = taps_map_splits(g.ntaps, g.CA, g.CB);
        plan_ranges(p, g.B);
        p.aux0 = taps_groups(g.ntaps);
        p.aux1 = g.per_group;
    } else {
        p.kernel = VQVAE_TRAIN_KERNEL_CONV_TAPS_WGRAD_BLK;
        p.items = ((long long)g.B * g.H * g.W + 31) / 32;
        const long long wgs = taps_tiles(g.CA, g.CB) * g.ntaps;
        p.want = (8LL * 256 + wgs - 1) / wgs;
        if (p.want > (p.items + 7) / 8) p.want = (p.items + 7) / 8;
        plan_ranges(p, kTwBlkMaxSplit);
    }
    return p;
}

int conv_taps_wgrad_plan(long long B, int H, int W, int Cin, int Cout, int ntaps, const int8_t *dy, const int8_t *dx, ReducePlan &p) {
    TapsWgGeom g;
    g.B = (int)B; g.H = H; g.W = W; g.CA = Cout; g.CB = Cin;
    const int rc = taps_fill(g, ntaps, dy, dx);
    if (rc == VQVAE_OK) p = taps_plan(g);
    return rc;
}

// ---------------------------------------------------------------------------------------------------- dgrad pack staging
// st[ci][co][t] = w[co][ci][t0 + t]: the per-tap transposed weight of a slice of the tap list
__global__ __launch_bounds__(256) void taps_transpose_kernel(const float *__restrict__ w, int wtaps, int t0, int k, int Cin, int Cout,
                                                             float *__restrict__ st) {
    const long long total = (long long)Cin * Cout * k;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int t = (int)(e % k);
        const long long r = e / k;
        const int co = (int)(r % Cout), ci = (int)(r / Cout);
        st[e] = w[((size_t)co * Cin + ci) * wtaps + t0 + t];
    }
}

// --------------------------------------------------------------------------------------------------- gated activation
// one workgroup per (image, 64-channel chunk): 4 pixel groups x 64 channels; every thread writes da / dg of its pixels and,
// with cond, adds them up in pixel order (fp64); the four groups are combined in group order
__global__ __launch_bounds__(256) void gated_backward_kernel(const float *__restrict__ t1, const float *__restrict__ t2,
                                                             const float *__restrict__ cond, const float *__restrict__ go, int HW,
                                                             int dim, float *__restrict__ gpre, const float *__restrict__ gc_in,
                                                             float *__restrict__ gc) {
    __shared__ double red[2][4][64];
    const long long b = blockIdx.x;
    const int tid = threadIdx.x, grp = tid >> 6, c = blockIdx.y * 64 + (tid & 63);
    double sa = 0.0, sg = 0.0;
    if (c < dim) {
        float ca = 0.0f, cg = 0.0f;
        if (cond) { ca = cond[(size_t)b * 2 * dim + c]; cg = cond[(size_t)b * 2 * dim + dim + c]; }
        for (int p = grp; p < HW; p += 4) {
            const size_t px = (size_t)b * HW + p;
            const size_t i = px * 2 * dim + c;
            float a = t1[i], gg = t1[i + dim];
            if (t2) { a = a + t2[i]; gg = gg + t2[i + dim]; }           // the forward's order (gated_activation_kernel)
            if (cond) { a = a + ca; gg = gg + cg; }
            const float th = tanhf(a), s = 1.0f / (1.0f + expf(-gg));
            const float o = go[px * dim + c];
            const float da = o * s * (1.0f - th * th);
            const float dg = o * th * (s * (1.0f - s));
            gpre[i] = da;
            gpre[i + dim] = dg;
            sa += (double)da;
            sg += (double)dg;
        }
    }
    if (!gc) return;
    red[0][grp][tid & 63] = sa;
    red[1][grp][tid & 63] = sg;
    __syncthreads();
    if (grp == 0 && c < dim) {
        const double ta = (red[0][0][tid] + red[0][1][tid]) + (red[0][2][tid] + red[0][3][tid]);
        const double tg = (red[1][0][tid] + red[1][1][tid]) + (red[1][2][tid] + red[1][3][tid]);
        float va = (float)ta, vg = (float)tg;
        if (gc_in) { va = gc_in[(size_t)b * 2 * dim + c] + va; vg = gc_in[(size_t)b * 2 * dim + dim + c] + vg; }
        gc[(size_t)b * 2 * dim + c] = va;
        gc[(size_t)b * 2 * dim + dim + c] = vg;
    }
}

// ------------------------------------------------------------------------------------------------- gather (embedding) backward
// the sorted segmented sum (launch_segsum, train_reduce.h), then per table row:
// grad_table[k][c] = sum of the code's units in unit order (0 for rows nobody read)
__global__ __launch_bounds__(256) void gb_final_kernel(const int *__restrict__ unit_start, const double *__restrict__ partial, int rows,
                                                       int C, float *__restrict__ gt) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)rows * C) return;
    const int k = (int)(e / C), c = (int)(e - (long long)k * C);
    double s = 0.0;
    for (int u = unit_start[k]; u < unit_start[k + 1]; ++u) s += partial[(size_t)u * C + c];
    gt[e] = (float)s;
}

// ----------------------------------------------------------------------------------------------------------- cross-entropy
// one wave per row: m = max, s = sum exp(l - m) in lane-strided order and a fixed butterfly; lse = m + log s
__device__ __forceinline__ void ce_row_stats(const float *__restrict__ l, int K, int lane, float &m, float &s) {
    m = -INFINITY;
    for (int k = lane; k < K; k += 64) m = fmaxf(m, l[k]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    s = 0.0f;
    for (int k = lane; k < K; k += 64) s += expf(l[k] - m);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
}

__global__ __launch_bounds__(256) void ce_rows_kernel(const float *__restrict__ logits, const long long *__restrict__ tgt, long long N,
                                                      int K, double *__restrict__ row_loss) {
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= N) return;
    const float *l = logits + (size_t)r * K;
    float m, s;
    ce_row_stats(l, K, lane, m, s);
    if (lane == 0) {
        const long long t = tgt[r];
        row_loss[r] = (t < 0 || t >= K) ? (double)NAN : ((double)m + (double)logf(s)) - (double)l[t];
    }
}

// mean over rows: one workgroup, 256 strided fp64 sums combined by a fixed tree
__global__ __launch_bounds__(256) void ce_mean_kernel(const double *__restrict__ row_loss, long long N, float *__restrict__ out) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (long long r = tid; r < N; r += 256) s += row_loss[r];
    block_sum_f64(red, tid, s);
    if (tid == 0) out[0] = (float)(red[0] / (double)N);
}

__global__ __launch_bounds__(256) void ce_backward_kernel(const float *__restrict__ logits, const long long *__restrict__ tgt,
                                                          long long N, int K, const float *__restrict__ gl, float *__restrict__ gx) {
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (r >= N) return;
    const float *l = logits + (size_t)r * K;
    float m, s;
    ce_row_stats(l, K, lane, m, s);
    const float scale = (gl ? gl[0] : 1.0f) / (float)N;
    const long long t = tgt[r];
    const bool bad = t < 0 || t >= K;
    for (int k = lane; k < K; k += 64) {
        const float p = expf(l[k] - m) / s;
        gx[(size_t)r * K + k] = bad ? NAN : (p - (k == t ? 1.0f : 0.0f)) * scale;
    }
}

// ------------------------------------------------------------------------------------------------------- wide column sums
// partial[block][c] = sum over the block's row range of g[row][c] (fp64, fixed order).  C <= 256: 256 / C row groups, combined in
// group order; wider rows: one group, channels in 256-wide passes.
__global__ __launch_bounds__(256) void bias_wide_partial_kernel(const float *__restrict__ g, long long P, int C, long long rpb,
                                                                double *__restrict__ partial) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const long long lo = (long long)blockIdx.x * rpb;
    long long hi = lo + rpb;
    if (hi > P) hi = P;
    if (C > 256) {
        for (int c = tid; c < C; c += 256) {
            double acc = 0.0;
            for (long long p = lo; p < hi; ++p) acc += (double)g[(size_t)p * C + c];
            partial[(size_t)blockIdx.x * C + c] = acc;
        }
        return;
    }
    const int G = 256 / C, grp = tid / C, c = tid - grp * C;
    double acc = 0.0;
    if (grp < G)
        for (long long p = lo + grp; p < hi; p += G) acc += (double)g[(size_t)p * C + c];
    red[tid] = acc;
    __syncthreads();
    if (tid < C) {
        double s = 0.0;
        for (int q = 0; q < G; ++q) s += red[q * C + tid];
        partial[(size_t)blockIdx.x * C + tid] = s;
    }
}

static bool misaligned(const void *p) { return reinterpret_cast<uintptr_t>(p) & 15; }

}  // namespace vqvae

using namespace vqvae;

extern "C" {

size_t vqvae_conv_taps_wgrad_workspace_bytes(int ntaps, int Cin, int Cout) {
    if (ntaps < 1 || ntaps > 32 || Cin < 1 || Cout < 1 || Cin % 4 || Cout % 4) return 0;
    // the larger of taps_plan's two bounds, whichever kernel the map size and the taps will select
    long long ns = kTwBlkMaxSplit;
    const long long nm = taps_map_splits(ntaps, Cout, Cin);
    if (nm > ns) ns = nm;
    return (size_t)ns * ntaps * Cin * Cout * sizeof(float);
}

int vqvae_conv_taps_wgrad_f32(const float *grad_y, const float *x, int64_t B, int H, int W, int Cin, int Cout, int ntaps,
                              const int8_t *dy, const int8_t *dx, float *grad_w, void *workspace, size_t workspace_bytes,
                              vqvae_stream_t stream) {
    if (!grad_y || !x || !dy || !dx || !grad_w) return VQVAE_ERR_NULL;
    if (B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || ntaps < 1) return VQVAE_ERR_SHAPE;
    if (ntaps > 32 || Cin % 4 || Cout % 4 || misaligned(grad_y) || misaligned(x)) return VQVAE_ERR_UNSUPPORTED;
    if (B * (int64_t)H * W > INT32_MAX || B * (int64_t)H * W * (Cin > Cout ? Cin : Cout) > ((int64_t)1 << 40)) return VQVAE_ERR_OVERFLOW;
    if (!workspace || workspace_bytes < vqvae_conv_taps_wgrad_workspace_bytes(ntaps, Cin, Cout)) return VQVAE_ERR_WORKSPACE;
    TapsWgGeom g;
    g.B = (int)B; g.H = H; g.W = W; g.CA = Cout; g.CB = Cin;
    const int rc = taps_fill(g, ntaps, dy, dx);
    if (rc != VQVAE_OK) return rc;
    const ReducePlan p = taps_plan(g);
    g.rows_per_split = p.per_split;
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *partial = static_cast<float *>(workspace);
    const long long tiles = taps_tiles(Cout, Cin);
    if (p.kernel == VQVAE_TRAIN_KERNEL_CONV_TAPS_WGRAD_MAP) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(taps_wgrad_map_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  96 * 1024);
        hipLaunchKernelGGL(taps_wgrad_map_kernel, dim3((unsigned)(tiles * p.aux0), (unsigned)p.splits), dim3(256), taps_map_lds(g), st,
                           grad_y, x, partial, g);
    } else {
        hipLaunchKernelGGL(taps_wgrad_blk_kernel, dim3((unsigned)(tiles * ntaps), (unsigned)p.splits), dim3(256), 0, st, grad_y, x,
                           partial, g);
    }
    launch_split_reduce(partial, (int)p.splits, ntaps, Cout, Cin, grad_w, st);
    return (int)hipGetLastError();
}

size_t vqvae_conv_taps_pack_dgrad_bytes(int ntaps, int Cin, int Cout) {
    const size_t pk = vqvae_conv_taps_packed_bytes(ntaps, Cout, Cin);
    if (pk == 0 || Cin % 4 || Cout % 4) return 0;
    return align_up(pk, 256) + (size_t)ntaps * Cin * Cout * sizeof(float);
}

int vqvae_conv_taps_pack_dgrad_f32(const float *w, int wtaps, int t0, int ntaps, const int8_t *dy, const int8_t *dx, int Cin, int Cout,
                                   float *packed, vqvae_stream_t stream) {
    if (!w || !dy || !dx || !packed) return VQVAE_ERR_NULL;
    if (Cin < 1 || Cout < 1 || ntaps < 1 || wtaps < 1 || t0 < 0 || t0 + ntaps > wtaps) return VQVAE_ERR_SHAPE;
    if (ntaps > 16 || Cin % 4 || Cout % 4) return VQVAE_ERR_UNSUPPORTED;
    if (reinterpret_cast<uintptr_t>(packed) & 15) return VQVAE_ERR_UNSUPPORTED;        // (before the staging launch, not behind it)
    int8_t ndy[16], ndx[16];
    for (int i = 0; i < ntaps; ++i) {
        if (dy[i] < -7 || dy[i] > 7 || dx[i] < -7 || dx[i] > 7) return VQVAE_ERR_UNSUPPORTED;
        ndy[i] = (int8_t)-dy[i];
        ndx[i] = (int8_t)-dx[i];
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *stage = reinterpret_cast<float *>(reinterpret_cast<char *>(packed) +
                                             align_up(vqvae_conv_taps_packed_bytes(ntaps, Cout, Cin), 256));
    hipLaunchKernelGGL(taps_transpose_kernel, dim3(grid_of((long long)Cin * Cout * ntaps, 4096)), dim3(256), 0, st, w, wtaps, t0, ntaps,
                       Cin, Cout, stage);
    const int rc = (int)hipGetLastError();
    if (rc != 0) return rc;
    // the data gradient conv reads the Cout channels of grad_y and writes Cin: its (Cout', Cin', taps) weight is the staging
    return vqvae_conv_taps_pack_f32(stage, ntaps, ndy, ndx, Cout, Cin, packed, stream);
}

int vqvae_gated_activation_backward_f32(const float *t1, const float *t2, const float *cond, const float *grad_out, int64_t B, int HW,
                                        int dim, float *grad_pre, const float *grad_cond_in, float *grad_cond, vqvae_stream_t stream) {
    if (!t1 || !grad_out || !grad_pre) return VQVAE_ERR_NULL;
    if ((grad_cond || grad_cond_in) && !cond) return VQVAE_ERR_NULL;
    if (grad_cond_in && !grad_cond) return VQVAE_ERR_NULL;
    if (B < 1 || HW < 1 || dim < 1) return VQVAE_ERR_SHAPE;
    if (B > 0x7fffffff) return VQVAE_ERR_OVERFLOW;
    hipLaunchKernelGGL(gated_backward_kernel, dim3((unsigned)B, (unsigned)((dim + 63) / 64)), dim3(256), 0, static_cast<hipStream_t>(stream),
                       t1, t2, cond, grad_out, HW, dim, grad_pre, grad_cond_in, grad_cond);
    return (int)hipGetLastError();
}

size_t vqvae_gather_rows_backward_workspace_bytes(int64_t n, int C, int rows) {
    if (n < 1 || n > INT32_MAX || C < 1 || rows < 1 || rows > (1 << 24)) return 0;
    return segsum_plan(n, rows, C).total;
}

int vqvae_gather_rows_backward_f32(const int64_t *idx, const float *grad_out, int64_t n, int C, int rows, float *grad_table,
                                   void *workspace, size_t workspace_bytes, vqvae_stream_t stream) {
    if (!idx || !grad_out || !grad_table) return VQVAE_ERR_NULL;
    if (n < 1 || C < 1 || rows < 1) return VQVAE_ERR_SHAPE;
    if (n > INT32_MAX || rows > (1 << 24)) return VQVAE_ERR_OVERFLOW;
    const SegsumPlan p = segsum_plan(n, rows, C);
    if (!workspace || workspace_bytes < p.total) return VQVAE_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char *ws = static_cast<char *>(workspace);
    const hipError_t e = launch_segsum(p, grad_out, reinterpret_cast<const long long *>(idx), n, rows, C, 1, 1, ws, st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(gb_final_kernel, dim3((unsigned)(((long long)rows * C + 255) / 256)), dim3(256), 0, st,
                       reinterpret_cast<const int *>(ws + p.off_units), reinterpret_cast<const double *>(ws + p.off_partials), rows, C,
                       grad_table);
    return (int)hipGetLastError();
}

size_t vqvae_cross_entropy_workspace_bytes(int64_t N) { return N < 1 ? 0 : (size_t)N * sizeof(double); }

int vqvae_cross_entropy_f32(const float *logits, const int64_t *targets, int64_t N, int K, float *loss, void *workspace,
                            size_t workspace_bytes, vqvae_stream_t stream) {
    if (!logits || !targets || !loss) return VQVAE_ERR_NULL;
    if (N < 1 || K < 1) return VQVAE_ERR_SHAPE;
    if (N * (int64_t)K > ((int64_t)1 << 40) || (N + 3) / 4 > 0x7fffffff) return VQVAE_ERR_OVERFLOW;
    if (!workspace || workspace_bytes < vqvae_cross_entropy_workspace_bytes(N)) return VQVAE_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    double *rl = static_cast<double *>(workspace);
    hipLaunchKernelGGL(ce_rows_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, logits, reinterpret_cast<const long long *>(targets),
                       (long long)N, K, rl);
    hipLaunchKernelGGL(ce_mean_kernel, dim3(1), dim3(256), 0, st, rl, (long long)N, loss);
    return (int)hipGetLastError();
}

int vqvae_cross_entropy_backward_f32(const float *logits, const int64_t *targets, int64_t N, int K, const float *grad_loss,
                                     float *grad_logits, vqvae_stream_t stream) {
    if (!logits || !targets || !grad_logits) return VQVAE_ERR_NULL;
    if (N < 1 || K < 1) return VQVAE_ERR_SHAPE;
    if (N * (int64_t)K > ((int64_t)1 << 40) || (N + 3) / 4 > 0x7fffffff) return VQVAE_ERR_OVERFLOW;
    hipLaunchKernelGGL(ce_backward_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, static_cast<hipStream_t>(stream), logits,
                       reinterpret_cast<const long long *>(targets), (long long)N, K, grad_loss, grad_logits);
    return (int)hipGetLastError();
}

size_t vqvae_bias_grad_wide_workspace_bytes(int C) { return C < 1 ? 0 : (size_t)kColsumBlocks * C * sizeof(double); }

int vqvae_bias_grad_wide_f32(const float *grad_y, int64_t P, int C, float *grad_b, void *workspace, size_t workspace_bytes,
                             vqvae_stream_t stream) {
    if (!grad_y || !grad_b) return VQVAE_ERR_NULL;
    if (P < 1 || C < 1) return VQVAE_ERR_SHAPE;
    if (P * (int64_t)C > ((int64_t)1 << 40)) return VQVAE_ERR_OVERFLOW;
    if (!workspace || workspace_bytes < vqvae_bias_grad_wide_workspace_bytes(C)) return VQVAE_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const ReducePlan p = bias_grad_wide_plan(P);
    double *partial = static_cast<double *>(workspace);
    hipLaunchKernelGGL(bias_wide_partial_kernel, dim3((unsigned)p.splits), dim3(256), 0, st, grad_y, (long long)P, C, p.per_split,
                       partial);
    launch_colsum_final(partial, (int)p.splits, C, grad_b, st);
    return (int)hipGetLastError();
}

}  // extern "C"
