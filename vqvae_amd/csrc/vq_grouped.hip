// Grouped (product) vector quantization (gfx950): the D channels of a latent row are cut into G groups of d = D / G channels and
// every group is quantized against its own (K, d) codebook (wav2vec 2.0's "groups", arXiv 2006.11477; vector-quantize-pytorch's
// heads with separate_codebook_per_head).  A position carries G indices; the implicit codebook has K^G entries at the memory and
// search cost of G K.
//   vqvae_vq_grouped_workspace_bytes            host only
//   vqvae_vq_grouped_forward_f32                1 x grp_split_kernel (z -> G dense slabs), G x vqvae_vq_forward_f32 (z_q = NULL:
//                                               indices, histogram, loss, perplexity of the group), 1 x grp_finish_kernel
//   vqvae_vq_grouped_decode_f32                 grp_finish_kernel without z: indices -> their code rows, side by side
//   vqvae_vq_grouped_backward_workspace_bytes   host only
//   vqvae_vq_grouped_backward_f32               grp_gradz_kernel; per group grp_split_kernel (the slab again), the shared sorted
//                                               segmented sum (launch_segsum, train_reduce.h) and grp_codebook_grad_kernel
// Every launch is on the caller's stream, one after the other: a forward captures into a graph as one linear chain.  No host sync,
// no allocation, no floating-point atomics, no memset node (every clear is a kernel: DESIGN.md section 5.4); the same bits in
// every run.
//
// THE CONTRACT (tests/vq_grouped_ref.py restates it on the CPU; the library is compiled with -ffp-contract=off, so every operation
// below is one IEEE operation in the stated precision).  1 <= G <= 16 groups, D % G == 0, d = D / G, codebooks E_0 .. E_{G-1}, each
// (K, d) fp32.  Rows and layouts are those of vqvae_vq_forward_f32: N = B H W rows, NCHW maps or, with VQVAE_VQ_ROWMAJOR, (N, D) rows.
//
//   slab_g = the channels [g d, (g + 1) d) of every row, bit for bit, in the layout of the input: a dense (B, d, H, W) map, or dense
//            (N, d) rows with VQVAE_VQ_ROWMAJOR.  The G slabs lie one after the other (in the workspace, or in slabs_out when given).
//   idx_g, hist_g, loss_g, perplexity_g = vqvae_vq_forward_f32's own outputs for (slab_g, E_g, beta) with z_q = NULL under the same
//            flags (the layout, VQVAE_VQ_CODEBOOK_PREPARED and the kernel-selection flags go to every group): the reference
//            quantizer's argmin, first-index ties and NaN-as-minimum included
//   z_q[row][g d + c] = z + (E_g[idx_g[row]][c] - z)    two fp32 operations (decode: the code's bits themselves)
//   loss = ((loss_0 + loss_1) + ...) / (float)G         fp32, group order, starting from loss_0 itself, one division, on the device
// Every group's loss is a mean over N d elements, so their mean is the reference's loss formula on the whole rows (a mean over N D
// elements).  With G = 1 every output has the bits of vqvae_vq_forward_f32.  An index outside [0, K) (decode, backward: indices that
// are not the forward's own) never reads a codebook: the d elements of that group's segment are NaN, and only those.
//
// Gradients: per group exactly those of vqvae_vq_backward_f32 on (slab_g, E_g, idx_g, grad_zq's channels of the group, g'), written
// into grad_z's channels of the group and into grad_codebooks[g].  g = the upstream gradient of loss (a device scalar, NULL = 1):
//   g'      = g / (float)G                              fp32
//   gs      = g' * s                                    fp32, s = fp32(2 / (N d)) rounded once from fp64; with
//                                                       VQVAE_VQ_BWD_COMMITMENT s = fp32(2 beta / (N d)): the EMA form's grad_z
//   grad_z  = grad_zq + gs * (z - e)                    (gs * (z - e) alone when grad_zq is NULL); one pass over z in its own layout
//   grad_E_g[k][c] = fp32(double(g') * (2 beta / (N d)) * (cnt_k * double(E_g[k][c]) - sum_{i: idx_g,i = k} double(slab_g,i[c])))
//                    the sum from the segmented sum's units as vqvae_vq_backward_f32 combines them (segsum_key_sum), on the slab
//                    re-materialised by the split kernel.
//
// The split, finish and grad_z kernels are streams: z (and grad_zq) and the output are the HBM traffic, the indices N G 8 bytes
// beside them, and the code rows come from the codebooks through L2 (G K d 4 = K D 4 bytes in all, 128 KiB at K = 512, D = 64).
// Row-major rows with d % 4 == 0, and NCHW maps with H W % 4 == 0, move 16 bytes per access when every tensor is 16-byte aligned;
// anything else goes element by element, with the same bits.  On row-major rows a code row is read 16 bytes at a time too; on NCHW
// maps every lane gathers E_g[k][c] for its own k.  256 threads a workgroup, a few registers a thread: the occupancy is the
// hardware's maximum, and the grid-stride loop caps the grid at 65536 workgroups.  Where N D < 2^32 the element arithmetic (an
// element's row, channel and group: divisions by d, D and H W) is 32-bit; larger tensors run the same bodies on 64-bit integers.
#include <initializer_list>

#include "train_reduce.h"
#include "vq_grouped.h"

namespace vqvae {

// the element-wise kernels: their bodies are vq_grouped.h's
// (I: unsigned element arithmetic where N D < 2^32, long long otherwise -- vq_grouped.h)
template <int V, typename I>
__global__ __launch_bounds__(256) void grp_split_kernel(GrpArgs a) { grp_split_body<V, I>(a); }
template <int V, typename I>
__global__ __launch_bounds__(256) void grp_finish_kernel(GrpArgs a, GrpBooks books) { grp_finish_body<V, I>(a, books); }
template <int V, typename I>
__global__ __launch_bounds__(256) void grp_gradz_kernel(GrpArgs a, GrpBooks books) { grp_gradz_body<V, I>(a, books); }

// vqb_codebook_grad_kernel's arithmetic (train.hip) for one group with the upstream gradient g' = g / (float)G
__global__ __launch_bounds__(256) void grp_codebook_grad_kernel(const float *__restrict__ cb, const int *__restrict__ offsets,
                                                                const int *__restrict__ unit_start,
                                                                const double *__restrict__ partial,
                                                                const float *__restrict__ g_loss, int K, int d, int G, double scale,
                                                                float *__restrict__ grad_cb) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)K * d) return;
    const int k = (int)(e / d), c = (int)(e - (long long)k * d);
    const double zsum = segsum_key_sum(unit_start, partial, k, c, d);
    const double cnt = (double)(offsets[k + 1] - offsets[k]);
    const float gq = (g_loss ? g_loss[0] : 1.0f) / (float)G;
    grad_cb[e] = (float)((double)gq * scale * (cnt * (double)cb[e] - zsum));
}

// ---- host side -----------------------------------------------------------------------------------------------------------------

constexpr int kGrpForwardFlags = VQVAE_VQ_ROWMAJOR | VQVAE_VQ_CODEBOOK_PREPARED | VQVAE_VQ_EXACT_SWEEP | VQVAE_VQ_BF16_FILTER |
                                 VQVAE_VQ_UNITS64_8WAVES | VQVAE_VQ_UNITS32_16WAVES | VQVAE_VQ_UNITS32_8WAVES;

static bool grp_envelope(long long N, int K, int D, int G) {
    return N >= 1 && N <= INT32_MAX && K >= 1 && K <= 16384 && D >= 1 && D <= 256 && G >= 1 && G <= kGrpMaxGroups && D % G == 0;
}

struct GrpPlan {
    size_t vq_bytes, off_slabs, total;    // G prepared codebook images (one quantizer workspace each), then the G slabs
};

// false: outside the envelope
static bool grp_plan(long long N, int K, int D, int G, GrpPlan &p) {
    if (!grp_envelope(N, K, D, G)) return false;
    const size_t one = vqvae_vq_workspace_bytes(N, K, D / G);
    if (one == 0) return false;
    p.vq_bytes = align_up(one, 256);
    p.off_slabs = p.vq_bytes * (size_t)G;
    p.total = p.off_slabs + align_up((size_t)N * D * sizeof(float), 256);
    return true;
}

struct GrpBwdPlan {
    SegsumPlan seg;
    size_t off_slab, total;               // the segmented sum's workspace, then one slab
};

static bool grp_bwd_plan(long long N, int K, int D, int G, GrpBwdPlan &p) {
    if (!grp_envelope(N, K, D, G)) return false;
    p.seg = segsum_plan(N, K, D / G);
    p.off_slab = align_up(p.seg.total, 256);
    p.total = p.off_slab + align_up((size_t)N * (D / G) * sizeof(float), 256);
    return true;
}

// shared argument checks: 0, or the error; HW and N on success
static int grp_check(int64_t B, int D, int H, int W, int K, int G, long long &HW, long long &N) {
    if (B < 1 || H < 1 || W < 1) return VQVAE_ERR_SHAPE;
    if (D < 1 || D > 256 || K < 1 || K > 16384 || G < 1 || G > kGrpMaxGroups || D % G) return VQVAE_ERR_UNSUPPORTED;
    HW = (long long)H * W;
    if (B > INT32_MAX || HW > INT32_MAX) return VQVAE_ERR_UNSUPPORTED;
    N = (long long)B * HW;
    if (N > INT32_MAX) return VQVAE_ERR_UNSUPPORTED;
    return VQVAE_OK;
}

struct GrpSpan {                          // a tensor as the bytes it covers (p == NULL: absent)
    const void *p;
    size_t bytes;
};

static bool grp_overlap(const GrpSpan &a, const GrpSpan &b) {
    if (!a.p || !b.p || !a.bytes || !b.bytes) return false;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a.p), b0 = reinterpret_cast<uintptr_t>(b.p);
    return a0 < b0 + b.bytes && b0 < a0 + a.bytes;
}

// does any output overlap any input?
static bool grp_any_overlap(std::initializer_list<GrpSpan> outs, std::initializer_list<GrpSpan> ins, const GrpBooks &books,
                            float *const *grad_books, int G, size_t book_bytes) {
    for (const GrpSpan &o : outs) {
        for (const GrpSpan &i : ins)
            if (grp_overlap(o, i)) return true;
        for (int g = 0; g < G; ++g)
            if (grp_overlap(o, GrpSpan{books.cb[g], book_bytes})) return true;
    }
    if (grad_books)
        for (int g = 0; g < G; ++g) {
            const GrpSpan o{grad_books[g], book_bytes};
            for (const GrpSpan &i : ins)
                if (grp_overlap(o, i)) return true;
            for (int h = 0; h < G; ++h)
                if (grp_overlap(o, GrpSpan{books.cb[h], book_bytes})) return true;
        }
    return false;
}

// the codebooks into the kernel argument: 0, or the error (a NULL entry, or one that is not 4-byte aligned)
static int grp_books(const float *const *codebooks, int G, GrpBooks &books) {
    if (!codebooks) return VQVAE_ERR_NULL;
    for (int g = 0; g < kGrpMaxGroups; ++g) books.cb[g] = nullptr;
    for (int g = 0; g < G; ++g) {
        books.cb[g] = codebooks[g];
        if (!books.cb[g]) return VQVAE_ERR_NULL;
    }
    for (int g = 0; g < G; ++g)
        if (reinterpret_cast<uintptr_t>(books.cb[g]) & 3) return VQVAE_ERR_UNSUPPORTED;
    return VQVAE_OK;
}

// may a launch move 16 bytes per access?  `ptrs`: every tensor it touches that way
static bool grp_vec4(const GrpArgs &a, std::initializer_list<const void *> ptrs) {
    if (any_misaligned(15, ptrs)) return false;
    return a.rowmajor ? (a.d & 3) == 0 : (a.HW & 3) == 0;
}

static bool grp_vec4_books(const GrpArgs &a, const GrpBooks &books, std::initializer_list<const void *> ptrs) {
    if (!grp_vec4(a, ptrs)) return false;
    if (a.rowmajor)                                                               // (NCHW: the codebooks are read element by element)
        for (int g = 0; g < a.G; ++g)
            if (reinterpret_cast<uintptr_t>(books.cb[g]) & 15) return false;
    return true;
}

static GrpArgs grp_args(const long long *idx, long long N, int D, long long HW, int K, int G, int rowmajor) {
    GrpArgs a = {};
    a.idx = idx;
    a.N = N;
    a.total = N * D;
    a.D = D;
    a.d = D / G;
    a.HW = (int)HW;
    a.K = K;
    a.rowmajor = rowmajor;
    a.G = G;
    a.g0 = 0;
    a.g1 = G;
    return a;
}

// may the element arithmetic be 32-bit?  Every element index of the whole rows, and the grid-stride sum past the last unit, fits
static bool grp_small(const GrpArgs &a) { return (unsigned long long)a.N * (unsigned)a.D < (1ULL << 32) - (1ULL << 26); }

// slabs [g0, g1) of z into out (and out2 when given), slab g0 first
static void grp_launch_split(GrpArgs a, const float *z, int g0, int g1, float *out, float *out2, hipStream_t st) {
    a.z = z;
    a.g0 = g0;
    a.g1 = g1;
    a.out = out;
    a.out2 = out2;
    a.total = a.N * a.d * (g1 - g0);
    const bool vec = grp_vec4(a, {z, out, out2});
    if (grp_small(a)) {
        if (vec) hipLaunchKernelGGL((grp_split_kernel<4, unsigned>), dim3(grid_of(a.total >> 2)), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((grp_split_kernel<1, unsigned>), dim3(grid_of(a.total)), dim3(256), 0, st, a);
    } else {
        if (vec) hipLaunchKernelGGL((grp_split_kernel<4, long long>), dim3(grid_of(a.total >> 2)), dim3(256), 0, st, a);
        else hipLaunchKernelGGL((grp_split_kernel<1, long long>), dim3(grid_of(a.total)), dim3(256), 0, st, a);
    }
}

#define GRP_LAUNCH(KERNEL, VEC, A, BOOKS, ST)                                                                              \
    do {                                                                                                                   \
        if (grp_small(A)) {                                                                                                \
            if (VEC) hipLaunchKernelGGL((KERNEL<4, unsigned>), dim3(grid_of((A).total >> 2)), dim3(256), 0, ST, A, BOOKS);     \
            else hipLaunchKernelGGL((KERNEL<1, unsigned>), dim3(grid_of((A).total)), dim3(256), 0, ST, A, BOOKS);              \
        } else {                                                                                                           \
            if (VEC) hipLaunchKernelGGL((KERNEL<4, long long>), dim3(grid_of((A).total >> 2)), dim3(256), 0, ST, A, BOOKS);    \
            else hipLaunchKernelGGL((KERNEL<1, long long>), dim3(grid_of((A).total)), dim3(256), 0, ST, A, BOOKS);             \
        }                                                                                                                  \
    } while (0)

}  // namespace vqvae

using namespace vqvae;

extern "C" {

size_t vqvae_vq_grouped_workspace_bytes(int64_t N, int K, int D, int G) {
    GrpPlan p;
    return grp_plan(N, K, D, G, p) ? p.total : 0;
}

int vqvae_vq_grouped_forward_f32(const float *z_e, const float *const *codebooks, int64_t B, int D, int H, int W, int K, int G,
                                 float beta, int flags, float *z_q, int64_t *idx, int32_t *hist, float *loss_group,
                                 float *perplexity_group, float *loss, float *slabs_out, void *workspace, size_t workspace_bytes,
                                 vqvae_stream_t stream) {
    if (!z_e || !codebooks || !idx || !hist || !loss_group || !perplexity_group || !loss) return VQVAE_ERR_NULL;
    long long HW = 0, N = 0;
    const int rc0 = grp_check(B, D, H, W, K, G, HW, N);
    if (rc0 != VQVAE_OK) return rc0;
    if (flags & ~kGrpForwardFlags) return VQVAE_ERR_UNSUPPORTED;
    GrpBooks books;
    const int rcb = grp_books(codebooks, G, books);
    if (rcb != VQVAE_OK) return rcb;
    GrpPlan p;
    if (!grp_plan(N, K, D, G, p)) return VQVAE_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < p.total) return VQVAE_ERR_WORKSPACE;
    // the per-group quantizer reads a codebook sixteen bytes at a time at the fixed slab widths (the slabs themselves lie aligned
    // in the workspace): refused here, before the split kernel, not by the quantizer of some later group
    if (vq_needs_align16(D / G))
        for (int g = 0; g < G; ++g)
            if (reinterpret_cast<uintptr_t>(books.cb[g]) & 15) return VQVAE_ERR_UNSUPPORTED;
    if (reinterpret_cast<uintptr_t>(workspace) & 15) return VQVAE_ERR_UNSUPPORTED;      // (the groups' quantizer workspaces and slabs)
    if (any_misaligned(3, {z_e, z_q, hist, loss_group, perplexity_group, loss, slabs_out}) || any_misaligned(7, {idx, workspace}))
        return VQVAE_ERR_UNSUPPORTED;
    const int d = D / G;
    const size_t map_bytes = (size_t)N * D * sizeof(float), book_bytes = (size_t)K * d * sizeof(float);
    if (grp_any_overlap({GrpSpan{z_q, map_bytes}, GrpSpan{idx, (size_t)G * N * sizeof(int64_t)}, GrpSpan{hist, (size_t)G * K * sizeof(int32_t)},
                         GrpSpan{loss_group, (size_t)G * sizeof(float)}, GrpSpan{perplexity_group, (size_t)G * sizeof(float)},
                         GrpSpan{loss, sizeof(float)}, GrpSpan{slabs_out, map_bytes}, GrpSpan{workspace, p.total}},
                        {GrpSpan{z_e, map_bytes}}, books, nullptr, G, book_bytes))
        return VQVAE_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char *ws = static_cast<char *>(workspace);
    const int rowmajor = (flags & VQVAE_VQ_ROWMAJOR) ? 1 : 0;
    const GrpArgs base = grp_args(reinterpret_cast<const long long *>(idx), N, D, HW, K, G, rowmajor);
    // The quantizers read the caller's slabs where those are 16-byte aligned, as every slab in the workspace is (a slab is a multiple
    // of 16 bytes wherever a layout allows 16-byte accesses); a less aligned slabs_out gets a second copy.
    float *ws_slabs = reinterpret_cast<float *>(ws + p.off_slabs);
    const bool direct = slabs_out && !any_misaligned(15, {slabs_out});
    float *slabs = direct ? slabs_out : ws_slabs;
    grp_launch_split(base, z_e, 0, G, slabs, (slabs_out && !direct) ? slabs_out : nullptr, st);
    for (int g = 0; g < G; ++g) {
        const int rc = vqvae_vq_forward_f32(slabs + (size_t)g * N * d, books.cb[g], B, d, H, W, K, beta, flags, nullptr,
                                            idx + (size_t)g * N, hist + (size_t)g * K, loss_group + g, perplexity_group + g,
                                            ws + (size_t)g * p.vq_bytes, p.vq_bytes, stream);
        // (not reachable for an argument reason: the envelope, the pointers and the workspace of every group were checked above,
        // before the split kernel and the earlier groups were launched; what comes back here is a launch error of the runtime)
        if (rc != VQVAE_OK) return rc;
    }
    GrpArgs a = base;
    a.z = z_e;
    a.out = z_q;
    a.loss_group = loss_group;
    a.loss = loss;
    if (!z_q) a.total = 0;                                                        // index-only: one workgroup, for the loss
    const bool vec = grp_vec4_books(a, books, {z_e, z_q});
    GRP_LAUNCH(grp_finish_kernel, vec, a, books, st);
    return (int)hipGetLastError();
}

int vqvae_vq_grouped_decode_f32(const int64_t *idx, const float *const *codebooks, int64_t B, int D, int H, int W, int K, int G,
                                int flags, float *z_q, vqvae_stream_t stream) {
    if (!idx || !codebooks || !z_q) return VQVAE_ERR_NULL;
    long long HW = 0, N = 0;
    const int rc0 = grp_check(B, D, H, W, K, G, HW, N);
    if (rc0 != VQVAE_OK) return rc0;
    if (flags & ~VQVAE_VQ_ROWMAJOR) return VQVAE_ERR_UNSUPPORTED;
    GrpBooks books;
    const int rcb = grp_books(codebooks, G, books);
    if (rcb != VQVAE_OK) return rcb;
    if (any_misaligned(3, {z_q}) || any_misaligned(7, {idx})) return VQVAE_ERR_UNSUPPORTED;
    if (grp_any_overlap({GrpSpan{z_q, (size_t)N * D * sizeof(float)}}, {GrpSpan{idx, (size_t)G * N * sizeof(int64_t)}}, books, nullptr, G,
                        (size_t)K * (D / G) * sizeof(float)))
        return VQVAE_ERR_UNSUPPORTED;
    GrpArgs a = grp_args(reinterpret_cast<const long long *>(idx), N, D, HW, K, G, (flags & VQVAE_VQ_ROWMAJOR) ? 1 : 0);
    a.out = z_q;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool vec = grp_vec4_books(a, books, {z_q});
    GRP_LAUNCH(grp_finish_kernel, vec, a, books, st);
    return (int)hipGetLastError();
}

size_t vqvae_vq_grouped_backward_workspace_bytes(int64_t N, int K, int D, int G) {
    GrpBwdPlan p;
    return grp_bwd_plan(N, K, D, G, p) ? p.total : 0;
}

int vqvae_vq_grouped_backward_f32(const float *z_e, const float *const *codebooks, const int64_t *idx, const float *grad_zq,
                                  const float *grad_loss, int64_t B, int D, int H, int W, int K, int G, float beta, int flags,
                                  float *grad_z, float *const *grad_codebooks, void *workspace, size_t workspace_bytes,
                                  vqvae_stream_t stream) {
    const bool commitment = (flags & VQVAE_VQ_BWD_COMMITMENT) != 0;
    if (!z_e || !codebooks || !idx || (!grad_z && !grad_codebooks) || (commitment && !grad_z)) return VQVAE_ERR_NULL;
    long long HW = 0, N = 0;
    const int rc0 = grp_check(B, D, H, W, K, G, HW, N);
    if (rc0 != VQVAE_OK) return rc0;
    if ((flags & ~(VQVAE_VQ_ROWMAJOR | VQVAE_VQ_BWD_COMMITMENT)) || (commitment && grad_codebooks)) return VQVAE_ERR_UNSUPPORTED;
    GrpBooks books;
    const int rcb = grp_books(codebooks, G, books);
    if (rcb != VQVAE_OK) return rcb;
    if (grad_codebooks)
        for (int g = 0; g < G; ++g) {
            if (!grad_codebooks[g]) return VQVAE_ERR_NULL;
            if (reinterpret_cast<uintptr_t>(grad_codebooks[g]) & 3) return VQVAE_ERR_UNSUPPORTED;
        }
    GrpBwdPlan p;
    if (!grp_bwd_plan(N, K, D, G, p)) return VQVAE_ERR_UNSUPPORTED;
    if (grad_codebooks && (!workspace || workspace_bytes < p.total)) return VQVAE_ERR_WORKSPACE;
    if (any_misaligned(3, {z_e, grad_zq, grad_loss, grad_z}) || any_misaligned(7, {idx, grad_codebooks ? workspace : nullptr}))
        return VQVAE_ERR_UNSUPPORTED;
    const int d = D / G;
    const size_t map_bytes = (size_t)N * D * sizeof(float);
    if (grp_any_overlap({GrpSpan{grad_z, map_bytes}, GrpSpan{grad_codebooks ? workspace : nullptr, p.total}},
                        {GrpSpan{z_e, map_bytes}, GrpSpan{idx, (size_t)G * N * sizeof(int64_t)}, GrpSpan{grad_zq, map_bytes},
                         GrpSpan{grad_loss, sizeof(float)}},
                        books, grad_codebooks, G, (size_t)K * d * sizeof(float)))
        return VQVAE_ERR_UNSUPPORTED;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rowmajor = (flags & VQVAE_VQ_ROWMAJOR) ? 1 : 0;
    const long long *idx_ll = reinterpret_cast<const long long *>(idx);
    const GrpArgs base = grp_args(idx_ll, N, D, HW, K, G, rowmajor);
    const double nd = (double)N * (double)d;                                      // a group's loss is a mean over N d elements
    if (grad_z) {
        GrpArgs a = base;
        a.z = z_e;
        a.out = grad_z;
        a.g_zq = grad_zq;
        a.g_loss = grad_loss;
        a.scale = commitment ? (float)(2.0 * (double)beta / nd) : (float)(2.0 / nd);
        const bool vec = grp_vec4_books(a, books, {z_e, grad_zq, grad_z});
        GRP_LAUNCH(grp_gradz_kernel, vec, a, books, st);
    }
    if (grad_codebooks) {
        char *ws = static_cast<char *>(workspace);
        float *slab = reinterpret_cast<float *>(ws + p.off_slab);
        const int *offsets = reinterpret_cast<const int *>(ws + p.seg.off_offsets);
        const int *unit_start = reinterpret_cast<const int *>(ws + p.seg.off_units);
        const double *partial = reinterpret_cast<const double *>(ws + p.seg.off_partials);
        for (int g = 0; g < G; ++g) {
            grp_launch_split(base, z_e, g, g + 1, slab, nullptr, st);
            const hipError_t e = launch_segsum(p.seg, slab, idx_ll + (size_t)g * N, N, K, d, (int)HW, rowmajor, ws, st);
            if (e != hipSuccess) return (int)e;
            hipLaunchKernelGGL(grp_codebook_grad_kernel, dim3((unsigned)(((long long)K * d + 255) / 256)), dim3(256), 0, st,
                               books.cb[g], offsets, unit_start, partial, grad_loss, K, d, G, 2.0 * (double)beta / nd,
                               grad_codebooks[g]);
        }
    }
    return (int)hipGetLastError();
}

}  // extern "C"
