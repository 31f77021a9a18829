// Residual vector quantization (gfx950): Q codebooks quantize the same latent position, each stage what the stage before it left
// over (RQ-VAE, arXiv 2203.01941; SoundStream's RVQ).
//   vqvae_vq_residual_workspace_bytes            host only
//   vqvae_vq_residual_forward_f32                Q x vqvae_vq_forward_f32 (z_q = NULL: indices, histogram, loss, perplexity of the
//                                                stage), Q - 1 x rvq_advance_kernel between them, 1 x rvq_finish_kernel
//   vqvae_vq_residual_decode_f32                 rvq_finish_kernel without z: indices -> the sum of their code rows
//   vqvae_vq_residual_backward_workspace_bytes   host only
//   vqvae_vq_residual_backward_f32               rvq_gradz_kernel; per stage rvq_advance_kernel (r_q again), the shared sorted
//                                                segmented sum (launch_segsum, train_reduce.h) and rvq_codebook_grad_kernel
// Every launch is on the caller's stream, one after the other: a forward captures into a graph as one linear chain.  No host sync,
// no allocation, no floating-point atomics; the same bits in every run and in either layout.
//
// THE OPERATION ORDER IS THE CONTRACT (tests/rvq_ref.py restates it on the CPU; the library is compiled with -ffp-contract=off, so
// every subtraction, addition and multiplication below is one IEEE operation in the stated precision).  1 <= Q <= 16 stages, codebooks
// E_0 .. E_{Q-1}, each (K, D) fp32; with VQVAE_VQ_RESIDUAL_SHARED every stage uses E_0.  Rows and layouts are those of
// vqvae_vq_forward_f32: N = B H W rows, NCHW maps or, with VQVAE_VQ_ROWMAJOR, (N, D) rows.
//
//   r_0 = z
//   stage q:  idx_q = the reference quantizer's argmin of the rows of r_q against E_q (models/quantizer.py:49-54: exactly what
//                     vqvae_vq_forward_f32 returns for those bits, first-index ties and NaN-as-minimum included)
//             e_q   = E_q[idx_q]                    the row's bits, gathered
//             loss_q, perplexity_q, hist_q = vqvae_vq_forward_f32's own outputs for (r_q, E_q, beta)
//             r_{q+1} = r_q - e_q                   one fp32 subtraction per element
//   S    = ((e_0 + e_1) + e_2) + ...                fp32, stage order, starting from e_0 itself
//   z_q  = z + (S - z)                              the straight-through value, as quantizer.py:67 (decode: z_q = S)
//   loss = ((loss_0 + loss_1) + ...)                fp32, stage order, starting from loss_0 itself, on the device
// ||r_q - e_q||^2 = ||z - sum_{i<=q} e_i||^2: the stage losses are RQ-VAE's partial-sum commitment terms, beta where the reference
// puts it.  With Q = 1 every output has the bits of vqvae_vq_forward_f32.  An index outside [0, K) (decode, backward: indices that
// are not the forward's own) never reads a codebook: its e_q is NaN.
//
// Gradients: what autograd derives when every stage is the reference quantizer and r_{q+1} = r_q - e_q.detach().  g = the
// upstream gradient of loss (a device scalar, NULL = 1), s = fp32(2 / (N D)) rounded once from fp64:
//   gs      = g * s                                 fp32
//   r_{q+1} = r_q - e_q                             the forward's chain again, in registers (r_q - e_q IS r_{q+1})
//   A       = ((r_1 + r_2) + ...) + r_Q             fp32, stage order, starting from r_1 itself
//   grad_z  = grad_zq + gs * A                      (gs * A alone when grad_zq is NULL)
//   grad_E_q[k][c] = fp32(double(g) * (2 beta / (N D)) * (cnt_k * double(E_q[k][c]) - sum_{i: idx_q,i = k} double(r_q,i[c])))
//                    the sum from the segmented sum's units as vqvae_vq_backward_f32 combines them (four interleaved running sums
//                    over a code's units, then (s0 + s1) + (s2 + s3)), on r_q re-materialised by the advance kernel.
//   shared: grad_E_0 = ((G_0 + G_1) + ...) of those fp32 stage results, fp32, stage order.
//
// The element-wise kernels take their code rows from the codebooks through L2 (K D 4 bytes, 128 KiB at the flagship shape, read by
// every workgroup): z and the indices are the only HBM streams.  Row-major rows with D % 4 == 0, and NCHW maps with H W % 4 == 0,
// move 16 bytes per access of z when every tensor is 16-byte aligned; anything else goes element by element.  On row-major rows
// the code row is read 16 bytes at a time too; on NCHW maps every lane gathers E[k][c] for its own k -- a cache line per lane and
// stage, so that layout is bound by L2 and the address path, not by HBM.
#include <initializer_list>

#include "train_reduce.h"
#include "vq_residual.h"

namespace vqvae {

// the three element-wise kernels: their bodies are vq_residual.h's
template <int V>
__global__ __launch_bounds__(256) void rvq_advance_kernel(RvqArgs a, RvqBooks books) { rvq_advance_body<V>(a, books); }
template <int V>
__global__ __launch_bounds__(256) void rvq_finish_kernel(RvqArgs a, RvqBooks books) { rvq_finish_body<V>(a, books); }
template <int V>
__global__ __launch_bounds__(256) void rvq_gradz_kernel(RvqArgs a, RvqBooks books) { rvq_gradz_body<V>(a, books); }

// vqb_codebook_grad_kernel's arithmetic (train.hip) for one stage, the code's units combined by the shared segsum_key_sum;
// accumulate: the shared codebook's later stages add their fp32 result to what the earlier ones left.
__global__ __launch_bounds__(256) void rvq_codebook_grad_kernel(const float *__restrict__ cb, const int *__restrict__ offsets,
                                                                const int *__restrict__ unit_start,
                                                                const double *__restrict__ partial,
                                                                const float *__restrict__ g_loss, int K, int D, double scale,
                                                                int accumulate, float *__restrict__ grad_cb) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)K * D) return;
    const int k = (int)(e / D), c = (int)(e - (long long)k * D);
    const double zsum = segsum_key_sum(unit_start, partial, k, c, D);
    const double cnt = (double)(offsets[k + 1] - offsets[k]);
    const double gl = g_loss ? (double)g_loss[0] : 1.0;
    const float v = (float)(gl * scale * (cnt * (double)cb[e] - zsum));
    grad_cb[e] = accumulate ? grad_cb[e] + v : v;
}

// ---- host side -----------------------------------------------------------------------------------------------------------------

constexpr int kRvqForwardFlags = VQVAE_VQ_ROWMAJOR | VQVAE_VQ_CODEBOOK_PREPARED | VQVAE_VQ_EXACT_SWEEP | VQVAE_VQ_BF16_FILTER |
                                 VQVAE_VQ_UNITS64_8WAVES | VQVAE_VQ_UNITS32_16WAVES | VQVAE_VQ_UNITS32_8WAVES | VQVAE_VQ_RESIDUAL_SHARED;

struct RvqPlan {
    int nbooks;                           // prepared codebook images: Q, or 1 when shared
    size_t vq_bytes, off_res, res_bytes, total;
};

// false: outside the envelope
static bool rvq_plan(long long N, int K, int D, int Q, int shared, RvqPlan &p) {
    if (N < 1 || N > INT32_MAX || K < 1 || K > 16384 || D < 1 || D > 256 || Q < 1 || Q > kRvqMaxStages) return false;
    const size_t one = vqvae_vq_workspace_bytes(N, K, D);
    if (one == 0) return false;
    p.nbooks = shared ? 1 : Q;
    p.vq_bytes = align_up(one, 256);
    p.off_res = p.vq_bytes * (size_t)p.nbooks;
    p.res_bytes = Q > 1 ? align_up((size_t)N * D * sizeof(float), 256) : 0;       // r_q, q >= 1 (one stage needs none)
    p.total = p.off_res + p.res_bytes;
    return true;
}

struct RvqBwdPlan {
    SegsumPlan seg;
    size_t off_res, total;
};

static bool rvq_bwd_plan(long long N, int K, int D, int Q, RvqBwdPlan &p) {
    if (N < 1 || N > INT32_MAX || K < 1 || K > 16384 || D < 1 || D > 256 || Q < 1 || Q > kRvqMaxStages) return false;
    p.seg = segsum_plan(N, K, D);
    p.off_res = align_up(p.seg.total, 256);
    p.total = p.off_res + (Q > 1 ? align_up((size_t)N * D * sizeof(float), 256) : 0);
    return true;
}

// shared argument checks: 0, or the error; HW and N on success
static int rvq_check(int64_t B, int D, int H, int W, int K, int Q, long long &HW, long long &N) {
    if (B < 1 || H < 1 || W < 1) return VQVAE_ERR_SHAPE;
    if (D < 1 || D > 256 || K < 1 || K > 16384 || Q < 1 || Q > kRvqMaxStages) return VQVAE_ERR_UNSUPPORTED;
    HW = (long long)H * W;
    if (B > INT32_MAX || HW > INT32_MAX) return VQVAE_ERR_UNSUPPORTED;
    N = (long long)B * HW;
    if (N > INT32_MAX) return VQVAE_ERR_UNSUPPORTED;
    return VQVAE_OK;
}

// may this launch move 16 bytes per access?  `ptrs`: every tensor the kernel touches with such an access, codebooks included
static bool rvq_vec4(const RvqArgs &a, const RvqBooks &books, std::initializer_list<const void *> ptrs) {
    if (any_misaligned(15, ptrs)) return false;
    if (!a.rowmajor) return (a.HW & 3) == 0;                                      // (the codebooks are read element by element)
    if (a.D & 3) return false;
    for (int q = a.q0; q < a.q1; ++q)
        if (reinterpret_cast<uintptr_t>(books.cb[q]) & 15) return false;
    return true;
}

#define RVQ_LAUNCH(KERNEL, VEC, A, BOOKS, ST)                                                                              \
    do {                                                                                                                   \
        if (VEC) hipLaunchKernelGGL(KERNEL<4>, dim3(grid_of((A).total >> 2)), dim3(256), 0, ST, A, BOOKS);                 \
        else hipLaunchKernelGGL(KERNEL<1>, dim3(grid_of((A).total)), dim3(256), 0, ST, A, BOOKS);                          \
    } while (0)

static RvqArgs rvq_args(const long long *idx, long long N, int D, long long HW, int K, int Q, int rowmajor) {
    RvqArgs a = {};
    a.idx = idx;
    a.N = N;
    a.total = N * D;
    a.D = D;
    a.HW = (int)HW;
    a.K = K;
    a.rowmajor = rowmajor;
    a.Q = Q;
    return a;
}

// r_{q+1} = r_q - E_q[idx_q] into res (from src: z for stage 0, res itself afterwards)
static void rvq_launch_advance(RvqArgs a, const RvqBooks &books, int q, const float *src, float *res, hipStream_t st) {
    a.z = src;
    a.out = res;
    a.q0 = q;
    a.q1 = q + 1;
    const bool vec = rvq_vec4(a, books, {src, res});
    RVQ_LAUNCH(rvq_advance_kernel, vec, a, books, st);
}

static bool rvq_books(const float *const *codebooks, int Q, int shared, RvqBooks &books) {
    if (!codebooks) return false;
    for (int q = 0; q < kRvqMaxStages; ++q) books.cb[q] = nullptr;
    for (int q = 0; q < Q; ++q) {
        books.cb[q] = codebooks[shared ? 0 : q];
        if (!books.cb[q]) return false;
    }
    return true;
}

}  // namespace vqvae

using namespace vqvae;

extern "C" {

size_t vqvae_vq_residual_workspace_bytes(int64_t N, int K, int D, int Q, int shared) {
    RvqPlan p;
    return rvq_plan(N, K, D, Q, shared, p) ? p.total : 0;
}

int vqvae_vq_residual_forward_f32(const float *z_e, const float *const *codebooks, int64_t B, int D, int H, int W, int K, int Q,
                                  float beta, int flags, float *z_q, int64_t *idx, int32_t *hist, float *loss_stage,
                                  float *perplexity_stage, float *loss, float *residual_out, void *workspace, size_t workspace_bytes,
                                  vqvae_stream_t stream) {
    if (!z_e || !codebooks || !idx || !hist || !loss_stage || !perplexity_stage || !loss) return VQVAE_ERR_NULL;
    long long HW = 0, N = 0;
    const int rc0 = rvq_check(B, D, H, W, K, Q, HW, N);
    if (rc0 != VQVAE_OK) return rc0;
    if (flags & ~kRvqForwardFlags) return VQVAE_ERR_UNSUPPORTED;
    const int shared = (flags & VQVAE_VQ_RESIDUAL_SHARED) ? 1 : 0;
    RvqBooks books;
    if (!rvq_books(codebooks, Q, shared, books)) return VQVAE_ERR_NULL;
    RvqPlan p;
    if (!rvq_plan(N, K, D, Q, shared, p)) return VQVAE_ERR_UNSUPPORTED;
    // what the per-stage quantizer would refuse (16-byte accesses on z_e and the codebooks at the fixed widths), before stage 0 runs
    if (vq_needs_align16(D)) {
        if (any_misaligned(15, {z_e})) return VQVAE_ERR_UNSUPPORTED;
        for (int q = 0; q < Q; ++q)
            if (any_misaligned(15, {books.cb[q]})) return VQVAE_ERR_UNSUPPORTED;
    }
    if ((reinterpret_cast<uintptr_t>(idx) & 7) || (reinterpret_cast<uintptr_t>(workspace) & 15)) return VQVAE_ERR_UNSUPPORTED;
    if (!workspace || workspace_bytes < p.total) return VQVAE_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char *ws = static_cast<char *>(workspace);
    float *res = reinterpret_cast<float *>(ws + p.off_res);
    const int rowmajor = (flags & VQVAE_VQ_ROWMAJOR) ? 1 : 0;
    const int qflags = flags & ~(VQVAE_VQ_RESIDUAL_SHARED | VQVAE_VQ_CODEBOOK_PREPARED);
    const RvqArgs base = rvq_args(reinterpret_cast<const long long *>(idx), N, D, HW, K, Q, rowmajor);
    for (int q = 0; q < Q; ++q) {
        const float *src = q == 0 ? z_e : res;
        // a shared codebook's image is prepared by stage 0 and stands for the later stages
        const int prepared = ((flags & VQVAE_VQ_CODEBOOK_PREPARED) || (shared && q > 0)) ? VQVAE_VQ_CODEBOOK_PREPARED : 0;
        const int rc = vqvae_vq_forward_f32(src, books.cb[q], B, D, H, W, K, beta, qflags | prepared, nullptr, idx + (size_t)q * N,
                                            hist + (size_t)q * K, loss_stage + q, perplexity_stage + q,
                                            ws + (size_t)(shared ? 0 : q) * p.vq_bytes, p.vq_bytes, stream);
        if (rc != VQVAE_OK) return rc;
        if (q + 1 < Q) rvq_launch_advance(base, books, q, src, res, st);
    }
    RvqArgs a = base;
    a.z = z_e;
    a.q0 = 0;
    a.q1 = Q;
    a.out = z_q;
    a.out_r = residual_out;
    a.loss_stage = loss_stage;
    a.loss = loss;
    if (!z_q && !residual_out) a.total = 0;                                      // index-only: one workgroup, for the loss
    const bool vec = rvq_vec4(a, books, {z_e, z_q, residual_out});
    RVQ_LAUNCH(rvq_finish_kernel, vec, a, books, st);
    return (int)hipGetLastError();
}

int vqvae_vq_residual_decode_f32(const int64_t *idx, const float *const *codebooks, int64_t B, int D, int H, int W, int K, int Q,
                                 int flags, float *z_q, vqvae_stream_t stream) {
    if (!idx || !codebooks || !z_q) return VQVAE_ERR_NULL;
    long long HW = 0, N = 0;
    const int rc0 = rvq_check(B, D, H, W, K, Q, HW, N);
    if (rc0 != VQVAE_OK) return rc0;
    if (flags & ~(VQVAE_VQ_ROWMAJOR | VQVAE_VQ_RESIDUAL_SHARED)) return VQVAE_ERR_UNSUPPORTED;
    RvqBooks books;
    if (!rvq_books(codebooks, Q, (flags & VQVAE_VQ_RESIDUAL_SHARED) ? 1 : 0, books)) return VQVAE_ERR_NULL;
    RvqArgs a = rvq_args(reinterpret_cast<const long long *>(idx), N, D, HW, K, Q, (flags & VQVAE_VQ_ROWMAJOR) ? 1 : 0);
    a.q0 = 0;
    a.q1 = Q;
    a.out = z_q;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool vec = rvq_vec4(a, books, {z_q});
    RVQ_LAUNCH(rvq_finish_kernel, vec, a, books, st);
    return (int)hipGetLastError();
}

size_t vqvae_vq_residual_backward_workspace_bytes(int64_t N, int K, int D, int Q) {
    RvqBwdPlan p;
    return rvq_bwd_plan(N, K, D, Q, p) ? p.total : 0;
}

int vqvae_vq_residual_backward_f32(const float *z_e, const float *const *codebooks, const int64_t *idx, const float *grad_zq,
                                   const float *grad_loss, int64_t B, int D, int H, int W, int K, int Q, float beta, int flags,
                                   float *grad_z, float *const *grad_codebooks, void *workspace, size_t workspace_bytes,
                                   vqvae_stream_t stream) {
    if (!z_e || !codebooks || !idx || (!grad_z && !grad_codebooks)) return VQVAE_ERR_NULL;
    long long HW = 0, N = 0;
    const int rc0 = rvq_check(B, D, H, W, K, Q, HW, N);
    if (rc0 != VQVAE_OK) return rc0;
    if (flags & ~(VQVAE_VQ_ROWMAJOR | VQVAE_VQ_RESIDUAL_SHARED)) return VQVAE_ERR_UNSUPPORTED;
    const int shared = (flags & VQVAE_VQ_RESIDUAL_SHARED) ? 1 : 0;
    RvqBooks books;
    if (!rvq_books(codebooks, Q, shared, books)) return VQVAE_ERR_NULL;
    if (grad_codebooks)
        for (int q = 0; q < (shared ? 1 : Q); ++q)
            if (!grad_codebooks[q]) return VQVAE_ERR_NULL;
    RvqBwdPlan p;
    if (!rvq_bwd_plan(N, K, D, Q, p)) return VQVAE_ERR_UNSUPPORTED;
    if (grad_codebooks && (!workspace || workspace_bytes < p.total)) return VQVAE_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int rowmajor = (flags & VQVAE_VQ_ROWMAJOR) ? 1 : 0;
    const long long *idx_ll = reinterpret_cast<const long long *>(idx);
    const RvqArgs base = rvq_args(idx_ll, N, D, HW, K, Q, rowmajor);
    const double nd = (double)N * (double)D;
    if (grad_z) {
        RvqArgs a = base;
        a.z = z_e;
        a.q0 = 0;
        a.q1 = Q;
        a.out = grad_z;
        a.g_zq = grad_zq;
        a.g_loss = grad_loss;
        a.scale = (float)(2.0 / nd);
        const bool vec = rvq_vec4(a, books, {z_e, grad_zq, grad_z});
        RVQ_LAUNCH(rvq_gradz_kernel, vec, a, books, st);
    }
    if (grad_codebooks) {
        char *ws = static_cast<char *>(workspace);
        float *res = reinterpret_cast<float *>(ws + p.off_res);
        const int *offsets = reinterpret_cast<const int *>(ws + p.seg.off_offsets);
        const int *unit_start = reinterpret_cast<const int *>(ws + p.seg.off_units);
        const double *partial = reinterpret_cast<const double *>(ws + p.seg.off_partials);
        for (int q = 0; q < Q; ++q) {
            if (q > 0) rvq_launch_advance(base, books, q - 1, q == 1 ? z_e : res, res, st);
            const float *src = q == 0 ? z_e : res;
            const hipError_t e = launch_segsum(p.seg, src, idx_ll + (size_t)q * N, N, K, D, (int)HW, rowmajor, ws, st);
            if (e != hipSuccess) return (int)e;
            hipLaunchKernelGGL(rvq_codebook_grad_kernel, dim3((unsigned)(((long long)K * D + 255) / 256)), dim3(256), 0, st,
                               books.cb[q], offsets, unit_start, partial, grad_loss, K, D, 2.0 * (double)beta / nd,
                               (shared && q > 0) ? 1 : 0, grad_codebooks[shared ? 0 : q]);
        }
    }
    return (int)hipGetLastError();
}

}  // extern "C"
