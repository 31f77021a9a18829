// Fused multi-tensor Adam / AMSGrad / AdamW step and the global gradient norm (gfx950): torch.optim.Adam.step() of main.py:59,80 and
// pixelcnn/gated_pixelcnn.py:78-99 over EVERY tensor of the optimizer in one launch.
//   vqvae_adam_plan_bytes / vqvae_adam_plan_write   host only: the plan blob (tensor table, chunk list, per-tensor scratch)
//   vqvae_adam_step_f32                             adam_prologue_kernel (one workgroup) + adam_update_kernel (one workgroup per chunk)
//   vqvae_grad_norm_workspace_bytes / vqvae_grad_norm_f32   grad_sq_partial_kernel (per chunk) + grad_norm_final_kernel (one workgroup)
//
// THE OPERATION ORDER IS THE CONTRACT.  Per element the step is evaluated in fp64 from the fp32 inputs (conversions exact), every
// operation one IEEE fp64 operation in the order written (the library is compiled with -ffp-contract=off: nothing is fused), and each
// of the three or four results is rounded to fp32 ONCE:
//     g1 = g * clip_coef                               only with a clip_coef pointer (an fp32 device scalar); else g1 = g
//     g1 = g1 + wd * p                                 coupled weight decay, wd != 0 (torch.optim.Adam)
//     m' = fp32(m + (1 - beta1) * (g1 - m))
//     v' = fp32(beta2 * v + ((1 - beta2) * g1) * g1)
//     vmax' = v' > vmax or v' is NaN ? v' : vmax       amsgrad (torch.maximum: NaN propagates); d = vmax', else d = v'
//     denom = sqrt(d) / sqrt(1 - beta2^t) + eps        from the STORED fp32 m', d: the new parameter is a function of the new state
//     q = (lr / (1 - beta1^t)) * (m' / denom)
//     p' = fp32(p - q)
//     p' = fp32(p * (1 - lr * wd) - q)                 instead, with decoupled weight decay, wd != 0 (AdamW)
// Why fp64: evaluated in fp32, as torch's CPU Adam does, the rounding errors of m' scale with
// max(|m|, |g1|), and where the two nearly cancel (g1 ~ -9 m at beta1 = 0.9) no bound relative to the step |p' - p| holds -- several
// times a bound of 2^-21 |p' - p| + 2^-23 |p'| on a few of 70 001 elements (tests/test_optim_cpu.py prints torch's figure); likewise
// g + wd * p where those cancel.  The kernel moves
// 40 bytes per element and is launch-bound; the fp64 arithmetic is not what it waits for.
// t is the tensor's counter AFTER this step's increment.  Inf and NaN get no special handling: they propagate as the expressions say.
// An element's result depends on nothing but its own inputs and its tensor's scalars -- not on the chunk it falls into, on the alignment
// path or on the other tensors -- so any partition of the same data into tensors gives the same bits.  (The same bits for one build
// of the library: beta^t comes from the device library's fp64 pow, which another ROCm release may round differently in the last place.)
//
// Counters live on the device, one fp32 scalar per tensor (the layout of torch's capturable / fused Adam state).  Only the prologue
// reads and writes them: it advances the counter of every tensor that has a gradient and leaves that tensor's scalars in the plan's
// scratch, which is all the update kernel reads.  No workgroup reads a counter another workgroup of the same launch writes; nothing
// here synchronises or reads device memory from the host, so a step captures into a hipGraph as a plain chain of two kernels.
#include <math.h>
#include <string.h>

#include "common.h"

namespace vqvae {

constexpr int kAdamChunk = VQVAE_ADAM_CHUNK;            // elements per workgroup: 256 lanes x four 16-byte vectors
constexpr long long kAdamMagic = 0x31304d4144415156LL;  // "VQADAM01"
static_assert(kAdamChunk == 256 * 4 * 4, "adam_update_kernel's full-chunk path keeps four 16-byte loads in flight per lane and array");

// the blob's layout (include/vqvae_hip.h describes it for callers that inspect a host plan)
struct AdamHeader { long long magic, n_tensors, n_chunks, chunk, off_tensors, off_chunks, off_scratch, total; };
struct AdamTensor { float *p, *g, *m, *v, *vmax, *step; long long numel; int group, pad; };
struct AdamChunkRef { int tensor, index; };               // elements [index * chunk, min(numel, (index + 1) * chunk)) of the tensor
struct AdamScalars { double step_size, bc2_sqrt, omb1, b2, omb2, eps, wd, decay; int flags, pad[3]; };
static_assert(sizeof(AdamHeader) == 64 && sizeof(AdamTensor) == 64 && sizeof(AdamChunkRef) == 8 && sizeof(AdamScalars) == 80, "plan layout");

struct AdamGroupArgs { double lr[VQVAE_ADAM_MAX_GROUPS], b1[VQVAE_ADAM_MAX_GROUPS], b2[VQVAE_ADAM_MAX_GROUPS];
                       double eps[VQVAE_ADAM_MAX_GROUPS], wd[VQVAE_ADAM_MAX_GROUPS];
                       int flags[VQVAE_ADAM_MAX_GROUPS]; };

static size_t adam_plan_size(long long n_tensors, long long n_chunks, size_t *off_chunks, size_t *off_scratch) {
    const size_t oc = sizeof(AdamHeader) + (size_t)n_tensors * sizeof(AdamTensor);
    const size_t os = align_up(oc + (size_t)n_chunks * sizeof(AdamChunkRef), 16);
    if (off_chunks) *off_chunks = oc;
    if (off_scratch) *off_scratch = os;
    return align_up(os + (size_t)n_tensors * sizeof(AdamScalars), 16);
}

// One workgroup: counters and per-tensor scalars.  A tensor without a gradient keeps its counter and is in no chunk.
__global__ __launch_bounds__(256) void adam_prologue_kernel(char *__restrict__ plan, AdamGroupArgs a) {
    const AdamHeader *hd = reinterpret_cast<const AdamHeader *>(plan);
    const AdamTensor *tens = reinterpret_cast<const AdamTensor *>(plan + hd->off_tensors);
    AdamScalars *sc = reinterpret_cast<AdamScalars *>(plan + hd->off_scratch);
    for (int i = threadIdx.x; i < (int)hd->n_tensors; i += 256) {
        const AdamTensor t = tens[i];
        if (!t.g) continue;
        const float s = *t.step + 1.0f;
        *t.step = s;
        const int gi = t.group;
        const double bc1 = 1.0 - pow(a.b1[gi], (double)s), bc2 = 1.0 - pow(a.b2[gi], (double)s);
        AdamScalars o;
        o.step_size = a.lr[gi] / bc1;
        o.bc2_sqrt = sqrt(bc2);
        o.omb1 = 1.0 - a.b1[gi]; o.b2 = a.b2[gi]; o.omb2 = 1.0 - a.b2[gi]; o.eps = a.eps[gi]; o.wd = a.wd[gi];
        o.decay = 1.0 - a.lr[gi] * a.wd[gi];
        o.flags = a.flags[gi]; o.pad[0] = o.pad[1] = o.pad[2] = 0;
        sc[i] = o;
    }
}

__device__ __forceinline__ void adam_element(float &p, float g, float &m, float &v, float &vmax, bool ams, bool clip, float coef,
                                             const AdamScalars &h) {
    const bool decay = h.wd != 0.0, decoupled = h.flags & VQVAE_ADAM_DECOUPLED_WD;
    double g1 = (double)g;
    if (clip) g1 = g1 * (double)coef;
    if (decay && !decoupled) g1 = g1 + h.wd * (double)p;
    m = (float)((double)m + h.omb1 * (g1 - (double)m));
    v = (float)(h.b2 * (double)v + (h.omb2 * g1) * g1);
    float d = v;
    if (ams) {
        vmax = (v > vmax || v != v) ? v : vmax;
        d = vmax;
    }
    const double denom = sqrt((double)d) / h.bc2_sqrt + h.eps;
    const double q = h.step_size * ((double)m / denom);
    p = (float)(decay && decoupled ? (double)p * h.decay - q : (double)p - q);
}

__device__ __forceinline__ void adam_vec(f32x4 &P, const f32x4 &G, f32x4 &M, f32x4 &V, f32x4 &X, bool ams, bool clip, float coef,
                                         const AdamScalars &h) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float p = P[c], m = M[c], v = V[c], x = X[c];
        adam_element(p, G[c], m, v, x, ams, clip, coef, h);
        P[c] = p; M[c] = m; V[c] = v; X[c] = x;
    }
}

// One workgroup per chunk of one tensor.  16-byte accesses where the tensor's four or five arrays are all 16-byte aligned (a chunk
// starts a multiple of 4096 elements in, so the tensor's alignment is the chunk's); a full chunk issues its sixteen or twenty loads
// per lane before the first use.  Other tensors (views into a flat buffer are only 4-byte aligned) and the last one to three
// elements of an aligned tensor go element by element.  zero: the consumed gradient elements are overwritten with +0.
__global__ __launch_bounds__(256) void adam_update_kernel(const char *__restrict__ plan, int zero, const float *__restrict__ clip_coef) {
    const AdamHeader *hd = reinterpret_cast<const AdamHeader *>(plan);
    if ((long long)blockIdx.x >= hd->n_chunks) return;
    const AdamChunkRef ck = reinterpret_cast<const AdamChunkRef *>(plan + hd->off_chunks)[blockIdx.x];
    const AdamTensor t = reinterpret_cast<const AdamTensor *>(plan + hd->off_tensors)[ck.tensor];
    const AdamScalars h = reinterpret_cast<const AdamScalars *>(plan + hd->off_scratch)[ck.tensor];
    const long long first = (long long)ck.index * kAdamChunk;
    const long long left = t.numel - first;
    if (!t.g || left <= 0) return;
    const int n = left < kAdamChunk ? (int)left : kAdamChunk;
    const bool ams = t.vmax != nullptr, clip = clip_coef != nullptr;
    const float coef = clip ? *clip_coef : 1.0f;
    float *p = t.p + first, *g = t.g + first, *m = t.m + first, *v = t.v + first, *x = ams ? t.vmax + first : nullptr;
    const int tid = threadIdx.x;
    const uintptr_t bits = reinterpret_cast<uintptr_t>(t.p) | reinterpret_cast<uintptr_t>(t.g) | reinterpret_cast<uintptr_t>(t.m) |
                           reinterpret_cast<uintptr_t>(t.v) | reinterpret_cast<uintptr_t>(t.vmax);
    int done = 0;                                             // elements of the chunk the vector path has covered
    if ((bits & 15) == 0) {
        f32x4 *p4 = reinterpret_cast<f32x4 *>(p), *g4 = reinterpret_cast<f32x4 *>(g), *m4 = reinterpret_cast<f32x4 *>(m),
              *v4 = reinterpret_cast<f32x4 *>(v), *x4 = reinterpret_cast<f32x4 *>(x);
        const int nvec = n >> 2;
        const f32x4 z4 = {0.0f, 0.0f, 0.0f, 0.0f};
        if (n == kAdamChunk) {
            f32x4 P[4], G[4], M[4], V[4], X[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int q = tid + 256 * j;
                P[j] = p4[q]; G[j] = g4[q]; M[j] = m4[q]; V[j] = v4[q];
                X[j] = ams ? x4[q] : z4;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int q = tid + 256 * j;
                adam_vec(P[j], G[j], M[j], V[j], X[j], ams, clip, coef, h);
                p4[q] = P[j]; m4[q] = M[j]; v4[q] = V[j];
                if (ams) x4[q] = X[j];
                if (zero) g4[q] = z4;
            }
        } else {
            for (int q = tid; q < nvec; q += 256) {
                f32x4 P = p4[q], G = g4[q], M = m4[q], V = v4[q], X = ams ? x4[q] : z4;
                adam_vec(P, G, M, V, X, ams, clip, coef, h);
                p4[q] = P; m4[q] = M; v4[q] = V;
                if (ams) x4[q] = X;
                if (zero) g4[q] = z4;
            }
        }
        done = nvec << 2;
    }
    for (int e = done + tid; e < n; e += 256) {
        float pe = p[e], me = m[e], ve = v[e], xe = ams ? x[e] : 0.0f;
        adam_element(pe, g[e], me, ve, xe, ams, clip, coef, h);
        p[e] = pe; m[e] = me; v[e] = ve;
        if (ams) x[e] = xe;
        if (zero) g[e] = 0.0f;
    }
}

// partial[chunk] = sum of g * g over the chunk, in fp64: each lane adds its elements in ascending order, then the fixed tree of
// block_sum_f64.  No atomics: the same bits in every run.
__global__ __launch_bounds__(256) void grad_sq_partial_kernel(const char *__restrict__ plan, double *__restrict__ partial) {
    __shared__ double red[256];
    const AdamHeader *hd = reinterpret_cast<const AdamHeader *>(plan);
    if ((long long)blockIdx.x >= hd->n_chunks) return;       // (uniform per workgroup: nobody is left at a barrier)
    const AdamChunkRef ck = reinterpret_cast<const AdamChunkRef *>(plan + hd->off_chunks)[blockIdx.x];
    const AdamTensor t = reinterpret_cast<const AdamTensor *>(plan + hd->off_tensors)[ck.tensor];
    const long long first = (long long)ck.index * kAdamChunk;
    const long long left = t.g ? t.numel - first : 0;
    const int n = left < kAdamChunk ? (left > 0 ? (int)left : 0) : kAdamChunk;
    const float *g = t.g ? t.g + first : nullptr;            // (never read when n == 0)
    const int tid = threadIdx.x;
    double s = 0.0;
    int done = 0;
    if ((reinterpret_cast<uintptr_t>(t.g) & 15) == 0) {
        const f32x4 *g4 = reinterpret_cast<const f32x4 *>(g);
        const int nvec = n >> 2;
        if (n == kAdamChunk) {
            f32x4 G[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) G[j] = g4[tid + 256 * j];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int c = 0; c < 4; ++c) s += (double)G[j][c] * (double)G[j][c];
        } else {
            for (int q = tid; q < nvec; q += 256) {
                const f32x4 G = g4[q];
#pragma unroll
                for (int c = 0; c < 4; ++c) s += (double)G[c] * (double)G[c];
            }
        }
        done = nvec << 2;
    }
    for (int e = done + tid; e < n; e += 256) s += (double)g[e] * (double)g[e];
    block_sum_f64(red, tid, s);
    if (tid == 0) partial[blockIdx.x] = red[0];
}

// One workgroup adds the partials (lane l takes chunks l, l + 256, ... in order, then the fixed tree) and writes
// total_norm = fp32(sqrt(sum)) and clip_coef = min(1, max_norm / (total_norm + 1e-6)) in fp32 (torch.nn.utils.clip_grad_norm_'s
// expression; a NaN stays a NaN as under torch.clamp).
__global__ __launch_bounds__(256) void grad_norm_final_kernel(const double *__restrict__ partial, long long n, float max_norm,
                                                              float *__restrict__ total_norm, float *__restrict__ clip_coef) {
    __shared__ double red[256];
    const int tid = threadIdx.x;
    double s = 0.0;
    for (long long i = tid; i < n; i += 256) s += partial[i];
    block_sum_f64(red, tid, s);
    if (tid == 0) {
        const float tn = (float)sqrt(red[0]);
        *total_norm = tn;
        if (clip_coef) {
            const float c = max_norm / (tn + 1e-6f);
            *clip_coef = c > 1.0f ? 1.0f : c;
        }
    }
}

static int plan_args_check(const void *plan, size_t plan_bytes, int n_tensors, int64_t n_chunks) {
    if (!plan) return VQVAE_ERR_NULL;
    if (n_tensors < 1 || n_chunks < 0) return VQVAE_ERR_SHAPE;
    if (n_chunks > 0x7fffffffLL) return VQVAE_ERR_OVERFLOW;
    if (reinterpret_cast<uintptr_t>(plan) & 15) return VQVAE_ERR_UNSUPPORTED;
    if (plan_bytes < adam_plan_size(n_tensors, n_chunks, nullptr, nullptr)) return VQVAE_ERR_WORKSPACE;
    return VQVAE_OK;
}

}  // namespace vqvae

using namespace vqvae;

extern "C" {

int vqvae_adam_chunk_elems(void) { return kAdamChunk; }

size_t vqvae_adam_plan_bytes(int n_tensors, const int64_t *numel_host) {
    if (n_tensors < 1 || !numel_host) return 0;
    long long chunks = 0;
    for (int i = 0; i < n_tensors; ++i) {
        if (numel_host[i] < 0) return 0;
        chunks += (numel_host[i] + kAdamChunk - 1) / kAdamChunk;
    }
    if (chunks > 0x7fffffffLL) return 0;
    return adam_plan_size(n_tensors, chunks, nullptr, nullptr);
}

int vqvae_adam_plan_write(int n_tensors, const int64_t *numel_host, void *const *param, void *const *grad, void *const *exp_avg,
                          void *const *exp_avg_sq, void *const *max_exp_avg_sq, void *const *step, const int *group, int n_groups,
                          void *plan_host, size_t plan_bytes, int64_t *n_chunks_out) {
    if (!numel_host || !param || !grad || !exp_avg || !exp_avg_sq || !step || !group || !plan_host || !n_chunks_out) return VQVAE_ERR_NULL;
    if (n_tensors < 1 || n_groups < 1) return VQVAE_ERR_SHAPE;
    if (n_groups > VQVAE_ADAM_MAX_GROUPS) return VQVAE_ERR_UNSUPPORTED;
    long long chunks = 0;
    for (int i = 0; i < n_tensors; ++i) {
        if (!param[i] || !exp_avg[i] || !exp_avg_sq[i] || !step[i]) return VQVAE_ERR_NULL;
        if (numel_host[i] < 0 || group[i] < 0 || group[i] >= n_groups) return VQVAE_ERR_SHAPE;
        const uintptr_t bits = reinterpret_cast<uintptr_t>(param[i]) | reinterpret_cast<uintptr_t>(grad[i]) |
                               reinterpret_cast<uintptr_t>(exp_avg[i]) | reinterpret_cast<uintptr_t>(exp_avg_sq[i]) |
                               reinterpret_cast<uintptr_t>(step[i]) |
                               (max_exp_avg_sq ? reinterpret_cast<uintptr_t>(max_exp_avg_sq[i]) : 0);
        if (bits & 3) return VQVAE_ERR_UNSUPPORTED;                                  // fp32 elements
        if (grad[i]) chunks += (numel_host[i] + kAdamChunk - 1) / kAdamChunk;
    }
    if (chunks > 0x7fffffffLL) return VQVAE_ERR_OVERFLOW;
    size_t off_chunks, off_scratch;
    const size_t total = adam_plan_size(n_tensors, chunks, &off_chunks, &off_scratch);
    if (plan_bytes < total) return VQVAE_ERR_WORKSPACE;
    char *blob = static_cast<char *>(plan_host);
    AdamHeader hd = {kAdamMagic, n_tensors, chunks, kAdamChunk, (long long)sizeof(AdamHeader), (long long)off_chunks,
                     (long long)off_scratch, (long long)total};
    memcpy(blob, &hd, sizeof(hd));
    AdamTensor *tens = reinterpret_cast<AdamTensor *>(blob + sizeof(AdamHeader));
    AdamChunkRef *ck = reinterpret_cast<AdamChunkRef *>(blob + off_chunks);
    long long c = 0;
    for (int i = 0; i < n_tensors; ++i) {
        tens[i] = {static_cast<float *>(param[i]), static_cast<float *>(grad[i]), static_cast<float *>(exp_avg[i]),
                   static_cast<float *>(exp_avg_sq[i]), max_exp_avg_sq ? static_cast<float *>(max_exp_avg_sq[i]) : nullptr,
                   static_cast<float *>(step[i]), (long long)numel_host[i], group[i], 0};
        if (!grad[i]) continue;
        const long long nc = (numel_host[i] + kAdamChunk - 1) / kAdamChunk;
        for (long long k = 0; k < nc; ++k) ck[c++] = {i, (int)k};
    }
    memset(blob + off_chunks + (size_t)chunks * sizeof(AdamChunkRef), 0, total - off_chunks - (size_t)chunks * sizeof(AdamChunkRef));
    *n_chunks_out = chunks;
    return VQVAE_OK;
}

int vqvae_adam_step_f32(void *plan_dev, size_t plan_bytes, int n_tensors, int64_t n_chunks, const VqvaeAdamGroup *groups_host,
                        int n_groups, int flags, const float *clip_coef, vqvae_stream_t stream) {
    if (!groups_host) return VQVAE_ERR_NULL;
    if (const int rc = plan_args_check(plan_dev, plan_bytes, n_tensors, n_chunks)) return rc;
    if (n_groups < 1) return VQVAE_ERR_SHAPE;
    if (n_groups > VQVAE_ADAM_MAX_GROUPS || (flags & ~VQVAE_ADAM_ZERO_GRAD)) return VQVAE_ERR_UNSUPPORTED;
    if (reinterpret_cast<uintptr_t>(clip_coef) & 3) return VQVAE_ERR_UNSUPPORTED;
    AdamGroupArgs a = {};
    for (int i = 0; i < n_groups; ++i) {
        const VqvaeAdamGroup &q = groups_host[i];
        if (!(isfinite(q.lr) && q.lr > 0.0) || !(isfinite(q.eps) && q.eps > 0.0)) return VQVAE_ERR_UNSUPPORTED;
        if (!(q.beta1 >= 0.0 && q.beta1 < 1.0) || !(q.beta2 >= 0.0 && q.beta2 < 1.0)) return VQVAE_ERR_UNSUPPORTED;
        if (!(isfinite(q.weight_decay) && q.weight_decay >= 0.0) || (q.flags & ~VQVAE_ADAM_DECOUPLED_WD)) return VQVAE_ERR_UNSUPPORTED;
        a.lr[i] = q.lr; a.b1[i] = q.beta1; a.b2[i] = q.beta2; a.eps[i] = q.eps; a.wd[i] = q.weight_decay; a.flags[i] = q.flags;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(adam_prologue_kernel, dim3(1), dim3(256), 0, st, static_cast<char *>(plan_dev), a);
    if (n_chunks > 0)
        hipLaunchKernelGGL(adam_update_kernel, dim3((unsigned)n_chunks), dim3(256), 0, st, static_cast<const char *>(plan_dev),
                           flags & VQVAE_ADAM_ZERO_GRAD, clip_coef);
    return (int)hipGetLastError();
}

size_t vqvae_grad_norm_workspace_bytes(int64_t n_chunks) {
    if (n_chunks < 0 || n_chunks > 0x7fffffffLL) return 0;
    return align_up((size_t)(n_chunks > 0 ? n_chunks : 1) * sizeof(double), 256);
}

int vqvae_grad_norm_f32(const void *plan_dev, size_t plan_bytes, int n_tensors, int64_t n_chunks, float max_norm,
                        float *total_norm_out, float *clip_coef_out, void *workspace, size_t workspace_bytes, vqvae_stream_t stream) {
    if (!total_norm_out) return VQVAE_ERR_NULL;
    if (const int rc = plan_args_check(plan_dev, plan_bytes, n_tensors, n_chunks)) return rc;
    if (!workspace) return VQVAE_ERR_WORKSPACE;
    if (clip_coef_out && !(max_norm > 0.0f)) return VQVAE_ERR_UNSUPPORTED;
    if ((reinterpret_cast<uintptr_t>(total_norm_out) | reinterpret_cast<uintptr_t>(clip_coef_out)) & 3) return VQVAE_ERR_UNSUPPORTED;
    if (reinterpret_cast<uintptr_t>(workspace) & 7) return VQVAE_ERR_UNSUPPORTED;
    if (workspace_bytes < vqvae_grad_norm_workspace_bytes(n_chunks)) return VQVAE_ERR_WORKSPACE;
    hipStream_t st = static_cast<hipStream_t>(stream);
    double *partial = static_cast<double *>(workspace);
    if (n_chunks > 0)
        hipLaunchKernelGGL(grad_sq_partial_kernel, dim3((unsigned)n_chunks), dim3(256), 0, st, static_cast<const char *>(plan_dev), partial);
    hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(256), 0, st, partial, (long long)n_chunks, max_norm, total_norm_out,
                       clip_coef_out);
    return (int)hipGetLastError();
}

}  // extern "C"
