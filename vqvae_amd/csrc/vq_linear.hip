// The per-row linear map of latent rows (gfx950): y = W x + b on every row, forward and backward, in either layout -- the projections
// of a factorized (low-dimensional) codebook (ViT-VQGAN, arXiv 2110.04627 section 3.2; `codebook_dim` in vector-quantize-pytorch),
// as an entry of its own.
//   vqvae_linear_rows_forward_f32               x -> y
//   vqvae_linear_rows_backward_workspace_bytes
//   vqvae_linear_rows_backward_f32              (x, grad_y) -> grad_x, grad_w, grad_b
// Rows and layouts are vqvae_vq_forward_f32's: N = B H W rows, (B, C, H, W) maps, or (N, C) rows with VQVAE_VQ_ROWMAJOR (the only
// flag).  x and grad_x have Cin channels, y and grad_y Cout channels, in the same layout; w is (Cout, Cin) row-major
// (nn.Linear.weight), b is (Cout).  1 <= Cin, Cout <= 256, 1 <= N <= INT32_MAX.
//
// THE ARITHMETIC IS THE CONTRACT (tests/vq_linear_ref.py restates it on the CPU; it is FSQ's projection, vq_fsq.hip):
//
//   y[n][j]      = float(double(b[j]) + sum_c double(w[j][c]) double(x[n][c]))      fp64, from b[j], c ascending, one rounding
//   grad_x[n][c] = float(sum_j double(w[j][c]) double(grad_y[n][j]))                fp64, from 0.0, j ascending, one rounding
//   grad_w[j][c] = float(sum_n double(grad_y[n][j]) double(x[n][c]))
//   grad_b[j]    = float(sum_n double(grad_y[n][j]))
//
// THE ORDER OF THE PARAMETER SUMS depends on N alone: rows are cut into blocks of 256 consecutive rows (the last one ragged); inside
// a block the terms are added in fp64 one row after the other, in ascending row order, starting from 0.0; a second launch adds the
// blocks' partials in ascending block order, starting from 0.0, and rounds once to fp32.  Both layouts and both access paths cut
// the same blocks and add in the same order: every output has the same bits in all of them, in every run and in a graph replay.
// There is no floating-point atomic anywhere.
//
// The product of two fp32 values is exact in fp64 (48 significant bits, exponents far inside fp64's range), so a fused multiply-add
// rounds exactly as the multiplication followed by the addition does: the kernels use v_fma_f64 (__builtin_fma) although the
// library is compiled with -ffp-contract=off.  The ORDER of the additions is the contract: an instruction that accumulates
// internally in another order (a matrix instruction) does not satisfy it.
//
// A non-finite x or grad_y stays in its own row of y / grad_x; the parameter gradients follow IEEE through the stated order.
//
// Mappings (bodies in vq_linear.h): the weights of R = 8 or 16 output channels are converted to fp64 once per workgroup and kept
// in LDS; a lane owns up to four rows and R sums of each in registers (up to 4 R independent chains; every weight is a broadcast
// read that serves the lane's rows); wider outputs are tiled over the OUTPUT channels -- 256 x 256 doubles do not fit LDS, and the
// order over the input channels is fixed.  NCHW maps: four pixels per lane (HW % 4 == 0 and 16-byte aligned maps) or one, every
// channel one coalesced access of the wave.  Row-major rows are staged through an LDS tile as vq_cosine.h's rows are, 256 rows of
// 16 channels per wave, in 16-byte accesses (channels % 4 == 0 and 16-byte aligned pointers) or element by element.  No scratch.
// No host sync, no allocation, no memset: one chain of launches on the caller's stream, capturable.
#include "common.h"
#include "vq_linear.h"

namespace vqvae {

template <int R, int P, int WD>
__global__ __launch_bounds__(kLinBlockRows) void lin_nchw_kernel(LinArgs a) {
    __shared__ double wl[WD];
    lin_nchw_body<R, P>(a, wl);
}

template <int R, int V, int WD>
__global__ __launch_bounds__(64 * kLinRowsWaves) void lin_rows_kernel(LinArgs a) {
    __shared__ __attribute__((aligned(16))) float tiles[kLinRowsWaves * kLinTileFloats];
    __shared__ double wl[WD];
    lin_rows_body<R, V>(a, tiles, wl);
}

template <bool ROWMAJOR, int V>
__global__ __launch_bounds__(kLinBlockRows) void lin_params_kernel(LinParamArgs a) {
    __shared__ __attribute__((aligned(16))) float tiles[kL2Waves * kL2TileFloats];
    __shared__ __attribute__((aligned(16))) float bt[kLinBlockRows * kLinBStride];
    lin_params_body<ROWMAJOR, V>(a, tiles, bt);
}

__global__ __launch_bounds__(kLinBlockRows) void lin_param_finalize_kernel(const double *partials, long long nblocks, int Cin, int Cout,
                                                                           float *grad_w, float *grad_b) {
    lin_param_finalize_body(partials, nblocks, Cin, Cout, grad_w, grad_b);
}

static int lin_partials(int Cin, int Cout) { return Cout * Cin + Cout; }        // lin_partial_count, for the host
static unsigned lin_grid(long long N) { return (unsigned)((N + kLinBlockRows - 1) / kLinBlockRows); }

template <int R>
static void lin_launch(const LinArgs &a, bool rowmajor, hipStream_t st) {
    constexpr int S = kLinWeightsSmall, M = kLinWeightsMax;
    const bool small = a.NI * R <= S;
    const bool aligned = !((reinterpret_cast<uintptr_t>(a.x) | reinterpret_cast<uintptr_t>(a.out)) & 15);
    if (!rowmajor) {
        const dim3 block(kLinBlockRows);
        if ((a.HW & 3) == 0 && aligned) {                                     // four pixels per lane
            const dim3 grid((unsigned)((a.N + 4 * kLinBlockRows - 1) / (4 * kLinBlockRows)));
            if (small) hipLaunchKernelGGL((lin_nchw_kernel<R, 4, S>), grid, block, 0, st, a);
            else hipLaunchKernelGGL((lin_nchw_kernel<R, 4, M>), grid, block, 0, st, a);
        } else {
            const dim3 grid(lin_grid(a.N));
            if (small) hipLaunchKernelGGL((lin_nchw_kernel<R, 1, S>), grid, block, 0, st, a);
            else hipLaunchKernelGGL((lin_nchw_kernel<R, 1, M>), grid, block, 0, st, a);
        }
        return;
    }
    constexpr int rows = kLinRowsWaves * kLinWaveRows;
    const dim3 grid((unsigned)((a.N + rows - 1) / rows)), block(64 * kLinRowsWaves);
    const bool wide = ((a.NI | a.NO) & 3) == 0 && aligned;
    if (wide && small) hipLaunchKernelGGL((lin_rows_kernel<R, 4, S>), grid, block, 0, st, a);
    else if (wide) hipLaunchKernelGGL((lin_rows_kernel<R, 4, M>), grid, block, 0, st, a);
    else if (small) hipLaunchKernelGGL((lin_rows_kernel<R, 1, S>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((lin_rows_kernel<R, 1, M>), grid, block, 0, st, a);
}

void launch_linear_rows(const LinArgs &a, bool rowmajor, hipStream_t st) {
    if (a.NO <= 8) lin_launch<8>(a, rowmajor, st);
    else lin_launch<16>(a, rowmajor, st);
}

void launch_linear_params(const LinParamArgs &a, bool rowmajor, float *grad_w, float *grad_b, hipStream_t st) {
    const dim3 grid(lin_grid(a.N)), block(kLinBlockRows);
    if (!rowmajor) {
        hipLaunchKernelGGL((lin_params_kernel<false, 1>), grid, block, 0, st, a);
    } else {
        // (the 16-byte copies bring the operand that lies across the lanes: the wider of the two)
        const bool swap = a.Cout > a.Cin;
        const int LA = swap ? a.Cout : a.Cin;
        const bool wide = (LA & 3) == 0 && !(reinterpret_cast<uintptr_t>(swap ? a.g : a.x) & 15);
        if (wide) hipLaunchKernelGGL((lin_params_kernel<true, 4>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((lin_params_kernel<true, 1>), grid, block, 0, st, a);
    }
    const int P = lin_partials(a.Cin, a.Cout);
    hipLaunchKernelGGL(lin_param_finalize_kernel, dim3((unsigned)((P + kLinBlockRows - 1) / kLinBlockRows)), block, 0, st, a.partials,
                       (long long)lin_grid(a.N), a.Cin, a.Cout, grad_w, grad_b);
}

// ---- the entries' checks: the header's codes, before any launch ---------------------------------------------------------------------

// -> N and HW, or the header's code
static int lin_shape(int64_t B, int Cin, int H, int W, int Cout, int flags, long long &N, int &HW) {
    if (B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1) return VQVAE_ERR_SHAPE;
    if (flags & ~VQVAE_VQ_ROWMAJOR) return VQVAE_ERR_UNSUPPORTED;
    if (Cin > 256 || Cout > 256) return VQVAE_ERR_UNSUPPORTED;
    return check_rows_shape(B, H, W, N, HW);
}

static size_t lin_backward_ws(long long N, int Cin, int Cout) {
    return (size_t)lin_grid(N) * (size_t)lin_partials(Cin, Cout) * sizeof(double);
}

}  // namespace vqvae

using namespace vqvae;

extern "C" {

int vqvae_linear_rows_forward_f32(const float *x, const float *w, const float *b, int64_t B, int Cin, int H, int W, int Cout,
                                  int flags, float *y, vqvae_stream_t stream) {
    if (!x || !w || !b || !y) return VQVAE_ERR_NULL;
    LinArgs a = {};
    int rc = lin_shape(B, Cin, H, W, Cout, flags, a.N, a.HW);
    if (rc != VQVAE_OK) return rc;
    const Span in[] = {{x, (size_t)a.N * Cin * 4, 4}, {w, (size_t)Cout * Cin * 4, 4}, {b, (size_t)Cout * 4, 4}};
    const Span out[] = {{y, (size_t)a.N * Cout * 4, 4}};
    if ((rc = check_pointers(in, 3, out, 1)) != VQVAE_OK) return rc;
    a.x = x; a.w = w; a.b = b; a.out = y;
    a.NI = Cin; a.NO = Cout; a.ws_o = Cin; a.ws_i = 1;
    launch_linear_rows(a, (flags & VQVAE_VQ_ROWMAJOR) != 0, static_cast<hipStream_t>(stream));
    return (int)hipGetLastError();
}

size_t vqvae_linear_rows_backward_workspace_bytes(int64_t N, int Cin, int Cout) {
    if (N < 1 || N > INT32_MAX || Cin < 1 || Cin > 256 || Cout < 1 || Cout > 256) return 0;
    return lin_backward_ws(N, Cin, Cout);
}

int vqvae_linear_rows_backward_f32(const float *x, const float *grad_y, const float *w, int64_t B, int Cin, int H, int W, int Cout,
                                   int flags, float *grad_x, float *grad_w, float *grad_b, void *workspace, size_t workspace_bytes,
                                   vqvae_stream_t stream) {
    const bool params = grad_w || grad_b;
    if (!x || !grad_y || !w || (!grad_x && !params)) return VQVAE_ERR_NULL;
    long long N;
    int HW;
    int rc = lin_shape(B, Cin, H, W, Cout, flags, N, HW);
    if (rc != VQVAE_OK) return rc;
    const size_t need = params ? lin_backward_ws(N, Cin, Cout) : 0;
    const Span in[] = {{x, (size_t)N * Cin * 4, 4}, {grad_y, (size_t)N * Cout * 4, 4}, {w, (size_t)Cout * Cin * 4, 4}};
    const Span out[] = {{grad_x, (size_t)N * Cin * 4, 4}, {grad_w, (size_t)Cout * Cin * 4, 4}, {grad_b, (size_t)Cout * 4, 4},
                           {params ? workspace : nullptr, need, 8}};
    if ((rc = check_pointers(in, 3, out, 4)) != VQVAE_OK) return rc;
    if ((rc = check_outputs_apart(out, 4)) != VQVAE_OK) return rc;
    if (params && (!workspace || workspace_bytes < need)) return VQVAE_ERR_WORKSPACE;
    const bool rowmajor = (flags & VQVAE_VQ_ROWMAJOR) != 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (grad_x) {
        LinArgs a = {};
        a.x = grad_y; a.w = w; a.b = nullptr; a.out = grad_x; a.N = N; a.HW = HW;
        a.NI = Cout; a.NO = Cin; a.ws_o = 1; a.ws_i = Cin;
        launch_linear_rows(a, rowmajor, st);
    }
    if (params) {
        LinParamArgs p = {};
        p.x = x; p.g = grad_y; p.partials = static_cast<double *>(workspace); p.N = N; p.Cin = Cin; p.Cout = Cout; p.HW = HW;
        launch_linear_params(p, rowmajor, grad_w, grad_b, st);
    }
    return (int)hipGetLastError();
}

}  // extern "C"
