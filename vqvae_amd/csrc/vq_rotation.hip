// The rotation-trick gradient of the quantizer's z (gfx950): vqvae_vq_backward_f32 with VQVAE_VQ_BWD_ROTATION (train.hip selects it).
// Fifty et al., "Restructuring Vector Quantization with the Rotation Trick", arXiv 2410.06424: instead of d z_q / d z = I
// (models/quantizer.py:67) every row uses the rotation-and-rescale that carries it onto its code, treated as a constant.  The forward
// does not change by a bit; only grad_z does.
//
// THE ARITHMETIC IS THE CONTRACT (tests/vq_rotation_ref.py restates it on the CPU; the library is compiled with -ffp-contract=off,
// so every operation written below is one IEEE operation).  For each of the N = B H W rows: e = the row of z, q = E[idx] its code,
// g = the row of grad_zq.  The trick defines z~_q = sg[lam R] e with
//     e^ = e / ||e||,  q^ = q / ||q||,  r = (e^ + q^) / ||e^ + q^||,  R = I - 2 r r^T + 2 q^ e^^T,  lam = ||q|| / ||e||.
// Its value is q; its gradient is lam R^T g = lam [g - 2 r (r^T g) + 2 e^ (q^^T g)]: five dot products.  All of it in fp64 from the
// fp32 inputs:
//
//   ee, qq, eq, eg, qg : s = 0.0; for c = 0 .. D-1 in ascending order: s = s + double(a_c) * double(b_c)
//                        (the product of two fp32 values is exact in fp64; only the additions round)
//   ne = sqrt(ee);  nq = sqrt(qq);  p = ne * nq
//   ns2 = 2.0 + 2.0 * (eq / p)                                   (= ||e^ + q^||^2)
//   rotate = ee > 0 && qq > 0 && ee, qq finite && ns2 >= 2^-20
//   a   = (eg / ne + qg / nq) / ns2
//   ce  = (2.0 * qg) / p - (2.0 * a) / ne
//   cq  = -((2.0 * a) / nq)
//   lam = nq / ne
//   rot_c = lam * ((double(g_c) + ce * double(e_c)) + cq * double(q_c))      rounded to fp32 once
//   rot_c = g_c where !rotate
//   grad_z_c = rot_c + gs * (z_c - q_c)                          in fp32, exactly as vqb_gradz_kernel forms g_zq + gs * (z - e)
//
// gs = g_loss * fp32(2 / (N D)), or fp32(2 beta / (N D)) with VQVAE_VQ_BWD_COMMITMENT.  A row with rotate == false falls back to the
// straight-through gradient: a zero row of z, a zero code, a non-finite norm, and a row antipodal to its code, where the reflection
// axis is undefined.  At ns2 < 2^-20 fewer than about 33 of fp64's 53 bits still determine r: the threshold is a rule of the
// contract, not a measurement.  A NaN in g or z stays in its own row.  The device's fp64 sqrt and division are correctly rounded
// (optim.hip relies on the same), so the results have the restatement's bits.
//
// One lane owns one row, in either layout, and adds in ascending channel order: the same bits in row-major and NCHW, and from run to
// run.  NCHW maps are read one dword per lane, coalesced across hw as they stand.  Row-major rows take 16 bytes per access when
// D % 4 == 0 and every tensor is 16-byte aligned, else one element per access; the lanes of a wave are then a row apart, so one
// access of a wave touches 64 lines, and the wave's following accesses find those lines in L1 / L2.  Rows of up to 64 channels stay
// in registers between the sums and the output; wider rows are read a second time right after the first.  Code rows come through
// L2.  No atomics, no host sync, no allocation, no LDS; the launch is on the caller's stream and is capturable.
#include "common.h"
#include "vq_rotation.h"

namespace vqvae {

template <int DREG, int V>
__global__ __launch_bounds__(256) void vq_rotation_gradz_kernel(RotArgs a) { rot_gradz_body<DREG, V>(a); }

template <int V>
static void rot_launch(const RotArgs &a, hipStream_t st) {
    const dim3 grid(grid_of(a.N)), block(256);
    if (a.D <= 16) hipLaunchKernelGGL((vq_rotation_gradz_kernel<16, V>), grid, block, 0, st, a);
    else if (a.D <= 64) hipLaunchKernelGGL((vq_rotation_gradz_kernel<64, V>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((vq_rotation_gradz_kernel<0, V>), grid, block, 0, st, a);
}

void launch_vq_rotation_gradz(const RotArgs &a, hipStream_t st) {
    const bool vec4 = a.rowmajor && (a.D & 3) == 0 &&
                      !((reinterpret_cast<uintptr_t>(a.z) | reinterpret_cast<uintptr_t>(a.cb) | reinterpret_cast<uintptr_t>(a.out) |
                         reinterpret_cast<uintptr_t>(a.g_zq)) & 15);
    if (vec4) rot_launch<4>(a, st);
    else rot_launch<1>(a, st);
}

}  // namespace vqvae
