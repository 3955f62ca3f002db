// conv_common.h — what the R3D-18 encoder's convolution units share (conv_igemm.hip: forward / dX,
// conv_dw.hip: weight gradient; BatchNorm3d, layout and pooling are bn3d.hip and share nothing with them).
//
// The R3D-18 encoder (BASELINE C4: ResNet-18 3D-conv, 32x112x112 clips, fp32).  The reference has no CNN
// encoder: these units replace what torch runs for a torchvision-style r3d_18
// behind the plugin surface (nn.Conv3d forward and its autograd dX / dW, nn.BatchNorm3d in training
// mode, the residual add + ReLU, nn.AdaptiveAvgPool3d(1)).
//
// MI355X design (include/vspike.h "R3D-18 video encoder"):
//   * Activations channels-last f32 [N][D][H][W][C]: every (voxel, tap) reads C contiguous floats, so
//     the implicit GEMM's operand gather is 16-B vector loads of whole channel runs.
//   * Conv3d = implicit GEMM, no im2col tensor (an explicit im2col of layer1 at 16 clips would be
//     11 GB written and read back per conv: 2x the conv's f32-MFMA time in HBM traffic).  Rows = output
//     voxels, k = (tap, channel), the A operand gathered per k-tile into LDS (zero outside the padded
//     volume), the weights K-contiguous [Co][taps][Ci] as the B operand; v_mfma_f32_16x16x4_f32 (exact
//     f32: a k-ordered fmaf chain).  128 x 64 output tile, 4 waves of 64 x 32, BK = 32, register-staged
//     prefetch into a 2-stage LDS ring (the loads of k-tile t+1 in flight under the MFMAs of t).
//   * dX of a stride-1 conv is the same kernel on dy with the flipped offsets; of a stride-2 conv one
//     launch per parity class of the input positions with only the taps that reach it (1..8 of 27),
//     so no MFMA multiplies a structural zero; weights regrouped per class ([Ci][class taps][Co]).
//   * dW: tiles of (64 out channels x 64 k) summed over the output voxels (the gather as the B
//     operand), split over the voxel rows; partial tiles summed in split order (no atomics).
//   * BatchNorm3d statistics ride in the forward conv's epilogue (per 128-row tile column sums of y and
//     of the squared deviations from the tile mean), merged in f64 in a fixed order (Chan); apply (+ residual + ReLU) and the backward are
//     channel-vectorised elementwise passes with fixed-order reductions.
#pragma once

#include "common.h"

namespace vs {

__device__ __forceinline__ int divq(int x, int d, float inv) {
  // x / d for 0 <= x < 2^24 by a float reciprocal and one correction step (24-bit multiply: full
  // rate, where v_mul_lo_u32 is a quarter-rate instruction)
  int q = (int)((float)x * inv);
  int r = x - (int)__umul24(q, d);
  if (r < 0) --q;
  else if (r >= d) ++q;
  return q;
}
__device__ __forceinline__ int mul24(int a, int b) { return (int)__umul24(a, b); }  // a, b in [0, 2^24)

// GEMM row m -> (clip n, grid position gd, gh, gw) of a row grid [N][Gd][Gh][Gw], by three divq with the
// reciprocals of the extents (the hosts keep the row count, hence every operand here, below 2^24)
struct RowPos {
  int n, gd, gh, gw;
};
__device__ __forceinline__ RowPos row_decode(int m, int Gd, int Gh, int Gw, float ihd, float ihh, float ihw) {
  const int q1 = divq(m, Gw, ihw), gw = m - mul24(q1, Gw);
  const int q2 = divq(q1, Gh, ihh), gh = q1 - mul24(q2, Gh);
  const int n = divq(q2, Gd, ihd), gd = q2 - mul24(n, Gd);
  return {n, gd, gh, gw};
}

// 16-B load through a raw buffer resource: an offset past num_records (kOob) returns zeros with no
// exec-mask branch or zeroing moves (the host keeps every operand below 2^31 bytes)
constexpr uint32_t kOob = 0x80000000u;
__device__ __forceinline__ __amdgpu_buffer_rsrc_t conv_rsrc(const float* base, int bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), (short)0, bytes, 0x00020000);
}
__device__ __forceinline__ float4 bload4(__amdgpu_buffer_rsrc_t r, uint32_t byte_off) {
  return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(r, byte_off, 0, 0));
}

// f32 MFMA operand images: row-major [rows][k], 34-float rows (conflict-free ds_read_b32 of 16 rows x
// 2 k per 32-lane half: bank = 2 row + k), filled by two ds_write_b64 per gathered float4
constexpr int kLdA = 34;

// ---- host side -------------------------------------------------------------------------------
inline int ilog2(int64_t v) {
  int s = 0;
  while ((1ll << s) < v) ++s;
  return (1ll << s) == v ? s : -1;
}

inline bool desc_ok(const vs_conv3d_desc* d) {
  if (!d || d->N <= 0 || d->Ci <= 0 || d->Co <= 0) return false;
  if (d->kd < 1 || d->kh < 1 || d->kw < 1 || d->sd < 1 || d->sh < 1 || d->sw < 1) return false;
  if (d->pd < 0 || d->ph < 0 || d->pw < 0) return false;
  return d->Do == (d->Di + 2 * d->pd - d->kd) / d->sd + 1 && d->Ho == (d->Hi + 2 * d->ph - d->kh) / d->sh + 1 &&
         d->Wo == (d->Wi + 2 * d->pw - d->kw) / d->sw + 1 && d->Do > 0 && d->Ho > 0 && d->Wo > 0;
}

inline double conv_flops(const vs_conv3d_desc* d) {
  return 2.0 * (double)(d->N * d->Do * d->Ho * d->Wo) * (double)d->Co * (double)(d->kd * d->kh * d->kw * d->Ci);
}

}  // namespace vs
