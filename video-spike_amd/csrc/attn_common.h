// attn_common.h — what the head-dim-64 attention units share (non-causal MHA over frame-patch
// tokens, mv:230-266, 286-294).
//
// bf16 (performance) path — v_mfma_f32_32x32x16_bf16, f32 accumulation, online softmax:
//   forward (attn_fwd.hip): workgroup = 4 waves = 128 queries of one (batch, head); each wave owns
//     32 queries.  S^T = K Q^T is computed with the KEY on the accumulator row and the QUERY on the
//     lane, so a lane owns one query's whole softmax state (max, sum) — no cross-lane reductions
//     except one xor-32 swap per 64-key tile.  The exponentiated S^T accumulator is directly the B
//     operand of O^T += V^T P^T (no LDS round trip); V^T fragments come from ds_read_tr16_b64 on the
//     V tile.  K/V tiles (64 keys) arrive by LDS-DMA in double-buffered, XOR-swizzled LDS images.
//   backward (attn_bwd.hip): two atomic-free passes in one launch.  dK/dV is key-major (each wave
//     keeps 32 keys' K, V as MFMA operands and dK^T, dV^T in accumulators while sweeping 32-query
//     blocks); dQ is query-major like the forward (LSE and delta are per-lane constants).  Summing
//     dQ across key blocks with f32 atomics instead was measured atomic-rate-bound (~489 MB of adds
//     per ViT-Tiny launch at ~1.3 TB/s: 466 us/launch, profiles/r01_v0_kernel_stats.csv), so dQ
//     recomputes S and dP.
// f32 (parity) path (attn_f32.hip) — exact-f32 VALU kernels: 4 lanes per query/key row, K/V (or
//   Q/dO) tiles in LDS, expf/logf in f32.  Used for the 1e-4-relative parity mode.
#pragma once
#include <math.h>
#include <stdlib.h>

#include <type_traits>

#include "common.h"

namespace vs {

constexpr float kLog2e = 1.4426950408889634f;
constexpr float kLn2 = 0.6931471805599453f;

// ---- XOR swizzles of the 128-B-row LDS images (16-B chunk index ^ swz(row))
__device__ __forceinline__ int swz_row(int r) { return (r >> 1) & 7; }           // 16-B chunk XOR
__device__ __forceinline__ int swz_half(int r) { return ((r >> 1) & 1) << 2; }   // 64-B half XOR
// the backward's images: conflict-free for BOTH the row reads (ds_read_b128) and the transposed reads
// (rows r..r+3 land in distinct bank quarters); swz_row puts rows r and r+2 of every tr read on the
// same banks
__device__ __forceinline__ int swz_rt(int r) {
  const int u = (r >> 1) & 7;
  return ((u & 1) << 2) | (u >> 1);
}

// byte offset of element (r, c) (c multiple of 4 for tr reads) in a 128-B-row image
__device__ __forceinline__ int off_halfswz(int r, int c) { return r * 128 + (((c >> 3) ^ swz_half(r)) << 4) + (c & 7) * 2; }
__device__ __forceinline__ int off_rtswz(int r, int c) { return r * 128 + (((c >> 3) ^ swz_rt(r)) << 4) + (c & 7) * 2; }

__device__ __forceinline__ bf16x8 tr_pair(const char* lds, int off0, int off1) {
  short4v t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((VS_LDS short4v*)(lds + off0));
  short4v t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((VS_LDS short4v*)(lds + off1));
  typedef __attribute__((ext_vector_type(8))) short short8v;
  short8v s = {t0[0], t0[1], t0[2], t0[3], t1[0], t1[1], t1[2], t1[3]};
  return __builtin_bit_cast(bf16x8, s);
}

typedef __attribute__((ext_vector_type(8))) float f32x8;
// 8 f32 -> 8 bf16 as four v_cvt_pk_bf16_f32 (element-wise casts cost one cvt per value)
__device__ __forceinline__ bf16x8 pack8f(const float* a) {
  const f32x8 v = {a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7]};
  return __builtin_convertvector(v, bf16x8);
}

__device__ __forceinline__ uint2 pack4(float a, float b, float c, float d) {
  uint2 u;
  u.x = (uint32_t)f2bf(a) | ((uint32_t)f2bf(b) << 16);
  u.y = (uint32_t)f2bf(c) | ((uint32_t)f2bf(d) << 16);
  return u;
}

__device__ __forceinline__ float max3f(float a, float b, float c) {
  float r;
  asm volatile("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
__device__ __forceinline__ float max16(const f32x16& x) {
  const float a = max3f(x[0], x[1], x[2]), b = max3f(x[3], x[4], x[5]), c = max3f(x[6], x[7], x[8]);
  const float d = max3f(x[9], x[10], x[11]), e = max3f(x[12], x[13], x[14]);
  return max3f(max3f(a, b, c), max3f(d, e, x[15]), -INFINITY);
}
// v_permlane32_swap(v, v) returns {v[lane & 31], v[32 + (lane & 31)]}: both halves' values in
// every lane, so a pair reduction over lanes l and l^32 needs no LDS round trip.
__device__ __forceinline__ float pair_max(float v) {
  auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return max3f(__uint_as_float(r[0]), __uint_as_float(r[1]), -INFINITY);
}
__device__ __forceinline__ float pair_sum(float v) {
  auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}

// VS_ATTN_PRIO (diagnostic builds): every 32x32x16 MFMA issued at raised wave priority
// (s_setprio 1 / 0 around it), so a wave with an MFMA ready wins the issue port over VALU work
__device__ __forceinline__ f32x16 mfma32p(const bf16x8& a, const bf16x8& b, const f32x16& c) {
#ifdef VS_ATTN_PRIO
  __builtin_amdgcn_s_setprio(1);
  const f32x16 r = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  __builtin_amdgcn_s_setprio(0);
  return r;
#else
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
#endif
}

// VS_ATTN_DIAG (diagnostic builds only): bit 0 = the forward streams only its first two K/V tiles,
// bit 1 = the backward (both passes) only its first two Q/dO or K/V slices: the rest of the tiles are
// computed on stale LDS data, which times the kernels without their LDS-DMA fill (results WRONG)
#ifndef VS_ATTN_DIAG
#define VS_ATTN_DIAG 0
#endif

// A workgroup's place in the 1D grids of the bf16 kernels: block `blk` (after xcd_remap) is 128-row
// block `xb` of head h of batch element b; row0 is the batch element's first row of qkv / o / dout.
struct AttnBlock {
  int xb, h, b, D;
  int64_t row0;
};
__device__ __forceinline__ AttnBlock attn_block(int blk, int N, int H) {
  const int nb128 = (N + 127) / 128;
  AttnBlock a;
  a.xb = blk % nb128;
  a.h = (blk / nb128) % H;
  a.b = blk / nb128 / H;
  a.D = H * 64;
  a.row0 = (int64_t)a.b * N;
  return a;
}

// 8 bf16 at p, scaled by c in f32 and rounded to bf16 once: the pre-scaled MFMA operand (the forward's
// and dQ's Q, dK/dV's K) -- every kernel rounds c * x the same way, so the backward's P is the forward's
__device__ __forceinline__ bf16x8 scaled_frag(const bf16_t* p, float c) {
  const bf16x8 x = *(const bf16x8*)p;
  f32x8 v;
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = (float)x[j] * c;
  return __builtin_convertvector(v, bf16x8);
}

// Scores of keys past N in a 32-key block of S^T starting at key0 -> -inf (p = 0).  Accumulator row r
// of lane half hh is key (r & 3) + 8 (r >> 2) + 4 hh of the block.  The caller tests key0 + 32 > N
// (wave-uniform): written inside this helper, that test is folded into the 16 selects and every block
// of every tile pays for them.  Arguments by reference, so that the callers' lambdas read hh and N where
// the selects are, as the loop written in place does (by value, the forward spills 9 SGPRs, not 2).
__device__ __forceinline__ void mask_keys_past_n(f32x16& acc, const int& key0, const int& hh, const int& N) {
#pragma unroll
  for (int r = 0; r < 16; ++r)
    if (key0 + (r & 3) + 8 * (r >> 2) + 4 * hh >= N) acc[r] = -INFINITY;
}

// exact-f32 kernels (attn_f32.hip), launched by vs_attn_fwd / vs_attn_bwd; `delta` is the backward's
// workspace ([B, H, N] f32)
void attn_fwd_f32_launch(hipStream_t s, int64_t B, int64_t N, int64_t H, const float* qkv, int64_t ld_qkv, float* o,
                         int64_t ld_o, float* lse, float scale);
void attn_bwd_f32_launch(hipStream_t s, int64_t B, int64_t N, int64_t H, const float* qkv, int64_t ld_qkv,
                         const float* o, int64_t ld_o, const float* dout, int64_t ld_do, const float* lse, float* dqkv,
                         int64_t ld_dqkv, float* delta, float scale);

}  // namespace vs

static inline int attn_check(int64_t B, int64_t N, int64_t H, int64_t Dh) {
  VS_REQUIRE(Dh == 64, "vs_attn: head dim must be 64");
  VS_REQUIRE(B > 0 && N > 0 && H > 0, "vs_attn: empty problem");
  VS_REQUIRE(B <= 65535 && H <= 65535 && N < (1 << 30), "vs_attn: extents out of range");
  return VS_OK;
}
