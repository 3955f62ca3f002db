// token_pool.hip — per-time-step mean of the encoder's tokens (+ the temporal position table) and its
// backward: the bridge between the VideoMAE encoder and the temporal transformer stage.
//
// Both kernels are HBM-bound streams (forward: G*S*D*4 bytes read for G*D*4 written; backward the
// reverse, plus a bf16 copy), so the layout is chosen for the memory system only:
//   * a workgroup owns one group g (one time step of one clip) and one 64-channel tile: 8 channel
//     lanes x 8 channels (32 B: two 16-byte accesses per lane, one 16-byte store of the bf16 copy),
//     32 row lanes (4 waves x 8).  A row's 8 channel lanes touch 256 contiguous bytes (two whole
//     128-B lines) of f32 and one whole line of bf16.  D % 64 == 0 leaves no partial tile.
//   * row lane r handles rows s = r, r + 32, r + 64, ..  of its group.
// Summation order of the forward (bitwise reproducible, a function of S alone — never of G, the
// grid or the channel count): every lane adds its rows in ascending s; the 32 row-lane partials of
// a channel are then added through LDS in ascending row-lane order (wave 0's eight lanes first, then
// wave 1's, ..), divided by S (correctly rounded division) and the position value added last.
#include "common.h"

namespace vs {

constexpr int kPoolRowLanes = 32;  // row lanes of a workgroup (256 threads / 8 channel lanes)
constexpr int kPoolTile = 64;      // channels of a workgroup

__device__ __forceinline__ uint4 pack_bf16x8(const float4& a, const float4& b) {
  uint4 u;
  u.x = (uint32_t)f2bf(a.x) | ((uint32_t)f2bf(a.y) << 16);
  u.y = (uint32_t)f2bf(a.z) | ((uint32_t)f2bf(a.w) << 16);
  u.z = (uint32_t)f2bf(b.x) | ((uint32_t)f2bf(b.y) << 16);
  u.w = (uint32_t)f2bf(b.z) | ((uint32_t)f2bf(b.w) << 16);
  return u;
}

__global__ __launch_bounds__(256) void token_pool_fwd_kernel(int64_t S, int tiles, int64_t D,
                                                             const float* __restrict__ x, int64_t ldx,
                                                             const float* __restrict__ pos, int64_t pos_rows,
                                                             float* __restrict__ out, bf16_t* __restrict__ out_lp) {
  __shared__ float part[kPoolRowLanes][kPoolTile + 4];  // + 4: row-lane rows land on different banks
  __shared__ float fin[kPoolTile];
  const int cl = threadIdx.x & 7, r = threadIdx.x >> 3;
  const int64_t g = blockIdx.x / tiles;
  const int tile = (int)(blockIdx.x - g * tiles);
  const int64_t c0 = (int64_t)tile * kPoolTile;
  const int64_t step = kPoolRowLanes * ldx;
  const float* p = x + (g * S + r) * ldx + c0 + cl * 8;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  int64_t s = r;
  for (; s + 3 * kPoolRowLanes < S; s += 4 * kPoolRowLanes, p += 4 * step) {  // 8 loads in flight
    float4 a[4], b[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      a[u] = *(const float4*)(p + u * step);
      b[u] = *(const float4*)(p + u * step + 4);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {  // ascending s
      acc[0] += a[u].x; acc[1] += a[u].y; acc[2] += a[u].z; acc[3] += a[u].w;
      acc[4] += b[u].x; acc[5] += b[u].y; acc[6] += b[u].z; acc[7] += b[u].w;
    }
  }
  for (; s < S; s += kPoolRowLanes, p += step) {
    const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
    acc[0] += a.x; acc[1] += a.y; acc[2] += a.z; acc[3] += a.w;
    acc[4] += b.x; acc[5] += b.y; acc[6] += b.z; acc[7] += b.w;
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) part[r][cl * 8 + k] = acc[k];
  __syncthreads();
  if (threadIdx.x < kPoolTile) {  // one channel per lane: the row-lane partials in ascending order
    const int t = threadIdx.x;
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < kPoolRowLanes; ++k) sum += part[k][t];
    float v = sum / (float)S;
    if (pos) v += pos[(g % pos_rows) * D + c0 + t];
    fin[t] = v;
  }
  __syncthreads();
  if (threadIdx.x < 8) {  // 16-byte stores: 8 channels per lane
    const int t = threadIdx.x * 8;
    const float4 a = {fin[t], fin[t + 1], fin[t + 2], fin[t + 3]};
    const float4 b = {fin[t + 4], fin[t + 5], fin[t + 6], fin[t + 7]};
    float* q = out + g * D + c0 + t;
    *(float4*)q = a;
    *(float4*)(q + 4) = b;
    if (out_lp) *(uint4*)(out_lp + g * D + c0 + t) = pack_bf16x8(a, b);
  }
}

// dx[g*S + s][c] = dpool[g][c] / S: each lane divides its 8 channels once (the S rows of a group are
// bitwise equal by construction), packs the bf16 copy once, and streams both out row by row.
__global__ __launch_bounds__(256) void token_pool_bwd_kernel(int64_t S, int tiles, int64_t D,
                                                             const float* __restrict__ dpool, float* __restrict__ dx,
                                                             bf16_t* __restrict__ dx_lp) {
  const int cl = threadIdx.x & 7, r = threadIdx.x >> 3;
  if (r >= S) return;
  const int64_t g = blockIdx.x / tiles;
  const int tile = (int)(blockIdx.x - g * tiles);
  const int64_t c = (int64_t)tile * kPoolTile + cl * 8;
  const float fs = (float)S;
  float4 a = *(const float4*)(dpool + g * D + c), b = *(const float4*)(dpool + g * D + c + 4);
  a.x /= fs; a.y /= fs; a.z /= fs; a.w /= fs;
  b.x /= fs; b.y /= fs; b.z /= fs; b.w /= fs;
  const uint4 u = pack_bf16x8(a, b);
  for (int64_t s = r; s < S; s += kPoolRowLanes) {
    const int64_t o = (g * S + s) * D + c;
    *(float4*)(dx + o) = a;
    *(float4*)(dx + o + 4) = b;
    if (dx_lp) *(uint4*)(dx_lp + o) = u;
  }
}

}  // namespace vs

using namespace vs;

extern "C" int vs_token_pool_fwd(int64_t G, int64_t S, int64_t D, const float* x, int64_t ldx, const float* pos,
                                 int64_t pos_rows, float* out, void* out_lp, void* stream) {
  VS_REQUIRE(x && out, "vs_token_pool_fwd: null pointer");
  VS_REQUIRE(G > 0 && S > 0 && D > 0, "vs_token_pool_fwd: G, S and D must be positive");
  VS_REQUIRE(D % kPoolTile == 0, "vs_token_pool_fwd: D must be a multiple of 64");
  VS_REQUIRE(ldx >= D && ldx % 4 == 0, "vs_token_pool_fwd: ldx >= D and ldx % 4 == 0");
  VS_REQUIRE(!pos || pos_rows > 0, "vs_token_pool_fwd: pos needs pos_rows > 0");
  VS_REQUIRE(aligned16(x) && aligned16(out) && aligned16(pos) && aligned16(out_lp),
             "vs_token_pool_fwd: pointers must be 16-byte aligned");
  const int64_t tiles = D / kPoolTile;
  VS_REQUIRE(G <= INT32_MAX / tiles, "vs_token_pool_fwd: G * D / 64 exceeds the grid limit");
  hipStream_t s = (hipStream_t)stream;
  ScopedTimer timer(VS_TIMER_MISC, s, (double)G * D * (4.0 * S + 4.0 + (pos ? 4.0 : 0.0) + (out_lp ? 2.0 : 0.0)));
  count_path(VS_PATH_TOKEN_POOL);
  hipLaunchKernelGGL(token_pool_fwd_kernel, dim3((unsigned)(G * tiles)), dim3(256), 0, s, S, (int)tiles, D, x, ldx, pos,
                     pos_rows, out, (bf16_t*)out_lp);
  VS_LAUNCH_CHECK();
  return VS_OK;
}

extern "C" int vs_token_pool_bwd(int64_t G, int64_t S, int64_t D, const float* dpool, float* dx, void* dx_lp,
                                 void* stream) {
  VS_REQUIRE(dpool && dx, "vs_token_pool_bwd: null pointer");
  VS_REQUIRE(G > 0 && S > 0 && D > 0, "vs_token_pool_bwd: G, S and D must be positive");
  VS_REQUIRE(D % kPoolTile == 0, "vs_token_pool_bwd: D must be a multiple of 64");
  VS_REQUIRE(aligned16(dpool) && aligned16(dx) && aligned16(dx_lp),
             "vs_token_pool_bwd: pointers must be 16-byte aligned");
  const int64_t tiles = D / kPoolTile;
  VS_REQUIRE(G <= INT32_MAX / tiles, "vs_token_pool_bwd: G * D / 64 exceeds the grid limit");
  hipStream_t s = (hipStream_t)stream;
  ScopedTimer timer(VS_TIMER_MISC, s, (double)G * D * (4.0 + S * (4.0 + (dx_lp ? 2.0 : 0.0))));
  count_path(VS_PATH_TOKEN_POOL);
  hipLaunchKernelGGL(token_pool_bwd_kernel, dim3((unsigned)(G * tiles)), dim3(256), 0, s, S, (int)tiles, D, dpool, dx,
                     (bf16_t*)dx_lp);
  VS_LAUNCH_CHECK();
  return VS_OK;
}
