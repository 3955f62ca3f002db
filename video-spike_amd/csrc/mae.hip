// mae.hip — the pieces HF ViTMAEForPreTraining adds around the encoder and decoder blocks: the masked token
// gather in front of the encoder, the decoder's sequence assembly (kept tokens unshuffled, mask tokens elsewhere,
// plus the decoder's position table) and the masked pixel loss, each with its backward.
//
// The index tensors are the host's: ids_keep [G, Lk] = the first Lk entries of argsort(noise), ids_restore [G, P]
// = argsort of that argsort; patch p of image g is kept iff ids_restore[g, p] < Lk, and then sits at token
// 1 + ids_restore[g, p] of the encoder's sequence.  An index outside its range selects nothing (zeros), it is
// never used as an address.
//
// The gathers are streams of 16 bytes per lane; the loss kernel reads and writes 4-byte elements (its target is a
// strided gather from the image).  The sums (d_cls, d_mask_token, the loss) run in an order fixed by
// the extents: no atomics, equal bits from equal inputs.
#include "common.h"

namespace vs {

__device__ __forceinline__ float4 mae_add4(const float4& a, const float4& b) {
  return float4{a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w};
}
__device__ __forceinline__ void mae_store4(float* p, const float4& v) { *(float4*)p = v; }
__device__ __forceinline__ void mae_store4(bf16_t* p, const float4& v) {
  uint2 u;
  u.x = (uint32_t)f2bf(v.x) | ((uint32_t)f2bf(v.y) << 16);
  u.y = (uint32_t)f2bf(v.z) | ((uint32_t)f2bf(v.w) << 16);
  *(uint2*)p = u;
}

// x0[g, 0] = cls + table[0];  x0[g, 1 + j] = patches[g, ids_keep[g, j]]: one lane per 4 channels of a row of x0
__global__ __launch_bounds__(256) void mae_embed_fwd_kernel(int64_t total4, int P, int Lk, int D4,
                                                            const float4* __restrict__ patches,
                                                            const int32_t* __restrict__ ids_keep,
                                                            const float4* __restrict__ cls,
                                                            const float4* __restrict__ table, float4* __restrict__ x0) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;
  const int64_t row = i / D4;
  const int c = (int)(i - row * D4);
  const int64_t g = row / (Lk + 1);
  const int t = (int)(row - g * (Lk + 1));
  float4 v = {0.f, 0.f, 0.f, 0.f};
  if (t == 0) {
    v = mae_add4(cls[c], table[c]);
  } else {
    const int p = ids_keep[g * Lk + t - 1];
    if ((unsigned)p < (unsigned)P) v = patches[(g * P + p) * D4 + c];
  }
  x0[i] = v;
}

// d_patches[g, p] = kept ? dx[g, 1 + ids_restore[g, p]] : 0: one lane per 4 channels of a compact patch row
template <typename T>
__global__ __launch_bounds__(256) void mae_embed_bwd_rows_kernel(int64_t total4, int P, int Lk, int D4,
                                                                 const float4* __restrict__ dx,
                                                                 const int32_t* __restrict__ ids_restore,
                                                                 T* __restrict__ dp) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;
  const int64_t row = i / D4;  // g * P + p
  const int c = (int)(i - row * D4);
  const int64_t g = row / P;
  const int r = ids_restore[row];
  float4 v = {0.f, 0.f, 0.f, 0.f};
  if ((unsigned)r < (unsigned)Lk) v = dx[(g * (Lk + 1) + 1 + r) * D4 + c];
  mae_store4(dp + i * 4, v);
}

// out[c] = sum_g src[g * row_stride4 + c], ascending g: one lane per 4 channels
__global__ __launch_bounds__(64) void mae_sum_rows_kernel(int64_t G, int64_t row_stride4, int D4,
                                                          const float4* __restrict__ src, float4* __restrict__ out) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  if (c >= D4) return;
  float4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int64_t g = 0; g < G; ++g) acc = mae_add4(acc, src[g * row_stride4 + c]);
  out[c] = acc;
}

// xd[g, 0] = e[g, 0] + tabd[0];  xd[g, 1 + p] = (kept ? e[g, 1 + ids_restore[g, p]] : mask_token) + tabd[1 + p]
__global__ __launch_bounds__(256) void mae_dec_assemble_fwd_kernel(int64_t total4, int P, int Lk, int D4,
                                                                   const float4* __restrict__ e,
                                                                   const int32_t* __restrict__ ids_restore,
                                                                   const float4* __restrict__ mask_token,
                                                                   const float4* __restrict__ tabd,
                                                                   float4* __restrict__ xd) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;
  const int64_t row = i / D4;
  const int c = (int)(i - row * D4);
  const int64_t g = row / (P + 1);
  const int t = (int)(row - g * (P + 1));
  float4 v;
  if (t == 0) {
    v = e[g * (Lk + 1) * D4 + c];
  } else {
    const int r = ids_restore[g * P + t - 1];
    v = (unsigned)r < (unsigned)Lk ? e[(g * (Lk + 1) + 1 + r) * D4 + c] : mask_token[c];
  }
  xd[i] = mae_add4(v, tabd[(int64_t)t * D4 + c]);
}

// d_e[g, 0] = dxd[g, 0];  d_e[g, 1 + j] = dxd[g, 1 + ids_keep[g, j]]
template <typename T>
__global__ __launch_bounds__(256) void mae_dec_assemble_bwd_rows_kernel(int64_t total4, int P, int Lk, int D4,
                                                                        const float4* __restrict__ dxd,
                                                                        const int32_t* __restrict__ ids_keep,
                                                                        T* __restrict__ de) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;
  const int64_t row = i / D4;
  const int c = (int)(i - row * D4);
  const int64_t g = row / (Lk + 1);
  const int t = (int)(row - g * (Lk + 1));
  float4 v = {0.f, 0.f, 0.f, 0.f};
  if (t == 0) {
    v = dxd[g * (P + 1) * D4 + c];
  } else {
    const int p = ids_keep[g * Lk + t - 1];
    if ((unsigned)p < (unsigned)P) v = dxd[(g * (P + 1) + 1 + p) * D4 + c];
  }
  mae_store4(de + i * 4, v);
}

// part[g, c] = sum over the masked patches p of image g, ascending p, of dxd[g, 1 + p, c]: grid (ceil(D4 / 64), G)
__global__ __launch_bounds__(64) void mae_mask_token_part_kernel(int P, int Lk, int D4, const float4* __restrict__ dxd,
                                                                 const int32_t* __restrict__ ids_restore,
                                                                 float4* __restrict__ part) {
  const int c = blockIdx.x * 64 + threadIdx.x;
  const int64_t g = blockIdx.y;
  if (c >= D4) return;
  float4 acc = {0.f, 0.f, 0.f, 0.f};
  const int32_t* ids = ids_restore + g * P;
  const float4* src = dxd + (g * (P + 1) + 1) * D4 + c;
  for (int p = 0; p < P; ++p)
    if ((unsigned)ids[p] >= (unsigned)Lk) acc = mae_add4(acc, src[(int64_t)p * D4]);
  part[g * D4 + c] = acc;
}

// One wave per row of pred [G, P + 1, K].  Masked patch rows: row_loss = mean_k (pred - target)^2 in f64 and
// d_pred = 2 (pred - target) / (K * n_masked); every other row (kept patches, the CLS row): 0 and zeros.
// target is HF's patchify of the f32 pixels: k = (i * patch + j) * C + c of patch (hp, wp) is pixel
// [g, c, hp * patch + i, wp * patch + j].
template <typename T>
__global__ __launch_bounds__(256) void mae_recon_rows_kernel(int64_t rows, int P, int Lk, int C, int S, int patch,
                                                             const float* __restrict__ pred, int64_t ld_pred,
                                                             const float* __restrict__ pixels,
                                                             const int32_t* __restrict__ ids_restore, double inv_kn,
                                                             double* __restrict__ row_loss, T* __restrict__ d_pred,
                                                             int64_t ld_dpred) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;  // wave-uniform
  const int K = patch * patch * C, w = S / patch;
  const int64_t g = row / (P + 1);
  const int t = (int)(row - g * (P + 1));
  const bool masked = t > 0 && (unsigned)ids_restore[g * P + t - 1] >= (unsigned)Lk;
  T* drow = d_pred + row * ld_dpred;
  double acc = 0.0;
  if (masked) {
    const int hp = (t - 1) / w, wp = (t - 1) - hp * w;
    const float* prow = pred + row * ld_pred;
    for (int k = lane; k < K; k += 64) {
      const int c = k % C, ij = k / C, i = ij / patch, j = ij - i * patch;
      const float tgt = pixels[((g * C + c) * S + hp * patch + i) * (int64_t)S + wp * patch + j];
      const float d = prow[k] - tgt;
      acc += (double)d * (double)d;
      Elem<T>::store(drow + k, (float)(2.0 * (double)d * inv_kn));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  } else {
    for (int k = lane; k < K; k += 64) Elem<T>::store(drow + k, 0.f);
  }
  if (lane == 0 && t > 0) row_loss[g * P + t - 1] = masked ? acc / (double)K : 0.0;
}

// loss = sum(row_loss) / n_masked: one workgroup, strided f64 partial sums and a fixed LDS tree
__global__ __launch_bounds__(256) void mae_recon_final_kernel(int64_t n, const double* __restrict__ row_loss,
                                                              double inv_masked, float* __restrict__ loss) {
  __shared__ double part[256];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) s += row_loss[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = (float)(part[0] * inv_masked);
}

}  // namespace vs

using namespace vs;

static int mae_check(int64_t G, int64_t P, int64_t Lk, int64_t D) {
  VS_REQUIRE(G > 0 && P > 0 && D > 0, "vs_mae: G, P and D must be positive");
  VS_REQUIRE(Lk >= 1 && Lk <= P, "vs_mae: the kept length must be in 1..P");
  VS_REQUIRE(D % 4 == 0, "vs_mae: D must be a multiple of 4");
  VS_REQUIRE(P < (1 << 24) && G <= INT32_MAX / ((P + 1) * (D / 4)), "vs_mae: G * (P + 1) * D exceeds the grid limit");
  return VS_OK;
}

static unsigned mae_blocks(int64_t total) { return (unsigned)cdiv(total, 256); }

extern "C" int vs_mae_embed_fwd(int64_t G, int64_t P, int64_t Lk, int64_t D, const float* patches,
                                const int32_t* ids_keep, const float* cls, const float* table, float* x0, void* stream) {
  VS_CALL(mae_check(G, P, Lk, D));
  VS_REQUIRE(patches && ids_keep && cls && table && x0, "vs_mae_embed_fwd: null pointer");
  VS_REQUIRE(aligned16(patches) && aligned16(cls) && aligned16(table) && aligned16(x0),
             "vs_mae_embed_fwd: pointers must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int64_t total4 = G * (Lk + 1) * (D / 4);
  ScopedTimer timer(VS_TIMER_MISC, s, 8.0 * D * (double)G * (Lk + 1));
  hipLaunchKernelGGL(mae_embed_fwd_kernel, dim3(mae_blocks(total4)), dim3(256), 0, s, total4, (int)P, (int)Lk,
                     (int)(D / 4), (const float4*)patches, ids_keep, (const float4*)cls, (const float4*)table,
                     (float4*)x0);
  VS_LAUNCH_CHECK();
  return VS_OK;
}

extern "C" int vs_mae_embed_bwd(int32_t out_dtype, int64_t G, int64_t P, int64_t Lk, int64_t D, const float* dx,
                                const int32_t* ids_restore, float* d_cls, void* d_patches, void* stream) {
  VS_REQUIRE(out_dtype == VS_F32 || out_dtype == VS_BF16, "vs_mae_embed_bwd: out dtype must be f32 or bf16");
  VS_CALL(mae_check(G, P, Lk, D));
  VS_REQUIRE(dx && ids_restore && d_cls && d_patches, "vs_mae_embed_bwd: null pointer");
  VS_REQUIRE(aligned16(dx) && aligned16(d_cls) && aligned16(d_patches),
             "vs_mae_embed_bwd: pointers must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int64_t total4 = G * P * (D / 4);
  ScopedTimer timer(VS_TIMER_MISC, s, (double)G * D * (4.0 * (Lk + 1) + (double)P * esize(out_dtype)));
  if (out_dtype == VS_F32)
    hipLaunchKernelGGL(mae_embed_bwd_rows_kernel<float>, dim3(mae_blocks(total4)), dim3(256), 0, s, total4, (int)P,
                       (int)Lk, (int)(D / 4), (const float4*)dx, ids_restore, (float*)d_patches);
  else
    hipLaunchKernelGGL(mae_embed_bwd_rows_kernel<bf16_t>, dim3(mae_blocks(total4)), dim3(256), 0, s, total4, (int)P,
                       (int)Lk, (int)(D / 4), (const float4*)dx, ids_restore, (bf16_t*)d_patches);
  VS_LAUNCH_CHECK();
  hipLaunchKernelGGL(mae_sum_rows_kernel, dim3((unsigned)cdiv(D / 4, 64)), dim3(64), 0, s, G, (Lk + 1) * (D / 4),
                     (int)(D / 4), (const float4*)dx, (float4*)d_cls);
  VS_LAUNCH_CHECK();
  return VS_OK;
}

extern "C" int vs_mae_dec_assemble_fwd(int64_t G, int64_t P, int64_t Lk, int64_t D, const float* e,
                                       const int32_t* ids_restore, const float* mask_token, const float* tabd,
                                       float* xd, void* stream) {
  VS_CALL(mae_check(G, P, Lk, D));
  VS_REQUIRE(e && ids_restore && mask_token && tabd && xd, "vs_mae_dec_assemble_fwd: null pointer");
  VS_REQUIRE(aligned16(e) && aligned16(mask_token) && aligned16(tabd) && aligned16(xd),
             "vs_mae_dec_assemble_fwd: pointers must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const int64_t total4 = G * (P + 1) * (D / 4);
  ScopedTimer timer(VS_TIMER_MISC, s, 4.0 * D * (double)G * (2.0 * (P + 1) + Lk + 1));
  hipLaunchKernelGGL(mae_dec_assemble_fwd_kernel, dim3(mae_blocks(total4)), dim3(256), 0, s, total4, (int)P, (int)Lk,
                     (int)(D / 4), (const float4*)e, ids_restore, (const float4*)mask_token, (const float4*)tabd,
                     (float4*)xd);
  VS_LAUNCH_CHECK();
  return VS_OK;
}

extern "C" size_t vs_mae_dec_assemble_bwd_workspace_bytes(int64_t G, int64_t D) {
  return G > 0 && D > 0 ? ((size_t)(G * D) * 4 + 255) / 256 * 256 : 0;  // the per-image partial sums of d_mask_token
}

extern "C" int vs_mae_dec_assemble_bwd(int32_t out_dtype, int64_t G, int64_t P, int64_t Lk, int64_t D, const float* dxd,
                                       const int32_t* ids_keep, const int32_t* ids_restore, void* d_e,
                                       float* d_mask_token, void* workspace, void* stream) {
  VS_REQUIRE(out_dtype == VS_F32 || out_dtype == VS_BF16, "vs_mae_dec_assemble_bwd: out dtype must be f32 or bf16");
  VS_CALL(mae_check(G, P, Lk, D));
  VS_REQUIRE(dxd && ids_keep && ids_restore && d_e && d_mask_token && workspace,
             "vs_mae_dec_assemble_bwd: null pointer");
  VS_REQUIRE(aligned16(dxd) && aligned16(d_e) && aligned16(d_mask_token) && aligned16(workspace),
             "vs_mae_dec_assemble_bwd: pointers must be 16-byte aligned");
  VS_REQUIRE(G <= 65535, "vs_mae_dec_assemble_bwd: G exceeds the grid limit");
  hipStream_t s = (hipStream_t)stream;
  const int64_t total4 = G * (Lk + 1) * (D / 4);
  const int D4 = (int)(D / 4);
  ScopedTimer timer(VS_TIMER_MISC, s, (double)G * D * (4.0 * (P + 1) + (double)(Lk + 1) * esize(out_dtype)));
  if (out_dtype == VS_F32)
    hipLaunchKernelGGL(mae_dec_assemble_bwd_rows_kernel<float>, dim3(mae_blocks(total4)), dim3(256), 0, s, total4,
                       (int)P, (int)Lk, D4, (const float4*)dxd, ids_keep, (float*)d_e);
  else
    hipLaunchKernelGGL(mae_dec_assemble_bwd_rows_kernel<bf16_t>, dim3(mae_blocks(total4)), dim3(256), 0, s, total4,
                       (int)P, (int)Lk, D4, (const float4*)dxd, ids_keep, (bf16_t*)d_e);
  VS_LAUNCH_CHECK();
  hipLaunchKernelGGL(mae_mask_token_part_kernel, dim3((unsigned)cdiv(D4, 64), (unsigned)G), dim3(64), 0, s, (int)P,
                     (int)Lk, D4, (const float4*)dxd, ids_restore, (float4*)workspace);
  VS_LAUNCH_CHECK();
  hipLaunchKernelGGL(mae_sum_rows_kernel, dim3((unsigned)cdiv(D4, 64)), dim3(64), 0, s, G, (int64_t)D4, D4,
                     (const float4*)workspace, (float4*)d_mask_token);
  VS_LAUNCH_CHECK();
  return VS_OK;
}

extern "C" size_t vs_mae_recon_loss_workspace_bytes(int64_t G, int64_t P) {
  return G > 0 && P > 0 ? ((size_t)(G * P) * 8 + 255) / 256 * 256 : 0;  // row_loss f64 [G, P]
}

extern "C" int vs_mae_recon_loss(int32_t out_dtype, int64_t G, int64_t C, int64_t S, int64_t patch, int64_t Lk,
                                 const float* pred, int64_t ld_pred, const float* pixels, const int32_t* ids_restore,
                                 float* loss, void* d_pred, int64_t ld_dpred, void* workspace, void* stream) {
  VS_REQUIRE(out_dtype == VS_F32 || out_dtype == VS_BF16, "vs_mae_recon_loss: out dtype must be f32 or bf16");
  VS_REQUIRE(G > 0 && C > 0 && S > 0 && patch > 0 && S % patch == 0 && S <= 32768,
             "vs_mae_recon_loss: image size must be a positive multiple of the patch size");
  const int64_t w = S / patch, P = w * w, K = patch * patch * C;
  VS_REQUIRE(Lk >= 1 && Lk < P, "vs_mae_recon_loss: the kept length must be in 1..P-1 (at least one masked patch)");
  VS_REQUIRE(pred && pixels && ids_restore && loss && d_pred && workspace, "vs_mae_recon_loss: null pointer");
  VS_REQUIRE(ld_pred >= K && ld_dpred >= K, "vs_mae_recon_loss: leading dims too small");
  VS_REQUIRE((((uintptr_t)workspace) & 7) == 0, "vs_mae_recon_loss: workspace must be 8-byte aligned");
  const int64_t rows = G * (P + 1);
  VS_REQUIRE(K <= (1 << 20) && cdiv(rows, 4) <= INT32_MAX, "vs_mae_recon_loss: extents out of range");
  hipStream_t s = (hipStream_t)stream;
  const double n_masked = (double)G * (double)(P - Lk);
  ScopedTimer timer(VS_TIMER_MISC, s, (double)G * (P - Lk) * K * 8.0 + (double)rows * K * esize(out_dtype));
  double* row_loss = (double*)workspace;
  if (out_dtype == VS_F32)
    hipLaunchKernelGGL(mae_recon_rows_kernel<float>, dim3((unsigned)cdiv(rows, 4)), dim3(256), 0, s, rows, (int)P,
                       (int)Lk, (int)C, (int)S, (int)patch, pred, ld_pred, pixels, ids_restore, 1.0 / (K * n_masked),
                       row_loss, (float*)d_pred, ld_dpred);
  else
    hipLaunchKernelGGL(mae_recon_rows_kernel<bf16_t>, dim3((unsigned)cdiv(rows, 4)), dim3(256), 0, s, rows, (int)P,
                       (int)Lk, (int)C, (int)S, (int)patch, pred, ld_pred, pixels, ids_restore, 1.0 / (K * n_masked),
                       row_loss, (bf16_t*)d_pred, ld_dpred);
  VS_LAUNCH_CHECK();
  hipLaunchKernelGGL(mae_recon_final_kernel, dim3(1), dim3(256), 0, s, G * P, row_loss, 1.0 / n_masked, loss);
  VS_LAUNCH_CHECK();
  return VS_OK;
}
