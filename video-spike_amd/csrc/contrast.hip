// contrast.hip — the ContrastViT plugin's pieces outside the block executor: the CLS
// token assembly of the 2-D patch embedding and its backward, the final LayerNorm -> projection ->
// L2-normalise head on the CLS row and its backward, and the InfoNCE loss with its gradients.
//
// All of it is small next to the blocks (the head touches one row of P + 1 per image; the loss works on
// n x m x E numbers), so the kernels are laid out for the memory system and for a FIXED summation order:
//   * streams (cls_embed_fwd / _bwd, the rows of embed_head_fwd / _bwd) move 16 bytes per lane per access; the
//     InfoNCE kernels do not: their rows are E floats (3 at the reference geometry), read as scalars, and for
//     d_ref only E lanes of a workgroup walk the m negatives — 9 KB in all, the call is launch latency;
//   * a workgroup's sum is: each lane adds its elements in ascending index order, the 64 lanes of a wave
//     are combined by the xor butterfly (offsets 32, 16, .., 1), and the four wave partials are added in
//     ascending wave order.  The order is a function of the reduced extent alone — never of G, the grid
//     or the other extents — and no atomics are used, so every output is bitwise reproducible;
//   * sums over images / reference rows (d_cls, dW_p, db_p, dgamma, dbeta, d_neg) are plain ascending
//     loops in one lane per output element.
// The InfoNCE row statistics and the loss parts are accumulated in f64 (the parts carry the detached
// shift c_i, which cancels in their sum: f32 partial sums would leave that cancellation to rounding).
#include "common.h"

namespace vs {

constexpr int kCtThreads = 256;
constexpr int kCtWaves = kCtThreads / 64;
constexpr int kMaxEmbed = 256;   // E: projection width
constexpr int kMaxHidden = 4096; // D: one f32 row in LDS

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}
// Sum over the 256 threads of a workgroup in the fixed order described above; every thread gets the
// result.  `part` holds kCtWaves values and may be reused after the call returns.
__device__ __forceinline__ float block_sum(float v, float* part) {
  v = wave_sum(v);
  __syncthreads();  // the previous use of `part` is over
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  float s = part[0];
#pragma unroll
  for (int w = 1; w < kCtWaves; ++w) s += part[w];
  return s;
}
__device__ __forceinline__ double block_sum_d(double v, double* part) {
  v = wave_sum_d(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = part[0];
#pragma unroll
  for (int w = 1; w < kCtWaves; ++w) s += part[w];
  return s;
}
__device__ __forceinline__ double block_max_d(double v, double* part) {
  v = wave_max_d(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = part[0];
#pragma unroll
  for (int w = 1; w < kCtWaves; ++w) s = fmax(s, part[w]);
  return s;
}

__device__ __forceinline__ uint2 pack_bf16x4(const float4& a) {
  uint2 u;
  u.x = (uint32_t)f2bf(a.x) | ((uint32_t)f2bf(a.y) << 16);
  u.y = (uint32_t)f2bf(a.z) | ((uint32_t)f2bf(a.w) << 16);
  return u;
}

// ---- CLS assembly ---------------------------------------------------------------------------------
// one lane per 4 channels of one row of x
__global__ __launch_bounds__(256) void cls_embed_fwd_kernel(int64_t total4, int64_t P, int64_t D4,
                                                            const float4* __restrict__ patches,
                                                            const float4* __restrict__ cls,
                                                            const float4* __restrict__ table, float4* __restrict__ x) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total4) return;
  const int64_t row = i / D4, c = i - row * D4;
  const int64_t g = row / (P + 1), t = row - g * (P + 1);
  float4 v;
  if (t == 0) {
    const float4 a = cls[c], b = table[c];
    v = float4{a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w};
  } else {
    v = patches[(g * P + t - 1) * D4 + c];
  }
  x[i] = v;
}

// rows 1..P of every image, compacted: one lane per 8 channels (two 16-byte loads; one 16-byte store of
// bf16, or two of f32)
template <typename T>
__global__ __launch_bounds__(256) void cls_embed_bwd_rows_kernel(int64_t total8, int64_t P, int64_t D8,
                                                                 const float* __restrict__ dx, T* __restrict__ dp) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total8) return;
  const int64_t row = i / D8, c = i - row * D8;  // row of the compact tensor
  const int64_t g = row / P, p = row - g * P;
  const float* src = dx + ((g * (P + 1) + 1 + p) * D8 + c) * 8;
  const float4 a = *(const float4*)src, b = *(const float4*)(src + 4);
  if constexpr (std::is_same<T, float>::value) {
    *(float4*)(dp + i * 8) = a;
    *(float4*)(dp + i * 8 + 4) = b;
  } else {
    const uint2 lo = pack_bf16x4(a), hi = pack_bf16x4(b);
    *(uint4*)(dp + i * 8) = uint4{lo.x, lo.y, hi.x, hi.y};
  }
}

// d_cls[d] = sum_g dx[g][0][d], ascending g: one lane per 4 channels
__global__ __launch_bounds__(64) void cls_embed_bwd_cls_kernel(int64_t G, int64_t row_stride4, int64_t D4,
                                                               const float4* __restrict__ dx,
                                                               float4* __restrict__ d_cls) {
  const int64_t c = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (c >= D4) return;
  float4 acc = {0.f, 0.f, 0.f, 0.f};
  const float4* p = dx + c;
  int64_t g = 0;
  for (; g + 4 <= G; g += 4, p += 4 * row_stride4) {  // 4 loads in flight, added in ascending g
    const float4 a = p[0], b = p[row_stride4], cc = p[2 * row_stride4], d = p[3 * row_stride4];
    acc.x += a.x; acc.y += a.y; acc.z += a.z; acc.w += a.w;
    acc.x += b.x; acc.y += b.y; acc.z += b.z; acc.w += b.w;
    acc.x += cc.x; acc.y += cc.y; acc.z += cc.z; acc.w += cc.w;
    acc.x += d.x; acc.y += d.y; acc.z += d.z; acc.w += d.w;
  }
  for (; g < G; ++g, p += row_stride4) {
    const float4 a = *p;
    acc.x += a.x; acc.y += a.y; acc.z += a.z; acc.w += a.w;
  }
  d_cls[c] = acc;
}

// ---- embedding head -------------------------------------------------------------------------------
// one workgroup per image
__global__ __launch_bounds__(kCtThreads) void embed_head_fwd_kernel(int64_t D, int E, const float* __restrict__ x,
                                                                    int64_t ldx, const float* __restrict__ gamma,
                                                                    const float* __restrict__ beta, float eps,
                                                                    const float* __restrict__ w,
                                                                    const float* __restrict__ b, float* __restrict__ h,
                                                                    float* __restrict__ mean, float* __restrict__ rstd,
                                                                    float* __restrict__ z_raw, float* __restrict__ nrm,
                                                                    float* __restrict__ z) {
  __shared__ __attribute__((aligned(16))) float row[kMaxHidden];
  __shared__ float zr[kMaxEmbed];
  __shared__ float part[kCtWaves];
  const int64_t g = blockIdx.x;
  const int tid = threadIdx.x;
  const float* xr = x + g * ldx;
  float s = 0.f;
  for (int64_t c = tid * 4; c < D; c += kCtThreads * 4) {
    const float4 v = *(const float4*)(xr + c);
    *(float4*)(row + c) = v;
    s += v.x; s += v.y; s += v.z; s += v.w;
  }
  const float mu = block_sum(s, part) / (float)D;
  float q = 0.f;
  for (int64_t c = tid * 4; c < D; c += kCtThreads * 4) {
    const float4 v = *(const float4*)(row + c);
    const float a0 = v.x - mu, a1 = v.y - mu, a2 = v.z - mu, a3 = v.w - mu;
    q += a0 * a0; q += a1 * a1; q += a2 * a2; q += a3 * a3;
  }
  const float rs = 1.0f / sqrtf(block_sum(q, part) / (float)D + eps);
  for (int64_t c = tid * 4; c < D; c += kCtThreads * 4) {
    const float4 v = *(const float4*)(row + c);
    const float4 ga = *(const float4*)(gamma + c), be = *(const float4*)(beta + c);
    const float4 o = {(v.x - mu) * rs * ga.x + be.x, (v.y - mu) * rs * ga.y + be.y, (v.z - mu) * rs * ga.z + be.z,
                      (v.w - mu) * rs * ga.w + be.w};
    *(float4*)(row + c) = o;  // each lane rewrites the elements it read
    *(float4*)(h + g * D + c) = o;
  }
  __syncthreads();
  // z_raw[e] = W[e] . h + b[e]: wave w takes e = w, w + 4, ..; lanes stride the row in 16-byte pieces
  const int wv = tid >> 6, lane = tid & 63;
  for (int e = wv; e < E; e += kCtWaves) {
    const float* we = w + (int64_t)e * D;
    float acc = 0.f;
    for (int64_t c = lane * 4; c < D; c += 64 * 4) {
      const float4 a = *(const float4*)(we + c), v = *(const float4*)(row + c);
      acc = fmaf(a.x, v.x, acc); acc = fmaf(a.y, v.y, acc); acc = fmaf(a.z, v.z, acc); acc = fmaf(a.w, v.w, acc);
    }
    acc = wave_sum(acc);
    if (lane == 0) zr[e] = acc + b[e];
  }
  __syncthreads();
  float ss = 0.f;
  for (int e = 0; e < E; ++e) ss = fmaf(zr[e], zr[e], ss);  // every lane: the same ascending sum
  const float nr = sqrtf(ss);
  if (tid < E) {
    z_raw[g * E + tid] = zr[tid];
    z[g * E + tid] = zr[tid] / nr;
  }
  if (tid == 0) {
    mean[g] = mu;
    rstd[g] = rs;
    nrm[g] = nr;
  }
}

// one workgroup per image: dz -> dz_raw -> dh -> LayerNorm backward into row 0, zeros into rows 1..P
__global__ __launch_bounds__(kCtThreads) void embed_head_bwd_kernel(
    int64_t P, int64_t D, int E, const float* __restrict__ dz, const float* __restrict__ x, int64_t ldx,
    const float* __restrict__ mean, const float* __restrict__ rstd, const float* __restrict__ z_raw,
    const float* __restrict__ nrm, const float* __restrict__ gamma, const float* __restrict__ w,
    float* __restrict__ dx, bf16_t* __restrict__ dx_lp, float* __restrict__ ws_dzr, float* __restrict__ ws_dh) {
  __shared__ __attribute__((aligned(16))) float dxh[kMaxHidden];  // dh * gamma
  __shared__ __attribute__((aligned(16))) float xh[kMaxHidden];   // (x - mean) * rstd
  __shared__ float dzr[kMaxEmbed];
  __shared__ float part[kCtWaves];
  const int64_t g = blockIdx.x;
  const int tid = threadIdx.x;
  // the zero rows first: the stream that dominates the kernel's bytes
  {
    const int64_t n4 = P * D / 4;
    float4* q = (float4*)(dx + (g * (P + 1) + 1) * D);
    const float4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int64_t i = tid; i < n4; i += kCtThreads) q[i] = zero;
    if (dx_lp) {
      const int64_t n8 = P * D / 8;
      uint4* ql = (uint4*)(dx_lp + (g * (P + 1) + 1) * D);
      const uint4 zl = {0u, 0u, 0u, 0u};
      for (int64_t i = tid; i < n8; i += kCtThreads) ql[i] = zl;
    }
  }
  const float nr = nrm[g];
  if (tid < E) dzr[tid] = dz[g * E + tid];
  __syncthreads();
  float dot = 0.f;
  for (int e = 0; e < E; ++e) dot = fmaf(z_raw[g * E + e] / nr, dzr[e], dot);  // z . dz, ascending e in every lane
  __syncthreads();
  if (tid < E) {
    const float zv = z_raw[g * E + tid] / nr;
    const float v = (dz[g * E + tid] - zv * dot) / nr;
    dzr[tid] = v;
    if (ws_dzr) ws_dzr[g * E + tid] = v;
  }
  __syncthreads();
  const float mu = mean[g], rs = rstd[g];
  const float* xr = x + g * ldx;
  float s1 = 0.f, s2 = 0.f;
  for (int64_t c = tid * 4; c < D; c += kCtThreads * 4) {
    float4 dh = {0.f, 0.f, 0.f, 0.f};
    for (int e = 0; e < E; ++e) {  // dh = W^T dz_raw, ascending e
      const float4 a = *(const float4*)(w + (int64_t)e * D + c);
      const float d = dzr[e];
      dh.x = fmaf(a.x, d, dh.x); dh.y = fmaf(a.y, d, dh.y); dh.z = fmaf(a.z, d, dh.z); dh.w = fmaf(a.w, d, dh.w);
    }
    if (ws_dh) *(float4*)(ws_dh + g * D + c) = dh;
    const float4 ga = *(const float4*)(gamma + c), xv = *(const float4*)(xr + c);
    const float4 a = {dh.x * ga.x, dh.y * ga.y, dh.z * ga.z, dh.w * ga.w};
    const float4 n = {(xv.x - mu) * rs, (xv.y - mu) * rs, (xv.z - mu) * rs, (xv.w - mu) * rs};
    *(float4*)(dxh + c) = a;
    *(float4*)(xh + c) = n;
    s1 += a.x; s1 += a.y; s1 += a.z; s1 += a.w;
    s2 = fmaf(a.x, n.x, s2); s2 = fmaf(a.y, n.y, s2); s2 = fmaf(a.z, n.z, s2); s2 = fmaf(a.w, n.w, s2);
  }
  const float m1 = block_sum(s1, part) / (float)D;
  const float m2 = block_sum(s2, part) / (float)D;
  float* o = dx + g * (P + 1) * D;
  for (int64_t c = tid * 4; c < D; c += kCtThreads * 4) {  // each lane reads back what it wrote
    const float4 a = *(const float4*)(dxh + c), n = *(const float4*)(xh + c);
    const float4 r = {rs * (a.x - m1 - n.x * m2), rs * (a.y - m1 - n.y * m2), rs * (a.z - m1 - n.z * m2),
                      rs * (a.w - m1 - n.w * m2)};
    *(float4*)(o + c) = r;
    if (dx_lp) *(uint2*)(dx_lp + g * (P + 1) * D + c) = pack_bf16x4(r);
  }
}

// Parameter gradients, each a sum over images in ascending g, one lane per 4 channels:
// blockIdx.y < E: dw[e][c] = sum_g dz_raw[g][e] h[g][c] (and db[e] = sum_g dz_raw[g][e] in the lane of c = 0);
// blockIdx.y == E: dgamma[c] = sum_g dh[g][c] xhat[g][c], dbeta[c] = sum_g dh[g][c].
__global__ __launch_bounds__(64) void embed_head_param_kernel(int64_t G, int64_t D, int E, const float* __restrict__ x,
                                                              int64_t ldx, const float* __restrict__ h,
                                                              const float* __restrict__ mean,
                                                              const float* __restrict__ rstd,
                                                              const float* __restrict__ ws_dzr,
                                                              const float* __restrict__ ws_dh, float* __restrict__ dw,
                                                              float* __restrict__ db, float* __restrict__ dgamma,
                                                              float* __restrict__ dbeta) {
  const int64_t c = ((int64_t)blockIdx.x * 64 + threadIdx.x) * 4;
  if (c >= D) return;
  const int e = blockIdx.y;
  if (e < E) {
    float4 acc = {0.f, 0.f, 0.f, 0.f};
    float sb = 0.f;
#pragma unroll 4
    for (int64_t g = 0; g < G; ++g) {
      const float d = ws_dzr[g * E + e];
      const float4 v = *(const float4*)(h + g * D + c);
      acc.x = fmaf(d, v.x, acc.x); acc.y = fmaf(d, v.y, acc.y); acc.z = fmaf(d, v.z, acc.z); acc.w = fmaf(d, v.w, acc.w);
      sb += d;
    }
    *(float4*)(dw + (int64_t)e * D + c) = acc;
    if (c == 0) db[e] = sb;
  } else {
    float4 ag = {0.f, 0.f, 0.f, 0.f}, ab = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int64_t g = 0; g < G; ++g) {
      const float mu = mean[g], rs = rstd[g];
      const float4 d = *(const float4*)(ws_dh + g * D + c), v = *(const float4*)(x + g * ldx + c);
      ag.x = fmaf(d.x, (v.x - mu) * rs, ag.x); ag.y = fmaf(d.y, (v.y - mu) * rs, ag.y);
      ag.z = fmaf(d.z, (v.z - mu) * rs, ag.z); ag.w = fmaf(d.w, (v.w - mu) * rs, ag.w);
      ab.x += d.x; ab.y += d.y; ab.z += d.z; ab.w += d.w;
    }
    *(float4*)(dgamma + c) = ag;
    *(float4*)(dbeta + c) = ab;
  }
}

// ---- InfoNCE --------------------------------------------------------------------------------------
// workspace: prob [n, m] f32 (softmax of each reference row over the negatives), then stat [n, 4] f64:
// pos_dist_i, c_i, logsumexp_j(neg_dist_ij - c_i), sum_j softmax_ij neg_dist_ij
__host__ __device__ inline size_t nce_prob_bytes(int64_t n, int64_t m) {
  return (size_t)(((n * m * 4) + 15) / 16 * 16);
}

// one workgroup per reference row
__global__ __launch_bounds__(kCtThreads) void info_nce_row_kernel(int64_t n, int64_t m, int E,
                                                                  const float* __restrict__ ref,
                                                                  const float* __restrict__ pos,
                                                                  const float* __restrict__ neg,
                                                                  const float* __restrict__ log_inv_tau,
                                                                  float* __restrict__ prob, double* __restrict__ stat,
                                                                  float* __restrict__ d_ref, float* __restrict__ d_pos,
                                                                  float grad_scale) {
  __shared__ float r[kMaxEmbed];
  __shared__ double part[kCtWaves];
  const int64_t i = blockIdx.x;
  const int tid = threadIdx.x;
  const double inv_tau = log_inv_tau ? exp((double)*log_inv_tau) : 1.0;
  if (tid < E) r[tid] = ref[i * E + tid];
  __syncthreads();
  float* pr = prob + i * m;
  double mx = -INFINITY;
  for (int64_t j = tid; j < m; j += kCtThreads) {
    const float* nj = neg + j * E;
    double acc = 0.0;
    for (int e = 0; e < E; ++e) acc = fma((double)r[e], (double)nj[e], acc);
    acc *= inv_tau;
    mx = fmax(mx, acc);
  }
  const double c = block_max_d(mx, part);
  // second pass: the distances again (n*m*E products are cheaper than an f64 round trip through memory);
  // each lane normalises below the entries it wrote here
  double se = 0.0, sw = 0.0;
  for (int64_t j = tid; j < m; j += kCtThreads) {
    const float* nj = neg + j * E;
    double acc = 0.0;
    for (int e = 0; e < E; ++e) acc = fma((double)r[e], (double)nj[e], acc);
    acc *= inv_tau;
    const double ex = exp(acc - c);
    se += ex;
    sw = fma(ex, acc, sw);
    pr[j] = (float)ex;
  }
  const double tot = block_sum_d(se, part);
  const double wsum = block_sum_d(sw, part);
  for (int64_t j = tid; j < m; j += kCtThreads) pr[j] = (float)((double)pr[j] / tot);
  if (tid == 0) {
    double pd = 0.0;
    for (int e = 0; e < E; ++e) pd = fma((double)r[e], (double)pos[i * E + e], pd);
    stat[i * 4 + 0] = pd * inv_tau;
    stat[i * 4 + 1] = c;
    stat[i * 4 + 2] = log(tot);
    stat[i * 4 + 3] = wsum / tot;
  }
  __syncthreads();  // pr[] of this row is complete (written by this workgroup)
  const float k = (float)((double)grad_scale * inv_tau / (double)n);
  if (tid < E) {
    if (d_ref) {
      float acc = 0.f;
      for (int64_t j = 0; j < m; ++j) acc = fmaf(pr[j], neg[j * E + tid], acc);  // ascending j
      d_ref[i * E + tid] = k * (acc - pos[i * E + tid]);
    }
    if (d_pos) d_pos[i * E + tid] = -k * r[tid];
  }
}

// one workgroup: the three losses and d_log_inv_tau from the row statistics
__global__ __launch_bounds__(kCtThreads) void info_nce_final_kernel(int64_t n, const double* __restrict__ stat,
                                                                    float* __restrict__ out,
                                                                    float* __restrict__ d_log_inv_tau) {
  __shared__ double part[kCtWaves];
  double sp = 0.0, sn = 0.0, spd = 0.0, sw = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += kCtThreads) {
    const double pd = stat[i * 4], c = stat[i * 4 + 1];
    sp += pd - c;
    sn += stat[i * 4 + 2];
    spd += pd;
    sw += stat[i * 4 + 3];
  }
  sp = block_sum_d(sp, part);
  sn = block_sum_d(sn, part);
  spd = block_sum_d(spd, part);
  sw = block_sum_d(sw, part);
  if (threadIdx.x == 0) {
    const double pl = -sp / (double)n, nl = sn / (double)n;
    out[0] = (float)(pl + nl);
    out[1] = (float)pl;
    out[2] = (float)nl;
    if (d_log_inv_tau) *d_log_inv_tau = (float)((sw - spd) / (double)n);
  }
}

// d_neg[j][e] = k * sum_i softmax_ij ref[i][e], ascending i: one lane per element
__global__ __launch_bounds__(256) void info_nce_dneg_kernel(int64_t n, int64_t m, int E, const float* __restrict__ ref,
                                                            const float* __restrict__ prob,
                                                            const float* __restrict__ log_inv_tau, float grad_scale,
                                                            float* __restrict__ d_neg) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= m * E) return;
  const int64_t j = t / E;
  const int e = (int)(t - j * E);
  const double inv_tau = log_inv_tau ? exp((double)*log_inv_tau) : 1.0;
  const float k = (float)((double)grad_scale * inv_tau / (double)n);
  float acc = 0.f;
#pragma unroll 4
  for (int64_t i = 0; i < n; ++i) acc = fmaf(prob[i * m + j], ref[i * E + e], acc);
  d_neg[t] = k * acc;
}

}  // namespace vs

using namespace vs;

extern "C" int vs_cls_embed_fwd(int64_t G, int64_t P, int64_t D, const float* patches, const float* cls,
                                const float* table, float* x, void* stream) {
  VS_REQUIRE(patches && cls && table && x, "vs_cls_embed_fwd: null pointer");
  VS_REQUIRE(G > 0 && P > 0 && D > 0, "vs_cls_embed_fwd: G, P and D must be positive");
  VS_REQUIRE(D % 8 == 0, "vs_cls_embed_fwd: D must be a multiple of 8");
  VS_REQUIRE(aligned16(patches) && aligned16(cls) && aligned16(table) && aligned16(x),
             "vs_cls_embed_fwd: pointers must be 16-byte aligned");
  const int64_t total4 = G * (P + 1) * (D / 4);
  VS_REQUIRE(G <= INT32_MAX / ((P + 1) * (D / 4)) && cdiv(total4, 256) <= INT32_MAX,
             "vs_cls_embed_fwd: G * (P + 1) * D exceeds the grid limit");
  hipStream_t s = (hipStream_t)stream;
  ScopedTimer timer(VS_TIMER_MISC, s, 4.0 * D * ((double)G * P + (double)G * (P + 1) + 2.0));
  count_path(VS_PATH_CLS_EMBED);
  hipLaunchKernelGGL(cls_embed_fwd_kernel, dim3((unsigned)cdiv(total4, 256)), dim3(256), 0, s, total4, P, D / 4,
                     (const float4*)patches, (const float4*)cls, (const float4*)table, (float4*)x);
  VS_LAUNCH_CHECK();
  return VS_OK;
}

extern "C" int vs_cls_embed_bwd(int32_t out_dtype, int64_t G, int64_t P, int64_t D, const float* dx, float* d_cls,
                                void* d_patches, void* stream) {
  VS_REQUIRE(out_dtype == VS_F32 || out_dtype == VS_BF16, "vs_cls_embed_bwd: out dtype must be f32 or bf16");
  VS_REQUIRE(dx && d_cls && d_patches, "vs_cls_embed_bwd: null pointer");
  VS_REQUIRE(G > 0 && P > 0 && D > 0, "vs_cls_embed_bwd: G, P and D must be positive");
  VS_REQUIRE(D % 8 == 0, "vs_cls_embed_bwd: D must be a multiple of 8");
  VS_REQUIRE(aligned16(dx) && aligned16(d_cls) && aligned16(d_patches),
             "vs_cls_embed_bwd: pointers must be 16-byte aligned");
  const int64_t total8 = G * P * (D / 8);
  VS_REQUIRE(G <= INT32_MAX / ((P + 1) * (D / 4)) && cdiv(total8, 256) <= INT32_MAX,
             "vs_cls_embed_bwd: G * (P + 1) * D exceeds the grid limit");
  hipStream_t s = (hipStream_t)stream;
  ScopedTimer timer(VS_TIMER_MISC, s,
                    (double)G * D * 4.0 + D * 4.0 + (double)G * P * D * (4.0 + (double)esize(out_dtype)));
  count_path(VS_PATH_CLS_EMBED);
  if (out_dtype == VS_F32)
    hipLaunchKernelGGL(cls_embed_bwd_rows_kernel<float>, dim3((unsigned)cdiv(total8, 256)), dim3(256), 0, s, total8, P,
                       D / 8, dx, (float*)d_patches);
  else
    hipLaunchKernelGGL(cls_embed_bwd_rows_kernel<bf16_t>, dim3((unsigned)cdiv(total8, 256)), dim3(256), 0, s, total8,
                       P, D / 8, dx, (bf16_t*)d_patches);
  VS_LAUNCH_CHECK();
  hipLaunchKernelGGL(cls_embed_bwd_cls_kernel, dim3((unsigned)cdiv(D / 4, 64)), dim3(64), 0, s, G, (P + 1) * (D / 4),
                     D / 4, (const float4*)dx, (float4*)d_cls);
  VS_LAUNCH_CHECK();
  return VS_OK;
}

extern "C" int vs_embed_head_fwd(int64_t G, int64_t D, int64_t E, const float* x, int64_t ldx, const float* gamma,
                                 const float* beta, float eps, const float* w, const float* b, float* h, float* mean,
                                 float* rstd, float* z_raw, float* nrm, float* z, void* stream) {
  VS_REQUIRE(x && gamma && beta && w && b && h && mean && rstd && z_raw && nrm && z,
             "vs_embed_head_fwd: null pointer");
  VS_REQUIRE(G > 0 && G <= INT32_MAX && D > 0, "vs_embed_head_fwd: G and D must be positive");
  VS_REQUIRE(D % 8 == 0 && D <= kMaxHidden, "vs_embed_head_fwd: D must be a multiple of 8, at most 4096");
  VS_REQUIRE(E >= 1 && E <= kMaxEmbed, "vs_embed_head_fwd: E must be in 1..256");
  VS_REQUIRE(ldx >= D && ldx % 4 == 0, "vs_embed_head_fwd: ldx >= D and ldx % 4 == 0");
  VS_REQUIRE(aligned16(x) && aligned16(gamma) && aligned16(beta) && aligned16(w) && aligned16(h),
             "vs_embed_head_fwd: pointers must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  ScopedTimer timer(VS_TIMER_MISC, s, 4.0 * ((double)G * (2.0 * D + 2.0 * E + 3.0) + 2.0 * D + (double)E * (D + 1)));
  count_path(VS_PATH_EMBED_HEAD);
  hipLaunchKernelGGL(embed_head_fwd_kernel, dim3((unsigned)G), dim3(kCtThreads), 0, s, D, (int)E, x, ldx, gamma, beta,
                     eps, w, b, h, mean, rstd, z_raw, nrm, z);
  VS_LAUNCH_CHECK();
  return VS_OK;
}

extern "C" size_t vs_embed_head_bwd_workspace_bytes(int64_t G, int64_t D, int64_t E) {
  if (G <= 0 || D <= 0 || E <= 0) return 0;
  return (size_t)(G * D * 4 + (G * E * 4 + 15) / 16 * 16);
}

extern "C" int vs_embed_head_bwd(int64_t G, int64_t P, int64_t D, int64_t E, const float* dz, const float* x,
                                 int64_t ldx, const float* h, const float* mean, const float* rstd, const float* z_raw,
                                 const float* nrm, const float* gamma, const float* w, float* dx, void* dx_lp,
                                 float* dw, float* db, float* dgamma, float* dbeta, void* workspace, void* stream) {
  VS_REQUIRE(dz && x && h && mean && rstd && z_raw && nrm && gamma && w && dx, "vs_embed_head_bwd: null pointer");
  const bool params = dw || db || dgamma || dbeta;
  VS_REQUIRE(!params || (dw && db && dgamma && dbeta && workspace),
             "vs_embed_head_bwd: dw, db, dgamma, dbeta and the workspace go together");
  VS_REQUIRE(G > 0 && G <= INT32_MAX && P > 0 && D > 0, "vs_embed_head_bwd: G, P and D must be positive");
  VS_REQUIRE(D % 8 == 0 && D <= kMaxHidden, "vs_embed_head_bwd: D must be a multiple of 8, at most 4096");
  VS_REQUIRE(E >= 1 && E <= kMaxEmbed, "vs_embed_head_bwd: E must be in 1..256");
  VS_REQUIRE(ldx >= D && ldx % 4 == 0, "vs_embed_head_bwd: ldx >= D and ldx % 4 == 0");
  VS_REQUIRE(aligned16(x) && aligned16(h) && aligned16(gamma) && aligned16(w) && aligned16(dx) && aligned16(dx_lp) &&
                 aligned16(dw) && aligned16(dgamma) && aligned16(dbeta) && aligned16(workspace),
             "vs_embed_head_bwd: pointers must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  float* ws_dh = params ? (float*)workspace : nullptr;
  float* ws_dzr = params ? ws_dh + G * D : nullptr;
  ScopedTimer timer(VS_TIMER_MISC, s,
                    (double)G * (P + 1) * D * (4.0 + (dx_lp ? 2.0 : 0.0)) + 4.0 * G * (D + 2.0 * E + 3.0) +
                        4.0 * D * (E + 1.0) + (params ? 4.0 * (G * D + (double)E * D + E + 2.0 * D) : 0.0));
  count_path(VS_PATH_EMBED_HEAD);
  hipLaunchKernelGGL(embed_head_bwd_kernel, dim3((unsigned)G), dim3(kCtThreads), 0, s, P, D, (int)E, dz, x, ldx, mean,
                     rstd, z_raw, nrm, gamma, w, dx, (bf16_t*)dx_lp, ws_dzr, ws_dh);
  VS_LAUNCH_CHECK();
  if (params) {
    hipLaunchKernelGGL(embed_head_param_kernel, dim3((unsigned)cdiv(D / 4, 64), (unsigned)(E + 1)), dim3(64), 0, s, G, D,
                       (int)E, x, ldx, h, mean, rstd, ws_dzr, ws_dh, dw, db, dgamma, dbeta);
    VS_LAUNCH_CHECK();
  }
  return VS_OK;
}

extern "C" size_t vs_info_nce_workspace_bytes(int64_t n, int64_t m) {
  if (n <= 0 || m <= 0) return 0;
  return nce_prob_bytes(n, m) + (size_t)n * 4 * sizeof(double);
}

extern "C" int vs_info_nce(int64_t n, int64_t m, int64_t E, const float* ref, const float* pos, const float* neg,
                           const float* log_inv_tau, float* out, float* d_ref, float* d_pos, float* d_neg,
                           float grad_scale, float* d_log_inv_tau, void* workspace, void* stream) {
  VS_REQUIRE(ref && pos && neg && out && workspace, "vs_info_nce: null pointer");
  VS_REQUIRE(n > 0 && m > 0, "vs_info_nce: n and m must be positive");
  VS_REQUIRE(E >= 1 && E <= kMaxEmbed, "vs_info_nce: E must be in 1..256");
  VS_REQUIRE(n <= INT32_MAX && m <= INT32_MAX / E && n <= INT64_MAX / 8 / m, "vs_info_nce: n, m exceed the grid limit");
  VS_REQUIRE(aligned16(workspace), "vs_info_nce: the workspace must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  float* prob = (float*)workspace;
  double* stat = (double*)((char*)workspace + nce_prob_bytes(n, m));
  ScopedTimer timer(VS_TIMER_MISC, s,
                    4.0 * E * (2.0 * n + m) + 12.0 + 4.0 * E * ((d_ref ? n : 0) + (d_pos ? n : 0) + (d_neg ? m : 0)));
  count_path(VS_PATH_INFO_NCE);
  hipLaunchKernelGGL(info_nce_row_kernel, dim3((unsigned)n), dim3(kCtThreads), 0, s, n, m, (int)E, ref, pos, neg,
                     log_inv_tau, prob, stat, d_ref, d_pos, grad_scale);
  VS_LAUNCH_CHECK();
  hipLaunchKernelGGL(info_nce_final_kernel, dim3(1), dim3(kCtThreads), 0, s, n, (const double*)stat, out,
                     d_log_inv_tau);
  VS_LAUNCH_CHECK();
  if (d_neg) {
    hipLaunchKernelGGL(info_nce_dneg_kernel, dim3((unsigned)cdiv(m * E, 256)), dim3(256), 0, s, n, m, (int)E, ref,
                       (const float*)prob, log_inv_tau, grad_scale, d_neg);
    VS_LAUNCH_CHECK();
  }
  return VS_OK;
}
