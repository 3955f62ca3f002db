// bn3d.hip — BatchNorm3d of the R3D-18 encoder (statistics merge, apply + residual + ReLU, backward) and
// the encoder's layout and pooling helpers.  They share the VS_TIMER_BN class and nothing with the
// convolutions (conv_igemm.hip, conv_dw.hip), whose forward epilogue writes the statistics partials
// merged here.
#include "common.h"

namespace vs {

// ------------------------------------------------------------------------------------------------
// BatchNorm3d
// ------------------------------------------------------------------------------------------------
// The partials are per 128-row tile t (rows [128 t, min(128 t + 128, count))): S_t = sum y and
// M2_t = sum (y - S_t / n_t)^2.  Merged in f64 in a fixed order with Chan's formula: over a set of
// tiles, S = sum S_t, mean = S / n, M2 = sum M2_t + sum n_t (S_t / n_t - mean)^2.
constexpr int kBnTile = 128;
__device__ __forceinline__ double bn_tile_n(int64_t t, int64_t count) {
  const int64_t r = count - t * kBnTile;
  return (double)(r < kBnTile ? r : kBnTile);
}
// the four thread groups' sums of channel l, added in group order
__device__ __forceinline__ double group_sum4(const double (&red)[4][64], int l) {
  return ((red[0][l] + red[1][l]) + red[2][l]) + red[3][l];
}

// level 1: tiles [r0, r0 + 256) of the [rows][2][C] partials, 64 channels per block -> (S_b, M2_b)
__global__ __launch_bounds__(256) void bn_stats_l1(const float* __restrict__ part, int64_t rows, int C,
                                                   int64_t count, double* __restrict__ out) {
  __shared__ double red[2][4][64];
  __shared__ double mean_b[64];
  const int l = threadIdx.x & 63, c = blockIdx.y * 64 + l, grp = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * 256;
  const int64_t r1 = r0 + 256 < rows ? r0 + 256 : rows;
  double s = 0.0;
  if (c < C)
    for (int64_t r = r0 + grp; r < r1; r += 4) s += (double)part[(r * 2) * C + c];
  red[0][grp][l] = s;
  __syncthreads();
  if (grp == 0) {
    const double n_b = fmin((double)(r1 - r0) * kBnTile, (double)(count - r0 * kBnTile));
    mean_b[l] = group_sum4(red[0], l) / n_b;
  }
  __syncthreads();
  const double mu = mean_b[l];
  double q = 0.0;
  if (c < C)
    for (int64_t r = r0 + grp; r < r1; r += 4) {
      const double n_t = bn_tile_n(r, count);
      const double d = (double)part[(r * 2) * C + c] / n_t - mu;
      q += (double)part[(r * 2 + 1) * C + c] + n_t * d * d;
    }
  red[1][grp][l] = q;
  __syncthreads();
  if (grp == 0 && c < C) {
    out[((int64_t)blockIdx.x * 2) * C + c] = group_sum4(red[0], l);
    out[((int64_t)blockIdx.x * 2 + 1) * C + c] = group_sum4(red[1], l);
  }
}

__global__ __launch_bounds__(256) void bn_stats_l2(const double* __restrict__ l1, int nblk, int C, int64_t count,
                                                   const float* __restrict__ gamma, const float* __restrict__ beta,
                                                   float eps, float momentum, float* mean, float* rstd, float* scale,
                                                   float* shift, float* rmean, float* rvar) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  double s = 0.0;
  for (int b = 0; b < nblk; ++b) s += l1[((int64_t)b * 2) * C + c];
  const double mu = s / (double)count;
  double m2 = 0.0;
  for (int b = 0; b < nblk; ++b) {   // block b holds tiles [256 b, 256 b + 256): rows [32768 b, ...)
    const int64_t rem = count - (int64_t)b * 256 * kBnTile;
    const double n_b = (double)(rem < 256 * kBnTile ? rem : 256 * kBnTile);
    const double d = l1[((int64_t)b * 2) * C + c] / n_b - mu;
    m2 += l1[((int64_t)b * 2 + 1) * C + c] + n_b * d * d;
  }
  double var = m2 / (double)count;
  if (var < 0.0) var = 0.0;
  const float rs = (float)(1.0 / sqrt(var + (double)eps));
  mean[c] = (float)mu;
  rstd[c] = rs;
  const float sc = gamma[c] * rs;
  scale[c] = sc;
  shift[c] = beta[c] - (float)mu * sc;
  if (rmean) rmean[c] = (1.f - momentum) * rmean[c] + momentum * (float)mu;
  if (rvar) {
    const double unb = count > 1 ? var * (double)count / (double)(count - 1) : var;
    rvar[c] = (1.f - momentum) * rvar[c] + momentum * (float)unb;
  }
}

__global__ __launch_bounds__(256) void bn_apply_kernel(int64_t n4, int C, const float4* __restrict__ y,
                                                       const float* __restrict__ scale,
                                                       const float* __restrict__ shift,
                                                       const float4* __restrict__ res, int relu,
                                                       float4* __restrict__ out) {
  // the grid stride (gridDim * 1024 floats) is a multiple of C (the host checks it), so a thread's
  // channel offset is loop-invariant: no 64-bit modulo per element
  const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c = (int)((i0 * 4) % C);
  const float4 a = *(const float4*)(scale + c), b = *(const float4*)(shift + c);
  for (int64_t i = i0; i < n4; i += (int64_t)gridDim.x * 256) {
    float4 v = y[i];
    v.x = fmaf(v.x, a.x, b.x); v.y = fmaf(v.y, a.y, b.y); v.z = fmaf(v.z, a.z, b.z); v.w = fmaf(v.w, a.w, b.w);
    if (res) {
      const float4 r = res[i];
      v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
    }
    if (relu) {
      v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);
    }
    out[i] = v;
  }
}

// the gradient that passes a ReLU: g where the activation's output is positive, else 0
__device__ __forceinline__ float4 relu_mask(float4 g, float4 out) {
  g.x = out.x > 0.f ? g.x : 0.f; g.y = out.y > 0.f ? g.y : 0.f;
  g.z = out.z > 0.f ? g.z : 0.f; g.w = out.w > 0.f ? g.w : 0.f;
  return g;
}

// backward, pass 1: per block over a contiguous row range, per channel sum g and sum g xhat
// (g = dout masked by out > 0 under ReLU); partial rows [blocks][2][C] in f64.  The sums are kept in
// f64 from the first add: mean(g) and mean(g xhat) are subtracted from EVERY element's gradient, so
// their rounding is a coherent error that the next conv's weight-gradient sum over ~10^6 voxels
// accumulates instead of averaging out (f32 running sums here put 6e-3 of the norm on layer1's dW
// at 16 clips, against 1e-3 at 2 clips: r05)
__global__ __launch_bounds__(256) void bn_bwd_reduce(int64_t M, int C, const float* __restrict__ dout,
                                                     const float* __restrict__ out, int relu,
                                                     const float* __restrict__ y, const float* __restrict__ mean,
                                                     const float* __restrict__ rstd, int64_t rows_per_blk,
                                                     double* __restrict__ part) {
  __shared__ double red[2][4][256];
  const int groups = C / 4;                  // float4 channel groups per row
  const int rpi = 256 / groups;              // rows per iteration (C <= 1024)
  const int t = threadIdx.x, cg = t % groups, ro = t / groups;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_blk;
  int64_t r1 = r0 + rows_per_blk;
  if (r1 > M) r1 = M;
  double s[4] = {0.0, 0.0, 0.0, 0.0}, q[4] = {0.0, 0.0, 0.0, 0.0};
  const float4 mu = *(const float4*)(mean + cg * 4), rs = *(const float4*)(rstd + cg * 4);
  // two rows per iteration, every load of both issued before the first f64 add (the adds stay in
  // row order r, r + rpi, ...)
  auto load = [&](int64_t r, float4& gv, float4& yv) {
    const int64_t i = r * C + cg * 4;
    gv = *(const float4*)(dout + i);
    if (relu) gv = relu_mask(gv, *(const float4*)(out + i));
    yv =*(const float4*)(y + i);
  };
  auto acc = [&](const float4& gv, const float4& yv) {
    s[0] += gv.x; s[1] += gv.y; s[2] += gv.z; s[3] += gv.w;
    q[0] += (double)gv.x * ((yv.x - mu.x) * rs.x);
    q[1] += (double)gv.y * ((yv.y - mu.y) * rs.y);
    q[2] += (double)gv.z * ((yv.z - mu.z) * rs.z);
    q[3] += (double)gv.w * ((yv.w - mu.w) * rs.w);
  };
  if (ro < rpi) {
    int64_t r = r0 + ro;
    for (; r + rpi < r1; r += 2 * rpi) {
      float4 g0, y0, g1, y1;
      load(r, g0, y0);
      load(r + rpi, g1, y1);
      acc(g0, y0);
      acc(g1, y1);
    }
    if (r < r1) {
      float4 g0, y0;
      load(r, g0, y0);
      acc(g0, y0);
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    red[0][k][t] = s[k];
    red[1][k][t] = q[k];
  }
  __syncthreads();
  if (t < groups) {       // fixed order over the row offsets
    double a[4], b[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      a[k] = red[0][k][t];
      b[k] = red[1][k][t];
    }
    for (int o = 1; o < rpi; ++o)
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        a[k] += red[0][k][o * groups + t];
        b[k] += red[1][k][o * groups + t];
      }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      part[((int64_t)blockIdx.x * 2) * C + t * 4 + k] = a[k];
      part[((int64_t)blockIdx.x * 2 + 1) * C + t * 4 + k] = b[k];
    }
  }
}

// pass 2: per channel the totals (f64, block order), dgamma / dbeta (+=), and the apply coefficients
// coef[0][c] = gamma rstd, coef[1][c] = gamma rstd mean(g), coef[2][c] = gamma rstd mean(g xhat)
// 64 channels per workgroup, the partial rows split over 16 thread groups (rows b = grp mod 16, in
// order) and the 16 group sums added in a fixed order: one thread per channel walking all the rows was
// a 116-us latency chain per call (r05 rocprof)
__global__ __launch_bounds__(1024) void bn_bwd_finalize(const double* __restrict__ part, int nblk, int C, int64_t M,
                                                        const float* __restrict__ gamma, const float* __restrict__ rstd,
                                                        float* dgamma, float* dbeta, float* __restrict__ coef,
                                                        int batch_stats) {
  constexpr int NG = 16;  // thread groups over the partial rows (rows b = grp mod NG, in order)
  __shared__ double red[2][NG][64];
  const int l = threadIdx.x & 63, grp = threadIdx.x >> 6, c = blockIdx.x * 64 + l;
  double s0 = 0.0, q0 = 0.0;
  if (c < C) {
    int b = grp;
    for (; b + 7 * NG < nblk; b += 8 * NG) {  // 8 rows' loads in flight, added in row order
      double vs[8], vq[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        vs[u] = part[((int64_t)(b + u * NG) * 2) * C + c];
        vq[u] = part[((int64_t)(b + u * NG) * 2 + 1) * C + c];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        s0 += vs[u];
        q0 += vq[u];
      }
    }
    for (; b < nblk; b += NG) {
      s0 += part[((int64_t)b * 2) * C + c];
      q0 += part[((int64_t)b * 2 + 1) * C + c];
    }
  }
  red[0][grp][l] = s0;
  red[1][grp][l] = q0;
  __syncthreads();
  if (grp != 0 || c >= C) return;
  double s = red[0][0][l], q = red[1][0][l];
#pragma unroll
  for (int k = 1; k < NG; ++k) {
    s += red[0][k][l];
    q += red[1][k][l];
  }
  if (dgamma) dgamma[c] += (float)q;
  if (dbeta) dbeta[c] += (float)s;
  const double a = (double)gamma[c] * (double)rstd[c];
  coef[c] = (float)a;
  // batch statistics (training mode): the mean and xhat terms of d(batch mean, batch var); running
  // statistics (eval mode) are constants, so dy = gamma rstd g
  coef[C + c] = batch_stats ? (float)(a * (s / (double)M)) : 0.f;
  coef[2 * C + c] = batch_stats ? (float)(a * (q / (double)M)) : 0.f;
}

// pass 3: dy = a g - b - c xhat;  dres = g
__global__ __launch_bounds__(256) void bn_bwd_apply(int64_t n4, int C, const float4* __restrict__ dout,
                                                    const float4* __restrict__ out, int relu,
                                                    const float4* __restrict__ y, const float* __restrict__ mean,
                                                    const float* __restrict__ rstd, const float* __restrict__ coef,
                                                    float4* __restrict__ dy, float4* __restrict__ dres) {
  const int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x;  // loop-invariant channel (as bn_apply_kernel)
  const int c = (int)((i0 * 4) % C);
  const float4 mu = *(const float4*)(mean + c), rs = *(const float4*)(rstd + c);
  const float4 a = *(const float4*)(coef + c), b = *(const float4*)(coef + C + c),
               cc = *(const float4*)(coef + 2 * C + c);
  for (int64_t i = i0; i < n4; i += (int64_t)gridDim.x * 256) {
    float4 gv = dout[i];
    if (relu) gv = relu_mask(gv, out[i]);
    if (dres) dres[i] = gv;
    const float4 yv = y[i];
    float4 o;
    o.x = fmaf(a.x, gv.x, -b.x) - cc.x * ((yv.x - mu.x) * rs.x);
    o.y = fmaf(a.y, gv.y, -b.y) - cc.y * ((yv.y - mu.y) * rs.y);
    o.z = fmaf(a.z, gv.z, -b.z) - cc.z * ((yv.z - mu.z) * rs.z);
    o.w = fmaf(a.w, gv.w, -b.w) - cc.w * ((yv.w - mu.w) * rs.w);
    dy[i] = o;
  }
}

// ------------------------------------------------------------------------------------------------
// layout and pooling helpers
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void to_channels_last_kernel(int64_t vox, int64_t HW, int C, int Cp,
                                                               const float* __restrict__ x,
                                                               float* __restrict__ out) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;  // voxel index over (B, T, H, W)
  if (v >= vox) return;
  const int64_t bt = v / HW, hw = v % HW;
  float o[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) o[c] = c < C ? x[(bt * C + c) * HW + hw] : 0.f;
  float* dst = out + v * Cp;
  *(float4*)dst = make_float4(o[0], o[1], o[2], o[3]);
  if (Cp == 8) *(float4*)(dst + 4) = make_float4(o[4], o[5], o[6], o[7]);
}

__global__ __launch_bounds__(256) void avgpool_kernel(int64_t S, int C, const float* __restrict__ x,
                                                      float* __restrict__ pooled) {
  const int n = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const float* p = x + (int64_t)n * S * C + c;
  float s = 0.f;
  for (int64_t i = 0; i < S; ++i) s += p[i * C];
  pooled[(int64_t)n * C + c] = s / (float)S;
}

__global__ __launch_bounds__(256) void avgpool_bwd_kernel(int64_t total, int64_t S, int C,
                                                          const float* __restrict__ dpool, float* __restrict__ dx) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C);
  const int64_t n = i / ((int64_t)S * C);
  dx[i] = dpool[n * C + c] / (float)S;
}

}  // namespace vs

using namespace vs;

extern "C" size_t vs_bn3d_stats_workspace_bytes(int64_t rows, int64_t C) {
  return (size_t)((rows + 255) / 256) * 2 * C * sizeof(double) + 256;
}

extern "C" int vs_bn3d_stats(int64_t rows, int64_t C, const float* part, int64_t count, const float* gamma,
                             const float* beta, float eps, float momentum, float* mean, float* rstd, float* scale,
                             float* shift, float* running_mean, float* running_var, void* workspace, void* stream) {
  VS_REQUIRE(part && gamma && beta && mean && rstd && scale && shift && workspace, "vs_bn3d_stats: null pointer");
  VS_REQUIRE(rows > 0 && C > 0 && count > 0 && C % 4 == 0 && (count + kBnTile - 1) / kBnTile == rows,
             "vs_bn3d_stats: bad extents (rows = ceil(count / 128) tiles)");
  hipStream_t s = (hipStream_t)stream;
  ScopedTimer timer(VS_TIMER_BN, s, (double)rows * 2.0 * (double)C * 4.0);
  const int64_t nblk = (rows + 255) / 256;
  double* l1 = (double*)workspace;   // level-1 f64 partial sums [nblk][2][C]
  hipLaunchKernelGGL(bn_stats_l1, dim3((unsigned)nblk, (unsigned)((C + 63) / 64)), dim3(256), 0, s, part, rows,
                     (int)C, count, l1);
  VS_LAUNCH_CHECK();
  hipLaunchKernelGGL(bn_stats_l2, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, (const double*)l1, (int)nblk,
                     (int)C, count, gamma, beta, eps, momentum, mean, rstd, scale, shift, running_mean, running_var);
  VS_LAUNCH_CHECK();
  return VS_OK;
}

namespace vs {
// ~8K elements per workgroup (<= 2,048 partial rows): the old rows-only rule (1,024 rows per block,
// <= 512 blocks) gave the deep layers 4-196 workgroups with 128-392 serial row steps per thread
// (bn_bwd_reduce averaged 219 us per call at C4, 3.4x its bytes at the apply pass's rate)
static int64_t bn_bwd_blocks(int64_t M, int64_t C) {
  const int64_t b = (M * C + 8191) / 8192;
  return b < 2048 ? (b > 0 ? b : 1) : 2048;
}
// grid of the elementwise BN passes: <= 4096 workgroups, and a stride (blocks x 1024 floats) that is
// a multiple of C so each thread's channel offset is fixed (C <= 1024 divides 1024, or 1 round)
static int64_t bn_ew_blocks(int64_t n4, int64_t C) {
  const int64_t need = (n4 + 255) / 256;
  if (need <= 4096) return need;
  int64_t b = 4096;
  while (b > 1 && (b * 1024) % C != 0) --b;
  return b;
}
}  // namespace vs

extern "C" int vs_bn3d_apply(int64_t M, int64_t C, const float* y, const float* scale, const float* shift,
                             const float* residual, int32_t relu, float* out, void* stream) {
  VS_REQUIRE(y && scale && shift && out, "vs_bn3d_apply: null pointer");
  VS_REQUIRE(C % 4 == 0 && aligned16(y) && aligned16(out) && (!residual || aligned16(residual)) && aligned16(scale) &&
                 aligned16(shift),
             "vs_bn3d_apply: C % 4 == 0 and 16-byte aligned pointers");
  if (M <= 0) return VS_OK;
  hipStream_t s = (hipStream_t)stream;
  ScopedTimer timer(VS_TIMER_BN, s, (double)M * C * (residual ? 12.0 : 8.0));
  const int64_t n4 = M * C / 4;
  const int64_t blocks = bn_ew_blocks(n4, C);
  hipLaunchKernelGGL(bn_apply_kernel, dim3((unsigned)blocks), dim3(256), 0, s, n4, (int)C, (const float4*)y, scale,
                     shift, (const float4*)residual, relu, (float4*)out);
  VS_LAUNCH_CHECK();
  return VS_OK;
}


extern "C" size_t vs_bn3d_bwd_workspace_bytes(int64_t M, int64_t C) {
  return (size_t)bn_bwd_blocks(M, C) * 2 * C * 8 + (size_t)3 * C * 4 + 256;
}

static int bn3d_bwd(int64_t M, int64_t C, const float* dout, const float* out, int32_t relu, const float* y,
                    const float* mean, const float* rstd, const float* gamma, float* dy, float* dres, float* dgamma,
                    float* dbeta, void* workspace, void* stream, int batch_stats) {
  VS_REQUIRE(dout && y && mean && rstd && gamma && dy && workspace && (!relu || out), "vs_bn3d_bwd: null pointer");
  VS_REQUIRE(C % 4 == 0 && C <= 1024 && aligned16(dout) && aligned16(y) && aligned16(dy) &&
                 (!out || aligned16(out)) && (!dres || aligned16(dres)) && aligned16(workspace),
             "vs_bn3d_bwd: C % 4 == 0, C <= 1024, 16-byte aligned pointers");
  if (M <= 0) return VS_OK;
  hipStream_t s = (hipStream_t)stream;
  ScopedTimer timer(VS_TIMER_BN, s, (double)M * C * (4.0 * (relu ? 3 : 2) + 4.0 + (dres ? 4.0 : 0.0)));
  const int64_t nblk = bn_bwd_blocks(M, C);
  const int64_t rpb = (M + nblk - 1) / nblk;
  double* part = (double*)workspace;
  float* coef = (float*)(part + nblk * 2 * C);
  hipLaunchKernelGGL(bn_bwd_reduce, dim3((unsigned)nblk), dim3(256), 0, s, M, (int)C, dout, out, relu, y, mean, rstd,
                     rpb, part);
  VS_LAUNCH_CHECK();
  hipLaunchKernelGGL(bn_bwd_finalize, dim3((unsigned)((C + 63) / 64)), dim3(1024), 0, s, (const double*)part,
                     (int)nblk, (int)C, M, gamma, rstd, dgamma, dbeta, coef, batch_stats);
  VS_LAUNCH_CHECK();
  const int64_t n4 = M * C / 4;
  const int64_t blocks = bn_ew_blocks(n4, C);
  hipLaunchKernelGGL(bn_bwd_apply, dim3((unsigned)blocks), dim3(256), 0, s, n4, (int)C, (const float4*)dout,
                     (const float4*)out, relu, (const float4*)y, mean, rstd, (const float*)coef, (float4*)dy,
                     (float4*)dres);
  VS_LAUNCH_CHECK();
  return VS_OK;
}

extern "C" int vs_bn3d_bwd(int64_t M, int64_t C, const float* dout, const float* out, int32_t relu, const float* y,
                           const float* mean, const float* rstd, const float* gamma, float* dy, float* dres,
                           float* dgamma, float* dbeta, void* workspace, void* stream) {
  return bn3d_bwd(M, C, dout, out, relu, y, mean, rstd, gamma, dy, dres, dgamma, dbeta, workspace, stream, 1);
}

extern "C" int vs_bn3d_bwd_eval(int64_t M, int64_t C, const float* dout, const float* out, int32_t relu,
                                const float* y, const float* mean, const float* rstd, const float* gamma, float* dy,
                                float* dres, float* dgamma, float* dbeta, void* workspace, void* stream) {
  return bn3d_bwd(M, C, dout, out, relu, y, mean, rstd, gamma, dy, dres, dgamma, dbeta, workspace, stream, 0);
}

extern "C" int vs_to_channels_last(int64_t B, int64_t T, int64_t C, int64_t H, int64_t W, int64_t Cp, const float* x,
                                   float* out, void* stream) {
  VS_REQUIRE(x && out && aligned16(out), "vs_to_channels_last: null / misaligned pointer");
  VS_REQUIRE(C >= 1 && C <= Cp && (Cp == 4 || Cp == 8), "vs_to_channels_last: C <= Cp, Cp = 4 or 8");
  hipStream_t s = (hipStream_t)stream;
  ScopedTimer timer(VS_TIMER_BN, s, (double)B * T * H * W * (C + Cp) * 4.0);
  const int64_t vox = B * T * H * W;
  hipLaunchKernelGGL(to_channels_last_kernel, dim3((unsigned)((vox + 255) / 256)), dim3(256), 0, s, vox, H * W,
                     (int)C, (int)Cp, x, out);
  VS_LAUNCH_CHECK();
  return VS_OK;
}

extern "C" int vs_avgpool3d(int64_t N, int64_t S, int64_t C, const float* x, float* pooled, void* stream) {
  VS_REQUIRE(x && pooled && N > 0 && S > 0 && C > 0, "vs_avgpool3d: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  ScopedTimer timer(VS_TIMER_BN, s, (double)N * S * C * 4.0);
  hipLaunchKernelGGL(avgpool_kernel, dim3((unsigned)((C + 255) / 256), (unsigned)N), dim3(256), 0, s, S, (int)C, x,
                     pooled);
  VS_LAUNCH_CHECK();
  return VS_OK;
}

extern "C" int vs_avgpool3d_bwd(int64_t N, int64_t S, int64_t C, const float* dpool, float* dx, void* stream) {
  VS_REQUIRE(dpool && dx && N > 0 && S > 0 && C > 0, "vs_avgpool3d_bwd: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  ScopedTimer timer(VS_TIMER_BN, s, (double)N * S * C * 4.0);
  const int64_t total = N * S * C;
  hipLaunchKernelGGL(avgpool_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, total, S, (int)C,
                     dpool, dx);
  VS_LAUNCH_CHECK();
  return VS_OK;
}
