// attn_f32.hip — the exact-f32 (parity) attention kernels, head dim 64: 4 lanes per query / key row,
// K/V (or Q/dO) tiles in LDS, expf / logf in f32 (attn_common.h has the overview).
#include "attn_common.h"

namespace vs {

__global__ __launch_bounds__(256) void attn_fwd_f32_kernel(const float* __restrict__ qkv, int64_t ldq,
                                                           float* __restrict__ o, int64_t ldo, float* __restrict__ lse,
                                                           int N, int H, float scale) {
  __shared__ float sK[64][68];
  __shared__ float sV[64][68];
  const int tid = threadIdx.x, sub = tid & 3;
  const int qi = blockIdx.x * 64 + (tid >> 2);
  const int h = blockIdx.y, b = blockIdx.z, D = H * 64;
  const int64_t row0 = (int64_t)b * N;
  const float* Qp = qkv + row0 * ldq + h * 64;
  const float* Kp = Qp + D;
  const float* Vp = Qp + 2 * D;
  float q[16], acc[16];
#pragma unroll
  for (int d = 0; d < 16; ++d) {
    q[d] = qi < N ? Qp[(int64_t)qi * ldq + sub * 16 + d] : 0.f;
    acc[d] = 0.f;
  }
  float m = -INFINITY, l = 0.f;
  const int nkt = (N + 63) / 64;
  for (int kt = 0; kt < nkt; ++kt) {
    __syncthreads();
    for (int e = tid; e < 64 * 64; e += 256) {
      const int r = e >> 6, c = e & 63, gk = kt * 64 + r;
      sK[r][c] = gk < N ? Kp[(int64_t)gk * ldq + c] : 0.f;
      sV[r][c] = gk < N ? Vp[(int64_t)gk * ldq + c] : 0.f;
    }
    __syncthreads();
    float s[64];
    float mt = -INFINITY;
#pragma unroll
    for (int kk = 0; kk < 64; ++kk) {
      float part = 0.f;
#pragma unroll
      for (int d = 0; d < 16; ++d) part = fmaf(q[d], sK[kk][sub * 16 + d], part);
      part += __shfl_xor(part, 1, 64);
      part += __shfl_xor(part, 2, 64);
      s[kk] = (kt * 64 + kk < N) ? part * scale : -INFINITY;
      mt = fmaxf(mt, s[kk]);
    }
    const float mn = fmaxf(m, mt);
    const float alpha = expf(m - mn);
    l *= alpha;
#pragma unroll
    for (int d = 0; d < 16; ++d) acc[d] *= alpha;
#pragma unroll
    for (int kk = 0; kk < 64; ++kk) {
      const float p = expf(s[kk] - mn);
      l += p;
#pragma unroll
      for (int d = 0; d < 16; ++d) acc[d] = fmaf(p, sV[kk][sub * 16 + d], acc[d]);
    }
    m = mn;
  }
  if (qi < N) {
    const float inv = 1.f / l;
#pragma unroll
    for (int d = 0; d < 16; ++d) o[(row0 + qi) * ldo + h * 64 + sub * 16 + d] = acc[d] * inv;
    if (sub == 0) lse[((int64_t)b * H + h) * N + qi] = m + logf(l);
  }
}

__global__ __launch_bounds__(256) void attn_bwd_dkdv_f32_kernel(const float* __restrict__ qkv, int64_t ldq,
                                                                const float* __restrict__ dout, int64_t lddo,
                                                                const float* __restrict__ lse,
                                                                const float* __restrict__ delta,
                                                                float* __restrict__ dqkv, int64_t ldd, int N, int H,
                                                                float scale) {
  __shared__ float sQ[64][68];
  __shared__ float sD[64][68];
  __shared__ float sL[64], sDel[64];
  const int tid = threadIdx.x, sub = tid & 3;
  const int ki = blockIdx.x * 64 + (tid >> 2);
  const int h = blockIdx.y, b = blockIdx.z, D = H * 64;
  const int64_t row0 = (int64_t)b * N;
  const float* Qp = qkv + row0 * ldq + h * 64;
  const float* Kp = Qp + D;
  const float* Vp = Qp + 2 * D;
  const float* Dp = dout + row0 * lddo + h * 64;
  const float* L = lse + ((int64_t)b * H + h) * N;
  const float* Del = delta + ((int64_t)b * H + h) * N;
  float k[16], v[16], dk[16], dv[16];
#pragma unroll
  for (int d = 0; d < 16; ++d) {
    k[d] = ki < N ? Kp[(int64_t)ki * ldq + sub * 16 + d] : 0.f;
    v[d] = ki < N ? Vp[(int64_t)ki * ldq + sub * 16 + d] : 0.f;
    dk[d] = dv[d] = 0.f;
  }
  const int nqt = (N + 63) / 64;
  for (int qt = 0; qt < nqt; ++qt) {
    __syncthreads();
    for (int e = tid; e < 64 * 64; e += 256) {
      const int r = e >> 6, c = e & 63, gq = qt * 64 + r;
      sQ[r][c] = gq < N ? Qp[(int64_t)gq * ldq + c] : 0.f;
      sD[r][c] = gq < N ? Dp[(int64_t)gq * lddo + c] : 0.f;
    }
    if (tid < 64) {
      const int gq = qt * 64 + tid;
      sL[tid] = gq < N ? L[gq] : INFINITY;
      sDel[tid] = gq < N ? Del[gq] : 0.f;
    }
    __syncthreads();
    for (int qq = 0; qq < 64; ++qq) {
      float s = 0.f, dp = 0.f;
#pragma unroll
      for (int d = 0; d < 16; ++d) {
        s = fmaf(sQ[qq][sub * 16 + d], k[d], s);
        dp = fmaf(sD[qq][sub * 16 + d], v[d], dp);
      }
      s += __shfl_xor(s, 1, 64);
      s += __shfl_xor(s, 2, 64);
      dp += __shfl_xor(dp, 1, 64);
      dp += __shfl_xor(dp, 2, 64);
      const float p = expf(s * scale - sL[qq]);
      const float ds = p * (dp - sDel[qq]);
#pragma unroll
      for (int d = 0; d < 16; ++d) {
        dv[d] = fmaf(p, sD[qq][sub * 16 + d], dv[d]);
        dk[d] = fmaf(ds, sQ[qq][sub * 16 + d], dk[d]);
      }
    }
  }
  if (ki < N) {
#pragma unroll
    for (int d = 0; d < 16; ++d) {
      dqkv[(row0 + ki) * ldd + D + h * 64 + sub * 16 + d] = dk[d] * scale;
      dqkv[(row0 + ki) * ldd + 2 * D + h * 64 + sub * 16 + d] = dv[d];
    }
  }
}

__global__ __launch_bounds__(256) void attn_bwd_dq_f32_kernel(const float* __restrict__ qkv, int64_t ldq,
                                                              const float* __restrict__ dout, int64_t lddo,
                                                              const float* __restrict__ lse,
                                                              const float* __restrict__ delta, float* __restrict__ dqkv,
                                                              int64_t ldd, int N, int H, float scale) {
  __shared__ float sK[64][68];
  __shared__ float sV[64][68];
  const int tid = threadIdx.x, sub = tid & 3;
  const int qi = blockIdx.x * 64 + (tid >> 2);
  const int h = blockIdx.y, b = blockIdx.z, D = H * 64;
  const int64_t row0 = (int64_t)b * N;
  const float* Qp = qkv + row0 * ldq + h * 64;
  const float* Kp = Qp + D;
  const float* Vp = Qp + 2 * D;
  const float* Dp = dout + row0 * lddo + h * 64;
  float q[16], g[16], dq[16];
#pragma unroll
  for (int d = 0; d < 16; ++d) {
    q[d] = qi < N ? Qp[(int64_t)qi * ldq + sub * 16 + d] : 0.f;
    g[d] = qi < N ? Dp[(int64_t)qi * lddo + sub * 16 + d] : 0.f;
    dq[d] = 0.f;
  }
  const float li = qi < N ? lse[((int64_t)b * H + h) * N + qi] : INFINITY;
  const float deli = qi < N ? delta[((int64_t)b * H + h) * N + qi] : 0.f;
  const int nkt = (N + 63) / 64;
  for (int kt = 0; kt < nkt; ++kt) {
    __syncthreads();
    for (int e = tid; e < 64 * 64; e += 256) {
      const int r = e >> 6, c = e & 63, gk = kt * 64 + r;
      sK[r][c] = gk < N ? Kp[(int64_t)gk * ldq + c] : 0.f;
      sV[r][c] = gk < N ? Vp[(int64_t)gk * ldq + c] : 0.f;
    }
    __syncthreads();
    const int lim = N - kt * 64 < 64 ? N - kt * 64 : 64;
    for (int kk = 0; kk < lim; ++kk) {
      float s = 0.f, dp = 0.f;
#pragma unroll
      for (int d = 0; d < 16; ++d) {
        s = fmaf(q[d], sK[kk][sub * 16 + d], s);
        dp = fmaf(g[d], sV[kk][sub * 16 + d], dp);
      }
      s += __shfl_xor(s, 1, 64);
      s += __shfl_xor(s, 2, 64);
      dp += __shfl_xor(dp, 1, 64);
      dp += __shfl_xor(dp, 2, 64);
      const float p = expf(s * scale - li);
      const float ds = p * (dp - deli);
#pragma unroll
      for (int d = 0; d < 16; ++d) dq[d] = fmaf(ds, sK[kk][sub * 16 + d], dq[d]);
    }
  }
  if (qi < N) {
#pragma unroll
    for (int d = 0; d < 16; ++d) dqkv[(row0 + qi) * ldd + h * 64 + sub * 16 + d] = dq[d] * scale;
  }
}

// delta[b,h,n] = sum_d dO[n, h*64+d] * O[n, h*64+d]   (one wave per (row, head))
__global__ __launch_bounds__(256) void attn_delta_kernel(const float* __restrict__ o, int64_t ldo,
                                                         const float* __restrict__ dout, int64_t lddo,
                                                         float* __restrict__ delta, int64_t rows, int N, int H) {
  const int lane = threadIdx.x & 63;
  const int64_t w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (w >= rows * H) return;
  const int64_t row = w / H;
  const int h = (int)(w % H);
  float v = o[row * ldo + h * 64 + lane] * dout[row * lddo + h * 64 + lane];
  v = wave_sum(v);
  if (lane == 0) {
    const int64_t b = row / N, n = row % N;
    delta[(b * H + h) * N + n] = v;
  }
}

void attn_fwd_f32_launch(hipStream_t s, int64_t B, int64_t N, int64_t H, const float* qkv, int64_t ld_qkv, float* o,
                         int64_t ld_o, float* lse, float scale) {
  dim3 grid((unsigned)cdiv(N, 64), (unsigned)H, (unsigned)B);
  hipLaunchKernelGGL(attn_fwd_f32_kernel, grid, dim3(256), 0, s, qkv, ld_qkv, o, ld_o, lse, (int)N, (int)H, scale);
}

void attn_bwd_f32_launch(hipStream_t s, int64_t B, int64_t N, int64_t H, const float* qkv, int64_t ld_qkv,
                         const float* o, int64_t ld_o, const float* dout, int64_t ld_do, const float* lse, float* dqkv,
                         int64_t ld_dqkv, float* delta, float scale) {
  const int64_t rows = B * N;
  hipLaunchKernelGGL(attn_delta_kernel, dim3((unsigned)cdiv(rows * H, 4)), dim3(256), 0, s, o, ld_o, dout, ld_do,
                     delta, rows, (int)N, (int)H);
  dim3 grid((unsigned)cdiv(N, 64), (unsigned)H, (unsigned)B);
  hipLaunchKernelGGL(attn_bwd_dkdv_f32_kernel, grid, dim3(256), 0, s, qkv, ld_qkv, dout, ld_do, lse, delta, dqkv,
                     ld_dqkv, (int)N, (int)H, scale);
  hipLaunchKernelGGL(attn_bwd_dq_f32_kernel, grid, dim3(256), 0, s, qkv, ld_qkv, dout, ld_do, lse, delta, dqkv,
                     ld_dqkv, (int)N, (int)H, scale);
}

}  // namespace vs
