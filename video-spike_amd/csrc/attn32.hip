// attn32.hip — short-sequence attention for head dim 32 (1 <= N <= 256): the MAE decoder's shape
// (512 wide, 16 heads; 82 tokens at 144^2, 197 at 224^2).
//
// At these lengths a head's whole K and V fit on the chip, so nothing here is a flash kernel: there is
// no running maximum, no rescale and no redo pass.  Every score of a query row is held at once, the row
// maximum is a plain maximum, and every sum runs in an order fixed by (N, lane layout) alone -- no
// atomics anywhere, so two calls on equal inputs give equal bits.
//
// bf16 (v_mfma_f32_16x16x32_bf16; head dim 32 is exactly one k-step of the score product):
//   forward   one workgroup per (batch, head, 64 queries), one wave per 16 queries.  The scores are
//             computed TRANSPOSED, S^T = K Q^T, so a lane owns one query column and its keys sit in the
//             accumulator registers: the row maximum and sum are in-lane plus two shuffles, and P^T is
//             already the B operand of O^T = V^T P^T (cdna_hip_programming.md, "an accumulator tile as
//             the next MFMA's operand").  Only V^T goes through LDS (8-byte fragment reads).
//   backward  one workgroup per (batch, head).  P is recomputed from lse.  Pass A: a wave owns 16
//             queries, dS^T = P^T o (V dO^T - delta) feeds dQ^T = K^T dS^T.  Pass B: a wave owns 16 keys
//             and loops over the query blocks with dK^T = Q^T dS and dV^T = dO^T P accumulated in
//             registers.  K^T, Q^T, dO^T, lse and delta live in LDS (51 KiB).
// f32 (the exact 1e-4 parity mode): one thread per query (forward, dQ) or per key (dK/dV), the other
//   side's rows broadcast from LDS; plain fmaf chains in index order.
#include "common.h"

namespace vs {

constexpr int kA32MaxN = 256;
constexpr int kA32Ld = 260;  // bf16 elements per row of a transposed [32][N] LDS image: 8-byte aligned rows
constexpr float kA32Log2e = 1.4426950408889634f;
constexpr float kA32Ln2 = 0.6931471805599453f;

__device__ __forceinline__ bf16x8 a32_frag(const bf16_t* p, bool ok) {
  const uint4 u = ok ? *(const uint4*)p : make_uint4(0u, 0u, 0u, 0u);
  return __builtin_bit_cast(bf16x8, u);
}
// the A operand of a product that sums over 32 rows held as two accumulator tiles (16-row tiles 2u and
// 2u + 1): element j < 4 is row 32u + 4g + j, element j >= 4 row 32u + 16 + 4g + (j - 4) -- the order
// in which a32_pack lays the two accumulator tiles out as the B operand
__device__ __forceinline__ bf16x8 a32_tfrag(const bf16_t* img, int row, int u, int g) {
  const bf16_t* p = img + row * kA32Ld + 32 * u + 4 * g;
  const uint2 lo = *(const uint2*)p, hi = *(const uint2*)(p + 16);
  return __builtin_bit_cast(bf16x8, make_uint4(lo.x, lo.y, hi.x, hi.y));
}
__device__ __forceinline__ bf16x8 a32_pack(const f32x4& a, const f32x4& b) {
  bf16x8 v;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    v[j] = (__bf16)a[j];
    v[4 + j] = (__bf16)b[j];
  }
  return v;
}
// rows [0, np32) of a [N][32] bf16 operand (zero past N) into a transposed [32][kA32Ld] LDS image
__device__ __forceinline__ void a32_stage_t(bf16_t* img, const bf16_t* src, int64_t ld, int N, int np32, int tid) {
  for (int idx = tid; idx < np32 * 4; idx += 256) {
    const int row = idx >> 2, c = idx & 3;
    const uint4 u = row < N ? *(const uint4*)(src + (int64_t)row * ld + 8 * c) : make_uint4(0u, 0u, 0u, 0u);
    const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      img[(8 * c + 2 * j) * kA32Ld + row] = (bf16_t)(w[j] & 0xffffu);
      img[(8 * c + 2 * j + 1) * kA32Ld + row] = (bf16_t)(w[j] >> 16);
    }
  }
}
__device__ __forceinline__ void a32_store4(bf16_t* p, const f32x4& v, float mul) {
  const uint32_t lo = (uint32_t)f2bf(v[0] * mul) | ((uint32_t)f2bf(v[1] * mul) << 16);
  const uint32_t hi = (uint32_t)f2bf(v[2] * mul) | ((uint32_t)f2bf(v[3] * mul) << 16);
  *(uint2*)p = make_uint2(lo, hi);
}

// ---------------------------------------------------------------------------------------------------
// bf16 forward: grid (ceil(N / 64), H, B), 256 threads
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void attn32_fwd_bf16_kernel(const bf16_t* __restrict__ qkv, int64_t ldq,
                                                              bf16_t* __restrict__ o, int64_t ldo,
                                                              float* __restrict__ lse, int N, int H, float scale_log2e) {
  __shared__ __attribute__((aligned(16))) bf16_t Vt[32 * kA32Ld];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, b = blockIdx.z;
  const int np32 = (N + 31) & ~31;
  const bf16_t* base = qkv + (int64_t)b * N * ldq;
  a32_stage_t(Vt, base + 32 * (2 * H + h), ldq, N, np32, tid);
  __syncthreads();
  const int q0 = blockIdx.x * 64 + 16 * w;
  if (q0 >= N) return;  // wave-uniform, after the only barrier
  const int qi = q0 + r;  // this lane's query: a column of S^T
  const bf16x8 qf = a32_frag(base + (int64_t)qi * ldq + 32 * h + 8 * g, qi < N);
  const int nt = np32 >> 4;  // 16-key tiles (an even count)
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 s[16];
  float m = -INFINITY;
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    if (t < nt) {
      const int key = 16 * t + r;
      const bf16x8 kf = a32_frag(base + (int64_t)key * ldq + 32 * (H + h) + 8 * g, key < N);
      s[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf, zero, 0, 0, 0);  // S^T[key 16t + 4g + i][query r]
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        s[t][i] = 16 * t + 4 * g + i < N ? s[t][i] * scale_log2e : -INFINITY;
        m = fmaxf(m, s[t][i]);
      }
    }
  }
  m = fmaxf(m, __shfl_xor(m, 16, 64));
  m = fmaxf(m, __shfl_xor(m, 32, 64));  // N >= 1: every query has a finite maximum
  float l = 0.f;
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    if (t < nt) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        s[t][i] = __builtin_amdgcn_exp2f(s[t][i] - m);
        l += s[t][i];
      }
    }
  }
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  f32x4 acc[2] = {zero, zero};  // O^T[d = 16 dt + 4g + i][query r], unnormalised
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    if (2 * u < nt) {
      const bf16x8 pf = a32_pack(s[2 * u], s[2 * u + 1]);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
        acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a32_tfrag(Vt, 16 * dt + r, u, g), pf, acc[dt], 0, 0, 0);
    }
  }
  if (qi >= N) return;
  const float inv = 1.0f / l;
  bf16_t* orow = o + ((int64_t)b * N + qi) * ldo + 32 * h + 4 * g;
  a32_store4(orow, acc[0], inv);
  a32_store4(orow + 16, acc[1], inv);
  if (g == 0) lse[((int64_t)b * H + h) * N + qi] = (m + log2f(l)) * kA32Ln2;
}

// ---------------------------------------------------------------------------------------------------
// bf16 backward: grid B * H, 256 threads
// ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void attn32_bwd_bf16_kernel(const bf16_t* __restrict__ qkv, int64_t ldq,
                                                              const bf16_t* __restrict__ o, int64_t ldo,
                                                              const bf16_t* __restrict__ dout, int64_t lddo,
                                                              const float* __restrict__ lse, bf16_t* __restrict__ dqkv,
                                                              int64_t ldd, int N, int H, float scale) {
  __shared__ __attribute__((aligned(16))) bf16_t Kt[32 * kA32Ld];
  __shared__ __attribute__((aligned(16))) bf16_t Qt[32 * kA32Ld];
  __shared__ __attribute__((aligned(16))) bf16_t dOt[32 * kA32Ld];
  __shared__ __attribute__((aligned(16))) float lse2[kA32MaxN];  // lse * log2(e); 0 past N
  __shared__ __attribute__((aligned(16))) float delta[kA32MaxN];  // sum_d dO * O; 0 past N
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const int np32 = (N + 31) & ~31;
  const bf16_t* base = qkv + (int64_t)b * N * ldq;
  const bf16_t* qb = base + 32 * h;
  const bf16_t* kb = base + 32 * (H + h);
  const bf16_t* vb = base + 32 * (2 * H + h);
  const bf16_t* dob = dout + (int64_t)b * N * lddo + 32 * h;
  a32_stage_t(Qt, qb, ldq, N, np32, tid);
  a32_stage_t(Kt, kb, ldq, N, np32, tid);
  a32_stage_t(dOt, dob, lddo, N, np32, tid);
  {
    float d = 0.f, l2 = 0.f;
    if (tid < N) {
      const bf16_t* orow = o + ((int64_t)b * N + tid) * ldo + 32 * h;
      const bf16_t* drow = dob + (int64_t)tid * lddo;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const bf16x8 ov = a32_frag(orow + 8 * c, true), dv = a32_frag(drow + 8 * c, true);
#pragma unroll
        for (int j = 0; j < 8; ++j) d = fmaf((float)dv[j], (float)ov[j], d);
      }
      l2 = lse[((int64_t)b * H + h) * N + tid] * kA32Log2e;
    }
    delta[tid] = d;
    lse2[tid] = l2;
  }
  __syncthreads();  // the only barrier
  const float scale_log2e = scale * kA32Log2e;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const int n16 = (N + 15) >> 4, n32 = np32 >> 5;
  bf16_t* dbase = dqkv + (int64_t)b * N * ldd;

  // ---- pass A: dQ^T[d][query] = scale * sum_key K^T[d][key] dS^T[key][query]
  for (int qt = w; qt < n16; qt += 4) {
    const int qi = 16 * qt + r;
    const bf16x8 qf = a32_frag(qb + (int64_t)qi * ldq + 8 * g, qi < N);
    const bf16x8 dof = a32_frag(dob + (int64_t)qi * lddo + 8 * g, qi < N);
    const float ql = lse2[qi], qd = delta[qi];
    f32x4 acc[2] = {zero, zero};
    for (int u = 0; u < n32; ++u) {
      f32x4 ds[2];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int key = 32 * u + 16 * e + r;
        const bf16x8 kf = a32_frag(kb + (int64_t)key * ldq + 8 * g, key < N);
        const bf16x8 vf = a32_frag(vb + (int64_t)key * ldq + 8 * g, key < N);
        const f32x4 st = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf, zero, 0, 0, 0);
        const f32x4 dpt = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, dof, zero, 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const bool ok = 32 * u + 16 * e + 4 * g + i < N && qi < N;
          const float p = __builtin_amdgcn_exp2f(st[i] * scale_log2e - ql);
          ds[e][i] = ok ? p * (dpt[i] - qd) : 0.f;
        }
      }
      const bf16x8 dsf = a32_pack(ds[0], ds[1]);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
        acc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a32_tfrag(Kt, 16 * dt + r, u, g), dsf, acc[dt], 0, 0, 0);
    }
    if (qi < N) {
      bf16_t* row = dbase + (int64_t)qi * ldd + 32 * h + 4 * g;
      a32_store4(row, acc[0], scale);
      a32_store4(row + 16, acc[1], scale);
    }
  }

  // ---- pass B: dK^T[d][key] = scale * sum_query Q^T[d][query] dS[query][key],  dV^T = sum_query dO^T P
  for (int kt = w; kt < n16; kt += 4) {
    const int kj = 16 * kt + r;
    const bf16x8 kf = a32_frag(kb + (int64_t)kj * ldq + 8 * g, kj < N);
    const bf16x8 vf = a32_frag(vb + (int64_t)kj * ldq + 8 * g, kj < N);
    f32x4 dk[2] = {zero, zero}, dv[2] = {zero, zero};
    for (int u = 0; u < n32; ++u) {
      f32x4 p[2], ds[2];
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        const int qrow = 32 * u + 16 * e + r;
        const bf16x8 qf = a32_frag(qb + (int64_t)qrow * ldq + 8 * g, qrow < N);
        const bf16x8 dof = a32_frag(dob + (int64_t)qrow * lddo + 8 * g, qrow < N);
        const f32x4 s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf, kf, zero, 0, 0, 0);  // S[query 4g + i][key r]
        const f32x4 dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(dof, vf, zero, 0, 0, 0);
        const int q4 = 32 * u + 16 * e + 4 * g;
        const f32x4 ql = *(const f32x4*)(lse2 + q4), qd = *(const f32x4*)(delta + q4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const bool ok = q4 + i < N && kj < N;
          const float pv = __builtin_amdgcn_exp2f(s[i] * scale_log2e - ql[i]);
          p[e][i] = ok ? pv : 0.f;
          ds[e][i] = ok ? pv * (dp[i] - qd[i]) : 0.f;
        }
      }
      const bf16x8 pf = a32_pack(p[0], p[1]), dsf = a32_pack(ds[0], ds[1]);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        dv[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a32_tfrag(dOt, 16 * dt + r, u, g), pf, dv[dt], 0, 0, 0);
        dk[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a32_tfrag(Qt, 16 * dt + r, u, g), dsf, dk[dt], 0, 0, 0);
      }
    }
    if (kj < N) {
      bf16_t* row = dbase + (int64_t)kj * ldd + 4 * g;
      a32_store4(row + 32 * (H + h), dk[0], scale);
      a32_store4(row + 32 * (H + h) + 16, dk[1], scale);
      a32_store4(row + 32 * (2 * H + h), dv[0], 1.0f);
      a32_store4(row + 32 * (2 * H + h) + 16, dv[1], 1.0f);
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// f32: grid B * H, 64 * ceil(N / 64) threads, 2 * N * 32 floats of dynamic LDS (at most 64 KiB)
// ---------------------------------------------------------------------------------------------------
// rows [0, N) of two [N][32] f32 operands into LDS, row-major
__device__ __forceinline__ void a32_stage_f32(float* dst0, const float* src0, int64_t ld0, float* dst1, const float* src1,
                                              int64_t ld1, int N) {
  for (int idx = threadIdx.x; idx < N * 8; idx += blockDim.x) {
    const int row = idx >> 3, c = (idx & 7) * 4;
    *(float4*)(dst0 + row * 32 + c) = *(const float4*)(src0 + (int64_t)row * ld0 + c);
    *(float4*)(dst1 + row * 32 + c) = *(const float4*)(src1 + (int64_t)row * ld1 + c);
  }
}
__device__ __forceinline__ void a32_load32(float (&v)[32], const float* p) {
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const float4 t = *(const float4*)(p + 4 * c);
    v[4 * c] = t.x; v[4 * c + 1] = t.y; v[4 * c + 2] = t.z; v[4 * c + 3] = t.w;
  }
}
__device__ __forceinline__ void a32_store32(float* p, const float (&v)[32], float mul) {
#pragma unroll
  for (int c = 0; c < 8; ++c)
    *(float4*)(p + 4 * c) = make_float4(v[4 * c] * mul, v[4 * c + 1] * mul, v[4 * c + 2] * mul, v[4 * c + 3] * mul);
}
__device__ __forceinline__ float a32_dot(const float (&a)[32], const float* b) {
  float s = 0.f;
#pragma unroll
  for (int d = 0; d < 32; ++d) s = fmaf(a[d], b[d], s);
  return s;
}

__global__ __launch_bounds__(256) void attn32_fwd_f32_kernel(const float* __restrict__ qkv, int64_t ldq,
                                                             float* __restrict__ o, int64_t ldo, float* __restrict__ lse,
                                                             int N, int H, float scale) {
  extern __shared__ __attribute__((aligned(16))) float a32_lds[];
  float* Ks = a32_lds;
  float* Vs = a32_lds + N * 32;
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const float* base = qkv + (int64_t)b * N * ldq;
  a32_stage_f32(Ks, base + 32 * (H + h), ldq, Vs, base + 32 * (2 * H + h), ldq, N);
  __syncthreads();
  const int i = threadIdx.x;
  if (i >= N) return;  // after the only barrier
  float q[32];
  a32_load32(q, base + (int64_t)i * ldq + 32 * h);
  float m = -INFINITY;
  for (int j = 0; j < N; ++j) m = fmaxf(m, a32_dot(q, Ks + j * 32) * scale);
  float l = 0.f, acc[32];
#pragma unroll
  for (int d = 0; d < 32; ++d) acc[d] = 0.f;
  for (int j = 0; j < N; ++j) {
    const float p = expf(a32_dot(q, Ks + j * 32) * scale - m);
    l += p;
#pragma unroll
    for (int d = 0; d < 32; ++d) acc[d] = fmaf(p, Vs[j * 32 + d], acc[d]);
  }
  a32_store32(o + ((int64_t)b * N + i) * ldo + 32 * h, acc, 1.0f / l);
  lse[((int64_t)b * H + h) * N + i] = m + logf(l);
}

// dQ and delta[b, h, i] = sum_d dO * O (read by the dK/dV kernel)
__global__ __launch_bounds__(256) void attn32_bwd_dq_f32_kernel(const float* __restrict__ qkv, int64_t ldq,
                                                                const float* __restrict__ o, int64_t ldo,
                                                                const float* __restrict__ dout, int64_t lddo,
                                                                const float* __restrict__ lse, float* __restrict__ delta,
                                                                float* __restrict__ dqkv, int64_t ldd, int N, int H,
                                                                float scale) {
  extern __shared__ __attribute__((aligned(16))) float a32_lds[];
  float* Ks = a32_lds;
  float* Vs = a32_lds + N * 32;
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const float* base = qkv + (int64_t)b * N * ldq;
  a32_stage_f32(Ks, base + 32 * (H + h), ldq, Vs, base + 32 * (2 * H + h), ldq, N);
  __syncthreads();
  const int i = threadIdx.x;
  if (i >= N) return;
  float q[32], dO[32], dq[32];
  a32_load32(q, base + (int64_t)i * ldq + 32 * h);
  a32_load32(dO, dout + ((int64_t)b * N + i) * lddo + 32 * h);
  const float dl = a32_dot(dO, o + ((int64_t)b * N + i) * ldo + 32 * h);
  const float li = lse[((int64_t)b * H + h) * N + i];
  delta[((int64_t)b * H + h) * N + i] = dl;
#pragma unroll
  for (int d = 0; d < 32; ++d) dq[d] = 0.f;
  for (int j = 0; j < N; ++j) {
    const float p = expf(a32_dot(q, Ks + j * 32) * scale - li);
    const float ds = p * (a32_dot(dO, Vs + j * 32) - dl);
#pragma unroll
    for (int d = 0; d < 32; ++d) dq[d] = fmaf(ds, Ks[j * 32 + d], dq[d]);
  }
  a32_store32(dqkv + ((int64_t)b * N + i) * ldd + 32 * h, dq, scale);
}

__global__ __launch_bounds__(256) void attn32_bwd_dkdv_f32_kernel(const float* __restrict__ qkv, int64_t ldq,
                                                                  const float* __restrict__ dout, int64_t lddo,
                                                                  const float* __restrict__ lse,
                                                                  const float* __restrict__ delta, float* __restrict__ dqkv,
                                                                  int64_t ldd, int N, int H, float scale) {
  extern __shared__ __attribute__((aligned(16))) float a32_lds[];
  float* Qs = a32_lds;
  float* dOs = a32_lds + N * 32;
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const float* base = qkv + (int64_t)b * N * ldq;
  a32_stage_f32(Qs, base + 32 * h, ldq, dOs, dout + (int64_t)b * N * lddo + 32 * h, lddo, N);
  __syncthreads();
  const int j = threadIdx.x;
  if (j >= N) return;
  float k[32], v[32], dk[32], dv[32];
  a32_load32(k, base + (int64_t)j * ldq + 32 * (H + h));
  a32_load32(v, base + (int64_t)j * ldq + 32 * (2 * H + h));
#pragma unroll
  for (int d = 0; d < 32; ++d) dk[d] = dv[d] = 0.f;
  const float* lrow = lse + ((int64_t)b * H + h) * N;
  const float* drow = delta + ((int64_t)b * H + h) * N;
  for (int i = 0; i < N; ++i) {
    const float p = expf(a32_dot(k, Qs + i * 32) * scale - lrow[i]);
    const float ds = p * (a32_dot(v, dOs + i * 32) - drow[i]);
#pragma unroll
    for (int d = 0; d < 32; ++d) {
      dv[d] = fmaf(p, dOs[i * 32 + d], dv[d]);
      dk[d] = fmaf(ds, Qs[i * 32 + d], dk[d]);
    }
  }
  float* row = dqkv + ((int64_t)b * N + j) * ldd;
  a32_store32(row + 32 * (H + h), dk, scale);
  a32_store32(row + 32 * (2 * H + h), dv, 1.0f);
}

}  // namespace vs

using namespace vs;

static int attn32_check(int32_t dtype, int64_t B, int64_t N, int64_t H) {
  VS_REQUIRE(dtype == VS_BF16 || dtype == VS_F32, "vs_attn32: bad dtype (VS_BF16 | VS_F32)");
  VS_REQUIRE(B > 0 && N > 0 && H > 0, "vs_attn32: empty problem");
  VS_REQUIRE(N <= kA32MaxN, "vs_attn32: sequence length must be in 1..256 (K and V of a head stay on the chip)");
  VS_REQUIRE(B <= 65535 && H <= 65535, "vs_attn32: extents out of range");
  return VS_OK;
}

// f32: float4 accesses; bf16: 16-byte fragment loads and 8-byte stores
static bool attn32_in_ok(int32_t dtype, const void* p, int64_t ld) {
  return aligned16(p) && ld % (dtype == VS_BF16 ? 8 : 4) == 0;
}
static bool attn32_out_ok(int32_t dtype, const void* p, int64_t ld) {
  return dtype == VS_BF16 ? ((((uintptr_t)p) & 7) == 0 && ld % 4 == 0) : (aligned16(p) && ld % 4 == 0);
}

extern "C" int vs_attn32_fwd(int32_t dtype, int64_t B, int64_t N, int64_t H, const void* qkv, int64_t ld_qkv, void* o,
                             int64_t ld_o, float* lse, float scale, void* stream) {
  VS_CALL(attn32_check(dtype, B, N, H));
  VS_REQUIRE(qkv && o && lse, "vs_attn32_fwd: null pointer");
  VS_REQUIRE(ld_qkv >= 3 * H * 32 && ld_o >= H * 32, "vs_attn32_fwd: leading dims too small");
  VS_REQUIRE(attn32_in_ok(dtype, qkv, ld_qkv) && attn32_out_ok(dtype, o, ld_o),
             "vs_attn32_fwd: rows must be 16-byte aligned (o: 8-byte in bf16)");
  hipStream_t s = (hipStream_t)stream;
  const double es = dtype == VS_BF16 ? 2.0 : 4.0;
  ScopedTimer timer(VS_TIMER_ATTN_FWD, s, (double)(B * N * H * 32) * 4.0 * es + (double)(B * H * N) * 4.0);
  if (dtype == VS_BF16) {
    dim3 grid((unsigned)cdiv(N, 64), (unsigned)H, (unsigned)B);
    hipLaunchKernelGGL(attn32_fwd_bf16_kernel, grid, dim3(256), 0, s, (const bf16_t*)qkv, ld_qkv, (bf16_t*)o, ld_o, lse,
                       (int)N, (int)H, scale * kA32Log2e);
  } else {
    hipLaunchKernelGGL(attn32_fwd_f32_kernel, dim3((unsigned)(B * H)), dim3((unsigned)(64 * cdiv(N, 64))),
                       (size_t)N * 256, s, (const float*)qkv, ld_qkv, (float*)o, ld_o, lse, (int)N, (int)H, scale);
  }
  VS_LAUNCH_CHECK();
  return VS_OK;
}

extern "C" size_t vs_attn32_bwd_workspace_bytes(int64_t B, int64_t N, int64_t H) {
  // delta [B, H, N] f32 (the f32 kernels; the bf16 kernel keeps it in LDS), 256-B padded
  return ((size_t)(B * H * N) * 4 + 255) / 256 * 256;
}

extern "C" int vs_attn32_bwd(int32_t dtype, int64_t B, int64_t N, int64_t H, const void* qkv, int64_t ld_qkv,
                             const void* o, int64_t ld_o, const void* dout, int64_t ld_do, const float* lse, void* dqkv,
                             int64_t ld_dqkv, void* workspace, float scale, void* stream) {
  VS_CALL(attn32_check(dtype, B, N, H));
  VS_REQUIRE(qkv && o && dout && lse && dqkv && workspace, "vs_attn32_bwd: null pointer");
  VS_REQUIRE(ld_qkv >= 3 * H * 32 && ld_dqkv >= 3 * H * 32 && ld_o >= H * 32 && ld_do >= H * 32,
             "vs_attn32_bwd: leading dims too small");
  VS_REQUIRE(attn32_in_ok(dtype, qkv, ld_qkv) && attn32_in_ok(dtype, o, ld_o) && attn32_in_ok(dtype, dout, ld_do) &&
                 attn32_out_ok(dtype, dqkv, ld_dqkv) && (((uintptr_t)workspace) & 3) == 0,
             "vs_attn32_bwd: rows must be 16-byte aligned (dqkv: 8-byte in bf16)");
  hipStream_t s = (hipStream_t)stream;
  const double es = dtype == VS_BF16 ? 2.0 : 4.0;
  ScopedTimer timer(VS_TIMER_ATTN_BWD, s, (double)(B * N * H * 32) * 8.0 * es + (double)(B * H * N) * 4.0);
  const dim3 grid((unsigned)(B * H));
  if (dtype == VS_BF16) {
    hipLaunchKernelGGL(attn32_bwd_bf16_kernel, grid, dim3(256), 0, s, (const bf16_t*)qkv, ld_qkv, (const bf16_t*)o, ld_o,
                       (const bf16_t*)dout, ld_do, lse, (bf16_t*)dqkv, ld_dqkv, (int)N, (int)H, scale);
  } else {
    const dim3 block((unsigned)(64 * cdiv(N, 64)));
    float* delta = (float*)workspace;
    hipLaunchKernelGGL(attn32_bwd_dq_f32_kernel, grid, block, (size_t)N * 256, s, (const float*)qkv, ld_qkv,
                       (const float*)o, ld_o, (const float*)dout, ld_do, lse, delta, (float*)dqkv, ld_dqkv, (int)N, (int)H,
                       scale);
    hipLaunchKernelGGL(attn32_bwd_dkdv_f32_kernel, grid, block, (size_t)N * 256, s, (const float*)qkv, ld_qkv,
                       (const float*)dout, ld_do, lse, delta, (float*)dqkv, ld_dqkv, (int)N, (int)H, scale);
  }
  VS_LAUNCH_CHECK();
  return VS_OK;
}
