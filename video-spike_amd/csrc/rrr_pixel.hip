// rrr_pixel.hip — the reduced-rank regression (RRR) baseline straight from the pixels: src/train_rrr.py's
// input_mod == 'whisker-video' (train_rrr.py:85-105,143-171), one session whose features are the C = h w pixels of
// a frame, 1 <= C <= 32,768.  Notation is rrr_wide.hip's (K trials, T bins, N neurons, C features + a column of
// ones, r components) plus F, the frames per trial: bin t reads frame idx[t].
// The video X [K][F][C] is stored once in its own dtype (uint8 or float32) and is the only thing of its size:
// an element is standardised on its way into LDS,
//   uint8:   (double(x) - mean[f,c]) / std[f,c]            f64 statistics (numpy's for an integer array)
//   float32: double(float((x - mean[f,c]) / std[f,c]))     f32 statistics, every step rounded to f32 as numpy does
// with a true division (the reference's values bit for bit).  VS_KNOB_RRR_PIXEL_RECIP = 1 multiplies by a reciprocal
// instead, for the A/B in scripts/rrr_pixel_bench.py (DESIGN.md section 7 has the measurement).  The bias column is an implicit 1.  There is no
// buffer of K T C, K F C or T C N elements.
//
// vs_rrr_pixel_stats: one thread per (f, c) column walking k.  np.mean / np.std / np.clip(., 1e-8) over the trials
//   in numpy's order and roundings (sums ascending in k, the square rounded before it is added).
// vs_rrr_pixel_loss_grad, 4 launches in loss-only mode, 6 with gradients:
//   1. rrp_fwd_kernel    rrw_fwd_kernel with the X tile formed from pixels: block = one bin t, 128 trials x 64
//                        neurons, the features through LDS 32 at a time.  Writes res [K][T][N].
//   2. rrp_sq_kernel     sum_k res^2 per (t, n), k ascending; one partial per (t, 256 neurons) in a fixed tree.
//   3. rrp_l2_kernel     l2 sum_t beta[n,c,t]^2 per (n, c) and l2 b[n,t]^2, one partial per 256 of them.
//   4. rrp_grad_kernel   block = 64 features x 64 neurons, walking every bin t in order.  Per bin G_t = X_t^T 2 res_t
//                        is accumulated on the MFMA over all K trials (32 per LDS stage) and folded while still in
//                        registers, in rrw_reduce_t_kernel's arithmetic:  H = G + 2 l2 beta,  dU[n,c,:] += H V[:,t],
//                        db[n,t] = H of the bias row, and the tile's share of dV[:,t] = sum U[n,c,:] H (a fixed
//                        tree over the block) goes to dVp[tile][j][t].  U[n,c,:] and the dU accumulators stay in
//                        registers for the whole walk (2 x 16 r doubles per lane), which is what caps r at 4.
//   5. rrp_dv_sum_kernel dV[j][t] = the tiles' partials added in tile order.
//   6. rrp_loss_kernel   the partials of 2. and 3. added in a fixed order.
// The loss runs through 1, 2, 3, 6 whether gradients are asked for or not: the same bits.  l2 = 0 makes every l2
// partial an exact 0.  No atomics; every sum's order is fixed by the extents.  Tails add exact zeros and nothing
// outside the operands and the stated workspace is read or written (rrw_fwd_kernel's comment).  A frame index
// outside [0, F) is clamped into it, so no address depends on the contents of idx (vspike.ops checks them).
// Workspace (doubles, each piece rounded up to 256 bytes):
//   K T N  (res)  +  T ceil(N/256) + ceil(N (C + T) / 256)  (loss partials)  +  ceil((C+1)/64) ceil(N/64) r T  (dV
//   partials)
// i.e. 0.17 GB at K 400, T 100, N 512, C 18,260, r 3.
// vs_rrr_pixel_score: rrp_fwd_kernel (standardised yhat to the workspace) + rrr_wide.hip's scoring kernels.
#include <math.h>

#include "common.h"
#include "rrr_wide.h"

namespace vs {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kRrpMaxC = 32768;
constexpr int kRrpMaxR = 4;
constexpr int kRrpTile = 64;        // neurons per block; features per block of the gradient product
constexpr int kRrpFwdTrials = 128;  // trials per block of the forward product
constexpr int kRrpStep = 32;        // reduction extent staged in LDS at a time (8 MFMA k-steps)
constexpr int kRrpXs = 36;          // forward X tile row stride (doubles)
constexpr int kRrpBs = 65;          // forward Beta tile row stride

template <typename XT> struct RrpStat;
template <> struct RrpStat<uint8_t> { typedef double type; };
template <> struct RrpStat<float> { typedef float type; };

// RECIP (VS_KNOB_RRR_PIXEL_RECIP, an A/B knob, off by default): the divisor of a column is inverted once per slice /
// bin and the elements are multiplied, which changes the last bit of about a quarter of the standardised values.
template <bool RECIP> __device__ __forceinline__ double rrp_div(double s) { return RECIP ? 1.0 / s : s; }
template <bool RECIP> __device__ __forceinline__ float rrp_div(float s) { return RECIP ? (float)(1.0 / (double)s) : s; }
template <bool RECIP> __device__ __forceinline__ double rrp_z(uint8_t x, double m, double q) {
  return RECIP ? ((double)x - m) * q : ((double)x - m) / q;
}
// the correctly rounded f32 quotient (53 >= 2 * 24 + 2 bits), widened
template <bool RECIP> __device__ __forceinline__ double rrp_z(float x, float m, float q) {
  const float d = x - m;
  return RECIP ? (double)(d * q) : (double)(float)((double)d / (double)q);
}
template <typename YT> __device__ __forceinline__ double rrp_ld(const YT* p) { return (double)*p; }
__device__ __forceinline__ int64_t rrp_frame(const int64_t* __restrict__ idx, int64_t t, int64_t F) {
  const int64_t f = idx[t];
  return f < 0 ? 0 : (f < F ? f : F - 1);
}

// ---- statistics ------------------------------------------------------------------------------------------------
// grid ceil(F C / 256).  The product d d passes through an opaque copy so that it is rounded before the sum (the
// compiler would fuse them), as in gauss_smooth_time_kernel.
template <typename XT>
__global__ __launch_bounds__(256) void rrp_stats_kernel(int64_t K, int64_t FC, const XT* __restrict__ X,
                                                        typename RrpStat<XT>::type* __restrict__ mean,
                                                        typename RrpStat<XT>::type* __restrict__ sd) {
  typedef typename RrpStat<XT>::type ST;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= FC) return;
  const XT* x = X + e;
  ST s = (ST)x[0];
  for (int64_t k = 1; k < K; ++k) s += (ST)x[k * FC];
  const ST m = (ST)((double)s / (double)K);
  ST q = 0;
  for (int64_t k = 0; k < K; ++k) {
    const ST d = (ST)x[k * FC] - m;
    ST p = d * d;
    asm volatile("" : "+v"(p));
    q = k == 0 ? p : q + p;
  }
  const ST var = (ST)((double)q / (double)K);
  ST v = (ST)sqrt((double)var);
  const ST lo = (ST)1e-8;
  v = v < lo ? lo : v;   // np.clip(std, 1e-8, None): a NaN stays a NaN
  mean[e] = m;
  sd[e] = v;
}

// ---- forward product ---------------------------------------------------------------------------------------------
// grid (ceil(N/64), T, ceil(K/128)).  SCORE: out = yhat, else out = yhat - y.  rrw_fwd_kernel's schedule (the raw U
// rows of r <= 4): the next 32-feature slice is loaded raw (pixels, their statistics, U rows) before the MFMAs of
// the current one and converted when it is staged.  Tails as there: trials >= K and neurons >= N are never
// stored (clamped loads); features > C add 0 x 1: the X value is 1 and the V factors are zeroed.
template <typename XT, typename YT, bool SCORE, bool RECIP>
__global__ __launch_bounds__(256) void rrp_fwd_kernel(int64_t K, int64_t F, int64_t T, int64_t N, int C, int r,
                                                      const XT* __restrict__ X, const int64_t* __restrict__ idx,
                                                      const typename RrpStat<XT>::type* __restrict__ mean,
                                                      const typename RrpStat<XT>::type* __restrict__ sd,
                                                      const YT* __restrict__ y, const double* __restrict__ U,
                                                      const double* __restrict__ V, const double* __restrict__ b,
                                                      double* __restrict__ out) {
  typedef typename RrpStat<XT>::type ST;
  constexpr int kMt = kRrpFwdTrials / 16;
  constexpr int kXl = kRrpFwdTrials * kRrpStep / 256;
  __shared__ double Xs[kRrpFwdTrials * kRrpXs];
  __shared__ double Bs[kRrpStep * kRrpBs];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lk = lane >> 4;
  const int64_t t = blockIdx.y;
  const int64_t n0 = (int64_t)blockIdx.x * kRrpTile, k0 = (int64_t)blockIdx.z * kRrpFwdTrials;
  const int C1 = C + 1;
  const int col = tid & 31, row0 = tid >> 5;       // staging: element e = tid + 256 i is (row0 + 8 i, col)
  const int64_t f = rrp_frame(idx, t, F);
  double v[kRrpMaxR];
#pragma unroll
  for (int j = 0; j < kRrpMaxR; ++j) v[j] = j < r ? V[(int64_t)j * T + t] : 0.0;
  f64x4 acc[kMt];
#pragma unroll
  for (int m = 0; m < kMt; ++m) acc[m] = f64x4{0.0, 0.0, 0.0, 0.0};
  XT xr[kXl];
  ST ms, ss;
  double ur[8][kRrpMaxR];
  auto load = [&](int c0) {
    const int c = c0 + col;
    const int cu = c < C ? c : C - 1;
    ms = mean[f * C + cu];
    ss = sd[f * C + cu];
#pragma unroll
    for (int i = 0; i < kXl; ++i) {                // X tile: 128 trials x 32 features
      const int64_t k = k0 + row0 + 8 * i;
      xr[i] = X[((k < K ? k : K - 1) * F + f) * C + cu];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {                  // Beta tile: 32 features x 64 neurons
      const int64_t n = n0 + row0 + 8 * i;
      const double* up = U + ((n < N ? n : N - 1) * C + cu) * r;
#pragma unroll
      for (int j = 0; j < kRrpMaxR; ++j) ur[i][j] = up[j < r ? j : 0];
    }
    if (c0 + kRrpStep > C) {                       // the slice that holds the bias row (block-uniform)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int64_t n = n0 + row0 + 8 * i;
        const double bv = b[(n < N ? n : N - 1) * T + t];
        ur[i][0] = c == C ? bv : ur[i][0];
      }
    }
  };
  load(0);
  for (int c0 = 0; c0 < C1; c0 += kRrpStep) {
    const int c = c0 + col;
    const ST qs = rrp_div<RECIP>(ss);
#pragma unroll
    for (int i = 0; i < kXl; ++i) Xs[(row0 + 8 * i) * kRrpXs + col] = c < C ? rrp_z<RECIP>(xr[i], ms, qs) : 1.0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      double s = 0.0;                              // rrw_beta's order: j ascending, fused
#pragma unroll
      for (int j = 0; j < kRrpMaxR; ++j)
        if (j < r) s = fma(ur[i][j], c < C ? v[j] : 0.0, s);
      Bs[col * kRrpBs + row0 + 8 * i] = c == C ? ur[i][0] : s;
    }
    __syncthreads();
    if (c0 + kRrpStep < C1) load(c0 + kRrpStep);
#pragma unroll
    for (int kk = 0; kk < kRrpStep / 4; ++kk) {
      const double bb = Bs[(kk * 4 + lk) * kRrpBs + 16 * w + li];
#pragma unroll
      for (int m = 0; m < kMt; ++m)
        acc[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(Xs[(16 * m + li) * kRrpXs + kk * 4 + lk], bb, acc[m], 0, 0, 0);
    }
    __syncthreads();
  }
  const int64_t n = n0 + 16 * w + li;
  if (n < N) {
#pragma unroll
    for (int m = 0; m < kMt; ++m)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t k = k0 + 16 * m + lk + 4 * q;
        if (k < K) {
          const int64_t at = (k * T + t) * N + n;
          out[at] = SCORE ? acc[m][q] : acc[m][q] - rrp_ld(y + at);
        }
      }
  }
}

// fixed-shape block reduction (256 threads); every thread gets the sum
__device__ double rrp_block_sum(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const double out = red[0];
  __syncthreads();
  return out;
}

// grid (ceil(N/256), T): lossp[t gridDim.x + blockIdx.x] = sum over the block's neurons of sum_k res^2 (k ascending)
__global__ __launch_bounds__(256) void rrp_sq_kernel(int64_t K, int64_t T, int64_t N, const double* __restrict__ R,
                                                     double* __restrict__ lossp) {
  __shared__ double red[256];
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t t = blockIdx.y;
  double sq = 0.0;
  if (n < N) {
    for (int64_t k = 0; k < K; ++k) {
      const double res = R[(k * T + t) * N + n];
      sq = fma(res, res, sq);
    }
  }
  sq = rrp_block_sum(sq, red);
  if (threadIdx.x == 0) lossp[t * gridDim.x + blockIdx.x] = sq;
}

// grid ceil(N (C + T) / 256): element e < N C is (n, c): l2 sum_t beta[n,c,t]^2, t ascending; the others are l2 b^2
__global__ __launch_bounds__(256) void rrp_l2_kernel(int64_t T, int64_t N, int C, int r, double l2,
                                                     const double* __restrict__ U, const double* __restrict__ V,
                                                     const double* __restrict__ b, double* __restrict__ lossp) {
  __shared__ double red[256];
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t NC = N * C;
  double term = 0.0;
  if (e < NC) {
    double u[kRrpMaxR];
#pragma unroll
    for (int j = 0; j < kRrpMaxR; ++j) u[j] = j < r ? U[e * r + j] : 0.0;
    for (int64_t t = 0; t < T; ++t) {
      double be = 0.0;
#pragma unroll
      for (int j = 0; j < kRrpMaxR; ++j)
        if (j < r) be = fma(u[j], V[(int64_t)j * T + t], be);
      term = fma(be, be, term);
    }
  } else if (e < NC + N * T) {
    const double bv = b[e - NC];
    term = bv * bv;
  }
  const double s = rrp_block_sum(l2 * term, red);
  if (threadIdx.x == 0) lossp[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void rrp_loss_kernel(int64_t count, const double* __restrict__ lossp,
                                                       double* __restrict__ loss) {
  __shared__ double red[256];
  double a = 0.0;
  for (int64_t i = threadIdx.x; i < count; i += 256) a += lossp[i];
  a = rrp_block_sum(a, red);
  if (threadIdx.x == 0) loss[0] = a;
}

// ---- gradient product with the fold --------------------------------------------------------------------------
// grid (ceil(N/64), ceil((C+1)/64)).  The MFMA's D element (m, q) of wave w, lane (li, lk) is feature
// c0 + 16 m + lk + 4 q and neuron n0 + 16 w + li.  Tails as in rrw_grad_kernel: trials >= K add exactly 0 (loads
// clamped, the residual's factor 2 becomes 0); features > C and neurons >= N are never stored and enter dV as 0.
template <typename XT, int R, bool RECIP>
__global__ __launch_bounds__(256) void rrp_grad_kernel(int64_t K, int64_t F, int64_t T, int64_t N, int C, double l2,
                                                       const XT* __restrict__ X, const int64_t* __restrict__ idx,
                                                       const typename RrpStat<XT>::type* __restrict__ mean,
                                                       const typename RrpStat<XT>::type* __restrict__ sd,
                                                       const double* __restrict__ Rres, const double* __restrict__ U,
                                                       const double* __restrict__ V, const double* __restrict__ b,
                                                       double* __restrict__ dU, double* __restrict__ db,
                                                       double* __restrict__ dVp) {
  typedef typename RrpStat<XT>::type ST;
  __shared__ double Xs[kRrpStep * kRrpTile];
  __shared__ double Rs[kRrpStep * kRrpTile];
  __shared__ double dvs[4 * R];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lk = lane >> 4;
  const int64_t n0 = (int64_t)blockIdx.x * kRrpTile;
  const int c0 = (int)blockIdx.y * kRrpTile;
  const int64_t tile = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
  const int col = tid & 63, row0 = tid >> 6;       // staging: element e = tid + 256 i is (row0 + 4 i, col)
  const bool feat = c0 + col < C;
  const int cc = feat ? c0 + col : C - 1;
  const int64_t nc = n0 + col < N ? n0 + col : N - 1;
  const int64_t n = n0 + 16 * w + li;              // this lane's neuron in the D tiles
  const bool nlive = n < N;
  double u[4][4][R], du[4][4][R];
#pragma unroll
  for (int m = 0; m < 4; ++m)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = c0 + 16 * m + lk + 4 * q;
#pragma unroll
      for (int j = 0; j < R; ++j) {
        u[m][q][j] = (nlive && c < C) ? U[(n * C + c) * R + j] : 0.0;
        du[m][q][j] = 0.0;
      }
    }
  XT xr[8];
  double rr[8];
  for (int64_t t = 0; t < T; ++t) {
    const int64_t f = rrp_frame(idx, t, F);
    const ST ms = mean[f * C + cc], qs = rrp_div<RECIP>(sd[f * C + cc]);
    double v[R];
#pragma unroll
    for (int j = 0; j < R; ++j) v[j] = V[(int64_t)j * T + t];
    f64x4 acc[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) acc[m] = f64x4{0.0, 0.0, 0.0, 0.0};
    auto load = [&](int64_t k0) {                  // the next 32 trials, in flight under the MFMAs
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int64_t k = k0 + row0 + 4 * i, kc = k < K ? k : K - 1;
        xr[i] = X[(kc * F + f) * C + cc];
        rr[i] = Rres[(kc * T + t) * N + nc] * (k < K ? 2.0 : 0.0);
      }
    };
    load(0);
    for (int64_t k0 = 0; k0 < K; k0 += kRrpStep) {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        Xs[tid + 256 * i] = feat ? rrp_z<RECIP>(xr[i], ms, qs) : 1.0;
        Rs[tid + 256 * i] = rr[i];
      }
      __syncthreads();
      if (k0 + kRrpStep < K) load(k0 + kRrpStep);
#pragma unroll
      for (int kk = 0; kk < kRrpStep / 4; ++kk) {
        const double bb = Rs[(kk * 4 + lk) * kRrpTile + 16 * w + li];
#pragma unroll
        for (int m = 0; m < 4; ++m)
          acc[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(Xs[(kk * 4 + lk) * kRrpTile + 16 * m + li], bb, acc[m], 0, 0, 0);
      }
      __syncthreads();
    }
    // the fold: rrw_reduce_t_kernel's H = G + 2 l2 beta, dU += H V^T, db; rrw_dv_kernel's sum U H over the tile
    double dv[R];
#pragma unroll
    for (int j = 0; j < R; ++j) dv[j] = 0.0;
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = c0 + 16 * m + lk + 4 * q;
        double be = 0.0;
#pragma unroll
        for (int j = 0; j < R; ++j) be = fma(u[m][q][j], v[j], be);
        if (c == C && nlive) be = b[n * T + t];
        const double h = fma(2.0 * l2, be, acc[m][q]);
        if (c == C && nlive) db[n * T + t] = h;
        const double hm = (nlive && c < C) ? h : 0.0;
#pragma unroll
        for (int j = 0; j < R; ++j) {
          du[m][q][j] = fma(hm, v[j], du[m][q][j]);
          dv[j] = fma(u[m][q][j], hm, dv[j]);
        }
      }
#pragma unroll
    for (int j = 0; j < R; ++j) {
      double s = dv[j];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
      if (lane == 0) dvs[w * R + j] = s;
    }
    __syncthreads();
    // the next write of dvs comes after the two barriers of the next bin's first stage
    if (tid < R) dVp[(tile * R + tid) * T + t] = ((dvs[tid] + dvs[R + tid]) + dvs[2 * R + tid]) + dvs[3 * R + tid];
  }
  if (nlive) {
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = c0 + 16 * m + lk + 4 * q;
        if (c < C) {
#pragma unroll
          for (int j = 0; j < R; ++j) dU[(n * C + c) * R + j] = du[m][q][j];
        }
      }
  }
}

// dV[j][t] = sum of the tiles' partials, ascending; grid ceil(r T / 256)
__global__ __launch_bounds__(256) void rrp_dv_sum_kernel(int64_t T, int r, int64_t tiles, const double* __restrict__ dVp,
                                                         double* __restrict__ dV) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)r * T) return;
  double s = 0.0;
  for (int64_t tl = 0; tl < tiles; ++tl) s += dVp[tl * r * T + i];
  dV[i] = s;
}

struct RrpWs {
  int64_t sq_parts, l2_parts, tiles;
  size_t res, lossp, dVp, total;  // byte offsets
};
static RrpWs rrp_ws(int64_t K, int64_t T, int64_t N, int64_t C, int64_t r) {
  RrpWs w;
  w.sq_parts = T * cdiv(N, 256);
  w.l2_parts = cdiv(N * (C + T), 256);
  w.tiles = cdiv(C + 1, kRrpTile) * cdiv(N, kRrpTile);
  auto al = [](size_t bytes) { return (bytes + 255) / 256 * 256; };
  size_t off = 0;
  w.res = off;   off += al((size_t)K * T * N * 8);
  w.lossp = off; off += al((size_t)(w.sq_parts + w.l2_parts) * 8);
  w.dVp = off;   off += al((size_t)w.tiles * r * T * 8);
  w.total = off;
  return w;
}

static bool rrp_dims_ok(int64_t K, int64_t F, int64_t T, int64_t N) {
  return K > 0 && F > 0 && T > 0 && N > 0 && T <= 65535 && cdiv(K, kRrpFwdTrials) <= 65535 && N <= (1 << 24);
}

template <typename XT, typename YT, bool SCORE>
static void rrp_launch_fwd(hipStream_t s, int64_t K, int64_t F, int64_t T, int64_t N, int C, int r, const void* X,
                           const int64_t* idx, const void* mean, const void* sd, const void* y, const double* U,
                           const double* V, const double* b, double* out) {
  typedef typename RrpStat<XT>::type ST;
  const dim3 grid((unsigned)cdiv(N, kRrpTile), (unsigned)T, (unsigned)cdiv(K, kRrpFwdTrials));
  if (knob(VS_KNOB_RRR_PIXEL_RECIP) == 1)
    hipLaunchKernelGGL((rrp_fwd_kernel<XT, YT, SCORE, true>), grid, dim3(256), 0, s, K, F, T, N, C, r, (const XT*)X, idx,
                       (const ST*)mean, (const ST*)sd, (const YT*)y, U, V, b, out);
  else
    hipLaunchKernelGGL((rrp_fwd_kernel<XT, YT, SCORE, false>), grid, dim3(256), 0, s, K, F, T, N, C, r, (const XT*)X, idx,
                       (const ST*)mean, (const ST*)sd, (const YT*)y, U, V, b, out);
}

template <typename XT, int R>
static void rrp_launch_grad(hipStream_t s, int64_t K, int64_t F, int64_t T, int64_t N, int C, double l2, const void* X,
                            const int64_t* idx, const void* mean, const void* sd, const double* res, const double* U,
                            const double* V, const double* b, double* dU, double* db, double* dVp) {
  typedef typename RrpStat<XT>::type ST;
  const dim3 grid((unsigned)cdiv(N, kRrpTile), (unsigned)cdiv(C + 1, kRrpTile));
  if (knob(VS_KNOB_RRR_PIXEL_RECIP) == 1)
    hipLaunchKernelGGL((rrp_grad_kernel<XT, R, true>), grid, dim3(256), 0, s, K, F, T, N, C, l2, (const XT*)X, idx,
                       (const ST*)mean, (const ST*)sd, res, U, V, b, dU, db, dVp);
  else
    hipLaunchKernelGGL((rrp_grad_kernel<XT, R, false>), grid, dim3(256), 0, s, K, F, T, N, C, l2, (const XT*)X, idx,
                       (const ST*)mean, (const ST*)sd, res, U, V, b, dU, db, dVp);
}

template <typename XT>
static void rrp_launch_grad_r(int r, hipStream_t s, int64_t K, int64_t F, int64_t T, int64_t N, int C, double l2,
                              const void* X, const int64_t* idx, const void* mean, const void* sd, const double* res,
                              const double* U, const double* V, const double* b, double* dU, double* db, double* dVp) {
  switch (r) {
    case 1: rrp_launch_grad<XT, 1>(s, K, F, T, N, C, l2, X, idx, mean, sd, res, U, V, b, dU, db, dVp); break;
    case 2: rrp_launch_grad<XT, 2>(s, K, F, T, N, C, l2, X, idx, mean, sd, res, U, V, b, dU, db, dVp); break;
    case 3: rrp_launch_grad<XT, 3>(s, K, F, T, N, C, l2, X, idx, mean, sd, res, U, V, b, dU, db, dVp); break;
    default: rrp_launch_grad<XT, 4>(s, K, F, T, N, C, l2, X, idx, mean, sd, res, U, V, b, dU, db, dVp); break;
  }
}

}  // namespace vs

using namespace vs;

extern "C" int vs_rrr_pixel_stats(int64_t K, int64_t F, int64_t C, const void* X, int32_t x_dtype, void* mean,
                                  void* sd, void* stream) {
  VS_REQUIRE(C >= 1 && C <= kRrpMaxC, "vs_rrr_pixel_stats: 1 <= C <= 32768 features");
  VS_REQUIRE(K > 0 && F > 0 && cdiv(F * C, 256) <= 0x7fffffff, "vs_rrr_pixel_stats: K, F must be positive (F C < 2^39)");
  VS_REQUIRE(x_dtype == VS_U8 || x_dtype == VS_F32, "vs_rrr_pixel_stats: X must be u8 or f32");
  VS_REQUIRE(X && mean && sd, "vs_rrr_pixel_stats: null pointer");
  hipStream_t s = (hipStream_t)stream;
  ScopedTimer timer(VS_TIMER_MISC, s, 2.0 * (double)K * F * C * (x_dtype == VS_U8 ? 1.0 : 4.0));
  count_rrr_pixel(VS_RRR_PIXEL_PATH_STATS);
  const dim3 grid((unsigned)cdiv(F * C, 256));
  if (x_dtype == VS_U8)
    hipLaunchKernelGGL(rrp_stats_kernel<uint8_t>, grid, dim3(256), 0, s, K, F * C, (const uint8_t*)X, (double*)mean,
                       (double*)sd);
  else
    hipLaunchKernelGGL(rrp_stats_kernel<float>, grid, dim3(256), 0, s, K, F * C, (const float*)X, (float*)mean,
                       (float*)sd);
  VS_LAUNCH_CHECK();
  return VS_OK;
}

extern "C" size_t vs_rrr_pixel_loss_grad_workspace_bytes(int64_t K, int64_t T, int64_t N, int64_t C, int64_t r) {
  if (K <= 0 || T <= 0 || N <= 0 || N > (1 << 24) || C < 1 || C > kRrpMaxC || r < 1 || r > kRrpMaxR) return 0;
  return rrp_ws(K, T, N, C, r).total;
}

extern "C" int vs_rrr_pixel_loss_grad(int64_t K, int64_t F, int64_t T, int64_t N, int64_t C, int64_t r, const void* X,
                                      int32_t x_dtype, const int64_t* idx, const void* mean, const void* sd,
                                      const void* y, int32_t y_dtype, const double* U, const double* V, const double* b,
                                      double l2, double* loss, double* dU, double* dV, double* db, void* workspace,
                                      void* stream) {
  VS_REQUIRE(C >= 1 && C <= kRrpMaxC, "vs_rrr_pixel_loss_grad: 1 <= C <= 32768 features (without the bias column)");
  VS_REQUIRE(r >= 1 && r <= kRrpMaxR, "vs_rrr_pixel_loss_grad: 1 <= r <= 4 components");
  VS_REQUIRE(rrp_dims_ok(K, F, T, N),
             "vs_rrr_pixel_loss_grad: K, F, T, N must be positive (T <= 65535, K <= 8388480, N <= 16777216)");
  VS_REQUIRE(cdiv(N * (C + T), 256) <= 0x7fffffff, "vs_rrr_pixel_loss_grad: N (C + T) must be below 2^39");
  VS_REQUIRE(x_dtype == VS_U8 || x_dtype == VS_F32, "vs_rrr_pixel_loss_grad: X must be u8 or f32");
  VS_REQUIRE(y_dtype == VS_F32 || y_dtype == VS_F64, "vs_rrr_pixel_loss_grad: y must be f32 or f64");
  VS_REQUIRE(X && idx && mean && sd && y && U && V && b && loss && workspace, "vs_rrr_pixel_loss_grad: null pointer");
  const bool grad = dU || dV || db;
  VS_REQUIRE(!grad || (dU && dV && db), "vs_rrr_pixel_loss_grad: dU, dV, db are given together or not at all");
  VS_REQUIRE((((uintptr_t)workspace) & 15u) == 0, "vs_rrr_pixel_loss_grad: workspace must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const RrpWs w = rrp_ws(K, T, N, C, r);
  char* ws = (char*)workspace;
  double* res = (double*)(ws + w.res);
  double* lossp = (double*)(ws + w.lossp);
  double* dVp = (double*)(ws + w.dVp);
  ScopedTimer timer(VS_TIMER_MISC, s,
                    (double)K * T * ((double)N * (y_dtype == VS_F32 ? 4.0 : 8.0) + C * (x_dtype == VS_U8 ? 1.0 : 4.0)));
  count_rrr_pixel(VS_RRR_PIXEL_PATH_PRODUCT);
  const bool u8 = x_dtype == VS_U8, y32 = y_dtype == VS_F32;
  if (u8 && y32)
    rrp_launch_fwd<uint8_t, float, false>(s, K, F, T, N, (int)C, (int)r, X, idx, mean, sd, y, U, V, b, res);
  else if (u8)
    rrp_launch_fwd<uint8_t, double, false>(s, K, F, T, N, (int)C, (int)r, X, idx, mean, sd, y, U, V, b, res);
  else if (y32)
    rrp_launch_fwd<float, float, false>(s, K, F, T, N, (int)C, (int)r, X, idx, mean, sd, y, U, V, b, res);
  else
    rrp_launch_fwd<float, double, false>(s, K, F, T, N, (int)C, (int)r, X, idx, mean, sd, y, U, V, b, res);
  VS_LAUNCH_CHECK();
  hipLaunchKernelGGL(rrp_sq_kernel, dim3((unsigned)cdiv(N, 256), (unsigned)T), dim3(256), 0, s, K, T, N,
                     (const double*)res, lossp);
  VS_LAUNCH_CHECK();
  hipLaunchKernelGGL(rrp_l2_kernel, dim3((unsigned)w.l2_parts), dim3(256), 0, s, T, N, (int)C, (int)r, l2, U, V, b,
                     lossp + w.sq_parts);
  VS_LAUNCH_CHECK();
  if (grad) {
    if (u8)
      rrp_launch_grad_r<uint8_t>((int)r, s, K, F, T, N, (int)C, l2, X, idx, mean, sd, res, U, V, b, dU, db, dVp);
    else
      rrp_launch_grad_r<float>((int)r, s, K, F, T, N, (int)C, l2, X, idx, mean, sd, res, U, V, b, dU, db, dVp);
    VS_LAUNCH_CHECK();
    hipLaunchKernelGGL(rrp_dv_sum_kernel, dim3((unsigned)cdiv(r * T, 256)), dim3(256), 0, s, T, (int)r, w.tiles,
                       (const double*)dVp, dV);
    VS_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(rrp_loss_kernel, dim3(1), dim3(256), 0, s, w.sq_parts + w.l2_parts, (const double*)lossp, loss);
  VS_LAUNCH_CHECK();
  return VS_OK;
}

extern "C" size_t vs_rrr_pixel_score_workspace_bytes(int64_t K, int64_t T, int64_t N) {
  if (K <= 0 || T <= 0 || N <= 0) return 0;
  return rrw_score_workspace_bytes(K, T, N);
}

extern "C" int vs_rrr_pixel_score(int64_t K, int64_t F, int64_t T, int64_t N, int64_t C, int64_t r, const void* X,
                                  int32_t x_dtype, const int64_t* idx, const void* mean, const void* sd,
                                  const double* U, const double* V, const double* b, const double* mean_y,
                                  const double* std_y, const void* gt, int32_t gt_dtype, double* pred, double* bps,
                                  double* r2, double* out, void* workspace, void* stream) {
  VS_REQUIRE(C >= 1 && C <= kRrpMaxC, "vs_rrr_pixel_score: 1 <= C <= 32768 features (without the bias column)");
  VS_REQUIRE(r >= 1 && r <= kRrpMaxR, "vs_rrr_pixel_score: 1 <= r <= 4 components");
  VS_REQUIRE(rrp_dims_ok(K, F, T, N),
             "vs_rrr_pixel_score: K, F, T, N must be positive (T <= 65535, K <= 8388480, N <= 16777216)");
  VS_REQUIRE(x_dtype == VS_U8 || x_dtype == VS_F32, "vs_rrr_pixel_score: X must be u8 or f32");
  VS_REQUIRE(gt_dtype == VS_F32 || gt_dtype == VS_F64, "vs_rrr_pixel_score: gt must be f32 or f64");
  VS_REQUIRE(X && idx && mean && sd && U && V && b && mean_y && std_y && gt && bps && r2 && out && workspace,
             "vs_rrr_pixel_score: null pointer");
  VS_REQUIRE((((uintptr_t)workspace) & 15u) == 0, "vs_rrr_pixel_score: workspace must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  ScopedTimer timer(VS_TIMER_MISC, s,
                    (double)K * T * ((double)N * ((gt_dtype == VS_F32 ? 4.0 : 8.0) + (pred ? 8.0 : 0.0)) +
                                     C * (x_dtype == VS_U8 ? 1.0 : 4.0)));
  count_rrr_pixel(VS_RRR_PIXEL_PATH_PRODUCT);
  double* yhat = (double*)workspace;   // rrw_score_yhat reads it at offset 0
  if (x_dtype == VS_U8)
    rrp_launch_fwd<uint8_t, double, true>(s, K, F, T, N, (int)C, (int)r, X, idx, mean, sd, nullptr, U, V, b, yhat);
  else
    rrp_launch_fwd<float, double, true>(s, K, F, T, N, (int)C, (int)r, X, idx, mean, sd, nullptr, U, V, b, yhat);
  VS_LAUNCH_CHECK();
  return rrw_score_yhat(s, K, T, N, mean_y, std_y, gt, gt_dtype, pred, bps, r2, out, workspace);
}
