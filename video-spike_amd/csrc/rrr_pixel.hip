// rrr_pixel.hip — the reduced-rank regression (RRR) baseline straight from the pixels: src/train_rrr.py's
// input_mod == 'whisker-video' (train_rrr.py:85-105,143-171), one session whose features are the C = h w pixels of
// a frame, 1 <= C <= 32,768.  Notation is rrr_wide.hip's (K trials, T bins, N neurons, C features + a column of
// ones, r components) plus F, the frames per trial: bin t reads frame idx[t].
// The video X [K][F][C] is stored once in its own dtype (uint8 or float32) and is the only thing of its size:
// an element is standardised on its way into LDS,
//   uint8:   (double(x) - mean[f,c]) / std[f,c]            f64 statistics (numpy's for an integer array)
//   float32: double(float((x - mean[f,c]) / std[f,c]))     f32 statistics, every step rounded to f32 as numpy does
// with a true division (the reference's values bit for bit; DESIGN.md section 7 has the measurement against a
// reciprocal multiply).  The bias column is an implicit 1.  There is no buffer of K T C, K F C or T C N elements.
//
// vs_rrr_pixel_stats: one thread per (f, c) column walking k.  np.mean / np.std / np.clip(., 1e-8) over the trials
//   in numpy's order and roundings (sums ascending in k, the square rounded before it is added).
// vs_rrr_pixel_loss_grad, 4 launches in loss-only mode, 6 with gradients:
//   1. rrr_fwd_kernel    (rrr_core.h) over RrpPixelSrc, the X tile formed from pixels: block = one bin t, 128 trials
//                        x 64 neurons, the features through LDS 32 at a time.  Writes res [K][T][N].
//   2. rrp_sq_kernel     sum_k res^2 per (t, n), k ascending; one partial per (t, 256 neurons) in a fixed tree.
//   3. rrp_l2_kernel     l2 sum_t beta[n,c,t]^2 per (n, c) and l2 b[n,t]^2, one partial per 256 of them.
//   4. rrp_grad_kernel   block = 64 features x 64 neurons, walking every bin t in order.  Per bin G_t = X_t^T 2 res_t
//                        is accumulated on the MFMA over all K trials (rrr_grad_tile, rrr_core.h) and folded while
//                        still in registers, in rrr_reduce_t_kernel's arithmetic:  H = G + 2 l2 beta,
//                        dU[n,c,:] += H V[:,t],  db[n,t] = H of the bias row, and the tile's share of
//                        dV[:,t] = sum U[n,c,:] H (a fixed tree over the block) goes to dVp[tile][j][t].
//                        U[n,c,:] and the dU accumulators stay in registers for the whole walk (2 x 16 r doubles
//                        per lane), which is what caps r at 4.
//   5. rrr_dv_sum_kernel dV[j][t] = the tiles' partials added in tile order.
//   6. rrr_loss_kernel   the partials of 2. and 3. added in a fixed order.
// The loss runs through 1, 2, 3, 6 whether gradients are asked for or not: the same bits.  l2 = 0 makes every l2
// partial an exact 0.  No atomics; every sum's order is fixed by the extents.  Tails add exact zeros and nothing
// outside the operands and the stated workspace is read or written (rrr_fwd_kernel's comment).  A frame index
// outside [0, F) is clamped into it, so no address depends on the contents of idx (vspike.ops checks them).
// Workspace (doubles, each piece rounded up to 256 bytes):
//   K T N  (res)  +  T ceil(N/256) + ceil(N (C + T) / 256)  (loss partials)  +  ceil((C+1)/64) ceil(N/64) r T  (dV
//   partials)
// i.e. 0.17 GB at K 400, T 100, N 512, C 18,260, r 3.
// vs_rrr_pixel_score: rrr_fwd_kernel (standardised yhat to the workspace) + rrr.hip's scoring kernels.
#include "rrr_core.h"

namespace vs {

constexpr int kRrpMaxC = 32768;
constexpr int kRrpMaxR = 4;

template <typename XT> struct RrpStat;
template <> struct RrpStat<uint8_t> { typedef double type; };
template <> struct RrpStat<float> { typedef float type; };

__device__ __forceinline__ double rrp_z(uint8_t x, double m, double q) { return ((double)x - m) / q; }
// the correctly rounded f32 quotient (53 >= 2 * 24 + 2 bits), widened
__device__ __forceinline__ double rrp_z(float x, float m, float q) {
  const float d = x - m;
  return (double)(float)((double)d / (double)q);
}

// The pixel video X [K][F][C], uint8 / float32 with mean / sd [F][C]: bin t reads frame idx[t] (an index outside
// [0, F) is clamped into it), an element is standardised when it is staged, and there is an implicit 1 at and past
// column C (their loads are clamped to column C - 1).
template <typename XT> struct RrpPixelSrc {
  typedef typename RrpStat<XT>::type ST;
  typedef XT Raw;
  struct Col { ST m, s; };
  const XT* X;
  const int64_t* idx;
  const ST *mean, *sd;
  int64_t F;
  __device__ __forceinline__ int64_t bin(int64_t t) const {
    const int64_t f = idx[t];
    return f < 0 ? 0 : (f < F ? f : F - 1);
  }
  __device__ __forceinline__ int clamp(int c, int C) const { return c < C ? c : C - 1; }
  __device__ __forceinline__ Col col(int64_t f, int cc, int C) const {
    const int64_t row = f * C;                     // wave-uniform: the row's base stays in scalar registers
    return Col{(mean + row)[cc], (sd + row)[cc]};
  }
  __device__ __forceinline__ XT load(int64_t k, int64_t f, int cc, int C) const { return X[(k * F + f) * C + cc]; }
  __device__ __forceinline__ double stage(XT x, Col s, int c, int C) const { return c < C ? rrp_z(x, s.m, s.s) : 1.0; }
};

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
  sq = rrr_block_sum(sq, red);
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
  const double s = rrr_block_sum(l2 * term, red);
  if (threadIdx.x == 0) lossp[blockIdx.x] = s;
}

// ---- gradient product with the fold --------------------------------------------------------------------------
// grid (ceil(N/64), ceil((C+1)/64)).  rrr_grad_tile's D element (m, q) of wave w, lane (li, lk) is feature
// c0 + 16 m + lk + 4 q and neuron n0 + 16 w + li; features > C and neurons >= N are never stored and enter dV as 0.
template <typename XT, int R>
__global__ __launch_bounds__(256) void rrp_grad_kernel(int64_t K, int64_t T, int64_t N, int C, double l2,
                                                       const RrpPixelSrc<XT> src, const double* __restrict__ Rres,
                                                       const double* __restrict__ U, const double* __restrict__ V,
                                                       const double* __restrict__ b, double* __restrict__ dU,
                                                       double* __restrict__ db, double* __restrict__ dVp) {
  __shared__ double Xs[kRrrStep * kRrrTile];
  __shared__ double Rs[kRrrStep * kRrrTile];
  __shared__ double dvs[4 * R];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lk = lane >> 4;
  const int64_t n0 = (int64_t)blockIdx.x * kRrrTile;
  const int c0 = (int)blockIdx.y * kRrrTile;
  const int64_t tile = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
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
  for (int64_t t = 0; t < T; ++t) {
    double v[R];
#pragma unroll
    for (int j = 0; j < R; ++j) v[j] = V[(int64_t)j * T + t];
    f64x4 acc[4];
    rrr_grad_tile(src, K, T, N, C, t, n0, c0, Rres, Xs, Rs, acc);
    // the fold: rrr_reduce_t_kernel's H = G + 2 l2 beta, dU += H V^T, db; rrw_dv_kernel's sum U H over the tile
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

struct RrpWs {
  int64_t sq_parts, l2_parts, tiles;
  size_t res, lossp, dVp, total;  // byte offsets
};
static RrpWs rrp_ws(int64_t K, int64_t T, int64_t N, int64_t C, int64_t r) {
  RrpWs w;
  w.sq_parts = T * cdiv(N, 256);
  w.l2_parts = cdiv(N * (C + T), 256);
  w.tiles = cdiv(C + 1, kRrrTile) * cdiv(N, kRrrTile);
  auto al = [](size_t bytes) { return (bytes + 255) / 256 * 256; };
  size_t off = 0;
  w.res = off;   off += al((size_t)K * T * N * 8);
  w.lossp = off; off += al((size_t)(w.sq_parts + w.l2_parts) * 8);
  w.dVp = off;   off += al((size_t)w.tiles * r * T * 8);
  w.total = off;
  return w;
}

static bool rrp_dims_ok(int64_t K, int64_t F, int64_t T, int64_t N) {
  return K > 0 && F > 0 && T > 0 && N > 0 && T <= 65535 && cdiv(K, kRrrFwdTrials) <= 65535 && N <= (1 << 24);
}

template <typename XT>
static RrpPixelSrc<XT> rrp_src(const void* X, const int64_t* idx, const void* mean, const void* sd, int64_t F) {
  typedef typename RrpStat<XT>::type ST;
  return RrpPixelSrc<XT>{(const XT*)X, idx, (const ST*)mean, (const ST*)sd, F};
}

template <typename XT, typename YT, bool SCORE>
static void rrp_launch_fwd(hipStream_t s, int64_t K, int64_t T, int64_t N, int C, int r, const RrpPixelSrc<XT>& src,
                           const void* y, const double* U, const double* V, const double* b, double* out) {
  const dim3 grid((unsigned)cdiv(N, kRrrTile), (unsigned)T, (unsigned)cdiv(K, kRrrFwdTrials));
  hipLaunchKernelGGL((rrr_fwd_kernel<RrpPixelSrc<XT>, YT, SCORE, 4>), grid, dim3(256), 0, s, K, T, N, C, r, src,
                     (const YT*)y, U, V, b, out);
}

template <typename XT, int R>
static void rrp_launch_grad(hipStream_t s, int64_t K, int64_t T, int64_t N, int C, double l2, const RrpPixelSrc<XT>& src,
                            const double* res, const double* U, const double* V, const double* b, double* dU,
                            double* db, double* dVp) {
  const dim3 grid((unsigned)cdiv(N, kRrrTile), (unsigned)cdiv(C + 1, kRrrTile));
  hipLaunchKernelGGL((rrp_grad_kernel<XT, R>), grid, dim3(256), 0, s, K, T, N, C, l2, src, res, U, V, b, dU, db, dVp);
}

// vs_rrr_pixel_loss_grad's launches for frames of type XT
template <typename XT>
static int rrp_loss_grad(hipStream_t s, int64_t K, int64_t T, int64_t N, int C, int r, const RrpPixelSrc<XT>& src,
                         const void* y, int32_t y_dtype, const double* U, const double* V, const double* b, double l2,
                         double* loss, double* dU, double* dV, double* db, const RrpWs& w, char* ws) {
  double* res = (double*)(ws + w.res);
  double* lossp = (double*)(ws + w.lossp);
  double* dVp = (double*)(ws + w.dVp);
  if (y_dtype == VS_F32)
    rrp_launch_fwd<XT, float, false>(s, K, T, N, C, r, src, y, U, V, b, res);
  else
    rrp_launch_fwd<XT, double, false>(s, K, T, N, C, r, src, y, U, V, b, res);
  VS_LAUNCH_CHECK();
  hipLaunchKernelGGL(rrp_sq_kernel, dim3((unsigned)cdiv(N, 256), (unsigned)T), dim3(256), 0, s, K, T, N,
                     (const double*)res, lossp);
  VS_LAUNCH_CHECK();
  hipLaunchKernelGGL(rrp_l2_kernel, dim3((unsigned)w.l2_parts), dim3(256), 0, s, T, N, C, r, l2, U, V, b,
                     lossp + w.sq_parts);
  VS_LAUNCH_CHECK();
  if (dU) {
    switch (r) {
      case 1: rrp_launch_grad<XT, 1>(s, K, T, N, C, l2, src, res, U, V, b, dU, db, dVp); break;
      case 2: rrp_launch_grad<XT, 2>(s, K, T, N, C, l2, src, res, U, V, b, dU, db, dVp); break;
      case 3: rrp_launch_grad<XT, 3>(s, K, T, N, C, l2, src, res, U, V, b, dU, db, dVp); break;
      default: rrp_launch_grad<XT, 4>(s, K, T, N, C, l2, src, res, U, V, b, dU, db, dVp); break;
    }
    VS_LAUNCH_CHECK();
    rrr_launch_dv_sum(s, T, r, w.tiles, r * T, dVp, dV);
    VS_LAUNCH_CHECK();
  }
  rrr_launch_loss(s, w.sq_parts + w.l2_parts, lossp, loss);
  VS_LAUNCH_CHECK();
  return VS_OK;
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
  VS_CALL(rrr_check_loss_grad("vs_rrr_pixel_loss_grad", y_dtype,
                              X && idx && mean && sd && y && U && V && b && loss && workspace, dU, dV, db, workspace));
  hipStream_t s = (hipStream_t)stream;
  const RrpWs w = rrp_ws(K, T, N, C, r);
  ScopedTimer timer(VS_TIMER_MISC, s,
                    (double)K * T * ((double)N * (y_dtype == VS_F32 ? 4.0 : 8.0) + C * (x_dtype == VS_U8 ? 1.0 : 4.0)));
  count_rrr_pixel(VS_RRR_PIXEL_PATH_PRODUCT);
  if (x_dtype == VS_U8)
    return rrp_loss_grad(s, K, T, N, (int)C, (int)r, rrp_src<uint8_t>(X, idx, mean, sd, F), y, y_dtype, U, V, b, l2,
                         loss, dU, dV, db, w, (char*)workspace);
  return rrp_loss_grad(s, K, T, N, (int)C, (int)r, rrp_src<float>(X, idx, mean, sd, F), y, y_dtype, U, V, b, l2, loss,
                       dU, dV, db, w, (char*)workspace);
}

extern "C" size_t vs_rrr_pixel_score_workspace_bytes(int64_t K, int64_t T, int64_t N) {
  if (K <= 0 || T <= 0 || N <= 0) return 0;
  return rrr_score_workspace_bytes(K, T, N, true);
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
  VS_CALL(rrr_check_score("vs_rrr_pixel_score", gt_dtype,
                          X && idx && mean && sd && U && V && b && mean_y && std_y && gt && bps && r2 && out && workspace,
                          workspace));
  hipStream_t s = (hipStream_t)stream;
  ScopedTimer timer(VS_TIMER_MISC, s,
                    (double)K * T * ((double)N * ((gt_dtype == VS_F32 ? 4.0 : 8.0) + (pred ? 8.0 : 0.0)) +
                                     C * (x_dtype == VS_U8 ? 1.0 : 4.0)));
  count_rrr_pixel(VS_RRR_PIXEL_PATH_PRODUCT);
  double* yhat = (double*)workspace;   // rrr_score_yhat reads it at offset 0
  if (x_dtype == VS_U8)
    rrp_launch_fwd<uint8_t, double, true>(s, K, T, N, (int)C, (int)r, rrp_src<uint8_t>(X, idx, mean, sd, F), nullptr, U,
                                          V, b, yhat);
  else
    rrp_launch_fwd<float, double, true>(s, K, T, N, (int)C, (int)r, rrp_src<float>(X, idx, mean, sd, F), nullptr, U, V,
                                        b, yhat);
  VS_LAUNCH_CHECK();
  return rrr_score_yhat(s, K, T, N, mean_y, std_y, gt, gt_dtype, pred, bps, r2, out, workspace);
}
