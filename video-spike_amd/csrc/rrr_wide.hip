// rrr_wide.hip — the reduced-rank regression (RRR) baseline for wide inputs (1 <= C <= 1024 features, e.g. the
// 768 of a ViT-Base embedding), and the Gaussian smoothing of its targets:
//   src/model/rrr.py:79-155,164-175   RRRGD's beta / predict / MSE / l2 term and the L-BFGS closure
//   src/train_rrr.py:118,193-236      gaussian_filter1d(y, 2, axis=1) and the scoring of the held-out trials
// Notation is rrr.hip's (K trials, T bins, N neurons, C features + a column of ones, r components).  rrr.hip
// keeps beta[n,:,t] in registers, which stops at C = 32; here each time bin is two f64 GEMMs on the f64 MFMA
// (v_mfma_f64_16x16x4_f64; A[i][k]: lane = i + 16 k, B[k][j]: lane = j + 16 k, D[i][j]: lane = j + 16 (i & 3),
// register i >> 2):
//   Yhat_t [K x N]     = X_t [K x (C+1)] . Beta_t [(C+1) x N]          res = Yhat - y
//   G_t    [(C+1) x N] = X_t^T . 2 res
// Beta_t is never stored: a B tile is formed from U[n,c,:] and V[:,t] (r FMAs per element) on its way into LDS.
// Everything is f64 (y / gt may be f32: converted in the load).  No atomics; every reduction runs in an order
// fixed by the extents alone, so two calls on the same inputs agree bitwise.  Tails (K, C+1, N not multiples of
// the tiles) add exact zeros, and nothing outside the operands is read or written (rrr_fwd_kernel's comment).
//
// vs_rrr_wide_loss_grad, 4 launches in loss-only mode, 7 with gradients:
//   1. rrr_fwd_kernel     (rrr_core.h) over RrwDenseSrc: block = one bin t, 128 trials x 64 neurons; the features go
//                         through LDS 32 at a time (X tile + Beta tile), the next slice's loads in flight under the
//                         MFMAs.  Writes res [K][T][N].
//   2. rrw_sq_kernel      sq[t][n] = sum_k res^2 (k ascending), the last row of G.
//   3. rrw_grad_kernel    block = one bin t, 64 features x 64 neurons: rrr_grad_tile (rrr_core.h), then the store of
//                         G[t][c][n] (rows 0..C; row C+1 = sq), the layout of rrr.hip's partials.
//   4. rrr_reduce_t_kernel (rrr_core.h, one partial, loss terms per block) / rrw_dv_kernel + rrr_dv_sum_kernel /
//                         rrr_loss_kernel: H = G + 2 l2 beta (in place), db, dU = H V^T, dV, the l2 terms and the
//                         loss, in the arithmetic of rrr.hip's tail (dV's sum over (n, c) is split into feature
//                         chunks whose partials are added in order).
// Workspace (doubles, each piece rounded up to 256 bytes):
//   K T N  (res)  +  T (C+2) N  (G, then H)  +  (C+2) ceil(N/64)  (loss terms)  +  chunks 8 T  (dV partials,
//   chunks <= 32)
// i.e. 0.48 GB at K 400, T 100, N 512, C 768.
// vs_rrr_wide_score: rrr_fwd_kernel (standardised yhat to the workspace, K T N doubles) + rrr.hip's scoring kernels
//   (rrr_score_yhat).
// vs_gauss_smooth_time: one thread per (k, n) column walking t; scipy's order of additions, no FMA.
#include "rrr_core.h"

namespace vs {

constexpr int kRrwMaxC = 1024;
constexpr int kRrwDvChunks = 32;

// The dense float64 X [K][T][C+1]: the bias column is read from memory, and columns past it are clamped to the
// row's own last column (against zeroed V factors).
struct RrwDenseSrc {
  typedef double Raw;
  struct Col {};
  const double* X;
  int64_t T;
  __device__ __forceinline__ int64_t bin(int64_t t) const { return t; }
  __device__ __forceinline__ int clamp(int c, int C) const { return c < C + 1 ? c : C; }
  __device__ __forceinline__ Col col(int64_t, int, int) const { return Col{}; }
  __device__ __forceinline__ double load(int64_t k, int64_t t, int cc, int C) const {
    return X[(k * T + t) * (C + 1) + cc];
  }
  __device__ __forceinline__ double stage(double x, Col, int, int) const { return x; }
};

// grid (ceil(N/256), T): G[t][C+1][n] = sum_k res[k,t,n]^2, k ascending
__global__ __launch_bounds__(256) void rrw_sq_kernel(int64_t K, int64_t T, int64_t N, int C,
                                                     const double* __restrict__ R, double* __restrict__ G) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t t = blockIdx.y;
  if (n >= N) return;
  double sq = 0.0;
  for (int64_t k = 0; k < K; ++k) {
    const double res = R[(k * T + t) * N + n];
    sq = fma(res, res, sq);
  }
  G[(t * (C + 2) + (C + 1)) * N + n] = sq;
}

// grid (ceil(N/64), T, ceil((C+1)/64)): G[t][c][n] = sum_k X[k,t,c] 2 res[k,t,n] (rrr_grad_tile's order)
__global__ __launch_bounds__(256) void rrw_grad_kernel(int64_t K, int64_t T, int64_t N, int C, const RrwDenseSrc src,
                                                       const double* __restrict__ R, double* __restrict__ G) {
  __shared__ double Xs[kRrrStep * kRrrTile];
  __shared__ double Rs[kRrrStep * kRrrTile];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int li = lane & 15, lk = lane >> 4;
  const int64_t t = blockIdx.y;
  const int64_t n0 = (int64_t)blockIdx.x * kRrrTile;
  const int c0 = (int)blockIdx.z * kRrrTile;
  f64x4 acc[4];
  rrr_grad_tile(src, K, T, N, C, t, n0, c0, R, Xs, Rs, acc);
  const int64_t n = n0 + 16 * w + li;
  if (n < N) {
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = c0 + 16 * m + lk + 4 * q;
        if (c < C + 1) G[(t * (C + 2) + c) * N + n] = acc[m][q];
      }
  }
}

// grid (T, chunks): dVp[ch][j][t] = sum over n and the chunk's features c of U[n,c,j] H[t][c][n]; a thread walks
// i = n cw + (c - c_lo) in steps of 256, so U is read along its rows
__global__ __launch_bounds__(256) void rrw_dv_kernel(int64_t T, int64_t N, int C, int r, int cper,
                                                     const double* __restrict__ U, const double* __restrict__ H,
                                                     double* __restrict__ dVp) {
  __shared__ double red[256];
  const int64_t t = blockIdx.x;
  const int ch = blockIdx.y;
  const int clo = ch * cper;
  const int cw = (clo + cper < C ? clo + cper : C) - clo;
  const double* h = H + t * (C + 2) * N;
  double acc[kRrrMaxR];
#pragma unroll
  for (int j = 0; j < kRrrMaxR; ++j) acc[j] = 0.0;
  for (int64_t i = threadIdx.x; i < (int64_t)cw * N; i += 256) {
    const int64_t n = i / cw;
    const int c = clo + (int)(i - n * cw);
    const double hv = h[(int64_t)c * N + n];
    const double* up = U + (n * C + c) * r;
#pragma unroll
    for (int j = 0; j < kRrrMaxR; ++j)
      if (j < r) acc[j] = fma(up[j], hv, acc[j]);
  }
  for (int j = 0; j < r; ++j) {
    const double s = rrr_block_sum(acc[j], red);
    if (threadIdx.x == 0) dVp[((int64_t)ch * kRrrMaxR + j) * T + t] = s;
  }
}

struct RrwWs {
  int chunks, cper;
  size_t res, G, lossp, dVp, total;  // byte offsets
};
static RrwWs rrw_ws(int64_t K, int64_t T, int64_t N, int64_t C) {
  RrwWs w;
  w.cper = (int)cdiv(C, kRrwDvChunks);
  w.chunks = (int)cdiv(C, w.cper);
  auto al = [](size_t bytes) { return (bytes + 255) / 256 * 256; };
  size_t off = 0;
  w.res = off;   off += al((size_t)K * T * N * 8);
  w.G = off;     off += al((size_t)T * (C + 2) * N * 8);
  w.lossp = off; off += al((size_t)(C + 2) * cdiv(N, 64) * 8);
  w.dVp = off;   off += al((size_t)w.chunks * kRrrMaxR * T * 8);
  w.total = off;
  return w;
}

static bool rrw_dims_ok(int64_t K, int64_t T, int64_t N) {
  return K > 0 && T > 0 && N > 0 && T <= 65535 && cdiv(K, kRrrFwdTrials) <= 65535 && cdiv(N, 64) <= 0x7fffffff;
}

template <typename YT, bool SCORE>
static void rrw_launch_fwd(hipStream_t s, int64_t K, int64_t T, int64_t N, int C, int r, const double* X, const void* y,
                           const double* U, const double* V, const double* b, double* out) {
  const dim3 grid((unsigned)cdiv(N, kRrrTile), (unsigned)T, (unsigned)cdiv(K, kRrrFwdTrials));
  const RrwDenseSrc src{X, T};
  if (r <= 4)
    hipLaunchKernelGGL((rrr_fwd_kernel<RrwDenseSrc, YT, SCORE, 4>), grid, dim3(256), 0, s, K, T, N, C, r, src,
                       (const YT*)y, U, V, b, out);
  else
    hipLaunchKernelGGL((rrr_fwd_kernel<RrwDenseSrc, YT, SCORE, 8>), grid, dim3(256), 0, s, K, T, N, C, r, src,
                       (const YT*)y, U, V, b, out);
}

// ---- Gaussian smoothing along time -----------------------------------------------------------------------
// scipy.ndimage.gaussian_filter1d(y, sigma, axis=1, mode='reflect'): the line is held in f64, the symmetric
// kernel is applied as  acc = in[t] w[R];  acc = (in[t-j] + in[t+j]) w[R-j] + acc  for j = R .. 1  with the
// product and the sum rounded separately (an FMA changes the bits), and the result is rounded once to y's dtype.
// reflect: index -1 -> 0, T -> T-1 (one reflection: radius <= T - 1).  grid (K, ceil(N/256)).
template <typename YT>
__global__ __launch_bounds__(256) void gauss_smooth_time_kernel(int64_t T, int64_t N, int radius,
                                                                const YT* __restrict__ y,
                                                                const double* __restrict__ wgt, YT* __restrict__ out) {
  const int64_t n = (int64_t)blockIdx.y * 256 + threadIdx.x;
  const int64_t k = blockIdx.x;
  if (n >= N) return;
  const YT* in = y + k * T * N + n;
  YT* o = out + k * T * N + n;
  for (int64_t t = 0; t < T; ++t) {
    double acc = __dmul_rn((double)in[t * N], wgt[radius]);
    for (int j = radius; j >= 1; --j) {
      int64_t lo = t - j, hi = t + j;
      if (lo < 0) lo = -lo - 1;
      if (hi >= T) hi = 2 * T - 1 - hi;
      const double pair = __dadd_rn((double)in[lo * N], (double)in[hi * N]);
      // __dmul_rn / __dadd_rn are plain * and + to the compiler, which fuses them (the contraction pragma is not
      // honoured under -ffp-contract=fast): the product passes through an opaque copy, so it is rounded first
      double prod = __dmul_rn(pair, wgt[radius - j]);
      asm volatile("" : "+v"(prod));
      acc = __dadd_rn(prod, acc);
    }
    o[t * N] = (YT)acc;
  }
}

}  // namespace vs

using namespace vs;

extern "C" size_t vs_rrr_wide_loss_grad_workspace_bytes(int64_t K, int64_t T, int64_t N, int64_t C) {
  if (K <= 0 || T <= 0 || N <= 0 || C < 1 || C > kRrwMaxC) return 0;
  return rrw_ws(K, T, N, C).total;
}

extern "C" int vs_rrr_wide_loss_grad(int64_t K, int64_t T, int64_t N, int64_t C, int64_t r, const double* X,
                                     const void* y, int32_t y_dtype, const double* U, const double* V, const double* b,
                                     double l2, double* loss, double* dU, double* dV, double* db, void* workspace,
                                     void* stream) {
  VS_REQUIRE(C >= 1 && C <= kRrwMaxC, "vs_rrr_wide_loss_grad: 1 <= C <= 1024 features (without the bias column)");
  VS_REQUIRE(r >= 1 && r <= kRrrMaxR, "vs_rrr_wide_loss_grad: 1 <= r <= 8 components");
  VS_REQUIRE(rrw_dims_ok(K, T, N), "vs_rrr_wide_loss_grad: K, T, N must be positive (T <= 65535, K <= 8388480)");
  VS_CALL(rrr_check_loss_grad("vs_rrr_wide_loss_grad", y_dtype, X && y && U && V && b && loss && workspace, dU, dV, db,
                              workspace));
  const bool grad = dU != nullptr;
  hipStream_t s = (hipStream_t)stream;
  const RrwWs w = rrw_ws(K, T, N, C);
  char* ws = (char*)workspace;
  double* res = (double*)(ws + w.res);
  double* G = (double*)(ws + w.G);
  double* lossp = (double*)(ws + w.lossp);
  double* dVp = (double*)(ws + w.dVp);
  ScopedTimer timer(VS_TIMER_MISC, s,
                    (double)K * T * ((double)N * (y_dtype == VS_F32 ? 4.0 : 8.0) + (C + 1) * 8.0));
  count_rrr(VS_RRR_PATH_WIDE);
  if (y_dtype == VS_F32)
    rrw_launch_fwd<float, false>(s, K, T, N, (int)C, (int)r, X, y, U, V, b, res);
  else
    rrw_launch_fwd<double, false>(s, K, T, N, (int)C, (int)r, X, y, U, V, b, res);
  VS_LAUNCH_CHECK();
  hipLaunchKernelGGL(rrw_sq_kernel, dim3((unsigned)cdiv(N, 256), (unsigned)T), dim3(256), 0, s, K, T, N, (int)C,
                     (const double*)res, G);
  VS_LAUNCH_CHECK();
  if (grad) {
    hipLaunchKernelGGL(rrw_grad_kernel, dim3((unsigned)cdiv(N, kRrrTile), (unsigned)T, (unsigned)cdiv(C + 1, kRrrTile)),
                       dim3(256), 0, s, K, T, N, (int)C, RrwDenseSrc{X, T}, (const double*)res, G);
    VS_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(rrr_reduce_t_kernel<true>, dim3((unsigned)cdiv(N, 64), (unsigned)(C + 2)), dim3(256), 0, s, T, N,
                     (int)C, (int)r, 1, l2, grad ? 1 : 0, G, U, V, b, dU, db, lossp);
  VS_LAUNCH_CHECK();
  if (grad) {
    hipLaunchKernelGGL(rrw_dv_kernel, dim3((unsigned)T, (unsigned)w.chunks), dim3(256), 0, s, T, N, (int)C, (int)r,
                       w.cper, U, (const double*)G, dVp);
    VS_LAUNCH_CHECK();
    rrr_launch_dv_sum(s, T, (int)r, w.chunks, kRrrMaxR * T, dVp, dV);
    VS_LAUNCH_CHECK();
  }
  rrr_launch_loss(s, (int64_t)(C + 2) * cdiv(N, 64), lossp, loss);
  VS_LAUNCH_CHECK();
  return VS_OK;
}

extern "C" size_t vs_rrr_wide_score_workspace_bytes(int64_t K, int64_t T, int64_t N) {
  if (K <= 0 || T <= 0 || N <= 0) return 0;
  return rrr_score_workspace_bytes(K, T, N, true);
}

extern "C" int vs_rrr_wide_score(int64_t K, int64_t T, int64_t N, int64_t C, int64_t r, const double* X,
                                 const double* U, const double* V, const double* b, const double* mean_y,
                                 const double* std_y, const void* gt, int32_t gt_dtype, double* pred, double* bps,
                                 double* r2, double* out, void* workspace, void* stream) {
  VS_REQUIRE(C >= 1 && C <= kRrwMaxC, "vs_rrr_wide_score: 1 <= C <= 1024 features (without the bias column)");
  VS_REQUIRE(r >= 1 && r <= kRrrMaxR, "vs_rrr_wide_score: 1 <= r <= 8 components");
  VS_REQUIRE(rrw_dims_ok(K, T, N), "vs_rrr_wide_score: K, T, N must be positive (T <= 65535, K <= 8388480)");
  VS_CALL(rrr_check_score("vs_rrr_wide_score", gt_dtype,
                          X && U && V && b && mean_y && std_y && gt && bps && r2 && out && workspace, workspace));
  hipStream_t s = (hipStream_t)stream;
  ScopedTimer timer(VS_TIMER_MISC, s,
                    (double)K * T * ((double)N * ((gt_dtype == VS_F32 ? 4.0 : 8.0) + (pred ? 8.0 : 0.0)) + (C + 1) * 8.0));
  count_rrr(VS_RRR_PATH_WIDE);
  rrw_launch_fwd<double, true>(s, K, T, N, (int)C, (int)r, X, nullptr, U, V, b, (double*)workspace);
  VS_LAUNCH_CHECK();
  return rrr_score_yhat(s, K, T, N, mean_y, std_y, gt, gt_dtype, pred, bps, r2, out, workspace);
}

extern "C" int vs_gauss_smooth_time(int64_t K, int64_t T, int64_t N, const void* y, int32_t dtype,
                                    const double* weights, int64_t radius, void* out, void* stream) {
  VS_REQUIRE(K > 0 && T > 0 && N > 0 && K <= 0x7fffffff && cdiv(N, 256) <= 65535,
             "vs_gauss_smooth_time: K, T, N must be positive (N <= 16776960)");
  VS_REQUIRE(radius >= 0 && radius <= 4096, "vs_gauss_smooth_time: 0 <= radius <= 4096");
  VS_REQUIRE(T >= radius + 1, "vs_gauss_smooth_time: T >= radius + 1 (a single reflection at each end)");
  VS_REQUIRE(dtype == VS_F32 || dtype == VS_F64, "vs_gauss_smooth_time: y must be f32 or f64");
  VS_REQUIRE(y && weights && out && y != out, "vs_gauss_smooth_time: null pointer (or out aliases y)");
  hipStream_t s = (hipStream_t)stream;
  ScopedTimer timer(VS_TIMER_MISC, s, 2.0 * (double)K * T * N * (dtype == VS_F32 ? 4.0 : 8.0));
  count_rrr(VS_RRR_PATH_SMOOTH);
  const dim3 grid((unsigned)K, (unsigned)cdiv(N, 256));
  if (dtype == VS_F32)
    hipLaunchKernelGGL(gauss_smooth_time_kernel<float>, grid, dim3(256), 0, s, T, N, (int)radius, (const float*)y,
                       weights, (float*)out);
  else
    hipLaunchKernelGGL(gauss_smooth_time_kernel<double>, grid, dim3(256), 0, s, T, N, (int)radius, (const double*)y,
                       weights, (double*)out);
  VS_LAUNCH_CHECK();
  return VS_OK;
}
