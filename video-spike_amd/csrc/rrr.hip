// rrr.hip — the reduced-rank regression (RRR) validation of the contrastive pretraining path:
//   src/model/rrr.py:79-155,164-175   RRRGD's beta / predict / MSE / l2 term and the L-BFGS closure
//   src/utils/utils.py:411-447        train_rrr's scoring (clip, bits_per_spike, sklearn r2_score per trial)
// K trials, T bins, N neurons, C features (X carries a trailing column of ones), r components:
//   beta[n,c,t] = sum_j U[n,c,j] V[j,t] (c < C),  beta[n,C,t] = b[n,t]
//   yhat[k,t,n] = sum_c X[k,t,c] beta[n,c,t],     loss = sum (yhat - y)^2 + l2 sum beta^2   (b^2 included)
// Everything is f64 (y / gt may be f32: converted in the load).  No atomics; every reduction runs in an order
// fixed by the extents alone, so two calls on the same inputs agree bitwise.
//
// vs_rrr_loss_grad, 4 launches (2 in loss-only mode):
//   1. rrr_accum_kernel    block = 64 neurons x 4 waves, one bin t.  A thread owns neuron n and keeps beta[n,:,t]
//                          in registers; X[k,t,:] is wave-uniform (scalar loads), y[k,t,n..n+63] one contiguous
//                          row piece.  Each wave takes a slice of the trials and accumulates sq = sum res^2 and
//                          G[c] = sum X[k,t,c] 2 res; waves 1..3 hand theirs to wave 0 through LDS (added in wave
//                          order).  When T * ceil(N/64) is a small grid the trials are also split over S blocks
//                          (ordered partials).  Writes part[s][t][c][n] (rows 0..C = G, row C+1 = sq):
//                          S T (C+2) N doubles, nothing of size K T N.  y and X are read exactly once.
//   2. rrr_reduce_t_kernel (rrr_core.h, loss terms per lane) sums the S partials and forms H = G + 2 l2 beta
//                          over partial 0 (kept [t][c][n], C+2 rows per bin, for step 3), db, dU and the loss terms.
//   3. rrr_dv_kernel       block = one bin t: dV[:,t] = sum_{n,c} U[n,c,:] H[t][c][n] (strided + LDS tree).
//   4. rrr_loss_kernel     one block: loss = sum of the (C+2) N loss terms (strided + LDS tree).
// Scoring, for all three units: rrr_score_kernel (block = 64 neurons x 4 waves, wave = a slice of the held-out
//   trials; a thread walks its neuron's T bins of one trial, so the trial's R^2 is complete in registers), over
//   where yhat comes from (computed here from X, U, V, b: vs_rrr_score; read from the workspace: the wide and
//   pixel entries through rrr_score_yhat) + rrr_score_final_kernel.
// This unit also holds the kernels of rrr_core.h that are not templates (rrr_loss_kernel, rrr_dv_sum_kernel) and
// the argument checks the three units' entries share.
#include <stdio.h>

#include "rrr_core.h"

namespace vs {

constexpr int kRrrMaxC = 32;
constexpr int kRrrMaxSplit = 16;

// CP: C + 1 rounded up to a compiled size (rows C+1 .. CP-1 are zeros)
template <typename YT, int CP, bool GRAD>
__global__ __launch_bounds__(256) void rrr_accum_kernel(int64_t K, int64_t T, int64_t N, int C, int r, int64_t kper,
                                                        const double* __restrict__ X, const YT* __restrict__ y,
                                                        const double* __restrict__ U, const double* __restrict__ V,
                                                        const double* __restrict__ b, double* __restrict__ part) {
  constexpr int kVals = GRAD ? CP + 1 : 1;
  __shared__ double red[(kRrrWaves - 1) * kVals * 64];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t t = blockIdx.y;
  const int64_t n = (int64_t)blockIdx.x * 64 + lane;
  const bool live = n < N;
  const int C1 = C + 1;
  double beta[CP];
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    beta[c] = 0.0;
    if (live && c < C) {
      double u[kRrrMaxR];
#pragma unroll
      for (int j = 0; j < kRrrMaxR; ++j) u[j] = j < r ? U[(n * C + c) * r + j] : 0.0;
      beta[c] = rrr_beta(u, V, r, T, t);
    } else if (live && c == C) {
      beta[c] = b[n * T + t];
    }
  }
  double G[GRAD ? CP : 1];
#pragma unroll
  for (int c = 0; c < (GRAD ? CP : 1); ++c) G[c] = 0.0;
  double sq = 0.0;
  const int64_t k0 = ((int64_t)blockIdx.z * kRrrWaves + w) * kper;
  const int64_t k1 = k0 + kper < K ? k0 + kper : K;
#pragma unroll 4
  for (int64_t k = k0; k < k1; ++k) {
    const double* xr = X + (k * T + t) * C1;
    const double yv = live ? ld_f64(y + (k * T + t) * N + n) : 0.0;
    double x[CP];
#pragma unroll
    for (int c = 0; c < CP; ++c) x[c] = c < C1 ? xr[c] : 0.0;
    double yh = 0.0;
#pragma unroll
    for (int c = 0; c < CP; ++c) yh = fma(x[c], beta[c], yh);
    const double res = yh - yv;
    sq = fma(res, res, sq);
    if (GRAD) {
      const double g = 2.0 * res;
#pragma unroll
      for (int c = 0; c < CP; ++c) G[c] = fma(x[c], g, G[c]);
    }
  }
  if (w > 0) {
    double* p = red + (size_t)(w - 1) * kVals * 64 + lane;
    p[0] = sq;
    if (GRAD) {
#pragma unroll
      for (int c = 0; c < CP; ++c) p[(c + 1) * 64] = G[c];
    }
  }
  __syncthreads();
  if (w == 0 && live) {
    for (int v = 1; v < kRrrWaves; ++v) {
      const double* p = red + (size_t)(v - 1) * kVals * 64 + lane;
      sq += p[0];
      if (GRAD) {
#pragma unroll
        for (int c = 0; c < CP; ++c) G[c] += p[(c + 1) * 64];
      }
    }
    double* o = part + (((int64_t)blockIdx.z * T + t) * (C + 2)) * N + n;
    if (GRAD) {
#pragma unroll
      for (int c = 0; c < CP; ++c)
        if (c < C1) o[(int64_t)c * N] = G[c];
    }
    o[(int64_t)(C + 1) * N] = sq;
  }
}

// block t: dV[j,t] = sum over i = c N + n (c < C) of U[n,c,j] H[t][c][n] (H: C+2 rows per bin)
__global__ __launch_bounds__(256) void rrr_dv_kernel(int64_t T, int64_t N, int C, int r, const double* __restrict__ U,
                                                     const double* __restrict__ H, double* __restrict__ dV) {
  __shared__ double red[256];
  const int64_t t = blockIdx.x;
  const double* h = H + t * (C + 2) * N;
  double acc[kRrrMaxR];
#pragma unroll
  for (int j = 0; j < kRrrMaxR; ++j) acc[j] = 0.0;
  for (int64_t i = threadIdx.x; i < (int64_t)C * N; i += 256) {
    const int64_t c = i / N, n = i - c * N;
    const double hv = h[i];
    const double* up = U + (n * C + c) * r;
#pragma unroll
    for (int j = 0; j < kRrrMaxR; ++j)
      if (j < r) acc[j] = fma(up[j], hv, acc[j]);
  }
  for (int j = 0; j < r; ++j) {
    const double s = rrr_block_sum(acc[j], red);
    if (threadIdx.x == 0) dV[(int64_t)j * T + t] = s;
  }
}

__global__ __launch_bounds__(256) void rrr_loss_kernel(int64_t count, const double* __restrict__ lossp,
                                                       double* __restrict__ loss) {
  __shared__ double red[256];
  double a = 0.0;
  for (int64_t i = threadIdx.x; i < count; i += 256) a += lossp[i];
  a = rrr_block_sum(a, red);
  if (threadIdx.x == 0) loss[0] = a;
}

void rrr_launch_loss(hipStream_t s, int64_t count, const double* lossp, double* loss) {
  hipLaunchKernelGGL(rrr_loss_kernel, dim3(1), dim3(256), 0, s, count, lossp, loss);
}

// grid ceil(r T / 256): dV[i] = sum of element i's partials, ascending
__global__ __launch_bounds__(256) void rrr_dv_sum_kernel(int64_t rT, int64_t count, int64_t stride,
                                                         const double* __restrict__ dVp, double* __restrict__ dV) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= rT) return;
  double s = 0.0;
  for (int64_t p = 0; p < count; ++p) s += dVp[p * stride + i];
  dV[i] = s;
}

void rrr_launch_dv_sum(hipStream_t s, int64_t T, int r, int64_t count, int64_t stride, const double* dVp, double* dV) {
  hipLaunchKernelGGL(rrr_dv_sum_kernel, dim3((unsigned)cdiv(r * T, 256)), dim3(256), 0, s, r * T, count, stride, dVp,
                     dV);
}

struct RrrWs {
  int S;
  int64_t kper;
  size_t part, lossp, total;  // byte offsets (H overwrites partial 0 of part)
};
static RrrWs rrr_ws(int64_t K, int64_t T, int64_t N, int64_t C) {
  RrrWs w;
  const int64_t blocks = T * cdiv(N, 64);
  int64_t S = blocks >= 512 ? 1 : cdiv(512, blocks);
  const int64_t cap = K / (2 * kRrrWaves);  // at least two trials per wave before splitting further
  if (S > cap) S = cap;
  if (S > kRrrMaxSplit) S = kRrrMaxSplit;
  if (S < 1) S = 1;
  w.kper = cdiv(K, S * kRrrWaves);
  w.S = (int)cdiv(K, w.kper * kRrrWaves);
  auto al = [](size_t bytes) { return (bytes + 255) / 256 * 256; };
  size_t off = 0;
  w.part = off;  off += al((size_t)w.S * T * (C + 2) * N * 8);
  w.lossp = off; off += al((size_t)(C + 2) * N * 8);
  // unused: the size callers were told before H moved into partial 0 (T (C+1) N doubles more) is kept
  w.total = off + al((size_t)T * (C + 1) * N * 8);
  return w;
}

template <typename YT, int CP>
static void rrr_launch_accum(bool grad, dim3 grid, hipStream_t s, int64_t K, int64_t T, int64_t N, int C, int r,
                             int64_t kper, const double* X, const void* y, const double* U, const double* V,
                             const double* b, double* part) {
  if (grad)
    hipLaunchKernelGGL((rrr_accum_kernel<YT, CP, true>), grid, dim3(256), 0, s, K, T, N, C, r, kper, X, (const YT*)y, U,
                       V, b, part);
  else
    hipLaunchKernelGGL((rrr_accum_kernel<YT, CP, false>), grid, dim3(256), 0, s, K, T, N, C, r, kper, X, (const YT*)y,
                       U, V, b, part);
}
template <typename YT>
static void rrr_dispatch_accum(int C1, bool grad, dim3 grid, hipStream_t s, int64_t K, int64_t T, int64_t N, int C,
                               int r, int64_t kper, const double* X, const void* y, const double* U, const double* V,
                               const double* b, double* part) {
#define VS_RRR_CASE(CP)                                                                       \
  if (C1 <= CP) {                                                                             \
    rrr_launch_accum<YT, CP>(grad, grid, s, K, T, N, C, r, kper, X, y, U, V, b, part);        \
    return;                                                                                   \
  }
  VS_RRR_CASE(2) VS_RRR_CASE(4) VS_RRR_CASE(6) VS_RRR_CASE(8) VS_RRR_CASE(12) VS_RRR_CASE(16) VS_RRR_CASE(24)
  VS_RRR_CASE(33)
#undef VS_RRR_CASE
}

// ---- scoring -------------------------------------------------------------------------------
// stats per neuron: [0] spike sum, [1] sum pred, [2] sum gt log pred, [3] sum R^2 over non-NaN trials, [4] their count
constexpr int kScoreStats = 5;
constexpr int kScoreMaxChunks = 256;

// where yhat[k,t,n] comes from: the narrow entry's operands (X[k,t,:] is wave-uniform) ...
struct RrrYhatComputed {
  const double *X, *U, *V, *b;
  int C, r;
  __device__ __forceinline__ double operator()(int64_t k, int64_t t, int64_t n, int64_t T, int64_t N) const {
    const double* xr = X + (k * T + t) * (C + 1);
    const double* un = U + n * C * r;
    double yh = 0.0;
    for (int c = 0; c < C; ++c) yh = fma(xr[c], rrr_beta(un + c * r, V, r, T, t), yh);
    return fma(xr[C], b[n * T + t], yh);
  }
};
// ... or the [K][T][N] a forward product left in the workspace
struct RrrYhatStored {
  const double* yhat;
  __device__ __forceinline__ double operator()(int64_t k, int64_t t, int64_t n, int64_t T, int64_t N) const {
    return yhat[(k * T + t) * N + n];
  }
};

// grid (ceil(N/64), chunks of the trials); wave w of a block takes a slice of the chunk.  stat [chunk][5][N].
template <typename YT, typename Yhat>
__global__ __launch_bounds__(256) void rrr_score_kernel(int64_t K, int64_t T, int64_t N, int64_t kchunk, const Yhat yhat,
                                                        const double* __restrict__ mean_y,
                                                        const double* __restrict__ std_y, const YT* __restrict__ gt,
                                                        double* __restrict__ pred, double* __restrict__ stat) {
  __shared__ double red[(kRrrWaves - 1) * kScoreStats * 64];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t n = (int64_t)blockIdx.x * 64 + lane;
  const bool live = n < N;
  const int64_t kw = dcdiv(kchunk, kRrrWaves);
  const int64_t kend = ((int64_t)blockIdx.y + 1) * kchunk < K ? ((int64_t)blockIdx.y + 1) * kchunk : K;
  const int64_t k0 = (int64_t)blockIdx.y * kchunk + (int64_t)w * kw;
  const int64_t k1 = k0 + kw < kend ? k0 + kw : kend;
  double st[kScoreStats] = {0, 0, 0, 0, 0};
  if (live) {
    for (int64_t k = k0; k < k1; ++k) {
      double sy = 0.0, res = 0.0;
      for (int64_t t = 0; t < T; ++t) {
        const int64_t at = (k * T + t) * N + n;
        double p = fma(yhat(k, t, n, T, N), std_y[t * N + n], mean_y[t * N + n]);
        p = p < 1e-3 ? 1e-3 : p;   // np.clip(pred, 1e-3, None): a NaN stays a NaN
        if (pred) pred[at] = p;
        const double g = ld_f64(gt + at);
        st[0] += g;
        st[1] += p;
        st[2] = fma(g, log(p), st[2]);
        sy += g;
        const double d = g - p;
        res = fma(d, d, res);
      }
      // SS_tot about the trial's own mean, in a second pass over the T counts (no cancellation)
      const double m = sy / (double)T;
      double tot = 0.0;
      for (int64_t t = 0; t < T; ++t) {
        const double e = ld_f64(gt + (k * T + t) * N + n) - m;
        tot = fma(e, e, tot);
      }
      double v;   // sklearn r2_score, 1-D, force_finite
      if (T < 2 || res != res || tot != tot) v = __builtin_nan("");
      else if (res == 0.0) v = 1.0;
      else if (tot == 0.0) v = 0.0;
      else v = 1.0 - res / tot;
      if (v == v) {
        st[3] += v;
        st[4] += 1.0;
      }
    }
  }
  if (w > 0) {
#pragma unroll
    for (int i = 0; i < kScoreStats; ++i) red[((size_t)(w - 1) * kScoreStats + i) * 64 + lane] = st[i];
  }
  __syncthreads();
  if (w == 0 && live) {
    for (int v = 1; v < kRrrWaves; ++v)
#pragma unroll
      for (int i = 0; i < kScoreStats; ++i) st[i] += red[((size_t)(v - 1) * kScoreStats + i) * 64 + lane];
#pragma unroll
    for (int i = 0; i < kScoreStats; ++i) stat[((int64_t)blockIdx.y * kScoreStats + i) * N + n] = st[i];
  }
}

// one block: per neuron bps and R^2 (chunks added in ascending order), then their NaN-ignoring means;
// out[0] = co_bps, out[1] = mean R^2
__global__ __launch_bounds__(256) void rrr_score_final_kernel(int64_t K, int64_t T, int64_t N, int chunks,
                                                              const double* __restrict__ stat,
                                                              double* __restrict__ bps, double* __restrict__ r2,
                                                              double* __restrict__ out) {
  __shared__ double red[256];
  const double nan = __builtin_nan("");
  const double cnt = (double)K * (double)T;
  double sb = 0, nb = 0, sr = 0, nr = 0;
  for (int64_t n = threadIdx.x; n < N; n += 256) {
    double st[kScoreStats] = {0, 0, 0, 0, 0};
    for (int ch = 0; ch < chunks; ++ch)
#pragma unroll
      for (int i = 0; i < kScoreStats; ++i) st[i] += stat[((int64_t)ch * kScoreStats + i) * N + n];
    const double S = st[0];
    double m = S / cnt;                       // the null model: the neuron's mean count
    if (m == 0.0) m = 1e-9;
    const double nll_null = cnt * m - S * log(m);
    const double nll_model = st[1] - st[2];   // the log(n!) terms of both likelihoods cancel
    double v = (nll_null - nll_model) / S / 0.69314718055994530942;
    if (isinf(v)) v = nan;
    const double q = st[4] > 0 ? st[3] / st[4] : nan;
    bps[n] = v;
    r2[n] = q;
    if (v == v) {
      sb += v;
      nb += 1;
    }
    if (q == q) {
      sr += q;
      nr += 1;
    }
  }
  sb = rrr_block_sum(sb, red);
  nb = rrr_block_sum(nb, red);
  sr = rrr_block_sum(sr, red);
  nr = rrr_block_sum(nr, red);
  if (threadIdx.x == 0) {
    out[0] = nb > 0 ? sb / nb : nan;
    out[1] = nr > 0 ? sr / nr : nan;
  }
}

struct ScoreWs {
  int chunks;
  int64_t kchunk;
  size_t stat, total;   // byte offsets; the yhat piece, when present, is at 0
};
static ScoreWs score_ws(int64_t K, int64_t T, int64_t N, bool yhat) {
  ScoreWs w;
  int64_t ch = cdiv(K, kRrrWaves);
  if (ch > kScoreMaxChunks) ch = kScoreMaxChunks;
  w.kchunk = cdiv(K, ch);
  w.chunks = (int)cdiv(K, w.kchunk);
  auto al = [](size_t bytes) { return (bytes + 255) / 256 * 256; };
  w.stat = yhat ? al((size_t)K * T * N * 8) : 0;
  w.total = w.stat + al((size_t)w.chunks * kScoreStats * N * 8);
  return w;
}

size_t rrr_score_workspace_bytes(int64_t K, int64_t T, int64_t N, bool yhat) { return score_ws(K, T, N, yhat).total; }

template <typename Yhat>
static int rrr_score_run(hipStream_t s, int64_t K, int64_t T, int64_t N, const ScoreWs& w, const Yhat& yhat,
                         const double* mean_y, const double* std_y, const void* gt, int32_t gt_dtype, double* pred,
                         double* bps, double* r2, double* out, void* workspace) {
  double* stat = (double*)((char*)workspace + w.stat);
  const dim3 grid((unsigned)cdiv(N, 64), (unsigned)w.chunks);
  if (gt_dtype == VS_F32)
    hipLaunchKernelGGL((rrr_score_kernel<float, Yhat>), grid, dim3(256), 0, s, K, T, N, w.kchunk, yhat, mean_y, std_y,
                       (const float*)gt, pred, stat);
  else
    hipLaunchKernelGGL((rrr_score_kernel<double, Yhat>), grid, dim3(256), 0, s, K, T, N, w.kchunk, yhat, mean_y, std_y,
                       (const double*)gt, pred, stat);
  VS_LAUNCH_CHECK();
  hipLaunchKernelGGL(rrr_score_final_kernel, dim3(1), dim3(256), 0, s, K, T, N, w.chunks, (const double*)stat, bps, r2,
                     out);
  VS_LAUNCH_CHECK();
  return VS_OK;
}

int rrr_score_yhat(hipStream_t s, int64_t K, int64_t T, int64_t N, const double* mean_y, const double* std_y,
                   const void* gt, int32_t gt_dtype, double* pred, double* bps, double* r2, double* out,
                   void* workspace) {
  return rrr_score_run(s, K, T, N, score_ws(K, T, N, true), RrrYhatStored{(const double*)workspace}, mean_y, std_y, gt,
                       gt_dtype, pred, bps, r2, out, workspace);
}

// ---- argument checks --------------------------------------------------------------------------------------
static int rrr_fail(const char* entry, const char* what) {
  char msg[160];
  snprintf(msg, sizeof(msg), "%s: %s", entry, what);
  set_error(msg);
  return VS_EINVAL;
}

int rrr_check_loss_grad(const char* entry, int32_t y_dtype, bool ptrs, const double* dU, const double* dV,
                        const double* db, const void* workspace) {
  if (y_dtype != VS_F32 && y_dtype != VS_F64) return rrr_fail(entry, "y must be f32 or f64");
  if (!ptrs) return rrr_fail(entry, "null pointer");
  if ((dU || dV || db) && !(dU && dV && db)) return rrr_fail(entry, "dU, dV, db are given together or not at all");
  if (!aligned16(workspace)) return rrr_fail(entry, "workspace must be 16-byte aligned");
  return VS_OK;
}

int rrr_check_score(const char* entry, int32_t gt_dtype, bool ptrs, const void* workspace) {
  if (gt_dtype != VS_F32 && gt_dtype != VS_F64) return rrr_fail(entry, "gt must be f32 or f64");
  if (!ptrs) return rrr_fail(entry, "null pointer");
  if (!aligned16(workspace)) return rrr_fail(entry, "workspace must be 16-byte aligned");
  return VS_OK;
}

static bool rrr_dims_ok(int64_t K, int64_t T, int64_t N, int64_t C, int64_t r) {
  return K > 0 && T > 0 && N > 0 && C >= 1 && C <= kRrrMaxC && r >= 1 && r <= kRrrMaxR && T <= 65535 &&
         cdiv(N, 64) <= 0x7fffffff;
}

}  // namespace vs

using namespace vs;

extern "C" size_t vs_rrr_loss_grad_workspace_bytes(int64_t K, int64_t T, int64_t N, int64_t C) {
  if (K <= 0 || T <= 0 || N <= 0 || C < 1 || C > kRrrMaxC) return 0;
  return rrr_ws(K, T, N, C).total;
}

extern "C" int vs_rrr_loss_grad(int64_t K, int64_t T, int64_t N, int64_t C, int64_t r, const double* X, const void* y,
                                int32_t y_dtype, const double* U, const double* V, const double* b, double l2,
                                double* loss, double* dU, double* dV, double* db, void* workspace, void* stream) {
  VS_REQUIRE(C >= 1 && C <= kRrrMaxC, "vs_rrr_loss_grad: 1 <= C <= 32 features (without the bias column)");
  VS_REQUIRE(r >= 1 && r <= kRrrMaxR, "vs_rrr_loss_grad: 1 <= r <= 8 components");
  VS_REQUIRE(rrr_dims_ok(K, T, N, C, r), "vs_rrr_loss_grad: K, T, N must be positive (T <= 65535)");
  VS_CALL(rrr_check_loss_grad("vs_rrr_loss_grad", y_dtype, X && y && U && V && b && loss && workspace, dU, dV, db,
                              workspace));
  const bool grad = dU != nullptr;
  hipStream_t s = (hipStream_t)stream;
  const RrrWs w = rrr_ws(K, T, N, C);
  char* ws = (char*)workspace;
  double* part = (double*)(ws + w.part);
  double* lossp = (double*)(ws + w.lossp);
  ScopedTimer timer(VS_TIMER_MISC, s,
                    (double)K * T * ((double)N * (y_dtype == VS_F32 ? 4.0 : 8.0) + (C + 1) * 8.0));
  const dim3 grid((unsigned)cdiv(N, 64), (unsigned)T, (unsigned)w.S);
  if (y_dtype == VS_F32)
    rrr_dispatch_accum<float>((int)C + 1, grad, grid, s, K, T, N, (int)C, (int)r, w.kper, X, y, U, V, b, part);
  else
    rrr_dispatch_accum<double>((int)C + 1, grad, grid, s, K, T, N, (int)C, (int)r, w.kper, X, y, U, V, b, part);
  VS_LAUNCH_CHECK();
  hipLaunchKernelGGL(rrr_reduce_t_kernel<false>, dim3((unsigned)cdiv(N, 64), (unsigned)(C + 2)), dim3(256), 0, s, T, N,
                     (int)C, (int)r, w.S, l2, grad ? 1 : 0, part, U, V, b, dU, db, lossp);
  VS_LAUNCH_CHECK();
  if (grad) {
    hipLaunchKernelGGL(rrr_dv_kernel, dim3((unsigned)T), dim3(256), 0, s, T, N, (int)C, (int)r, U, (const double*)part,
                       dV);
    VS_LAUNCH_CHECK();
  }
  rrr_launch_loss(s, (int64_t)(C + 2) * N, lossp, loss);
  VS_LAUNCH_CHECK();
  return VS_OK;
}

extern "C" size_t vs_rrr_score_workspace_bytes(int64_t K, int64_t N) {
  if (K <= 0 || N <= 0) return 0;
  return rrr_score_workspace_bytes(K, 1, N, false);
}

extern "C" int vs_rrr_score(int64_t K, int64_t T, int64_t N, int64_t C, int64_t r, const double* X, const double* U,
                            const double* V, const double* b, const double* mean_y, const double* std_y,
                            const void* gt, int32_t gt_dtype, double* pred, double* bps, double* r2, double* out,
                            void* workspace, void* stream) {
  VS_REQUIRE(C >= 1 && C <= kRrrMaxC, "vs_rrr_score: 1 <= C <= 32 features (without the bias column)");
  VS_REQUIRE(r >= 1 && r <= kRrrMaxR, "vs_rrr_score: 1 <= r <= 8 components");
  VS_REQUIRE(rrr_dims_ok(K, T, N, C, r), "vs_rrr_score: K, T, N must be positive (T <= 65535)");
  VS_CALL(rrr_check_score("vs_rrr_score", gt_dtype,
                          X && U && V && b && mean_y && std_y && gt && bps && r2 && out && workspace, workspace));
  hipStream_t s = (hipStream_t)stream;
  ScopedTimer timer(VS_TIMER_MISC, s,
                    (double)K * T * ((double)N * ((gt_dtype == VS_F32 ? 4.0 : 8.0) + (pred ? 8.0 : 0.0)) + (C + 1) * 8.0));
  return rrr_score_run(s, K, T, N, score_ws(K, T, N, false), RrrYhatComputed{X, U, V, b, (int)C, (int)r}, mean_y, std_y,
                       gt, gt_dtype, pred, bps, r2, out, workspace);
}
