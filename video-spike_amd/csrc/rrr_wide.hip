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
// the tiles) add exact zeros, and nothing outside the operands is read or written (rrw_fwd_kernel's comment).
//
// vs_rrr_wide_loss_grad, 4 launches in loss-only mode, 7 with gradients:
//   1. rrw_fwd_kernel     block = one bin t, 128 trials x 64 neurons, 4 waves (16 neurons each, 8 MFMA row tiles);
//                         the features go through LDS 32 at a time (X tile + Beta tile), the next slice's loads in
//                         flight under the MFMAs.  Writes res [K][T][N].
//   2. rrw_sq_kernel      sq[t][n] = sum_k res^2 (k ascending), the last row of G.
//   3. rrw_grad_kernel    block = one bin t, 64 features x 64 neurons; all K trials go through LDS 32 at a time, in
//                         order, prefetched the same way.  Writes G[t][c][n] (rows 0..C; row C+1 = sq), the layout
//                         of rrr.hip's partials.
//   4. rrw_reduce_t_kernel / rrw_dv_kernel + rrw_dv_sum_kernel / rrw_loss_kernel: H = G + 2 l2 beta (in place),
//                         db, dU = H V^T, dV, the l2 terms and the loss, in the arithmetic of rrr.hip's tail
//                         (dV's sum over (n, c) is split into feature chunks whose partials are added in order).
// Workspace (doubles, each piece rounded up to 256 bytes):
//   K T N  (res)  +  T (C+2) N  (G, then H)  +  (C+2) ceil(N/64)  (loss terms)  +  chunks 8 T  (dV partials,
//   chunks <= 32)
// i.e. 0.48 GB at K 400, T 100, N 512, C 768.
// vs_rrr_wide_score: rrw_fwd_kernel (standardised yhat to the workspace, K T N doubles) + rrw_score_kernel
//   (rrr_score_kernel's statistics read from yhat) + rrw_score_final_kernel.
// vs_gauss_smooth_time: one thread per (k, n) column walking t; scipy's order of additions, no FMA.
#include <math.h>

#include "common.h"
#include "rrr_wide.h"

namespace vs {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kRrwMaxC = 1024;
constexpr int kRrwMaxR = 8;
constexpr int kRrwWaves = 4;
constexpr int kRrwTile = 64;      // neurons per block; features per block of the gradient product
constexpr int kRrwFwdTrials = 128; // trials per block of the forward product
constexpr int kRrwStep = 32;      // reduction extent staged in LDS at a time (8 MFMA k-steps)
constexpr int kRrwXs = 36;        // forward X tile row stride (doubles): the A reads go down a column
constexpr int kRrwBs = 65;        // forward Beta tile row stride: the staging writes go down a column
constexpr int kRrwDvChunks = 32;

template <typename YT> __device__ __forceinline__ double rrw_ld(const YT* p) { return (double)*p; }
__device__ __forceinline__ int64_t rrw_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// beta[n,c,t] for c < C, rrr.hip's order (j ascending, fused)
__device__ __forceinline__ double rrw_beta(const double* u, const double* __restrict__ V, int r, int64_t T, int64_t t) {
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < kRrwMaxR; ++j)
    if (j < r) s = fma(u[j], V[(int64_t)j * T + t], s);
  return s;
}

// grid (ceil(N/64), T, ceil(K/128)).  SCORE: out = yhat, else out = yhat - y.  The next 32-feature slice is loaded
// into registers (X values and, for r <= 4, the raw U rows) before the MFMAs of the current one, so the loads are
// in flight under them; RR = 4: r <= 4 (U rows prefetched raw), RR = 8: beta is formed at the load.
template <typename YT, bool SCORE, int RR>
__global__ __launch_bounds__(256) void rrw_fwd_kernel(int64_t K, int64_t T, int64_t N, int C, int r,
                                                      const double* __restrict__ X, const YT* __restrict__ y,
                                                      const double* __restrict__ U, const double* __restrict__ V,
                                                      const double* __restrict__ b, double* __restrict__ out) {
  constexpr int kMt = kRrwFwdTrials / 16;          // MFMA row tiles per wave
  constexpr int kXl = kRrwFwdTrials * kRrwStep / 256;
  constexpr int kUr = RR == 4 ? 4 : 1;
  __shared__ double Xs[kRrwFwdTrials * kRrwXs];
  __shared__ double Bs[kRrwStep * kRrwBs];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lk = lane >> 4;
  const int64_t t = blockIdx.y;
  const int64_t n0 = (int64_t)blockIdx.x * kRrwTile, k0 = (int64_t)blockIdx.z * kRrwFwdTrials;
  const int C1 = C + 1;
  const int col = tid & 31, row0 = tid >> 5;       // staging: element e = tid + 256 i is (row0 + 8 i, col)
  double v[kRrwMaxR];
#pragma unroll
  for (int j = 0; j < kRrwMaxR; ++j) v[j] = j < r ? V[(int64_t)j * T + t] : 0.0;
  f64x4 acc[kMt];
#pragma unroll
  for (int m = 0; m < kMt; ++m) acc[m] = f64x4{0.0, 0.0, 0.0, 0.0};
  double xr[kXl], ur[8][kUr];
  // Tails without lane predicates on the loads (a load under a predicate compiles to a branch with its own wait,
  // which serialises the latencies of a slice).  Trials >= K and neurons >= N are rows / columns of the product that
  // are never stored: their loads are clamped to the last trial / neuron.  Features >= C+1 must add exactly 0: X is
  // clamped to the row's own last column, U to the neuron's own last row, and the V factors are zeroed, so the
  // product is 0 x a value the same output already depends on.
  auto load = [&](int c0) {
    const int c = c0 + col;
    const int cx = c < C1 ? c : C, cu = c < C ? c : C - 1;
#pragma unroll
    for (int i = 0; i < kXl; ++i) {                // X tile: 128 trials x 32 features
      const int64_t k = k0 + row0 + 8 * i;
      xr[i] = X[((k < K ? k : K - 1) * T + t) * C1 + cx];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {                  // Beta tile: 32 features x 64 neurons
      const int64_t n = n0 + row0 + 8 * i;
      const double* up = U + ((n < N ? n : N - 1) * C + cu) * r;
      if (RR == 4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) ur[i][j] = up[j < r ? j : 0];
      } else {
        double be = 0.0;
#pragma unroll
        for (int j = 0; j < kRrwMaxR; ++j)
          if (j < r) be = fma(up[j], c < C ? v[j] : 0.0, be);
        ur[i][0] = be;
      }
    }
    if (c0 + kRrwStep > C) {                       // the slice that holds the bias row (block-uniform)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int64_t n = n0 + row0 + 8 * i;
        const double bv = b[(n < N ? n : N - 1) * T + t];
        ur[i][0] = c == C ? bv : ur[i][0];
      }
    }
  };
  load(0);
  for (int c0 = 0; c0 < C1; c0 += kRrwStep) {
    const int c = c0 + col;
#pragma unroll
    for (int i = 0; i < kXl; ++i) Xs[(row0 + 8 * i) * kRrwXs + col] = xr[i];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      double be = ur[i][0];
      if (RR == 4) {                               // rrw_beta's order: j ascending, fused
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < r) s = fma(ur[i][j], c < C ? v[j] : 0.0, s);
        be = c == C ? be : s;
      }
      Bs[col * kRrwBs + row0 + 8 * i] = be;
    }
    __syncthreads();
    if (c0 + kRrwStep < C1) load(c0 + kRrwStep);
#pragma unroll
    for (int kk = 0; kk < kRrwStep / 4; ++kk) {
      const double bb = Bs[(kk * 4 + lk) * kRrwBs + 16 * w + li];
#pragma unroll
      for (int m = 0; m < kMt; ++m)
        acc[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(Xs[(16 * m + li) * kRrwXs + kk * 4 + lk], bb, acc[m], 0, 0, 0);
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
          out[at] = SCORE ? acc[m][q] : acc[m][q] - rrw_ld(y + at);
        }
      }
  }
}

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

// grid (ceil(N/64), T, ceil((C+1)/64)): G[t][c][n] = sum_k X[k,t,c] 2 res[k,t,n], k ascending within the MFMA's
// own k order (4 trials per instruction, 32 per LDS stage)
__global__ __launch_bounds__(256) void rrw_grad_kernel(int64_t K, int64_t T, int64_t N, int C,
                                                       const double* __restrict__ X, const double* __restrict__ R,
                                                       double* __restrict__ G) {
  __shared__ double Xs[kRrwStep * kRrwTile];
  __shared__ double Rs[kRrwStep * kRrwTile];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lk = lane >> 4;
  const int64_t t = blockIdx.y;
  const int64_t n0 = (int64_t)blockIdx.x * kRrwTile;
  const int c0 = (int)blockIdx.z * kRrwTile;
  const int C1 = C + 1;
  f64x4 acc[4];
#pragma unroll
  for (int m = 0; m < 4; ++m) acc[m] = f64x4{0.0, 0.0, 0.0, 0.0};
  const int col = tid & 63, row0 = tid >> 6;       // staging: element e = tid + 256 i is (row0 + 4 i, col)
  double xr[8], rr[8];
  const int cc = c0 + col < C1 ? c0 + col : C;
  const int64_t nc = n0 + col < N ? n0 + col : N - 1;
  auto load = [&](int64_t k0) {                    // the next 32 trials, in flight under the MFMAs
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      // tails as in the forward: features >= C+1 and neurons >= N are never stored (clamped loads); trials >= K
      // must add exactly 0: both loads are clamped to the last trial and the residual's factor 2 becomes 0
      const int64_t k = k0 + row0 + 4 * i, kc = k < K ? k : K - 1;
      xr[i] = X[(kc * T + t) * C1 + cc];
      rr[i] = R[(kc * T + t) * N + nc] * (k < K ? 2.0 : 0.0);
    }
  };
  load(0);
  for (int64_t k0 = 0; k0 < K; k0 += kRrwStep) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      Xs[tid + 256 * i] = xr[i];
      Rs[tid + 256 * i] = rr[i];
    }
    __syncthreads();
    if (k0 + kRrwStep < K) load(k0 + kRrwStep);
#pragma unroll
    for (int kk = 0; kk < kRrwStep / 4; ++kk) {
      const double bb = Rs[(kk * 4 + lk) * kRrwTile + 16 * w + li];
#pragma unroll
      for (int m = 0; m < 4; ++m)
        acc[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(Xs[(kk * 4 + lk) * kRrwTile + 16 * m + li], bb, acc[m], 0, 0, 0);
    }
    __syncthreads();
  }
  const int64_t n = n0 + 16 * w + li;
  if (n < N) {
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = c0 + 16 * m + lk + 4 * q;
        if (c < C1) G[(t * (C + 2) + c) * N + n] = acc[m][q];
      }
  }
}

// rrr_reduce_t_kernel's arithmetic on G[t][c][n] (C+2 rows per bin); H overwrites G in place (each element is read
// and written by the same thread).  grid (ceil(N/64), C+2).
__global__ __launch_bounds__(256) void rrw_reduce_t_kernel(int64_t T, int64_t N, int C, int r, double l2, int grad,
                                                           double* __restrict__ G, const double* __restrict__ U,
                                                           const double* __restrict__ V, const double* __restrict__ b,
                                                           double* __restrict__ dU, double* __restrict__ db,
                                                           double* __restrict__ lossp) {
  __shared__ double red[(kRrwWaves - 1) * (kRrwMaxR + 1) * 64];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int c = blockIdx.y;
  const int64_t n = (int64_t)blockIdx.x * 64 + lane;
  const bool live = n < N;
  const int C1 = C + 1;
  const int64_t tper = rrw_cdiv(T, kRrwWaves);
  const int64_t t0 = (int64_t)w * tper;
  const int64_t t1 = t0 + tper < T ? t0 + tper : T;
  double u[kRrwMaxR], du[kRrwMaxR];
#pragma unroll
  for (int j = 0; j < kRrwMaxR; ++j) {
    u[j] = (live && c < C && j < r) ? U[(n * C + c) * r + j] : 0.0;
    du[j] = 0.0;
  }
  double term = 0.0;  // sum beta^2 (rows 0..C) or sum res^2 (row C+1)
  if (live) {
    for (int64_t t = t0; t < t1; ++t) {
      double* gp = G + (t * (C + 2) + c) * N + n;
      double g = 0.0;
      if (grad || c == C1) g += *gp;
      if (c == C1) {
        term += g;
        continue;
      }
      const double be = c < C ? rrw_beta(u, V, r, T, t) : b[n * T + t];
      term = fma(be, be, term);
      if (grad) {
        const double h = fma(2.0 * l2, be, g);
        *gp = h;
        if (c == C) {
          db[n * T + t] = h;
        } else {
#pragma unroll
          for (int j = 0; j < kRrwMaxR; ++j)
            if (j < r) du[j] = fma(h, V[(int64_t)j * T + t], du[j]);
        }
      }
    }
  }
  if (w > 0) {
    double* p = red + (size_t)(w - 1) * (kRrwMaxR + 1) * 64 + lane;
    p[0] = term;
#pragma unroll
    for (int j = 0; j < kRrwMaxR; ++j) p[(j + 1) * 64] = du[j];
  }
  __syncthreads();
  if (w == 0 && live) {
    for (int v = 1; v < kRrwWaves; ++v) {
      const double* p = red + (size_t)(v - 1) * (kRrwMaxR + 1) * 64 + lane;
      term += p[0];
#pragma unroll
      for (int j = 0; j < kRrwMaxR; ++j) du[j] += p[(j + 1) * 64];
    }
    if (grad && c < C) {
#pragma unroll
      for (int j = 0; j < kRrwMaxR; ++j)
        if (j < r) dU[(n * C + c) * r + j] = du[j];
    }
  }
  // the block's 64 loss terms in a fixed tree (dead lanes add 0): one value per (row, neuron block), so the final sum
  // walks (C+2) ceil(N/64) values, not (C+2) N (one block over 394,000 values took 0.6 ms at C 768, N 512)
  if (w == 0) {
    double v = live ? (c == C1 ? term : l2 * term) : 0.0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) lossp[(int64_t)c * gridDim.x + blockIdx.x] = v;
  }
}

// fixed-shape block reduction (256 threads); every thread gets the sum
__device__ double rrw_block_sum(double v, double* red) {
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
  double acc[kRrwMaxR];
#pragma unroll
  for (int j = 0; j < kRrwMaxR; ++j) acc[j] = 0.0;
  for (int64_t i = threadIdx.x; i < (int64_t)cw * N; i += 256) {
    const int64_t n = i / cw;
    const int c = clo + (int)(i - n * cw);
    const double hv = h[(int64_t)c * N + n];
    const double* up = U + (n * C + c) * r;
#pragma unroll
    for (int j = 0; j < kRrwMaxR; ++j)
      if (j < r) acc[j] = fma(up[j], hv, acc[j]);
  }
  for (int j = 0; j < r; ++j) {
    const double s = rrw_block_sum(acc[j], red);
    if (threadIdx.x == 0) dVp[((int64_t)ch * kRrwMaxR + j) * T + t] = s;
  }
}

// dV[j][t] = sum of the chunks' partials, ascending
__global__ __launch_bounds__(256) void rrw_dv_sum_kernel(int64_t T, int r, int chunks, const double* __restrict__ dVp,
                                                         double* __restrict__ dV) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)r * T) return;
  const int64_t j = i / T, t = i - j * T;
  double s = 0.0;
  for (int ch = 0; ch < chunks; ++ch) s += dVp[((int64_t)ch * kRrwMaxR + j) * T + t];
  dV[i] = s;
}

__global__ __launch_bounds__(256) void rrw_loss_kernel(int64_t count, const double* __restrict__ lossp,
                                                       double* __restrict__ loss) {
  __shared__ double red[256];
  double a = 0.0;
  for (int64_t i = threadIdx.x; i < count; i += 256) a += lossp[i];
  a = rrw_block_sum(a, red);
  if (threadIdx.x == 0) loss[0] = a;
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
  w.dVp = off;   off += al((size_t)w.chunks * kRrwMaxR * T * 8);
  w.total = off;
  return w;
}

static bool rrw_dims_ok(int64_t K, int64_t T, int64_t N) {
  return K > 0 && T > 0 && N > 0 && T <= 65535 && cdiv(K, kRrwFwdTrials) <= 65535 && cdiv(N, 64) <= 0x7fffffff;
}

template <typename YT, bool SCORE>
static void rrw_launch_fwd(hipStream_t s, int64_t K, int64_t T, int64_t N, int C, int r, const double* X, const void* y,
                           const double* U, const double* V, const double* b, double* out) {
  const dim3 grid((unsigned)cdiv(N, kRrwTile), (unsigned)T, (unsigned)cdiv(K, kRrwFwdTrials));
  if (r <= 4)
    hipLaunchKernelGGL((rrw_fwd_kernel<YT, SCORE, 4>), grid, dim3(256), 0, s, K, T, N, C, r, X, (const YT*)y, U, V, b,
                       out);
  else
    hipLaunchKernelGGL((rrw_fwd_kernel<YT, SCORE, 8>), grid, dim3(256), 0, s, K, T, N, C, r, X, (const YT*)y, U, V, b,
                       out);
}

// ---- scoring: rrr.hip's statistics, yhat read from the workspace -------------------------------------------
// stats per neuron: [0] spike sum, [1] sum pred, [2] sum gt log pred, [3] sum R^2 over non-NaN trials, [4] their count
constexpr int kRrwStats = 5;
constexpr int kRrwMaxChunks = 256;

// grid (ceil(N/64), chunks of the trials); wave w of a block takes a slice of the chunk.  stat [chunk][5][N].
template <typename YT>
__global__ __launch_bounds__(256) void rrw_score_kernel(int64_t K, int64_t T, int64_t N, int64_t kchunk,
                                                        const double* __restrict__ yhat,
                                                        const double* __restrict__ mean_y,
                                                        const double* __restrict__ std_y, const YT* __restrict__ gt,
                                                        double* __restrict__ pred, double* __restrict__ stat) {
  __shared__ double red[(kRrwWaves - 1) * kRrwStats * 64];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t n = (int64_t)blockIdx.x * 64 + lane;
  const bool live = n < N;
  const int64_t kw = rrw_cdiv(kchunk, kRrwWaves);
  const int64_t kend = ((int64_t)blockIdx.y + 1) * kchunk < K ? ((int64_t)blockIdx.y + 1) * kchunk : K;
  const int64_t k0 = (int64_t)blockIdx.y * kchunk + (int64_t)w * kw;
  const int64_t k1 = k0 + kw < kend ? k0 + kw : kend;
  double st[kRrwStats] = {0, 0, 0, 0, 0};
  if (live) {
    for (int64_t k = k0; k < k1; ++k) {
      double sy = 0.0, res = 0.0;
      for (int64_t t = 0; t < T; ++t) {
        const int64_t at = (k * T + t) * N + n;
        double p = fma(yhat[at], std_y[t * N + n], mean_y[t * N + n]);
        p = p < 1e-3 ? 1e-3 : p;   // np.clip(pred, 1e-3, None): a NaN stays a NaN
        if (pred) pred[at] = p;
        const double g = rrw_ld(gt + at);
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
        const double e = rrw_ld(gt + (k * T + t) * N + n) - m;
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
    for (int i = 0; i < kRrwStats; ++i) red[((size_t)(w - 1) * kRrwStats + i) * 64 + lane] = st[i];
  }
  __syncthreads();
  if (w == 0 && live) {
    for (int v = 1; v < kRrwWaves; ++v)
#pragma unroll
      for (int i = 0; i < kRrwStats; ++i) st[i] += red[((size_t)(v - 1) * kRrwStats + i) * 64 + lane];
#pragma unroll
    for (int i = 0; i < kRrwStats; ++i) stat[((int64_t)blockIdx.y * kRrwStats + i) * N + n] = st[i];
  }
}

// one block: per neuron bps and R^2 (chunks added in ascending order), then their NaN-ignoring means;
// out[0] = co_bps, out[1] = mean R^2
__global__ __launch_bounds__(256) void rrw_score_final_kernel(int64_t K, int64_t T, int64_t N, int chunks,
                                                              const double* __restrict__ stat,
                                                              double* __restrict__ bps, double* __restrict__ r2,
                                                              double* __restrict__ out) {
  __shared__ double red[256];
  const double nan = __builtin_nan("");
  const double cnt = (double)K * (double)T;
  double sb = 0, nb = 0, sr = 0, nr = 0;
  for (int64_t n = threadIdx.x; n < N; n += 256) {
    double st[kRrwStats] = {0, 0, 0, 0, 0};
    for (int ch = 0; ch < chunks; ++ch)
#pragma unroll
      for (int i = 0; i < kRrwStats; ++i) st[i] += stat[((int64_t)ch * kRrwStats + i) * N + n];
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
  sb = rrw_block_sum(sb, red);
  nb = rrw_block_sum(nb, red);
  sr = rrw_block_sum(sr, red);
  nr = rrw_block_sum(nr, red);
  if (threadIdx.x == 0) {
    out[0] = nb > 0 ? sb / nb : nan;
    out[1] = nr > 0 ? sr / nr : nan;
  }
}

struct RrwScoreWs {
  int chunks;
  int64_t kchunk;
  size_t yhat, stat, total;
};
static RrwScoreWs rrw_score_ws(int64_t K, int64_t T, int64_t N) {
  RrwScoreWs w;
  int64_t ch = cdiv(K, kRrwWaves);
  if (ch > kRrwMaxChunks) ch = kRrwMaxChunks;
  w.kchunk = cdiv(K, ch);
  w.chunks = (int)cdiv(K, w.kchunk);
  auto al = [](size_t bytes) { return (bytes + 255) / 256 * 256; };
  w.yhat = 0;
  w.stat = al((size_t)K * T * N * 8);
  w.total = w.stat + al((size_t)w.chunks * kRrwStats * N * 8);
  return w;
}

size_t rrw_score_workspace_bytes(int64_t K, int64_t T, int64_t N) { return rrw_score_ws(K, T, N).total; }

int rrw_score_yhat(hipStream_t s, int64_t K, int64_t T, int64_t N, const double* mean_y, const double* std_y,
                   const void* gt, int32_t gt_dtype, double* pred, double* bps, double* r2, double* out,
                   void* workspace) {
  const RrwScoreWs w = rrw_score_ws(K, T, N);
  const double* yhat = (const double*)((char*)workspace + w.yhat);
  double* stat = (double*)((char*)workspace + w.stat);
  const dim3 grid((unsigned)cdiv(N, 64), (unsigned)w.chunks);
  if (gt_dtype == VS_F32)
    hipLaunchKernelGGL(rrw_score_kernel<float>, grid, dim3(256), 0, s, K, T, N, w.kchunk, yhat, mean_y, std_y,
                       (const float*)gt, pred, stat);
  else
    hipLaunchKernelGGL(rrw_score_kernel<double>, grid, dim3(256), 0, s, K, T, N, w.kchunk, yhat, mean_y, std_y,
                       (const double*)gt, pred, stat);
  VS_LAUNCH_CHECK();
  hipLaunchKernelGGL(rrw_score_final_kernel, dim3(1), dim3(256), 0, s, K, T, N, w.chunks, (const double*)stat, bps, r2,
                     out);
  VS_LAUNCH_CHECK();
  return VS_OK;
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
  VS_REQUIRE(r >= 1 && r <= kRrwMaxR, "vs_rrr_wide_loss_grad: 1 <= r <= 8 components");
  VS_REQUIRE(rrw_dims_ok(K, T, N), "vs_rrr_wide_loss_grad: K, T, N must be positive (T <= 65535, K <= 8388480)");
  VS_REQUIRE(y_dtype == VS_F32 || y_dtype == VS_F64, "vs_rrr_wide_loss_grad: y must be f32 or f64");
  VS_REQUIRE(X && y && U && V && b && loss && workspace, "vs_rrr_wide_loss_grad: null pointer");
  const bool grad = dU || dV || db;
  VS_REQUIRE(!grad || (dU && dV && db), "vs_rrr_wide_loss_grad: dU, dV, db are given together or not at all");
  VS_REQUIRE((((uintptr_t)workspace) & 15u) == 0, "vs_rrr_wide_loss_grad: workspace must be 16-byte aligned");
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
    hipLaunchKernelGGL(rrw_grad_kernel, dim3((unsigned)cdiv(N, kRrwTile), (unsigned)T, (unsigned)cdiv(C + 1, kRrwTile)),
                       dim3(256), 0, s, K, T, N, (int)C, X, (const double*)res, G);
    VS_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(rrw_reduce_t_kernel, dim3((unsigned)cdiv(N, 64), (unsigned)(C + 2)), dim3(256), 0, s, T, N, (int)C,
                     (int)r, l2, grad ? 1 : 0, G, U, V, b, dU, db, lossp);
  VS_LAUNCH_CHECK();
  if (grad) {
    hipLaunchKernelGGL(rrw_dv_kernel, dim3((unsigned)T, (unsigned)w.chunks), dim3(256), 0, s, T, N, (int)C, (int)r,
                       w.cper, U, (const double*)G, dVp);
    VS_LAUNCH_CHECK();
    hipLaunchKernelGGL(rrw_dv_sum_kernel, dim3((unsigned)cdiv(r * T, 256)), dim3(256), 0, s, T, (int)r, w.chunks,
                       (const double*)dVp, dV);
    VS_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(rrw_loss_kernel, dim3(1), dim3(256), 0, s, (int64_t)(C + 2) * cdiv(N, 64), (const double*)lossp,
                     loss);
  VS_LAUNCH_CHECK();
  return VS_OK;
}

extern "C" size_t vs_rrr_wide_score_workspace_bytes(int64_t K, int64_t T, int64_t N) {
  if (K <= 0 || T <= 0 || N <= 0) return 0;
  return rrw_score_ws(K, T, N).total;
}

extern "C" int vs_rrr_wide_score(int64_t K, int64_t T, int64_t N, int64_t C, int64_t r, const double* X,
                                 const double* U, const double* V, const double* b, const double* mean_y,
                                 const double* std_y, const void* gt, int32_t gt_dtype, double* pred, double* bps,
                                 double* r2, double* out, void* workspace, void* stream) {
  VS_REQUIRE(C >= 1 && C <= kRrwMaxC, "vs_rrr_wide_score: 1 <= C <= 1024 features (without the bias column)");
  VS_REQUIRE(r >= 1 && r <= kRrwMaxR, "vs_rrr_wide_score: 1 <= r <= 8 components");
  VS_REQUIRE(rrw_dims_ok(K, T, N), "vs_rrr_wide_score: K, T, N must be positive (T <= 65535, K <= 8388480)");
  VS_REQUIRE(gt_dtype == VS_F32 || gt_dtype == VS_F64, "vs_rrr_wide_score: gt must be f32 or f64");
  VS_REQUIRE(X && U && V && b && mean_y && std_y && gt && bps && r2 && out && workspace,
             "vs_rrr_wide_score: null pointer");
  VS_REQUIRE((((uintptr_t)workspace) & 15u) == 0, "vs_rrr_wide_score: workspace must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const RrwScoreWs w = rrw_score_ws(K, T, N);
  double* yhat = (double*)((char*)workspace + w.yhat);
  ScopedTimer timer(VS_TIMER_MISC, s,
                    (double)K * T * ((double)N * ((gt_dtype == VS_F32 ? 4.0 : 8.0) + (pred ? 8.0 : 0.0)) + (C + 1) * 8.0));
  count_rrr(VS_RRR_PATH_WIDE);
  rrw_launch_fwd<double, true>(s, K, T, N, (int)C, (int)r, X, nullptr, U, V, b, yhat);
  VS_LAUNCH_CHECK();
  return rrw_score_yhat(s, K, T, N, mean_y, std_y, gt, gt_dtype, pred, bps, r2, out, workspace);
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
