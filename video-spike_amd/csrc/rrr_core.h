// rrr_core.h — what the three reduced-rank regression units share (csrc/rrr.hip: C <= 32 in registers,
// csrc/rrr_wide.hip: C <= 1024 on the f64 MFMA, csrc/rrr_pixel.hip: raw pixels, C <= 32,768): the small device
// pieces, the two MFMA products over a compile-time operand source, the reduction over the bins, and the host
// side of the scoring, the final sums and the argument checks.  Notation is rrr.hip's.  The kernels that are not
// templates live in rrr.hip behind the host functions declared at the end.
//
// An operand source `Src` says where the X operand of a product comes from.  It is a kernel argument (a few
// pointers), never a run-time flag, and the shared bodies do not test which caller they serve:
//   Raw                        the type an X element has in memory
//   Col                        what a column (feature) needs besides its elements, loaded once per slice / bin
//   bin(t)                     the row of X that time bin t reads (the bin itself, or its frame)
//   clamp(c, C)                the column whose address stands in for column c of a tail
//   col(f, cc, C)              the Col of clamped column cc in row f
//   load(k, f, cc, C)          the raw element of trial k, row f, clamped column cc
//   stage(x, col, c, C)        the double that goes into LDS for the raw x of (unclamped) column c
// Two sources exist: RrwDenseSrc (rrr_wide.hip) and RrpPixelSrc<XT> (rrr_pixel.hip).
#pragma once

#include <math.h>

#include "common.h"

namespace vs {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int kRrrMaxR = 8;
constexpr int kRrrWaves = 4;
constexpr int kRrrTile = 64;        // neurons per block; features per block of the gradient product
constexpr int kRrrFwdTrials = 128;  // trials per block of the forward product
constexpr int kRrrStep = 32;        // reduction extent staged in LDS at a time (8 MFMA k-steps)
constexpr int kRrrXs = 36;          // forward X tile row stride (doubles): the A reads go down a column
constexpr int kRrrBs = 65;          // forward Beta tile row stride: the staging writes go down a column

template <typename YT> __device__ __forceinline__ double ld_f64(const YT* p) { return (double)*p; }
__device__ __forceinline__ int64_t dcdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// beta[n,c,t] for c < C (u = U[n,c,:] in registers): j ascending, fused
__device__ __forceinline__ double rrr_beta(const double* u, const double* __restrict__ V, int r, int64_t T, int64_t t) {
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < kRrrMaxR; ++j)
    if (j < r) s = fma(u[j], V[(int64_t)j * T + t], s);
  return s;
}

// fixed-shape block reduction (256 threads); every thread gets the sum
__device__ inline double rrr_block_sum(double v, double* red) {
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

// ---- forward product: Yhat_t [K x N] = X_t [K x (C+1)] . Beta_t [(C+1) x N] ---------------------------------
// v_mfma_f64_16x16x4_f64 (A[i][k]: lane = i + 16 k, B[k][j]: lane = j + 16 k, D[i][j]: lane = j + 16 (i & 3),
// register i >> 2).  Beta_t is never stored: a B tile is formed from U[n,c,:] and V[:,t] (r FMAs per element) on
// its way into LDS.
// grid (ceil(N/64), T, ceil(K/128)); block = one bin t, 128 trials x 64 neurons, 4 waves (16 neurons each, 8 MFMA
// row tiles).  SCORE: out = yhat, else out = yhat - y.  The next 32-feature slice is loaded into registers (raw X
// values, their column state and, for r <= 4, the raw U rows) before the MFMAs of the current one, so the loads
// are in flight under them, and converted when it is staged; RR = 4: r <= 4 (U rows prefetched raw), RR = 8: beta
// is formed at the load.
template <typename Src, typename YT, bool SCORE, int RR>
__global__ __launch_bounds__(256) void rrr_fwd_kernel(int64_t K, int64_t T, int64_t N, int C, int r, const Src src,
                                                      const YT* __restrict__ y, const double* __restrict__ U,
                                                      const double* __restrict__ V, const double* __restrict__ b,
                                                      double* __restrict__ out) {
  constexpr int kMt = kRrrFwdTrials / 16;          // MFMA row tiles per wave
  constexpr int kXl = kRrrFwdTrials * kRrrStep / 256;
  constexpr int kUr = RR == 4 ? 4 : 1;
  __shared__ double Xs[kRrrFwdTrials * kRrrXs];
  __shared__ double Bs[kRrrStep * kRrrBs];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lk = lane >> 4;
  const int64_t t = blockIdx.y;
  const int64_t n0 = (int64_t)blockIdx.x * kRrrTile, k0 = (int64_t)blockIdx.z * kRrrFwdTrials;
  const int C1 = C + 1;
  const int col = tid & 31, row0 = tid >> 5;       // staging: element e = tid + 256 i is (row0 + 8 i, col)
  const int64_t f = src.bin(t);
  double v[RR];
#pragma unroll
  for (int j = 0; j < RR; ++j) v[j] = j < r ? V[(int64_t)j * T + t] : 0.0;
  f64x4 acc[kMt];
#pragma unroll
  for (int m = 0; m < kMt; ++m) acc[m] = f64x4{0.0, 0.0, 0.0, 0.0};
  typename Src::Raw xr[kXl];
  typename Src::Col xc;
  double ur[8][kUr];
  // Tails without lane predicates on the loads (a load under a predicate compiles to a branch with its own wait,
  // which serialises the latencies of a slice).  Trials >= K and neurons >= N are rows / columns of the product that
  // are never stored: their loads are clamped to the last trial / neuron.  Features >= C+1 must add exactly 0: X is
  // clamped by the source (the dense one to the row's own last column, the pixel one stages a 1), U to the neuron's
  // own last row, and the V factors are zeroed, so the product is 0 x a value the same output already depends on.
  auto load = [&](int c0) {
    const int c = c0 + col;
    const int cx = src.clamp(c, C), cu = c < C ? c : C - 1;
    xc = src.col(f, cx, C);
#pragma unroll
    for (int i = 0; i < kXl; ++i) {                // X tile: 128 trials x 32 features
      const int64_t k = k0 + row0 + 8 * i;
      xr[i] = src.load(k < K ? k : K - 1, f, cx, C);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {                  // Beta tile: 32 features x 64 neurons
      const int64_t n = n0 + row0 + 8 * i;
      const double* up = U + ((n < N ? n : N - 1) * C + cu) * r;
      if constexpr (RR == 4) {
#pragma unroll
        for (int j = 0; j < 4; ++j) ur[i][j] = up[j < r ? j : 0];
      } else {
        double be = 0.0;
#pragma unroll
        for (int j = 0; j < kRrrMaxR; ++j)
          if (j < r) be = fma(up[j], c < C ? v[j] : 0.0, be);
        ur[i][0] = be;
      }
    }
    if (c0 + kRrrStep > C) {                       // the slice that holds the bias row (block-uniform)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int64_t n = n0 + row0 + 8 * i;
        const double bv = b[(n < N ? n : N - 1) * T + t];
        ur[i][0] = c == C ? bv : ur[i][0];
      }
    }
  };
  load(0);
  for (int c0 = 0; c0 < C1; c0 += kRrrStep) {
    const int c = c0 + col;
#pragma unroll
    for (int i = 0; i < kXl; ++i) Xs[(row0 + 8 * i) * kRrrXs + col] = src.stage(xr[i], xc, c, C);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      double be = ur[i][0];
      if constexpr (RR == 4) {                     // rrr_beta's order: j ascending, fused
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < r) s = fma(ur[i][j], c < C ? v[j] : 0.0, s);
        be = c == C ? be : s;
      }
      Bs[col * kRrrBs + row0 + 8 * i] = be;
    }
    __syncthreads();
    if (c0 + kRrrStep < C1) load(c0 + kRrrStep);
#pragma unroll
    for (int kk = 0; kk < kRrrStep / 4; ++kk) {
      const double bb = Bs[(kk * 4 + lk) * kRrrBs + 16 * w + li];
#pragma unroll
      for (int m = 0; m < kMt; ++m)
        acc[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(Xs[(16 * m + li) * kRrrXs + kk * 4 + lk], bb, acc[m], 0, 0, 0);
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
          out[at] = SCORE ? acc[m][q] : acc[m][q] - ld_f64(y + at);
        }
      }
  }
}

// ---- gradient product: G_t [(C+1) x N] = X_t^T . 2 res_t -----------------------------------------------------
// Leaves acc[4] = the block's 64 features (from c0) x 64 neurons (from n0) of bin t in registers: D element (m, q)
// of wave w, lane (li, lk) is feature c0 + 16 m + lk + 4 q and neuron n0 + 16 w + li.  All K trials go through the
// caller's Xs / Rs (kRrrStep x kRrrTile doubles each) 32 at a time, in order (k ascending within the MFMA's own k
// order, 4 trials per instruction), the next 32 in flight under the MFMAs.  Tails as in the forward: features >=
// C+1 and neurons >= N are never stored (clamped loads); trials >= K must add exactly 0: both loads are clamped to
// the last trial and the residual's factor 2 becomes 0.  Ends on a barrier, so Xs / Rs are free on return.
template <typename Src>
__device__ __forceinline__ void rrr_grad_tile(const Src& src, int64_t K, int64_t T, int64_t N, int C, int64_t t,
                                              int64_t n0, int c0, const double* __restrict__ R, double* Xs, double* Rs,
                                              f64x4 (&acc)[4]) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lk = lane >> 4;
  const int col = tid & 63, row0 = tid >> 6;       // staging: element e = tid + 256 i is (row0 + 4 i, col)
  const int cc = src.clamp(c0 + col, C);
  const int64_t nc = n0 + col < N ? n0 + col : N - 1;
  const int64_t f = src.bin(t);
  const typename Src::Col xc = src.col(f, cc, C);
#pragma unroll
  for (int m = 0; m < 4; ++m) acc[m] = f64x4{0.0, 0.0, 0.0, 0.0};
  typename Src::Raw xr[8];
  double rr[8];
  auto load = [&](int64_t k0) {                    // the next 32 trials, in flight under the MFMAs
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int64_t k = k0 + row0 + 4 * i, kc = k < K ? k : K - 1;
      xr[i] = src.load(kc, f, cc, C);
      rr[i] = R[(kc * T + t) * N + nc] * (k < K ? 2.0 : 0.0);
    }
  };
  load(0);
  for (int64_t k0 = 0; k0 < K; k0 += kRrrStep) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      Xs[tid + 256 * i] = src.stage(xr[i], xc, c0 + col, C);
      Rs[tid + 256 * i] = rr[i];
    }
    __syncthreads();
    if (k0 + kRrrStep < K) load(k0 + kRrrStep);
#pragma unroll
    for (int kk = 0; kk < kRrrStep / 4; ++kk) {
      const double bb = Rs[(kk * 4 + lk) * kRrrTile + 16 * w + li];
#pragma unroll
      for (int m = 0; m < 4; ++m)
        acc[m] = __builtin_amdgcn_mfma_f64_16x16x4f64(Xs[(kk * 4 + lk) * kRrrTile + 16 * m + li], bb, acc[m], 0, 0, 0);
    }
    __syncthreads();
  }
}

// ---- reduction over the bins ----------------------------------------------------------------------------------
// grid (ceil(N/64), C+2), block = 64 neurons x 4 waves, one row c: row c <= C of H / dU / db and its l2 term, row
// C+1 the squared residuals.  part holds S partials [s][t][c][n] (C+2 rows per bin: rows 0..C = G, row C+1 = sq);
// their sum (s ascending) gives G, and H = G + 2 l2 beta overwrites partial 0 in place (each element is read, all
// S partials of it, and written by the same thread), db = H[:,C,:], and over a wave's slice of the bins
// dU[n,c,:] += H V[:,t] and the loss terms; waves combine through LDS in wave order.
// grad == 0 (loss only): rows 0..C have no partials and only their l2 terms are formed.
// BLOCK_LOSS = false: lossp[c][n], one loss term per lane.  true: the block's 64 terms in a fixed tree (dead lanes
// add 0) to lossp[c][neuron block], so the final sum walks (C+2) ceil(N/64) values, not (C+2) N (one block over
// 394,000 values took 0.6 ms at C 768, N 512).
template <bool BLOCK_LOSS>
__global__ __launch_bounds__(256) void rrr_reduce_t_kernel(int64_t T, int64_t N, int C, int r, int S, double l2, int grad,
                                                           double* part, const double* __restrict__ U,
                                                           const double* __restrict__ V, const double* __restrict__ b,
                                                           double* __restrict__ dU, double* __restrict__ db,
                                                           double* __restrict__ lossp) {
  __shared__ double red[(kRrrWaves - 1) * (kRrrMaxR + 1) * 64];
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int c = blockIdx.y;
  const int64_t n = (int64_t)blockIdx.x * 64 + lane;
  const bool live = n < N;
  const int C1 = C + 1;
  const int64_t tper = dcdiv(T, kRrrWaves);
  const int64_t t0 = (int64_t)w * tper;
  const int64_t t1 = t0 + tper < T ? t0 + tper : T;
  double u[kRrrMaxR], du[kRrrMaxR];
#pragma unroll
  for (int j = 0; j < kRrrMaxR; ++j) {
    u[j] = (live && c < C && j < r) ? U[(n * C + c) * r + j] : 0.0;
    du[j] = 0.0;
  }
  double term = 0.0;  // sum beta^2 (rows 0..C) or sum res^2 (row C+1)
  if (live) {
    for (int64_t t = t0; t < t1; ++t) {
      double g = 0.0;
      if (grad || c == C1)
        for (int s = 0; s < S; ++s) g += part[(((int64_t)s * T + t) * (C + 2) + c) * N + n];
      if (c == C1) {
        term += g;
        continue;
      }
      const double be = c < C ? rrr_beta(u, V, r, T, t) : b[n * T + t];
      term = fma(be, be, term);
      if (grad) {
        const double h = fma(2.0 * l2, be, g);
        part[(t * (C + 2) + c) * N + n] = h;
        if (c == C) {
          db[n * T + t] = h;
        } else {
#pragma unroll
          for (int j = 0; j < kRrrMaxR; ++j)
            if (j < r) du[j] = fma(h, V[(int64_t)j * T + t], du[j]);
        }
      }
    }
  }
  if (w > 0) {
    double* p = red + (size_t)(w - 1) * (kRrrMaxR + 1) * 64 + lane;
    p[0] = term;
#pragma unroll
    for (int j = 0; j < kRrrMaxR; ++j) p[(j + 1) * 64] = du[j];
  }
  __syncthreads();
  if (w == 0 && live) {
    for (int v = 1; v < kRrrWaves; ++v) {
      const double* p = red + (size_t)(v - 1) * (kRrrMaxR + 1) * 64 + lane;
      term += p[0];
#pragma unroll
      for (int j = 0; j < kRrrMaxR; ++j) du[j] += p[(j + 1) * 64];
    }
    if (!BLOCK_LOSS) lossp[(int64_t)c * N + n] = c == C1 ? term : l2 * term;
    if (grad && c < C) {
#pragma unroll
      for (int j = 0; j < kRrrMaxR; ++j)
        if (j < r) dU[(n * C + c) * r + j] = du[j];
    }
  }
  if (BLOCK_LOSS && w == 0) {
    double v = live ? (c == C1 ? term : l2 * term) : 0.0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0) lossp[(int64_t)c * gridDim.x + blockIdx.x] = v;
  }
}

// ---- host side (defined in rrr.hip) ---------------------------------------------------------------------------
// loss[0] = the sum of `count` partials: strided over 256 threads + the fixed tree (one block)
void rrr_launch_loss(hipStream_t s, int64_t count, const double* lossp, double* loss);
// dV[i] = sum over p < count of dVp[p stride + i], p ascending, for the r T elements i = j T + t
void rrr_launch_dv_sum(hipStream_t s, int64_t T, int r, int64_t count, int64_t stride, const double* dVp, double* dV);

// The scoring workspace: the standardised yhat [K][T][N] a forward product leaves at offset 0 (`yhat` true: the
// wide and pixel entries; the narrow one computes yhat in the statistics kernel), then the statistics.
size_t rrr_score_workspace_bytes(int64_t K, int64_t T, int64_t N, bool yhat);
// The statistics kernel on that yhat + the final kernel: pred (may be null), bps, r2 and out as vs_rrr_score writes
// them.  gt_dtype VS_F32 or VS_F64.
int rrr_score_yhat(hipStream_t s, int64_t K, int64_t T, int64_t N, const double* mean_y, const double* std_y,
                   const void* gt, int32_t gt_dtype, double* pred, double* bps, double* r2, double* out,
                   void* workspace);

// What every vs_rrr*_loss_grad / vs_rrr*_score entry requires alike, under the entry's name: the dtype code of y /
// gt, no null pointer (`ptrs`: the entry's own conjunction), dU / dV / db together or not at all, the workspace's
// alignment.  VS_OK or VS_EINVAL with the message set.
int rrr_check_loss_grad(const char* entry, int32_t y_dtype, bool ptrs, const double* dU, const double* dV,
                        const double* db, const void* workspace);
int rrr_check_score(const char* entry, int32_t gt_dtype, bool ptrs, const void* workspace);

}  // namespace vs
