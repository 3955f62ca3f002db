// pca.hip — PCA of a video by block subspace iteration: the kernels under vspike.pca.PCA, which is the reference's
//   src/utils/utils.py:350-360   get_pca_embedding (sklearn PCA(n_components).fit_transform on the [n t, h w] pixels)
//   src/use_cebra.py:59-97       its use for the RRR baseline's input_mod 'pca'
// X [M, D] row-major, uint8 or f32, is stored once (M frames of D pixels: 60,000 x 18,260 for one session); the
// centred matrix Xc = X - 1 mu^T is never written.  An element is centred on its way into LDS: x - mu_d in f64,
// rounded once to f32 (uint8 pixels are exact in either).  Both products run on the exact-f32 MFMA
// (v_mfma_f32_16x16x4_f32; A[i][k]: lane = i + 16 k, B[k][j]: lane = j + 16 k, D[i][j]: lane = j + 16 (i >> 2),
// register i & 3).  A wave's f32 accumulators are added to f64 registers every 64 (project) / 128 (xty) terms of
// the reduction, so an f32 sum never runs over more than 128 products.  No atomics; partial sums of different
// workgroups are added in f64 in ascending order, so two calls on the same inputs agree bitwise.
//
// Tails add exact zeros and read nothing outside the operands: a load past the last row / column is clamped to
// the last row / column of X and its centred value replaced by 0; Q is copied to f32 with zero rows up to a
// multiple of 64 and zero columns up to 32, Y is stored with zero rows up to a multiple of 128.
//
//   vs_pca_colmean     pca_colsum_kernel (grid ceil(D/256) x chunks: a thread walks its column down the chunk's rows)
//                      + pca_colmean_kernel (chunks added in ascending order, / M).
//   vs_pca_project     pca_q32_kernel (Q -> f32) + pca_project_kernel: block = 128 rows, 4 waves x 32 rows, all D
//                      through LDS 64 columns at a time (X tile + Q tile), the next slice's loads in flight under the
//                      MFMAs.  Y[m, l] f64.
//   vs_pca_gram_apply  pca_q32_kernel + pca_project_kernel (Y as f32 [roundup(M,128)][32] in the workspace)
//                      + pca_xty_kernel: block = 128 columns x one chunk of rows, 4 waves x 32 columns, the rows
//                      through LDS 32 at a time; partial W [chunk][D][L] f64
//                      + pca_wsum_kernel: W = the chunks' partials added in ascending order.
//                      X is read twice per step.  (One kernel would have to hold a row block's X tile, 128 x D, on
//                      chip between the two products; DESIGN.md section 7 has the measurements.)
// chunks(M) = min(ceil(M / 512), 16); a chunk is ceil(M / chunks) rows rounded up to a multiple of 128.
// Workspace (bytes, each piece rounded up to 256):
//   colmean     chunks D 8
//   project     roundup(D, 64) 32 4
//   gram_apply  roundup(D, 64) 32 4  +  roundup(M, 128) 32 4  +  chunks D L 8
// i.e. 45 MB for gram_apply at M 60,000, D 18,260, L 15, against 1.1 GB of uint8 X.
#include "common.h"

namespace vs {

constexpr int kPcaMaxL = 32;
constexpr int kPcaRows = 128;       // rows per block of the Y product (4 waves x 2 MFMA row tiles)
constexpr int kPcaStep = 64;        // columns of X staged in LDS at a time by the Y product
constexpr int kPcaXs = 68;          // its X tile's row stride (floats): the A reads go down a column
constexpr int kPcaCols = 128;       // columns per block of the W product (4 waves x 2 MFMA row tiles of X^T)
constexpr int kPcaMStep = 32;       // rows of X staged in LDS at a time by the W product
constexpr int kPcaCs = 144;         // its X tile's row stride: 16 k + i is a different bank for k = 0, 1
constexpr int kPcaFlush = 4;        // W product: stages between two flushes of the f32 accumulators to f64
constexpr int kPcaChunkRows = 512;  // a reduction over the rows is split once per this many rows ...
constexpr int kPcaMaxChunks = 16;   // ... into at most this many chunks

template <typename XT> __device__ __forceinline__ double pca_ld(const XT* p) { return (double)*p; }

struct PcaChunks {
  int chunks;
  int64_t rows;  // per chunk, a multiple of kPcaRows
};
static PcaChunks pca_chunks(int64_t M) {
  int64_t ch = cdiv(M, kPcaChunkRows);
  if (ch > kPcaMaxChunks) ch = kPcaMaxChunks;
  PcaChunks c;
  c.rows = cdiv(cdiv(M, ch), kPcaRows) * kPcaRows;
  c.chunks = (int)cdiv(M, c.rows);
  return c;
}

// grid (ceil(D/256), chunks): part[ch][d] = sum of X[m][d] over the chunk's rows, ascending, f64
template <typename XT>
__global__ __launch_bounds__(256) void pca_colsum_kernel(int64_t M, int64_t D, int64_t rows,
                                                         const XT* __restrict__ X, double* __restrict__ part) {
  const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (d >= D) return;
  const int64_t m0 = (int64_t)blockIdx.y * rows;
  const int64_t m1 = m0 + rows < M ? m0 + rows : M;
  double s = 0.0;
  int64_t m = m0;
  for (; m + 8 <= m1; m += 8) {
    double v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = pca_ld(X + (m + i) * D + d);
#pragma unroll
    for (int i = 0; i < 8; ++i) s += v[i];
  }
  for (; m < m1; ++m) s += pca_ld(X + m * D + d);
  part[(int64_t)blockIdx.y * D + d] = s;
}

__global__ __launch_bounds__(256) void pca_colmean_kernel(int64_t M, int64_t D, int chunks,
                                                          const double* __restrict__ part, double* __restrict__ mu) {
  const int64_t d = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (d >= D) return;
  double s = 0.0;
  for (int ch = 0; ch < chunks; ++ch) s += part[(int64_t)ch * D + d];
  mu[d] = s / (double)M;
}

// Qf [Dp][32] f32 = Q [D][L] f64 rounded, zero elsewhere (Dp = roundup(D, 64)).  One thread per element of Qf.
__global__ __launch_bounds__(256) void pca_q32_kernel(int64_t D, int64_t Dp, int L, const double* __restrict__ Q,
                                                      float* __restrict__ Qf) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= Dp * kPcaMaxL) return;
  const int64_t d = e / kPcaMaxL;
  const int l = (int)(e - d * kPcaMaxL);
  Qf[e] = (d < D && l < L) ? (float)Q[d * L + l] : 0.f;
}

// grid ceil(M/128).  NT = column tiles of 16 (L <= 16: 1, else 2).  F32OUT: Yf [roundup(M,128)][32] f32 with zero
// rows past M (columns 16 NT .. 31 are not written and not read by the W product of the same NT); else Y [M][L] f64.
template <typename XT, int NT, bool F32OUT>
__global__ __launch_bounds__(256) void pca_project_kernel(int64_t M, int64_t D, int L, const XT* __restrict__ X,
                                                          const double* __restrict__ mu,
                                                          const float* __restrict__ Qf, double* __restrict__ Y,
                                                          float* __restrict__ Yf) {
  constexpr int kXl = kPcaRows * kPcaStep / 256;   // X elements per thread and stage
  constexpr int kQl = kPcaStep * 16 * NT / 256;    // Q elements per thread and stage
  __shared__ float Xs[kPcaRows * kPcaXs];
  __shared__ float Qs[kPcaStep * 16 * NT];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lk = lane >> 4;
  const int64_t m0 = (int64_t)blockIdx.x * kPcaRows;
  const int col = tid & 63, row0 = tid >> 6;       // staging: element (row0 + 4 i, col)
  XT xr[kXl];
  float qr[kQl];
  double mur;
  // Rows >= M are rows of the product that are never stored as such (F32OUT stores zeros there): their loads are
  // clamped to the last row.  Columns >= D must add exactly 0: the load is clamped to the row's last column, the
  // centred value is replaced by 0 and Qf's rows there are 0.
  auto load = [&](int64_t d0) {
    const int64_t d = d0 + col, dc = d < D ? d : D - 1;
    mur = mu[dc];
#pragma unroll
    for (int i = 0; i < kXl; ++i) {
      const int64_t m = m0 + row0 + 4 * i;
      xr[i] = X[(m < M ? m : M - 1) * D + dc];
    }
#pragma unroll
    for (int i = 0; i < kQl; ++i) {
      const int e = tid + 256 * i;                 // (row e / (16 NT), column e % (16 NT)) of the Q tile
      qr[i] = Qf[(d0 + e / (16 * NT)) * kPcaMaxL + e % (16 * NT)];
    }
  };
  f32x4 acc[2][NT];
  double accd[2][NT][4];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      acc[a][n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int q = 0; q < 4; ++q) accd[a][n][q] = 0.0;
    }
  load(0);
  for (int64_t d0 = 0; d0 < D; d0 += kPcaStep) {
    const bool live = d0 + col < D;
#pragma unroll
    for (int i = 0; i < kXl; ++i)
      Xs[(row0 + 4 * i) * kPcaXs + col] = live ? (float)((double)xr[i] - mur) : 0.f;
#pragma unroll
    for (int i = 0; i < kQl; ++i) Qs[tid + 256 * i] = qr[i];
    __syncthreads();
    if (d0 + kPcaStep < D) load(d0 + kPcaStep);
#pragma unroll
    for (int kk = 0; kk < kPcaStep / 4; ++kk) {
      float bf[NT];
#pragma unroll
      for (int n = 0; n < NT; ++n) bf[n] = Qs[(kk * 4 + lk) * 16 * NT + 16 * n + li];
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const float af = Xs[(32 * w + 16 * a + li) * kPcaXs + kk * 4 + lk];
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[a][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(af, bf[n], acc[a][n], 0, 0, 0);
      }
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int n = 0; n < NT; ++n) {
#pragma unroll
        for (int q = 0; q < 4; ++q) accd[a][n][q] += (double)acc[a][n][q];
        acc[a][n] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t m = m0 + 32 * w + 16 * a + 4 * lk + q;
        const int l = 16 * n + li;
        if (F32OUT) {
          Yf[m * kPcaMaxL + l] = m < M ? (float)accd[a][n][q] : 0.f;
        } else if (m < M && l < L) {
          Y[m * L + l] = accd[a][n][q];
        }
      }
}

// grid (ceil(D/128), chunks): Wp[ch][d][l] = sum over the chunk's rows m (ascending) of Xc[m][d] Yf[m][l].
// A = Xc^T: A[i = column][k = row].  Yf has zero rows up to roundup(M, 128) >= every row a stage touches.
template <typename XT, int NT>
__global__ __launch_bounds__(256) void pca_xty_kernel(int64_t M, int64_t D, int L, int64_t rows,
                                                      const XT* __restrict__ X, const double* __restrict__ mu,
                                                      const float* __restrict__ Yf, double* __restrict__ Wp) {
  constexpr int kXl = kPcaMStep * kPcaCols / 256;   // X elements per thread and stage
  constexpr int kYl = kPcaMStep * 16 * NT / 256;    // Y elements per thread and stage
  __shared__ float Xs[kPcaMStep * kPcaCs];
  __shared__ float Ys[kPcaMStep * 16 * NT];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lk = lane >> 4;
  const int64_t d0 = (int64_t)blockIdx.x * kPcaCols;
  const int64_t mb = (int64_t)blockIdx.y * rows;
  const int64_t me = mb + rows < M ? mb + rows : M;
  const int col = tid & 127, row0 = tid >> 7;       // staging: element (row0 + 2 i, col)
  const bool live = d0 + col < D;                   // columns >= D are never stored: clamped loads
  const int64_t dc = live ? d0 + col : D - 1;
  const double mur = mu[dc];
  XT xr[kXl];
  float yr[kYl];
  auto load = [&](int64_t ms) {
#pragma unroll
    for (int i = 0; i < kXl; ++i) {
      const int64_t m = ms + row0 + 2 * i;
      xr[i] = X[(m < M ? m : M - 1) * D + dc];
    }
#pragma unroll
    for (int i = 0; i < kYl; ++i) {
      const int e = tid + 256 * i;                  // (row e / (16 NT), column e % (16 NT)) of the Y tile
      yr[i] = Yf[(ms + e / (16 * NT)) * kPcaMaxL + e % (16 * NT)];
    }
  };
  f32x4 acc[2][NT];
  double accd[2][NT][4];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      acc[a][n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int q = 0; q < 4; ++q) accd[a][n][q] = 0.0;
    }
  auto flush = [&]() {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int n = 0; n < NT; ++n) {
#pragma unroll
        for (int q = 0; q < 4; ++q) accd[a][n][q] += (double)acc[a][n][q];
        acc[a][n] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
  };
  load(mb);
  int stage = 0;
  for (int64_t ms = mb; ms < me; ms += kPcaMStep) {
    // rows >= M must add exactly 0: the load was clamped to the last row, the centred value is replaced by 0
    // (and Yf's rows there are 0)
#pragma unroll
    for (int i = 0; i < kXl; ++i) {
      const int r = row0 + 2 * i;
      Xs[r * kPcaCs + col] = ms + r < M ? (float)((double)xr[i] - mur) : 0.f;
    }
#pragma unroll
    for (int i = 0; i < kYl; ++i) Ys[tid + 256 * i] = yr[i];
    __syncthreads();
    if (ms + kPcaMStep < me) load(ms + kPcaMStep);
#pragma unroll
    for (int kk = 0; kk < kPcaMStep / 4; ++kk) {
      float bf[NT];
#pragma unroll
      for (int n = 0; n < NT; ++n) bf[n] = Ys[(kk * 4 + lk) * 16 * NT + 16 * n + li];
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const float af = Xs[(kk * 4 + lk) * kPcaCs + 32 * w + 16 * a + li];
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[a][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(af, bf[n], acc[a][n], 0, 0, 0);
      }
    }
    if (++stage == kPcaFlush) {
      flush();
      stage = 0;
    }
    __syncthreads();
  }
  flush();
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t d = d0 + 32 * w + 16 * a + 4 * lk + q;
        const int l = 16 * n + li;
        if (d < D && l < L) Wp[((int64_t)blockIdx.y * D + d) * L + l] = accd[a][n][q];
      }
}

// W[e] = sum of the chunks' partials, ascending (e over D L)
__global__ __launch_bounds__(256) void pca_wsum_kernel(int64_t count, int chunks, const double* __restrict__ Wp,
                                                       double* __restrict__ W) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= count) return;
  double s = 0.0;
  for (int ch = 0; ch < chunks; ++ch) s += Wp[(int64_t)ch * count + e];
  W[e] = s;
}

struct PcaWs {
  PcaChunks c;
  int64_t Dp, Mp;
  size_t q, y, wp, total;  // byte offsets
};
static PcaWs pca_ws(int64_t M, int64_t D, int64_t L, bool gram) {
  PcaWs w;
  w.c = pca_chunks(M);
  w.Dp = cdiv(D, kPcaStep) * kPcaStep;
  w.Mp = cdiv(M, kPcaRows) * kPcaRows;
  auto al = [](size_t bytes) { return (bytes + 255) / 256 * 256; };
  size_t off = 0;
  w.q = off;  off += al((size_t)w.Dp * kPcaMaxL * 4);
  w.y = off;  if (gram) off += al((size_t)w.Mp * kPcaMaxL * 4);
  w.wp = off; if (gram) off += al((size_t)w.c.chunks * D * L * 8);
  w.total = off;
  return w;
}

// every grid's x extent (the largest are ceil(M/128) and roundup(D,64)/8 blocks) stays below 2^31, and M D, the
// element count of X, below 2^61
static bool pca_dims_ok(int64_t M, int64_t D) {
  return M >= 2 && D >= 1 && M <= ((int64_t)1 << 30) && D <= ((int64_t)1 << 30);
}

template <typename XT>
static void pca_launch_project(hipStream_t s, int64_t M, int64_t D, int L, const XT* X, const double* mu,
                               const float* Qf, double* Y, float* Yf) {
  const dim3 grid((unsigned)cdiv(M, kPcaRows));
  if (Yf) {
    if (L <= 16)
      hipLaunchKernelGGL((pca_project_kernel<XT, 1, true>), grid, dim3(256), 0, s, M, D, L, X, mu, Qf, Y, Yf);
    else
      hipLaunchKernelGGL((pca_project_kernel<XT, 2, true>), grid, dim3(256), 0, s, M, D, L, X, mu, Qf, Y, Yf);
  } else {
    if (L <= 16)
      hipLaunchKernelGGL((pca_project_kernel<XT, 1, false>), grid, dim3(256), 0, s, M, D, L, X, mu, Qf, Y, Yf);
    else
      hipLaunchKernelGGL((pca_project_kernel<XT, 2, false>), grid, dim3(256), 0, s, M, D, L, X, mu, Qf, Y, Yf);
  }
}

template <typename XT>
static void pca_launch_xty(hipStream_t s, int64_t M, int64_t D, int L, const PcaChunks& c, const XT* X,
                           const double* mu, const float* Yf, double* Wp) {
  const dim3 grid((unsigned)cdiv(D, kPcaCols), (unsigned)c.chunks);
  if (L <= 16)
    hipLaunchKernelGGL((pca_xty_kernel<XT, 1>), grid, dim3(256), 0, s, M, D, L, c.rows, X, mu, Yf, Wp);
  else
    hipLaunchKernelGGL((pca_xty_kernel<XT, 2>), grid, dim3(256), 0, s, M, D, L, c.rows, X, mu, Yf, Wp);
}

static void pca_launch_q32(hipStream_t s, int64_t D, int64_t Dp, int L, const double* Q, float* Qf) {
  hipLaunchKernelGGL(pca_q32_kernel, dim3((unsigned)cdiv(Dp * kPcaMaxL, 256)), dim3(256), 0, s, D, Dp, L, Q, Qf);
}

}  // namespace vs

using namespace vs;

#define PCA_COMMON_CHECKS(name)                                                                                  \
  VS_REQUIRE(pca_dims_ok(M, D), name ": M >= 2 rows and D >= 1 columns");                                         \
  VS_REQUIRE(x_dtype == VS_U8 || x_dtype == VS_F32, name ": X must be uint8 or f32");                             \
  VS_REQUIRE(x_dtype == VS_U8 || (((uintptr_t)X) & 3u) == 0, name ": an f32 X must be 4-byte aligned");           \
  VS_REQUIRE((((uintptr_t)workspace) & 15u) == 0, name ": workspace must be 16-byte aligned")

extern "C" size_t vs_pca_colmean_workspace_bytes(int64_t M, int64_t D) {
  if (!pca_dims_ok(M, D)) return 0;
  return ((size_t)pca_chunks(M).chunks * D * 8 + 255) / 256 * 256;
}

extern "C" int vs_pca_colmean(int64_t M, int64_t D, const void* X, int32_t x_dtype, double* mu, void* workspace,
                              void* stream) {
  PCA_COMMON_CHECKS("vs_pca_colmean");
  VS_REQUIRE(X && mu && workspace, "vs_pca_colmean: null pointer");
  VS_REQUIRE((((uintptr_t)mu) & 7u) == 0, "vs_pca_colmean: mu must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const PcaChunks c = pca_chunks(M);
  double* part = (double*)workspace;
  ScopedTimer timer(VS_TIMER_MISC, s, (double)M * D * (x_dtype == VS_U8 ? 1.0 : 4.0));
  count_pca(VS_PCA_PATH_COLMEAN);
  const dim3 grid((unsigned)cdiv(D, 256), (unsigned)c.chunks);
  if (x_dtype == VS_U8)
    hipLaunchKernelGGL(pca_colsum_kernel<uint8_t>, grid, dim3(256), 0, s, M, D, c.rows, (const uint8_t*)X, part);
  else
    hipLaunchKernelGGL(pca_colsum_kernel<float>, grid, dim3(256), 0, s, M, D, c.rows, (const float*)X, part);
  VS_LAUNCH_CHECK();
  hipLaunchKernelGGL(pca_colmean_kernel, dim3((unsigned)cdiv(D, 256)), dim3(256), 0, s, M, D, c.chunks,
                     (const double*)part, mu);
  VS_LAUNCH_CHECK();
  return VS_OK;
}

extern "C" size_t vs_pca_project_workspace_bytes(int64_t M, int64_t D, int64_t L) {
  if (!pca_dims_ok(M, D) || L < 1 || L > kPcaMaxL) return 0;
  return pca_ws(M, D, L, false).total;
}

extern "C" int vs_pca_project(int64_t M, int64_t D, int64_t L, const void* X, int32_t x_dtype, const double* mu,
                              const double* Q, double* Y, void* workspace, void* stream) {
  PCA_COMMON_CHECKS("vs_pca_project");
  VS_REQUIRE(L >= 1 && L <= kPcaMaxL, "vs_pca_project: 1 <= L <= 32 columns of Q");
  VS_REQUIRE(X && mu && Q && Y && workspace, "vs_pca_project: null pointer");
  VS_REQUIRE(((((uintptr_t)mu) | ((uintptr_t)Q) | ((uintptr_t)Y)) & 7u) == 0,
             "vs_pca_project: mu, Q, Y must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const PcaWs w = pca_ws(M, D, L, false);
  float* Qf = (float*)((char*)workspace + w.q);
  ScopedTimer timer(VS_TIMER_MISC, s, (double)M * D * (x_dtype == VS_U8 ? 1.0 : 4.0) + (double)M * L * 8.0);
  count_pca(VS_PCA_PATH_PROJECT);
  pca_launch_q32(s, D, w.Dp, (int)L, Q, Qf);
  VS_LAUNCH_CHECK();
  if (x_dtype == VS_U8)
    pca_launch_project<uint8_t>(s, M, D, (int)L, (const uint8_t*)X, mu, Qf, Y, nullptr);
  else
    pca_launch_project<float>(s, M, D, (int)L, (const float*)X, mu, Qf, Y, nullptr);
  VS_LAUNCH_CHECK();
  return VS_OK;
}

extern "C" size_t vs_pca_gram_apply_workspace_bytes(int64_t M, int64_t D, int64_t L) {
  if (!pca_dims_ok(M, D) || L < 1 || L > kPcaMaxL) return 0;
  return pca_ws(M, D, L, true).total;
}

extern "C" int vs_pca_gram_apply(int64_t M, int64_t D, int64_t L, const void* X, int32_t x_dtype, const double* mu,
                                 const double* Q, double* W, void* workspace, void* stream) {
  PCA_COMMON_CHECKS("vs_pca_gram_apply");
  VS_REQUIRE(L >= 1 && L <= kPcaMaxL, "vs_pca_gram_apply: 1 <= L <= 32 columns of Q");
  VS_REQUIRE(X && mu && Q && W && workspace, "vs_pca_gram_apply: null pointer");
  VS_REQUIRE(((((uintptr_t)mu) | ((uintptr_t)Q) | ((uintptr_t)W)) & 7u) == 0,
             "vs_pca_gram_apply: mu, Q, W must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const PcaWs w = pca_ws(M, D, L, true);
  float* Qf = (float*)((char*)workspace + w.q);
  float* Yf = (float*)((char*)workspace + w.y);
  double* Wp = (double*)((char*)workspace + w.wp);
  ScopedTimer timer(VS_TIMER_MISC, s, 2.0 * (double)M * D * (x_dtype == VS_U8 ? 1.0 : 4.0));
  count_pca(VS_PCA_PATH_GRAM);
  pca_launch_q32(s, D, w.Dp, (int)L, Q, Qf);
  VS_LAUNCH_CHECK();
  if (x_dtype == VS_U8) {
    pca_launch_project<uint8_t>(s, M, D, (int)L, (const uint8_t*)X, mu, Qf, nullptr, Yf);
    VS_LAUNCH_CHECK();
    pca_launch_xty<uint8_t>(s, M, D, (int)L, w.c, (const uint8_t*)X, mu, Yf, Wp);
  } else {
    pca_launch_project<float>(s, M, D, (int)L, (const float*)X, mu, Qf, nullptr, Yf);
    VS_LAUNCH_CHECK();
    pca_launch_xty<float>(s, M, D, (int)L, w.c, (const float*)X, mu, Yf, Wp);
  }
  VS_LAUNCH_CHECK();
  hipLaunchKernelGGL(pca_wsum_kernel, dim3((unsigned)cdiv(D * L, 256)), dim3(256), 0, s, D * L, w.c.chunks,
                     (const double*)Wp, W);
  VS_LAUNCH_CHECK();
  return VS_OK;
}

extern "C" int vs_pca_tiles(int32_t* out) {
  VS_REQUIRE(out, "vs_pca_tiles: null pointer");
  out[0] = kPcaRows;
  out[1] = kPcaCols;
  out[2] = kPcaChunkRows;
  out[3] = kPcaMaxChunks;
  return VS_OK;
}
