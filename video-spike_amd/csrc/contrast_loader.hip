// contrast_loader.hip — the frame transform of the contrastive pretraining loader, which is the reference's
//   src/loader/contrast.py:65-93   ContrastDataset.__getitem__ (index a frame, Resize, Normalize: one frame at a time)
//   src/pretrain.py:60-66          transforms.Resize((144, 144)), transforms.Normalize([0.5], [0.5])
// as one launch over a video that stays on the device in its own dtype:
//   out[g, 0] = ((Resize(frame[idx[g]] / 255) - mean) / std),   g = 0 .. G-1.
// Resize is torchvision's for a float tensor: F.interpolate(bilinear, align_corners=False, antialias=True), a
// separable triangle filter, width first, then height.  Per axis and output index i:
//   scale = in / out, support = max(scale, 1), center = scale (i + 0.5),
//   xmin = max(int(center - support + 0.5), 0), xsize = min(int(center + support + 0.5), in) - xmin,
//   w_j = max(0, 1 - |(j + xmin - center + 0.5) / support|) / (their sum),   j = 0 .. xsize-1.
// torch computes the weights and both sums in f32.  Here the weights are f64, computed once into a small table
// (cf_weights_kernel: [S][tx] for the width, [S][ty] for the height; a caller that keeps the table skips it), and
// each sum is accumulated in f64 and rounded once to f32 (the intermediate image of the width pass is f32, as
// torch's is), so the result is within about one f32 rounding per pass of the exact filter.  x = f32(pixel) / 255
// and the last step (v - mean) / std are f32 operations with IEEE results, as torch's; with in == out the weights
// are (1, 0), so the output equals (f32(pixel) / 255 - mean) / std bit for bit.
//
// Work split: workgroup (band, g) makes `rows` consecutive output rows of frame g.
//   phase 1  a thread owns an output column x: its width weights live in registers (3, 8 or 17 of them: the kernel
//            instance is chosen by the geometry's widest window) and it walks down the source rows the band needs,
//            reading the taps straight from global memory (neighbouring lanes read neighbouring bytes; an 18 KB
//            uint8 frame stays in L2 for the bands that share it, so HBM delivers each source byte once) and
//            writing tmp[row][x] f32 to LDS.
//   phase 2  a thread makes four consecutive outputs of a row from ds_read_b128 reads of tmp, the row's height
//            weights coming from the table (one address per row: a broadcast), and stores them with one 16-byte
//            store, a wave 1 KiB contiguous (scalar stores when S % 4 != 0 or `out` is not 16-byte aligned).
// The windows are recomputed where they are used from cf_window(), the same function on the host and the device
// (`scale` is computed once on the host and passed in; no contraction), so the LDS size, the tap bucket and the
// band's source rows the host plans are exactly what the kernel uses, and what the table holds cannot move a read:
// the table carries weights only.
// An index outside [0, F) reads nothing: its output frame is filled with NaN.  No atomics; equal inputs give
// equal bits.
#include <algorithm>
#include <cmath>

#include "common.h"

namespace vs {

constexpr int kCfMaxTaps = 17;       // in <= 8 out: support <= 8, a window holds at most 16 pixel centres
constexpr int kCfMaxS = 512;
constexpr int kCfThreads = 256;
constexpr int kCfLdsBudget = 48 << 10;  // tmp per workgroup: three workgroups per CU and more

struct CfWindow {
  int xmin, xsize;
};
struct CfAxis {
  double scale;  // in / out
  int in;
  int taps;      // the widest window of the axis = the table's row length
};

// The filter window of output index i (see the header).  Plain IEEE f64 without contraction: the host plans with
// the same values the device computes.
__host__ __device__ inline CfWindow cf_window(const CfAxis& a, int i, double* center_out = nullptr) {
#pragma clang fp contract(off)
  const double support = a.scale < 1.0 ? 1.0 : a.scale;
  const double center = a.scale * ((double)i + 0.5);
  int lo = (int)(center - support + 0.5);
  if (lo < 0) lo = 0;
  int hi = (int)(center + support + 0.5);
  if (hi > a.in) hi = a.in;
  if (center_out) *center_out = center;
  CfWindow w;
  w.xmin = lo;
  w.xsize = hi - lo;
  return w;
}

static CfAxis cf_axis(int in, int out) {
  CfAxis a;
  a.scale = (double)in / (double)out;
  a.in = in;
  a.taps = 1;
  for (int i = 0; i < out; ++i) a.taps = std::max(a.taps, cf_window(a, i).xsize);
  return a;
}

// table[i][0 .. taps) = the normalised f64 weights of output index i, zeros past its window.  One thread per output
// index of either axis: blockIdx.y = 0 the width table, 1 the height table.
__global__ __launch_bounds__(kCfThreads) void cf_weights_kernel(CfAxis ax, CfAxis ay, int S, double* __restrict__ wx,
                                                                double* __restrict__ wy) {
  const int i = blockIdx.x * kCfThreads + threadIdx.x;
  if (i >= S) return;
  const CfAxis a = blockIdx.y ? ay : ax;
  double* row = (blockIdx.y ? wy : wx) + (size_t)i * a.taps;
  double center;
  const CfWindow win = cf_window(a, i, &center);
  const double support = a.scale < 1.0 ? 1.0 : a.scale;
  double total = 0.0;
  for (int j = 0; j < win.xsize; ++j) {
    const double t = fabs(((double)(j + win.xmin) - center + 0.5) / support);
    total += t < 1.0 ? 1.0 - t : 0.0;
  }
  for (int j = 0; j < a.taps; ++j) {
    const double t = fabs(((double)(j + win.xmin) - center + 0.5) / support);
    const double v = (j < win.xsize && t < 1.0) ? 1.0 - t : 0.0;
    row[j] = total != 0.0 ? v / total : v;
  }
}

// x = f32(pixel) / 255, correctly rounded (torch's `tensor(video, dtype=float32).div_(255.0)` on the CPU).  A byte
// takes the quotient's textbook refinement instead of the division's ten-odd instructions: q = p r with
// r = RN(1 / 255), then q + (p - 255 q) r in two fused operations is RN(p / 255) (Markstein; all 256 values are
// checked against the division by tests/test_gpu_contrast_loader.py's identity case).
__device__ __forceinline__ float cf_unit(uint8_t p) {
  const float r = 1.0f / 255.0f, x = (float)p;
  const float q = __fmul_rn(x, r);
  return __fmaf_rn(__fmaf_rn(-q, 255.0f, x), r, q);
}
__device__ __forceinline__ float cf_unit(float p) { return __fdiv_rn(p, 255.0f); }

struct CfPlan {
  CfAxis ax, ay;
  int rows;      // output rows per band
  int bands;
  int src_rows;  // most source rows any band needs
  int nc_shift;  // phase 1: 1 << nc_shift columns per pass, 256 >> nc_shift row groups
  size_t lds;
};

static int cf_band_src_rows(const CfAxis& ay, int y0, int y1) {
  const CfWindow a = cf_window(ay, y0), b = cf_window(ay, y1 - 1);
  return b.xmin + b.xsize - a.xmin;
}

static CfPlan cf_plan(int H, int W, int S) {
  thread_local int last_key[3] = {0, 0, 0};  // a loader asks for one geometry over and over
  thread_local CfPlan last_plan;
  if (last_key[0] == H && last_key[1] == W && last_key[2] == S) return last_plan;
  CfPlan p;
  p.ax = cf_axis(W, S);
  p.ay = cf_axis(H, S);
  // the largest band (at most a quarter of the frame, so that a small batch still fills the chip) within the budget
  int rows = std::max(1, (S + 3) / 4);
  for (;; --rows) {
    int most = 0;
    for (int y0 = 0; y0 < S; y0 += rows) most = std::max(most, cf_band_src_rows(p.ay, y0, std::min(S, y0 + rows)));
    p.src_rows = most;
    p.lds = (size_t)most * S * sizeof(float);
    if (p.lds <= (size_t)kCfLdsBudget || rows == 1) break;
  }
  p.rows = rows;
  p.bands = (int)cdiv(S, rows);
  // columns per pass of phase 1: the power of two in 64 .. 256 that leaves the fewest idle threads
  int best = 6;
  int64_t best_slots = cdiv(S, 64) * 64;
  for (int sh = 7; sh <= 8; ++sh) {
    const int64_t slots = cdiv(S, 1 << sh) << sh;
    if (slots <= best_slots) best = sh, best_slots = slots;
  }
  p.nc_shift = best;
  last_key[0] = H, last_key[1] = W, last_key[2] = S;
  last_plan = p;
  return p;
}

static size_t cf_table_bytes(const CfPlan& p, int S) { return (size_t)S * (p.ax.taps + p.ay.taps) * sizeof(double); }

struct CfNorm {
  float mean, stdv, inv_std;  // inv_std != 0: std is a power of two and the product with 1 / std is the quotient
};

template <int V>
__device__ __forceinline__ void cf_phase2(const float* tmp, const double* __restrict__ wy, const CfAxis& ay, int r0,
                                          int nsrc, int y0, int nrows_out, int S, CfNorm nrm,
                                          float* __restrict__ dst) {
  const int per_row = S / V;
  for (int e = threadIdx.x; e < nrows_out * per_row; e += kCfThreads) {
    const int yl = e / per_row, x = (e - yl * per_row) * V;
    const CfWindow win = cf_window(ay, y0 + yl);
    int n = win.xsize;
    if (n > r0 + nsrc - win.xmin) n = r0 + nsrc - win.xmin;  // never (windows are monotone): no read past tmp
    const float* col = tmp + (size_t)(win.xmin - r0) * S + x;
    const double* w = wy + (size_t)(y0 + yl) * ay.taps;
    double acc[V];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = 0.0;
    for (int j = 0; j < n; ++j) {
      const double wj = w[j];
      float t[V];
      if constexpr (V == 4) {
        const f32x4 q = *(const f32x4*)(col + (size_t)j * S);
        t[0] = q.x, t[1] = q.y, t[2] = q.z, t[3] = q.w;
      } else {
        t[0] = col[(size_t)j * S];
      }
#pragma unroll
      for (int v = 0; v < V; ++v) acc[v] = fma(wj, (double)t[v], acc[v]);
    }
    float o[V];
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const float c = __fsub_rn((float)acc[v], nrm.mean);
      o[v] = nrm.inv_std != 0.f ? __fmul_rn(c, nrm.inv_std) : __fdiv_rn(c, nrm.stdv);
    }
    float* q = dst + (size_t)(y0 + yl) * S + x;
    if constexpr (V == 4) {
      f32x4 r = {o[0], o[1], o[2], o[3]};
      *(f32x4*)q = r;
    } else {
      q[0] = o[0];
    }
  }
}

// grid (bands, G), 256 threads, dynamic LDS src_cap * S floats
template <typename TI, int TX>
__global__ __launch_bounds__(kCfThreads) void contrast_frames_kernel(const TI* __restrict__ video, int64_t F, CfAxis ax,
                                                                     CfAxis ay, const int64_t* __restrict__ idx, int S,
                                                                     int rows, int src_cap, int nc_shift,
                                                                     const double* __restrict__ wx,
                                                                     const double* __restrict__ wy, CfNorm nrm, int vec,
                                                                     float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) float cf_tmp[];
  const int tid = threadIdx.x;
  const int H = ay.in, W = ax.in;
  const int y0 = blockIdx.x * rows;
  const int y1 = y0 + rows < S ? y0 + rows : S;
  const int nrows_out = y1 - y0;
  float* dst = out + (int64_t)blockIdx.y * S * S;
  const int64_t f = idx[blockIdx.y];
  if (f < 0 || f >= F) {  // nothing is read for a bad index; the frame says so
    for (int e = tid; e < nrows_out * S; e += kCfThreads) dst[(size_t)y0 * S + e] = __builtin_nanf("");
    return;
  }
  const TI* src = video + f * (int64_t)H * W;
  const CfWindow first = cf_window(ay, y0), last = cf_window(ay, y1 - 1);
  const int r0 = first.xmin;
  int nsrc = last.xmin + last.xsize - r0;
  if (nsrc > src_cap) nsrc = src_cap;  // never: the host planned src_cap with the same function

  // phase 1: tmp[r][x] = sum_j wx[x][j] * src[r0 + r][xmin[x] + j] / 255
  const int nc = 1 << nc_shift;
  const int c = tid & (nc - 1), rg = tid >> nc_shift, nrg = kCfThreads >> nc_shift;
  for (int x = c; x < S; x += nc) {
    const CfWindow win = cf_window(ax, x);
    double w[TX];
    int off[TX];  // a tap past the window has weight 0 and re-reads a pixel of the row
#pragma unroll
    for (int j = 0; j < TX; ++j) {
      w[j] = (j < ax.taps && j < win.xsize) ? wx[(size_t)x * ax.taps + j] : 0.0;
      off[j] = win.xmin + j < W ? win.xmin + j : W - 1;
    }
#pragma unroll(TX <= 3 && sizeof(TI) == 1 ? 4 : 1)  // bytes, narrow windows: four rows' loads in flight (measured:
                                                    // 26.2 -> 24.8 us at the workload; on f32 frames 27 -> 34 us)
    for (int r = rg; r < nsrc; r += nrg) {
      const TI* row = src + (int64_t)(r0 + r) * W;
      TI p[TX];
#pragma unroll
      for (int j = 0; j < TX; ++j) p[j] = row[off[j]];
      double acc = 0.0;
#pragma unroll
      for (int j = 0; j < TX; ++j) acc = fma(w[j], j < win.xsize ? (double)cf_unit(p[j]) : 0.0, acc);
      cf_tmp[(size_t)r * S + x] = (float)acc;
    }
  }
  __syncthreads();

  // phase 2: out[y][x] = (sum_j wy[y][j] * tmp[ymin[y] - r0 + j][x] - mean) / std
  if (vec)
    cf_phase2<4>(cf_tmp, wy, ay, r0, nsrc, y0, nrows_out, S, nrm, dst);
  else
    cf_phase2<1>(cf_tmp, wy, ay, r0, nsrc, y0, nrows_out, S, nrm, dst);
}

template <typename TI, int TX>
static int cf_launch(hipStream_t s, const CfPlan& p, const TI* video, int64_t F, const int64_t* idx, int64_t G, int S,
                     const double* wx, const double* wy, CfNorm nrm, int vec, float* out) {
  auto kern = contrast_frames_kernel<TI, TX>;
  hipLaunchKernelGGL(kern, dim3((unsigned)p.bands, (unsigned)G), dim3(kCfThreads), p.lds, s, video, F, p.ax, p.ay, idx,
                     S, p.rows, p.src_rows, p.nc_shift, wx, wy, nrm, vec, out);
  VS_LAUNCH_CHECK();
  return VS_OK;
}

template <typename TI>
static int cf_dispatch(hipStream_t s, const CfPlan& p, const void* video, int64_t F, const int64_t* idx, int64_t G,
                       int S, const double* wx, const double* wy, CfNorm nrm, int vec, float* out) {
  const TI* v = (const TI*)video;
  if (p.ax.taps <= 3) return cf_launch<TI, 3>(s, p, v, F, idx, G, S, wx, wy, nrm, vec, out);
  if (p.ax.taps <= 8) return cf_launch<TI, 8>(s, p, v, F, idx, G, S, wx, wy, nrm, vec, out);
  return cf_launch<TI, kCfMaxTaps>(s, p, v, F, idx, G, S, wx, wy, nrm, vec, out);
}

static bool cf_extents_ok(int64_t H, int64_t W, int64_t S) {
  return S >= 1 && S <= kCfMaxS && H >= 1 && W >= 1 && H <= 8 * S && W <= 8 * S;
}

}  // namespace vs

using namespace vs;

extern "C" size_t vs_contrast_frames_workspace_bytes(int64_t H, int64_t W, int64_t S) {
  if (!cf_extents_ok(H, W, S)) return 0;
  return cf_table_bytes(cf_plan((int)H, (int)W, (int)S), (int)S);
}

extern "C" int vs_contrast_frames(int32_t in_dtype, int64_t F, int64_t H, int64_t W, const void* video,
                                  const int64_t* idx, int64_t G, int64_t S, float mean, float std, float* out,
                                  void* workspace, int32_t weights_ready, void* stream) {
  VS_REQUIRE(in_dtype == VS_F32 || in_dtype == VS_U8, "vs_contrast_frames: in_dtype must be VS_F32 or VS_U8");
  VS_REQUIRE(S >= 1 && S <= kCfMaxS, "vs_contrast_frames: 1 <= S <= 512");
  VS_REQUIRE(H >= 1 && W >= 1 && H <= 8 * S && W <= 8 * S, "vs_contrast_frames: 1 <= H, W <= 8 S");
  VS_REQUIRE(F >= 1 && G >= 0 && G <= 65535, "vs_contrast_frames: F >= 1 frames, 0 <= G <= 65535 indices");
  VS_REQUIRE(std != 0.f && std == std && mean == mean, "vs_contrast_frames: std must be non-zero");
  if (G == 0) return VS_OK;
  VS_REQUIRE(video && idx && out && workspace, "vs_contrast_frames: null pointer");
  VS_REQUIRE((((uintptr_t)idx) & 7u) == 0 && (((uintptr_t)workspace) & 7u) == 0 && (((uintptr_t)out) & 3u) == 0 &&
                 (in_dtype == VS_U8 || (((uintptr_t)video) & 3u) == 0),
             "vs_contrast_frames: idx and workspace must be 8-byte aligned, f32 tensors 4-byte aligned");
  const CfPlan p = cf_plan((int)H, (int)W, (int)S);
  VS_REQUIRE(p.ax.taps <= kCfMaxTaps && p.ay.taps <= kCfMaxTaps && p.lds <= (size_t)(64 << 10),
             "vs_contrast_frames: filter window beyond 17 taps");
  int e = 0;
  const float m = std::frexp(std, &e);
  CfNorm nrm;
  nrm.mean = mean;
  nrm.stdv = std;
  nrm.inv_std = (m == 0.5f || m == -0.5f) && e > -120 && e < 120 ? 1.0f / std : 0.f;
  const int vec = (S % 4 == 0) && aligned16(out);
  double* wx = (double*)workspace;
  double* wy = wx + (size_t)S * p.ax.taps;
  hipStream_t s = (hipStream_t)stream;
  ScopedTimer timer(VS_TIMER_MISC, s, (double)G * ((double)H * W * (in_dtype == VS_U8 ? 1.0 : 4.0) + (double)S * S * 4.0));
  if (!weights_ready) {
    hipLaunchKernelGGL(cf_weights_kernel, dim3((unsigned)cdiv(S, kCfThreads), 2), dim3(kCfThreads), 0, s, p.ax, p.ay,
                       (int)S, wx, wy);
    VS_LAUNCH_CHECK();
  }
  if (in_dtype == VS_U8) return cf_dispatch<uint8_t>(s, p, video, F, idx, G, (int)S, wx, wy, nrm, vec, out);
  return cf_dispatch<float>(s, p, video, F, idx, G, (int)S, wx, wy, nrm, vec, out);
}

// out[0..5] = the plan for (H, W, S): rows per band, bands, source rows per band, width taps, height taps,
// LDS bytes: what a test needs to see which kernel instance and split a geometry takes
extern "C" int vs_contrast_frames_plan(int64_t H, int64_t W, int64_t S, int32_t* out) {
  VS_REQUIRE(out, "vs_contrast_frames_plan: null pointer");
  VS_REQUIRE(cf_extents_ok(H, W, S), "vs_contrast_frames_plan: 1 <= S <= 512, 1 <= H, W <= 8 S");
  const CfPlan p = cf_plan((int)H, (int)W, (int)S);
  out[0] = p.rows, out[1] = p.bands, out[2] = p.src_rows, out[3] = p.ax.taps, out[4] = p.ay.taps, out[5] = (int)p.lds;
  return VS_OK;
}
