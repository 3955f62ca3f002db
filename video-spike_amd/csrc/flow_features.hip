// flow_features.hip — the per-frame scalars of the RRR behaviour baselines, which are the reference's
//   src/utils/ibl_data_utils.py:1103-1243  get_optic_flow (motion energy, clipped mean flow, per-frame medians of |flow|)
//   src/utils/utils.py:226-304             get_rrr_data   (np.median of each signed flow component per frame)
// from a dense flow field flow[K][F-1][H*W][2] f32 and a video[K][F][H*W] u8 / f32 that stay where they are.
//
// Order statistics are exact: a value is mapped to a uint32 key whose unsigned order is the float order
// (sign bit set: ~bits, else bits | 0x80000000), and the key of rank k is found MSB first, eight bits per pass, from
// 256-bin histograms of the keys that share the prefix found so far (radix select; four passes).
//
//   vs_flow_median2    one workgroup of 1024 threads per frame, both components at once.  Pass 0 reads the interleaved
//                      field once with 8-byte loads and, while H W <= kFfStageMax, leaves BOTH components' keys in LDS
//                      (2 x 4 H W bytes + 2 KiB of histograms: 146 KB of the CU's 160 KiB at 110 x 166, one workgroup
//                      per CU, sixteen waves); the later passes read LDS only.  Above that the passes re-read the frame
//                      from global memory.  The rank is (n - 1) / 2; for an even n the other middle element is the same
//                      key (when the last bin holds more than the rank's own element) or the smallest larger key (one
//                      more pass), and the result is (a + b) / 2 in f32, numpy's mean of the two.  A NaN in a frame's
//                      component gives NaN for that component.  Histogram adds are LDS integer atomics; a thread first
//                      merges runs of equal digits, since the top byte of a flow field takes two or three values.
//   vs_flow_quantiles  per (trial, component) the order statistics of |flow| that np.percentile(., q) interpolates between
//                      for two percentiles, over n = (F - 1) H W values.  Per pass a count kernel (chunks of kFqChunk
//                      pixels, LDS histograms, non-zero bins added to the trial's histogram in the workspace with integer
//                      atomics) and a pick kernel (one workgroup per (trial, component): the bin of each of the four
//                      ranks, the new prefixes, histogram zeroed).  Ranks that share a prefix share a histogram.  The
//                      last pick interpolates as numpy's _lerp does, in f32 with one rounding per operation.
//                      Integer sums do not depend on their order: two calls give the same bits.
//   vs_flow_clip_mean  per frame the mean over (h, w, 2) of clip(|flow|, lo[c], hi[c]); vs_motion_energy per frame
//                      pair the mean of |x[f+1] - x[f]| (bytes: v_sad_u8 on dwords, an exact integer sum).  f64 sums in
//                      an order fixed by H W (thread-strided, wave butterfly, waves in order), rounded once to f32.
#include <cmath>

#include "common.h"

namespace vs {

constexpr int kFfThreads = 1024;
constexpr int kFfStageMax = 20000;       // pixels: (528 + 2 * 20000) * 4 = 162,112 B of LDS
constexpr int kFfHdr = 528;              // LDS words before the keys: hist[2][256], state[16]
constexpr int64_t kFfMaxHW = 1 << 20;
constexpr int kFqThreads = 256;
constexpr int kFqChunk = 32768;          // pixels per workgroup of the quantile count pass
constexpr int kFmThreads = 256;          // the two mean kernels

__device__ __forceinline__ uint32_t ff_key(float x, int absolute) {
  uint32_t u = __float_as_uint(x);
  if (absolute) u &= 0x7fffffffu;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ff_unkey(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// One histogram's pick by one wave: lane l owns bins 4 l .. 4 l + 3.  Returns true in the single lane whose bins hold
// rank k; there `bin` is the bin, `rest` the rank inside it and `count` the bin's count.
__device__ __forceinline__ bool ff_pick(const uint32_t* hist, uint32_t k, int lane, uint32_t& bin, uint32_t& rest,
                                        uint32_t& count) {
  const uint32_t c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2], c3 = hist[4 * lane + 3];
  const uint32_t s = c0 + c1 + c2 + c3;
  uint32_t incl = s;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  const uint32_t excl = incl - s;
  if (!(k >= excl && k < incl)) return false;
  uint32_t r = k - excl;
  if (r < c0) {
    bin = 4 * lane, count = c0;
  } else if ((r -= c0) < c1) {
    bin = 4 * lane + 1, count = c1;
  } else if ((r -= c1) < c2) {
    bin = 4 * lane + 2, count = c2;
  } else {
    r -= c2;
    bin = 4 * lane + 3, count = c3;
  }
  rest = r;
  return true;
}

// A thread's run of equal digits, merged before the LDS atomic.
struct FfRun {
  int cur;
  uint32_t n;
  __device__ __forceinline__ void add(uint32_t* hist, int digit) {
    if (digit == cur) {
      ++n;
    } else {
      if (n) atomicAdd(&hist[cur], n);
      cur = digit, n = 1;
    }
  }
  __device__ __forceinline__ void flush(uint32_t* hist) {
    if (n) atomicAdd(&hist[cur], n);
    n = 0;
  }
};

// grid (frames), 1024 threads, dynamic LDS (kFfHdr + (STAGED ? 2 hw : 0)) words
template <bool STAGED>
__global__ __launch_bounds__(kFfThreads) void flow_median2_kernel(const float* __restrict__ flow, int hw, int absolute,
                                                                  float* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) uint32_t ff_lds[];
  uint32_t* hist = ff_lds;          // [2][256]
  uint32_t* st = ff_lds + 512;      // [c * 4 + {0: prefix, 1: rank left, 2: next element has the same key}], 8 + c: NaN seen,
                                    // 10 + c: smallest key above the median's
  uint32_t* keys = ff_lds + kFfHdr; // [2][hw]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const f32x2* src = (const f32x2*)flow + (size_t)blockIdx.x * hw;

  if (tid < 512) hist[tid] = 0;
  if (tid < 16) st[tid] = 0;
  if (tid < 2) st[tid * 4 + 1] = (uint32_t)(hw - 1) / 2;
  if (tid < 2) st[10 + tid] = 0xffffffffu;
  __syncthreads();

  bool nan0 = false, nan1 = false;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const uint32_t mask = pass ? 0xffffffffu << (shift + 8) : 0u;
    const uint32_t p0 = st[0], p1 = st[4];
    FfRun r0 = {0, 0}, r1 = {0, 0};
    for (int i = tid; i < hw; i += kFfThreads) {
      uint32_t k0, k1;
      if (STAGED && pass) {
        k0 = keys[i], k1 = keys[hw + i];
      } else {
        const f32x2 v = src[i];
        nan0 |= v.x != v.x, nan1 |= v.y != v.y;
        k0 = ff_key(v.x, absolute), k1 = ff_key(v.y, absolute);
        if (STAGED) keys[i] = k0, keys[hw + i] = k1;
      }
      if ((k0 & mask) == p0) r0.add(hist, (k0 >> shift) & 255);
      if ((k1 & mask) == p1) r1.add(hist + 256, (k1 >> shift) & 255);
    }
    r0.flush(hist);
    r1.flush(hist + 256);
    __syncthreads();
    if (wave < 2) {
      uint32_t bin, rest, count;
      if (ff_pick(hist + 256 * wave, st[wave * 4 + 1], lane, bin, rest, count)) {
        st[wave * 4 + 0] |= bin << shift;
        st[wave * 4 + 1] = rest;
        st[wave * 4 + 2] = rest + 1 < count;
      }
    }
    __syncthreads();
    if (tid < 512) hist[tid] = 0;
    __syncthreads();
  }
  if (nan0) st[8] = 1;  // every writer stores the same value
  if (nan1) st[9] = 1;

  const bool even = (hw & 1) == 0;
  if (even && !(st[2] && st[6])) {  // some component's upper middle element is a larger key: the smallest one
    const uint32_t a0 = st[0], a1 = st[4];
    uint32_t m0 = 0xffffffffu, m1 = 0xffffffffu;
    for (int i = tid; i < hw; i += kFfThreads) {
      uint32_t k0, k1;
      if (STAGED) {
        k0 = keys[i], k1 = keys[hw + i];
      } else {
        const f32x2 v = src[i];
        k0 = ff_key(v.x, absolute), k1 = ff_key(v.y, absolute);
      }
      if (k0 > a0 && k0 < m0) m0 = k0;
      if (k1 > a1 && k1 < m1) m1 = k1;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t t0 = __shfl_xor(m0, o, 64), t1 = __shfl_xor(m1, o, 64);
      m0 = t0 < m0 ? t0 : m0, m1 = t1 < m1 ? t1 : m1;
    }
    if (lane == 0) atomicMin(&st[10], m0), atomicMin(&st[11], m1);
  }
  __syncthreads();
  if (tid < 2) {
    const float a = ff_unkey(st[tid * 4]);
    float r = a;
    if (even) {
      const float b = st[tid * 4 + 2] ? a : ff_unkey(st[10 + tid]);
      r = __fmul_rn(__fadd_rn(a, b), 0.5f);
    }
    if (st[8 + tid]) r = __builtin_nanf("");
    out[(size_t)blockIdx.x * 2 + tid] = r;
  }
}

// ---- per-trial quantiles ---------------------------------------------------------------------------------------
struct FqState {          // one per (trial, component), 64 bytes
  uint32_t prefix[4];
  uint32_t k[4];          // rank left inside the prefix
  int32_t alias[4];       // the first rank with the same prefix: its histogram is the one counted
  uint32_t nan;
  uint32_t pad[3];
};
struct FqRanks {
  uint32_t k[4];          // ranks of: q_lo's previous and next element, q_hi's previous and next
  float gamma[2];
};

// grid (2 K), 256 threads
__global__ __launch_bounds__(kFqThreads) void flow_quant_init_kernel(FqState* __restrict__ state,
                                                                     uint32_t* __restrict__ ghist, FqRanks ranks) {
  const int tid = threadIdx.x;
  uint32_t* h = ghist + (size_t)blockIdx.x * 1024;
  for (int b = tid; b < 1024; b += kFqThreads) h[b] = 0;
  FqState* s = state + blockIdx.x;
  if (tid < 4) s->prefix[tid] = 0, s->k[tid] = ranks.k[tid], s->alias[tid] = 0;
  if (tid == 0) s->nan = 0;
}

// grid (blocks per trial, K), 256 threads: counts a chunk of kFqChunk pixels of one trial
__global__ __launch_bounds__(kFqThreads) void flow_quant_count_kernel(const float* __restrict__ flow, int64_t n,
                                                                      FqState* __restrict__ state,
                                                                      uint32_t* __restrict__ ghist, int pass) {
  __shared__ uint32_t hist[2 * 4 * 256];
  const int tid = threadIdx.x;
  const int64_t trial = blockIdx.y;
  for (int b = tid; b < 2048; b += kFqThreads) hist[b] = 0;
  const FqState s0 = state[trial * 2], s1 = state[trial * 2 + 1];
  __syncthreads();
  const int shift = 24 - 8 * pass;
  const uint32_t mask = pass ? 0xffffffffu << (shift + 8) : 0u;
  const f32x2* src = (const f32x2*)flow + trial * n;
  const int64_t i0 = (int64_t)blockIdx.x * kFqChunk;
  const int64_t i1 = i0 + kFqChunk < n ? i0 + kFqChunk : n;
  FfRun run[2][4];
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int j = 0; j < 4; ++j) run[c][j].cur = 0, run[c][j].n = 0;
  bool nan0 = false, nan1 = false;
  for (int64_t i = i0 + tid; i < i1; i += kFqThreads) {
    const f32x2 v = src[i];
    nan0 |= v.x != v.x, nan1 |= v.y != v.y;
    const uint32_t k0 = ff_key(v.x, 1), k1 = ff_key(v.y, 1);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (s0.alias[j] == j && (k0 & mask) == s0.prefix[j]) run[0][j].add(hist + j * 256, (k0 >> shift) & 255);
      if (s1.alias[j] == j && (k1 & mask) == s1.prefix[j]) run[1][j].add(hist + 1024 + j * 256, (k1 >> shift) & 255);
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) run[0][j].flush(hist + j * 256), run[1][j].flush(hist + 1024 + j * 256);
  if (pass == 0) {
    if (nan0) atomicOr(&state[trial * 2].nan, 1u);
    if (nan1) atomicOr(&state[trial * 2 + 1].nan, 1u);
  }
  __syncthreads();
  uint32_t* g = ghist + trial * 2048;
  for (int b = tid; b < 2048; b += kFqThreads) {
    const uint32_t v = hist[b];
    if (v) atomicAdd(&g[b], v);
  }
}

// numpy's _lerp(a, b, t) on f32 operands: one rounding per operation.  Contraction is switched off for the function:
// the _rn intrinsics are plain operators to the compiler, which would fuse the product into the sum.
__device__ __forceinline__ float fq_lerp(float a, float b, float t) {
#pragma clang fp contract(off)
  const float d = b - a;
  const float up = d * t;
  float r = a + up;
  if (t >= 0.5f) {
    const float down = d * (1.0f - t);
    r = b - down;
  }
  return r;
}

// grid (2 K), 256 threads: wave j picks rank j's bin; the last pass writes the bounds
__global__ __launch_bounds__(kFqThreads) void flow_quant_pick_kernel(FqState* __restrict__ state,
                                                                     uint32_t* __restrict__ ghist, int pass,
                                                                     FqRanks ranks, float* __restrict__ bounds,
                                                                     float* __restrict__ stats) {
  __shared__ uint32_t np[4], nk[4];
  const int tid = threadIdx.x, lane = tid & 63, j = tid >> 6;
  FqState* s = state + blockIdx.x;
  uint32_t* h = ghist + (size_t)blockIdx.x * 1024;
  const int shift = 24 - 8 * pass;
  const uint32_t prefix = s->prefix[j], k = s->k[j];
  const int alias = s->alias[j];
  if (lane == 0) np[j] = prefix, nk[j] = k;
  uint32_t bin, rest, count;
  const bool mine = ff_pick(h + 256 * alias, k, lane, bin, rest, count);
  __syncthreads();
  if (mine) np[j] = prefix | (bin << shift), nk[j] = rest;
  __syncthreads();
  for (int b = tid; b < 1024; b += kFqThreads) h[b] = 0;
  if (tid == 0) {
    for (int i = 0; i < 4; ++i) {
      int a = i;
      for (int e = i - 1; e >= 0; --e)
        if (np[e] == np[i]) a = e;
      s->prefix[i] = np[i], s->k[i] = nk[i], s->alias[i] = a;
    }
    if (pass == 3) {
      const float v0 = ff_unkey(np[0]), v1 = ff_unkey(np[1]), v2 = ff_unkey(np[2]), v3 = ff_unkey(np[3]);
      float lo = fq_lerp(v0, v1, ranks.gamma[0]), hi = fq_lerp(v2, v3, ranks.gamma[1]);
      if (s->nan) lo = hi = __builtin_nanf("");
      bounds[(size_t)blockIdx.x * 2] = lo, bounds[(size_t)blockIdx.x * 2 + 1] = hi;
      if (stats) {
        float* q = stats + (size_t)blockIdx.x * 4;
        q[0] = v0, q[1] = v1, q[2] = v2, q[3] = v3;
      }
    }
  }
}

// The ranks and weight of np.percentile(x, q, method="linear") for a float32 x of n values and a Python scalar q,
// as numpy 2 computes them: the quantile q / 100 and the virtual index (n - 1) q are FLOAT32 (the divisor takes the
// array's dtype), so is floor's result and "previous + 1".  The volatile floats keep every step a float32 value of
// its own on the host: no wider intermediate, no fused product.
static void fq_rank(int64_t n, float percent, uint32_t* prev, uint32_t* next, float* gamma) {
  const volatile float q = percent / 100.0f;
  const volatile float last = (float)(n - 1);
  const volatile float v = last * q;
  int64_t p, x;
  if (v >= last) {
    p = x = n - 1;                       // numpy's index -1
    *gamma = (float)((double)v + 1.0);
  } else {
    const volatile float fl = floorf(v);
    const volatile float nx = fl + 1.0f;
    p = (int64_t)fl, x = (int64_t)nx;
    *gamma = (float)((double)v - (double)p);
  }
  if (p < 0) p = 0;
  if (x < 0) x = 0;
  if (p > n - 1) p = n - 1;
  if (x > n - 1) x = n - 1;
  *prev = (uint32_t)p, *next = (uint32_t)x;
}

// ---- per-frame means -------------------------------------------------------------------------------------------
__device__ __forceinline__ double fm_block_sum(double v, double* part) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) part[wave] = v;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < kFmThreads / 64; ++w) t += part[w];
  return t;
}

// grid (K (F-1)), 256 threads
__global__ __launch_bounds__(kFmThreads) void flow_clip_mean_kernel(const float* __restrict__ flow, int hw, int fp,
                                                                    const float* __restrict__ bounds,
                                                                    float* __restrict__ out) {
  __shared__ double part[kFmThreads / 64];
  const f32x2* src = (const f32x2*)flow + (size_t)blockIdx.x * hw;
  const float* bd = bounds + (size_t)(blockIdx.x / fp) * 4;
  const float lo0 = bd[0], hi0 = bd[1], lo1 = bd[2], hi1 = bd[3];
  const bool bad0 = lo0 != lo0 || hi0 != hi0, bad1 = lo1 != lo1 || hi1 != hi1;
  double acc = 0.0;
  for (int i = threadIdx.x; i < hw; i += kFmThreads) {
    const f32x2 v = src[i];
    float x = fabsf(v.x), y = fabsf(v.y);   // np.clip = minimum(maximum(x, lo), hi), NaN from either side
    x = x < lo0 ? lo0 : x, x = x > hi0 ? hi0 : x;
    y = y < lo1 ? lo1 : y, y = y > hi1 ? hi1 : y;
    if (bad0) x = __builtin_nanf("");
    if (bad1) y = __builtin_nanf("");
    acc += (double)x;
    acc += (double)y;
  }
  const double t = fm_block_sum(acc, part);
  if (threadIdx.x == 0) out[blockIdx.x] = (float)(t / (2.0 * (double)hw));
}

// grid (K (F-1)), 256 threads
template <typename TI>
__global__ __launch_bounds__(kFmThreads) void motion_energy_kernel(const TI* __restrict__ video, int hw, int frames,
                                                                   int words, float* __restrict__ out) {
  __shared__ double part[kFmThreads / 64];
  const int64_t k = blockIdx.x / (frames - 1), f = blockIdx.x % (frames - 1);
  const TI* a = video + (k * frames + f) * (int64_t)hw;
  const TI* b = a + hw;
  double acc = 0.0;
  if constexpr (sizeof(TI) == 1) {
    uint32_t sum = 0;  // at most 255 * 2^20 / 256 * 4 per thread
    if (words) {       // hw % 4 == 0 and a 4-byte aligned video: dwords, four differences per v_sad_u8
      const uint32_t* aw = (const uint32_t*)a;
      const uint32_t* bw = (const uint32_t*)b;
      for (int i = threadIdx.x; i < words; i += kFmThreads) sum = __builtin_amdgcn_sad_u8(bw[i], aw[i], sum);
    } else {
      for (int i = threadIdx.x; i < hw; i += kFmThreads) {
        const int d = (int)b[i] - (int)a[i];
        sum += (uint32_t)(d < 0 ? -d : d);
      }
    }
    acc = (double)sum;
  } else {
    for (int i = threadIdx.x; i < hw; i += kFmThreads) acc += (double)fabsf(__fsub_rn(b[i], a[i]));
  }
  const double t = fm_block_sum(acc, part);
  if (threadIdx.x == 0) out[blockIdx.x] = (float)(t / (double)hw);
}

static size_t fq_state_bytes(int64_t K) { return (size_t)cdiv(2 * K * (int64_t)sizeof(FqState), 256) * 256; }

}  // namespace vs

using namespace vs;

extern "C" int vs_flow_plan(int32_t* out) {
  VS_REQUIRE(out, "vs_flow_plan: null pointer");
  out[0] = kFfStageMax, out[1] = kFqChunk, out[2] = kFfThreads;
  return VS_OK;
}

extern "C" int vs_flow_median2(int64_t frames, int64_t HW, const float* flow, int32_t absolute, float* out,
                               void* stream) {
  VS_REQUIRE(HW >= 1 && HW <= kFfMaxHW, "vs_flow_median2: 1 <= H W <= 2^20");
  VS_REQUIRE(frames >= 0 && frames <= 0x7fffffff, "vs_flow_median2: 0 <= frames < 2^31");
  VS_REQUIRE(absolute == 0 || absolute == 1, "vs_flow_median2: absolute is 0 (signed) or 1 (|x|)");
  if (frames == 0) return VS_OK;
  VS_REQUIRE(flow && out, "vs_flow_median2: null pointer");
  VS_REQUIRE((((uintptr_t)flow) & 7u) == 0 && (((uintptr_t)out) & 3u) == 0,
             "vs_flow_median2: flow must be 8-byte aligned, out 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  ScopedTimer timer(VS_TIMER_MISC, s, (double)frames * (double)HW * 8.0);
  const bool staged = HW <= kFfStageMax;
  const size_t lds = (size_t)(kFfHdr + (staged ? 2 * HW : 0)) * sizeof(uint32_t);
  auto kern = staged ? flow_median2_kernel<true> : flow_median2_kernel<false>;
  if (lds > (size_t)(64 << 10)) {
    static thread_local size_t allowed = 0;  // the opt-in for more than 64 KiB of dynamic LDS, raised when needed
    if (lds > allowed) {
      hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
      if (e != hipSuccess) return (int)e;
      allowed = lds;
    }
  }
  hipLaunchKernelGGL(kern, dim3((unsigned)frames), dim3(kFfThreads), lds, s, flow, (int)HW, (int)absolute, out);
  VS_LAUNCH_CHECK();
  return VS_OK;
}

extern "C" size_t vs_flow_quantiles_workspace_bytes(int64_t K) {
  if (K < 1 || K > 65535) return 0;
  return fq_state_bytes(K) + (size_t)K * 2 * 1024 * sizeof(uint32_t);
}

extern "C" int vs_flow_quantiles(int64_t K, int64_t Fp, int64_t HW, const float* flow, float q_lo, float q_hi,
                                 float* bounds, float* stats, void* workspace, void* stream) {
  VS_REQUIRE(HW >= 1 && HW <= kFfMaxHW, "vs_flow_quantiles: 1 <= H W <= 2^20");
  VS_REQUIRE(K >= 0 && K <= 65535, "vs_flow_quantiles: 0 <= K <= 65535 trials");
  VS_REQUIRE(Fp >= 1 && Fp * HW <= 0x7fffffff, "vs_flow_quantiles: 1 <= (F - 1) H W < 2^31 values per trial");
  VS_REQUIRE(q_lo >= 0.f && q_lo <= 100.f && q_hi >= 0.f && q_hi <= 100.f,
             "vs_flow_quantiles: percentiles in [0, 100]");
  if (K == 0) return VS_OK;
  VS_REQUIRE(flow && bounds && workspace, "vs_flow_quantiles: null pointer");
  VS_REQUIRE((((uintptr_t)flow) & 7u) == 0 && (((uintptr_t)workspace) & 15u) == 0 && (((uintptr_t)bounds) & 3u) == 0 &&
                 (((uintptr_t)stats) & 3u) == 0,
             "vs_flow_quantiles: flow must be 8-byte aligned, the workspace 16-byte, bounds and stats 4-byte");
  const int64_t n = Fp * HW;
  FqRanks ranks;
  fq_rank(n, q_lo, &ranks.k[0], &ranks.k[1], &ranks.gamma[0]);
  fq_rank(n, q_hi, &ranks.k[2], &ranks.k[3], &ranks.gamma[1]);
  FqState* state = (FqState*)workspace;
  uint32_t* ghist = (uint32_t*)((char*)workspace + fq_state_bytes(K));
  hipStream_t s = (hipStream_t)stream;
  ScopedTimer timer(VS_TIMER_MISC, s, 4.0 * (double)K * (double)n * 8.0);
  hipLaunchKernelGGL(flow_quant_init_kernel, dim3((unsigned)(2 * K)), dim3(kFqThreads), 0, s, state, ghist, ranks);
  VS_LAUNCH_CHECK();
  const unsigned nblk = (unsigned)cdiv(n, kFqChunk);
  for (int pass = 0; pass < 4; ++pass) {
    hipLaunchKernelGGL(flow_quant_count_kernel, dim3(nblk, (unsigned)K), dim3(kFqThreads), 0, s, flow, n, state, ghist,
                       pass);
    VS_LAUNCH_CHECK();
    hipLaunchKernelGGL(flow_quant_pick_kernel, dim3((unsigned)(2 * K)), dim3(kFqThreads), 0, s, state, ghist, pass,
                       ranks, bounds, stats);
    VS_LAUNCH_CHECK();
  }
  return VS_OK;
}

extern "C" int vs_flow_clip_mean(int64_t K, int64_t Fp, int64_t HW, const float* flow, const float* bounds, float* out,
                                 void* stream) {
  VS_REQUIRE(HW >= 1 && HW <= kFfMaxHW, "vs_flow_clip_mean: 1 <= H W <= 2^20");
  VS_REQUIRE(K >= 0 && Fp >= 1 && K * Fp <= 0x7fffffff, "vs_flow_clip_mean: K >= 0 trials of F - 1 >= 1 frames, fewer than 2^31");
  if (K == 0) return VS_OK;
  VS_REQUIRE(flow && bounds && out, "vs_flow_clip_mean: null pointer");
  VS_REQUIRE((((uintptr_t)flow) & 7u) == 0 && (((uintptr_t)bounds) & 3u) == 0 && (((uintptr_t)out) & 3u) == 0,
             "vs_flow_clip_mean: flow must be 8-byte aligned, bounds and out 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  ScopedTimer timer(VS_TIMER_MISC, s, (double)K * (double)Fp * (double)HW * 8.0);
  hipLaunchKernelGGL(flow_clip_mean_kernel, dim3((unsigned)(K * Fp)), dim3(kFmThreads), 0, s, flow, (int)HW, (int)Fp,
                     bounds, out);
  VS_LAUNCH_CHECK();
  return VS_OK;
}

extern "C" int vs_motion_energy(int32_t in_dtype, int64_t K, int64_t F, int64_t HW, const void* video, float* out,
                                void* stream) {
  VS_REQUIRE(in_dtype == VS_F32 || in_dtype == VS_U8, "vs_motion_energy: in_dtype must be VS_F32 or VS_U8");
  VS_REQUIRE(HW >= 1 && HW <= kFfMaxHW, "vs_motion_energy: 1 <= H W <= 2^20");
  VS_REQUIRE(K >= 0 && F >= 2 && K * (F - 1) <= 0x7fffffff, "vs_motion_energy: K >= 0 trials of F >= 2 frames, fewer than 2^31 pairs");
  if (K == 0) return VS_OK;
  VS_REQUIRE(video && out, "vs_motion_energy: null pointer");
  VS_REQUIRE((((uintptr_t)out) & 3u) == 0 && (in_dtype == VS_U8 || (((uintptr_t)video) & 3u) == 0),
             "vs_motion_energy: f32 tensors must be 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  ScopedTimer timer(VS_TIMER_MISC, s, (double)K * (double)F * (double)HW * (in_dtype == VS_U8 ? 1.0 : 4.0));
  const dim3 grid((unsigned)(K * (F - 1)));
  if (in_dtype == VS_U8) {
    const int words = (HW % 4 == 0 && (((uintptr_t)video) & 3u) == 0) ? (int)(HW / 4) : 0;
    hipLaunchKernelGGL(motion_energy_kernel<uint8_t>, grid, dim3(kFmThreads), 0, s, (const uint8_t*)video, (int)HW,
                       (int)F, words, out);
  } else {
    hipLaunchKernelGGL(motion_energy_kernel<float>, grid, dim3(kFmThreads), 0, s, (const float*)video, (int)HW, (int)F,
                       0, out);
  }
  VS_LAUNCH_CHECK();
  return VS_OK;
}
