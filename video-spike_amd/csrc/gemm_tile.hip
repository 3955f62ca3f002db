// gemm_tile.hip — the generic tiles of vs_gemm (gemm.hip has the overview): the register-staged bf16
// kernel, the exact-f32 kernel, the split-K reduce kernels and the tile / split plan every generic
// path (panel, whole-K, ring, these tiles) shares.  The fallback of the dispatch: they take any shape,
// layout and epilogue vs_gemm accepts.
#include "common.h"
#include "gemm_common.h"
#include "gemm_paths.h"
#include "gemm_tiles.h"

namespace vs {

// ----------------------------------------------------------------------------------------------
// bf16 kernel
// ----------------------------------------------------------------------------------------------
template <int BM, int BN, bool AKC, bool BKC, uint32_t EF>
__global__ __launch_bounds__(256, 2) void gemm_bf16_kernel(const bf16_t* __restrict__ A, int64_t lda,
                                                           const bf16_t* __restrict__ B, int64_t ldb, int64_t K,
                                                           GridMap g, EpiParams e) {
  using OA = OperandBf16<BM, AKC>;
  using OB = OperandBf16<BN, BKC>;
  constexpr int WM = BM / 2, WN = BN / 2, TM = WM / 16, TN = WN / 16;
  constexpr int STAGE = OA::BYTES + OB::BYTES;
  constexpr int SMEM = CMax<2 * STAGE, BM*(BN + 4) * 4>::v;
  __shared__ __attribute__((aligned(16))) char smem[SMEM];

  int nt, mt, split;
  map_block(g, nt, mt, split);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;
  const int64_t m0 = (int64_t)mt * BM, n0 = (int64_t)nt * BN;
  const int64_t k_begin = (int64_t)split * g.k_per_split;
  const int64_t k_end = k_begin + g.k_per_split < K ? k_begin + g.k_per_split : K;
  const int nk = (int)((k_end - k_begin + 63) / 64);

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // fused bias gradient: only the first column tile's wc == 0 waves (wave-uniform condition)
  const bool rowsum_on = e.a_rowsum != nullptr && nt == 0 && wc == 0;
  float rs[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) rs[i] = 0.f;

  uint4 ra[OA::CHUNKS], rb[OB::CHUNKS];
  if (nk > 0) {
    OA::load(ra, A, lda, m0, e.M, k_begin, k_end, tid);
    OB::load(rb, B, ldb, n0, e.N, k_begin, k_end, tid);
    OA::store(smem, ra, tid);
    OB::store(smem + OA::BYTES, rb, tid);
  }
  __syncthreads();

  for (int t = 0; t < nk; ++t) {
    const char* sa = smem + (t & 1) * STAGE;
    const char* sb = sa + OA::BYTES;
    const bool more = t + 1 < nk;
    if (more) {
      const int64_t kn = k_begin + (int64_t)(t + 1) * 64;
      OA::load(ra, A, lda, m0, e.M, kn, k_end, tid);
      OB::load(rb, B, ldb, n0, e.N, kn, k_end, tid);
    }
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 af[TM], bfr[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) af[i] = OA::frag(sa, wr * WM + i * 16, kk, lane);
#pragma unroll
      for (int j = 0; j < TN; ++j) bfr[j] = OB::frag(sb, wc * WN + j * 16, kk, lane);
      if (rowsum_on) {
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
          for (int q = 0; q < 8; ++q) rs[i] += (float)af[i][q];
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
    if (more) {
      char* dst = smem + ((t + 1) & 1) * STAGE;
      OA::store(dst, ra, tid);
      OB::store(dst + OA::BYTES, rb, tid);
    }
    __syncthreads();
  }
  if (rowsum_on) flush_rowsum<TM>(e.a_rowsum, rs, m0 + wr * WM, e.M, lane);
  store_tile<BM, BN, TM, TN, EF>(e, (float*)smem, acc, m0, n0, split);
}

// ----------------------------------------------------------------------------------------------
// f32 kernel (exact: v_mfma_f32_16x16x4_f32 is a k-ordered fmaf chain)
// ----------------------------------------------------------------------------------------------
template <bool KC>
struct OperandF32 {
  static constexpr int R = 64, BK = 32, LD = 80;  // LD % 32 == 16 -> conflict-free ds_read_b32
  static constexpr int BYTES = BK * LD * 4;
  __device__ __forceinline__ static void load(float4 (&reg)[2], const float* __restrict__ p, int64_t ld, int64_t r0,
                                              int64_t rows, int64_t k0, int64_t k_end, int tid) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int i = tid + 256 * s;
      int64_t gr, gk;
      if constexpr (KC) {
        gr = r0 + (i >> 3);
        gk = k0 + (i & 7) * 4;
      } else {
        gk = k0 + (i >> 4);
        gr = r0 + (i & 15) * 4;
      }
      const bool ok = gr < rows && gk < k_end;
      const float* src = KC ? p + gr * ld + gk : p + gk * ld + gr;
      reg[s] = ok ? *(const float4*)src : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  __device__ __forceinline__ static void store(float* lds, const float4 (&reg)[2], int tid) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int i = tid + 256 * s;
      if constexpr (KC) {
        const int r = i >> 3, k = (i & 7) * 4;
        lds[(k + 0) * LD + r] = reg[s].x;
        lds[(k + 1) * LD + r] = reg[s].y;
        lds[(k + 2) * LD + r] = reg[s].z;
        lds[(k + 3) * LD + r] = reg[s].w;
      } else {
        const int k = i >> 4, r = (i & 15) * 4;
        *(float4*)(lds + k * LD + r) = reg[s];
      }
    }
  }
};

template <bool AKC, bool BKC>
__global__ __launch_bounds__(256, 2) void gemm_f32_kernel(const float* __restrict__ A, int64_t lda,
                                                          const float* __restrict__ B, int64_t ldb, int64_t K,
                                                          GridMap g, EpiParams e) {
  using OA = OperandF32<AKC>;
  using OB = OperandF32<BKC>;
  constexpr int LD = OA::LD;
  constexpr int STAGE = (OA::BYTES + OB::BYTES) / 4;  // floats
  constexpr int SMEM = CMax<2 * STAGE, 64 * 68>::v;
  __shared__ __attribute__((aligned(16))) float smem[SMEM];

  int nt, mt, split;
  map_block(g, nt, mt, split);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;
  const int64_t m0 = (int64_t)mt * 64, n0 = (int64_t)nt * 64;
  const int64_t k_begin = (int64_t)split * g.k_per_split;
  const int64_t k_end = k_begin + g.k_per_split < K ? k_begin + g.k_per_split : K;
  const int nk = (int)((k_end - k_begin + 31) / 32);

  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const bool rowsum_on = e.a_rowsum != nullptr && nt == 0 && wc == 0;
  float rs[2] = {0.f, 0.f};

  float4 ra[2], rb[2];
  if (nk > 0) {
    OA::load(ra, A, lda, m0, e.M, k_begin, k_end, tid);
    OB::load(rb, B, ldb, n0, e.N, k_begin, k_end, tid);
    OA::store(smem, ra, tid);
    OB::store(smem + OA::BYTES / 4, rb, tid);
  }
  __syncthreads();
  for (int t = 0; t < nk; ++t) {
    const float* sa = smem + (t & 1) * STAGE;
    const float* sb = sa + OA::BYTES / 4;
    const bool more = t + 1 < nk;
    if (more) {
      const int64_t kn = k_begin + (int64_t)(t + 1) * 32;
      OA::load(ra, A, lda, m0, e.M, kn, k_end, tid);
      OB::load(rb, B, ldb, n0, e.N, kn, k_end, tid);
    }
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int k = 4 * s + (lane >> 4);
      float af[2], bfr[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) af[i] = sa[k * LD + wr * 32 + i * 16 + (lane & 15)];
#pragma unroll
      for (int j = 0; j < 2; ++j) bfr[j] = sb[k * LD + wc * 32 + j * 16 + (lane & 15)];
      if (rowsum_on) {
        rs[0] += af[0];
        rs[1] += af[1];
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
    if (more) {
      float* dst = smem + ((t + 1) & 1) * STAGE;
      OA::store(dst, ra, tid);
      OB::store(dst + OA::BYTES / 4, rb, tid);
    }
    __syncthreads();
  }
  if (rowsum_on) flush_rowsum<2>(e.a_rowsum, rs, m0 + wr * 32, e.M, lane);
  store_tile<64, 64, 2, 2, kEpiRuntime>(e, smem, acc, m0, n0, split);
}

// ----------------------------------------------------------------------------------------------
// host: launches, the split-K reduce, the plan
// ----------------------------------------------------------------------------------------------
template <int BM, int BN>
static void launch_bf16(const vs_gemm_desc* d, unsigned nblk, const GridMap& g, const EpiParams& e, hipStream_t s) {
  const bf16_t* a = (const bf16_t*)d->a;
  const bf16_t* b = (const bf16_t*)d->b;
  with_epilogue(e.flags, [&](auto ef) {
    with_layout(d->a_kcontig, d->b_kcontig, [&](auto akc, auto bkc) {
      hipLaunchKernelGGL((gemm_bf16_kernel<BM, BN, decltype(akc)::value, decltype(bkc)::value, decltype(ef)::value>),
                         dim3(nblk), dim3(256), 0, s, a, d->lda, b, d->ldb, d->K, g, e);
    });
  });
}

void launch_tile(const vs_gemm_desc* d, const EpiParams& e, const GemmPlan& p, hipStream_t s) {
  const GridMap& g = p.g;
  const unsigned nblk = (unsigned)((int64_t)g.tiles_n * g.tiles_m * g.splits);
  if (p.BM == 128 && p.BN == 128) launch_bf16<128, 128>(d, nblk, g, e, s);
  else if (p.BM == 128) launch_bf16<128, 64>(d, nblk, g, e, s);
  else if (p.BN == 128) launch_bf16<64, 128>(d, nblk, g, e, s);
  else launch_bf16<64, 64>(d, nblk, g, e, s);
}

void launch_f32(const vs_gemm_desc* d, const EpiParams& e, const GemmPlan& p, hipStream_t s) {
  const GridMap& g = p.g;
  const float* a = (const float*)d->a;
  const float* b = (const float*)d->b;
  const dim3 grid((unsigned)((int64_t)g.tiles_n * g.tiles_m * g.splits));
  with_layout(d->a_kcontig, d->b_kcontig, [&](auto akc, auto bkc) {
    hipLaunchKernelGGL((gemm_f32_kernel<decltype(akc)::value, decltype(bkc)::value>), grid, dim3(256), 0, s, a, d->lda, b,
                       d->ldb, d->K, g, e);
  });
}

// Split-K for the token reductions (dW): aim at ~2 blocks per CU, at least 8 k-tiles per split
// (the f32 atomics of every split's tile cost ~1.3 TB/s chip-wide: fewer, longer splits).
static int pick_splits(int64_t tiles, int64_t nk, int want, bool atomic_ok) {
  if (!atomic_ok) return 1;
  if (want > 0) return (int)(want < nk ? want : nk);
  if (tiles >= 384 || nk < 16) return 1;
  int64_t s = (512 + tiles - 1) / tiles;
  const int64_t max_s = nk / 8;
  if (s > max_s) s = max_s;
  return s < 1 ? 1 : (int)s;
}

// C[m, n] += bias[n] + sum_s part[s][m][n].  Vector path: a workgroup owns 64 float4 of C and
// its 4 waves split the splits (wave w sums s = w, w+4, ...: every load of a wave's share is
// issued before the first add), then the 4 partial float4 are added in wave order through LDS
// (deterministic: the order depends only on `splits`).  The dW partials are 7-13 MB spread over
// ~150 workgroups at one float4 per thread: that version was latency-bound at ~20 us per launch.
__global__ __launch_bounds__(256) void gemm_splitk_reduce(const float* __restrict__ part, int splits, int64_t M,
                                                          int64_t N, float* __restrict__ c, int64_t ldc,
                                                          const float* __restrict__ bias, int vec) {
  const int64_t MN = M * N;
  if (vec) {
    __shared__ float4 red[4][64];
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int64_t e4 = ((int64_t)blockIdx.x * 64 + l) * 4;
    const bool live = e4 < MN;
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) {
      for (int sp0 = w; sp0 < splits; sp0 += 4 * 16) {
        float4 v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          const int sp = sp0 + 4 * u;
          v[u] = sp < splits ? *(const float4*)(part + sp * MN + e4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          acc.x += v[u].x; acc.y += v[u].y; acc.z += v[u].z; acc.w += v[u].w;
        }
      }
    }
    red[w][l] = acc;
    __syncthreads();
    if (w == 0 && live) {
      float4 a = red[0][l];
#pragma unroll
      for (int k = 1; k < 4; ++k) {
        const float4 b = red[k][l];
        a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
      }
      const int64_t m = e4 / N, n = e4 % N;
      if (bias) {
        const float4 bb = *(const float4*)(bias + n);
        a.x += bb.x; a.y += bb.y; a.z += bb.z; a.w += bb.w;
      }
      float4* dst = (float4*)(c + m * ldc + n);
      float4 o = *dst;
      o.x += a.x; o.y += a.y; o.z += a.z; o.w += a.w;
      *dst = o;
    }
  } else {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= MN) return;
    const int64_t m = i / N, n = i % N;
    float acc = 0.f;
    for (int sp0 = 0; sp0 < splits; sp0 += 32) {
      float v[32];
#pragma unroll
      for (int u = 0; u < 32; ++u) v[u] = sp0 + u < splits ? part[(sp0 + u) * MN + i] : 0.f;
#pragma unroll
      for (int u = 0; u < 32; ++u) acc += v[u];
    }
    if (bias) acc += bias[n];
    c[m * ldc + n] += acc;
  }
}

// Few outputs, many splits (the head's z = x W_enc^T: 16 x 64 outputs, 512 splits of K): the
// per-output kernel above runs as ONE workgroup whose threads each walk 512 splits (24 us).  Here a
// workgroup owns one float4 of C, its 256 threads stride over the splits, and a fixed-shape LDS tree
// adds the 256 partial sums (deterministic: the order depends only on `splits`).
__global__ __launch_bounds__(256) void gemm_splitk_reduce_wide(const float* __restrict__ part, int splits, int64_t M,
                                                               int64_t N, float* __restrict__ c, int64_t ldc,
                                                               const float* __restrict__ bias, int relu = 0) {
  __shared__ float4 red[256];
  const int64_t MN = M * N;
  const int64_t e4 = (int64_t)blockIdx.x * 4;
  const int t = threadIdx.x;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int sp = t; sp < splits; sp += 256) {
    const float4 v = *(const float4*)(part + (int64_t)sp * MN + e4);
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  red[t] = acc;
  __syncthreads();
#pragma unroll
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) {
      const float4 o = red[t + w];
      float4 a = red[t];
      a.x += o.x; a.y += o.y; a.z += o.z; a.w += o.w;
      red[t] = a;
    }
    __syncthreads();
  }
  if (t == 0) {
    float4 s = red[0];
    const int64_t m = e4 / N, n = e4 % N;
    if (bias) {
      const float4 bb = *(const float4*)(bias + n);
      s.x += bb.x; s.y += bb.y; s.z += bb.z; s.w += bb.w;
    }
    float4* dst = (float4*)(c + m * ldc + n);
    float4 o = *dst;
    o.x += s.x; o.y += s.y; o.z += s.z; o.w += s.w;
    if (relu) {  // VS_EPI_ATOMIC | VS_EPI_RELU on the skinny path: C = relu(C + sum)
      o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f);
    }
    *dst = o;
  }
}

void launch_splitk_reduce(const vs_gemm_desc* d, const float* part, int splits, bool skinny, hipStream_t s) {
  const uint32_t f = d->epilogue;
  float* c = (float*)d->c;
  const float* bias = (f & VS_EPI_BIAS) ? d->bias : nullptr;
  if (skinny) {
    const int64_t n4 = d->M * d->N / 4;
    hipLaunchKernelGGL(gemm_splitk_reduce_wide, dim3((unsigned)n4), dim3(256), 0, s, part, splits, d->M, d->N, c, d->ldc,
                       bias, (f & VS_EPI_RELU) ? 1 : 0);
    return;
  }
  const int vec = d->N % 4 == 0 && d->ldc % 4 == 0 && aligned16(d->c) && (!(f & VS_EPI_BIAS) || aligned16(d->bias));
  const int64_t n_items = vec ? d->M * d->N / 4 : d->M * d->N;
  if (vec && splits >= 64 && n_items <= 4096)
    hipLaunchKernelGGL(gemm_splitk_reduce_wide, dim3((unsigned)n_items), dim3(256), 0, s, part, splits, d->M, d->N, c,
                       d->ldc, bias);
  else
    hipLaunchKernelGGL(gemm_splitk_reduce, dim3((unsigned)cdiv(n_items, vec ? 64 : 256)), dim3(256), 0, s, part, splits,
                       d->M, d->N, c, d->ldc, bias, vec);
}

GemmPlan plan_gemm(int dtype, int64_t M, int64_t N, int64_t K, int want_split, bool atomic_ok, int64_t ws_bytes) {
  GemmPlan p;
  if (dtype == VS_BF16) {
    p.BM = M <= 64 ? 64 : 128;
    p.BN = (N <= 64 || (N % 128 != 0 && N % 64 == 0 && N < 1024)) ? 64 : 128;
    p.BK = 64;
  } else {
    p.BM = p.BN = 64;
    p.BK = 32;
  }
  p.g.tiles_n = (int)cdiv(N, p.BN);
  p.g.tiles_m = (int)cdiv(M, p.BM);
  const int64_t nk = cdiv(K, p.BK);
  int splits = pick_splits((int64_t)p.g.tiles_n * p.g.tiles_m, nk, want_split, atomic_ok);
  if (ws_bytes > 0 && splits > 1) {  // partials must fit the workspace
    const int64_t fit = ws_bytes / (M * N * 4);
    if (splits > fit) splits = (int)(fit < 1 ? 1 : fit);
  }
  p.g.k_per_split = cdiv(nk, splits) * p.BK;
  p.g.splits = (int)(K > 0 ? cdiv(K, p.g.k_per_split) : 1);
  return p;
}

}  // namespace vs
