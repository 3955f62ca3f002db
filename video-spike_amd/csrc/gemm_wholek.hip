// gemm_wholek.hip — the two vs_gemm kernels for K <= 192 that hold the whole K extent on chip (gemm.hip
// has the overview): the per-tile whole-K kernel and the persistent row-panel kernel.  They share the
// VS_STAMP diagnostic buffer (a __device__ global is private to its translation unit), so they share
// this file.
#include "common.h"
#include "gemm_common.h"
#include "gemm_paths.h"
#include "gemm_tiles.h"

namespace vs {

// ----------------------------------------------------------------------------------------------
// bf16, whole K in LDS (K = 64 * KT <= 256, no split): the skinny projections of the ViT block
// (K = D = 192, and the N = 192 dX products of the attention/MLP inputs).  With only 3 k-steps the
// register-staged pipeline of gemm_bf16_kernel (gemm_tile.hip) pays one global-load latency per
// k-step; here every k-step of A and B is DMA'd into LDS in one burst (global_load_lds, no staging registers), one wait, one
// barrier, then all MFMAs and the epilogue — one latency per tile, and 2 blocks per CU overlap
// one block's loads with the other's MFMAs and stores.
// ----------------------------------------------------------------------------------------------
#ifdef VS_STAMP
// diagnostic build only: per-wave shader-clock phase marks of the whole-K kernel (vs_dbg_gstamps)
__device__ unsigned long long g_gstamp[8 * 8192];
#define VS_GMARK(slot)                                                                        \
  do {                                                                                        \
    const int w_ = blockIdx.x * 4 + (threadIdx.x >> 6);                                       \
    if ((threadIdx.x & 63) == 0 && w_ < 8192) g_gstamp[8 * w_ + (slot)] = __builtin_amdgcn_s_memtime(); \
  } while (0)
#else
#define VS_GMARK(slot)
#endif

template <int BM, int BN, int KT, bool AKC, bool BKC, uint32_t EF>
__global__ __launch_bounds__(256, 2) void gemm_bf16_fullk_kernel(const bf16_t* __restrict__ A, int64_t lda,
                                                                 const bf16_t* __restrict__ B, int64_t ldb,
                                                                 GridMap g, EpiParams e) {
  using OA = OperandBf16<BM, AKC>;
  using OB = OperandBf16<BN, BKC>;
  constexpr int WM = BM / 2, WN = BN / 2, TM = WM / 16, TN = WN / 16;
  constexpr int SMEM = CMax<KT * (OA::BYTES + OB::BYTES), BM*(BN + 4) * 4>::v;
  __shared__ __attribute__((aligned(16))) char smem[SMEM];

  VS_GMARK(0);
  int nt, mt, split;
  map_block(g, nt, mt, split);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;
  const int64_t m0 = (int64_t)mt * BM, n0 = (int64_t)nt * BN;
#pragma unroll
  for (int t = 0; t < KT; ++t) {
    OA::dma(smem + t * OA::BYTES, A, lda, m0, e.M, t * 64, wid, lane);
    OB::dma(smem + KT * OA::BYTES + t * OB::BYTES, B, ldb, n0, e.N, t * 64, wid, lane);
  }
  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  VS_GMARK(1);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  VS_GMARK(2);
#pragma unroll
  for (int t = 0; t < KT; ++t) {
    const char* sa = smem + t * OA::BYTES;
    const char* sb = smem + KT * OA::BYTES + t * OB::BYTES;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 af[TM], bfr[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) af[i] = OA::frag(sa, wr * WM + i * 16, kk, lane);
#pragma unroll
      for (int j = 0; j < TN; ++j) bfr[j] = OB::frag(sb, wc * WN + j * 16, kk, lane);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
  }
  (void)split;
  VS_GMARK(3);
  store_tile<BM, BN, TM, TN, EF>(e, (float*)smem, acc, m0, n0, 0);
  VS_GMARK(4);
#ifdef VS_STAMP
  if ((threadIdx.x & 63) == 0) {
    const int w_ = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w_ < 8192) {
      g_gstamp[8 * w_ + 5] = __builtin_amdgcn_s_getreg((31 << 11) | 4);
      g_gstamp[8 * w_ + 6] = __builtin_amdgcn_s_memrealtime();
    }
  }
#endif
}

// ----------------------------------------------------------------------------------------------
// bf16 row-panel kernel for K <= 192 (the ViT block's K = D projections and dX products:
// qkv, proj, fc1 + GELU, do, da * GELU').  These shapes are HBM-bound on the activations they
// write (M = 25,088 tokens x N = 192..768 columns); the per-tile kernels re-read the A panel
// once per 64-column tile (12x for fc1) and pay one load latency per tile.  Here a persistent
// workgroup owns a contiguous range of (128-row panel, 64-column chunk) items, panel-major:
//   * A: each wave keeps its 32 rows x K of the panel in registers as MFMA fragments (loaded from
//     global once per panel, 48 VGPRs at K = 192) — A is read from HBM about once;
//   * W: the 64 x K chunk of the weight (L2-resident) is register-staged: its global loads for
//     chunk i+1 are in flight while chunk i computes, then written into one LDS image between two
//     barriers (guide T14);
//   * epilogue: each wave stages its 32 x 64 f32 tile in a wave-private LDS image and writes it
//     in the NEXT item's iteration (after the next chunk's loads are issued), whole 8-column
//     groups per lane with 16-B accesses (bias, GELU, GELU', residual fused as elsewhere).
// Grid = min(items, 2 workgroups x 256 CUs): one round, every CU busy, 2 workgroups per CU
// overlap one's epilogue stores with the other's MFMAs.
// ----------------------------------------------------------------------------------------------
template <int KT, bool BKC, uint32_t EF>
__global__ __launch_bounds__(256, 2) void gemm_bf16_panel_kernel(const bf16_t* __restrict__ A, int64_t lda,
                                                                 const bf16_t* __restrict__ B, int64_t ldb,
                                                                 int64_t items, EpiParams e) {
  using OB = OperandBf16<64, BKC>;
  constexpr int KS = 2 * KT;           // 32-deep MFMA k-steps
  constexpr int LDT = 64 + 4;          // staging row stride (floats)
  __shared__ __attribute__((aligned(16))) char wimg[KT * OB::BYTES];
  __shared__ __attribute__((aligned(16))) float stage[4][32 * LDT];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int64_t chunks = e.N / 64;
  const int64_t G = gridDim.x;
  const int64_t it0 = (int64_t)blockIdx.x * items / G, it1 = ((int64_t)blockIdx.x + 1) * items / G;
  if (it0 >= it1) return;
  VS_GMARK(0);
#ifdef VS_STAMP
  if ((threadIdx.x & 63) == 0 && blockIdx.x * 4 + (threadIdx.x >> 6) < 8192)
    g_gstamp[8 * (blockIdx.x * 4 + (threadIdx.x >> 6)) + 7] = __builtin_amdgcn_s_memrealtime();
#endif

  bf16x8 af[2][KS];
  auto load_a = [&](int64_t panel) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      int64_t r = panel * 128 + wid * 32 + i * 16 + (lane & 15);
      r = r < e.M ? r : e.M - 1;  // rows past M: finite data, never stored
      const bf16_t* p = A + r * lda + 8 * (lane >> 4);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) af[i][ks] = *(const bf16x8*)(p + 32 * ks);
    }
  };
  uint4 wreg[KT][OB::CHUNKS];
  auto load_w = [&](int64_t chunk) {
#pragma unroll
    for (int t = 0; t < KT; ++t) OB::load(wreg[t], B, ldb, chunk * 64, e.N, t * 64, KT * 64, tid);
  };
  float* st = stage[wid];
  auto stage_acc = [&](const f32x4 (&acc)[2][4]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) st[(i * 16 + (lane >> 4) * 4 + r) * LDT + j * 16 + (lane & 15)] = acc[i][j][r] * e.alpha;
  };
  // epilogue of a staged item: lane -> rows (lane >> 3) + 8p, 8-column group lane & 7
  auto epilogue = [&](int64_t item) {
    const int64_t m0 = (item / chunks) * 128 + wid * 32, n = (item % chunks) * 64 + (lane & 7) * 8;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int rr = p * 8 + (lane >> 3);
      const int64_t m = m0 + rr;
      if (m < e.M) {
        const float* src = st + rr * LDT + (lane & 7) * 8;
        float v[8];
        const float4 a = *(const float4*)src;
        const float4 b = *(const float4*)(src + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        epi_eight<EF>(e, m, n, v, false);
      }
    }
  };

  int64_t panel = it0 / chunks;
  load_a(panel);
  load_w(it0 % chunks);
  for (int64_t it = it0; it < it1; ++it) {
    __syncthreads();  // every wave is done reading the W image of the previous item
#pragma unroll
    for (int t = 0; t < KT; ++t) OB::store(wimg + t * OB::BYTES, wreg[t], tid);
    __syncthreads();  // W image of item `it` complete
    if (it == it0) VS_GMARK(1);
    if (it + 1 < it1) load_w((it + 1) % chunks);  // in flight under this item's MFMAs
    if (it > it0) epilogue(it - 1);              // previous item's staged tile (wave-private)
    if (it / chunks != panel) {
      panel = it / chunks;
      load_a(panel);
    }
    f32x4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      bf16x8 bfr[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) bfr[j] = OB::frag(wimg + (ks >> 1) * OB::BYTES, j * 16, ks & 1, lane);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i][ks], bfr[j], acc[i][j], 0, 0, 0);
    }
    stage_acc(acc);
    if (it == it0) VS_GMARK(2);
  }
  VS_GMARK(3);
  epilogue(it1 - 1);
  VS_GMARK(4);
#ifdef VS_STAMP
  if ((threadIdx.x & 63) == 0) {
    const int w_ = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w_ < 8192) {
      g_gstamp[8 * w_ + 5] = __builtin_amdgcn_s_getreg((31 << 11) | 4);
      g_gstamp[8 * w_ + 6] = __builtin_amdgcn_s_memrealtime();
    }
  }
#endif
}

// ----------------------------------------------------------------------------------------------
// host
// ----------------------------------------------------------------------------------------------
bool panel_ok(const vs_gemm_desc* d, const EpiParams& e, const GemmPlan& p) {
  const uint32_t f = e.flags;
  // the kernel: bf16, K-contiguous A rows held as fragments (K = 64, 128, 192), whole 64-column chunks
  // with 16-B epilogue accesses, one pass (no split, no row sums, no read-modify-write of C)
  const bool can = d->dtype == VS_BF16 && d->a_kcontig && p.g.splits == 1 && d->K % 64 == 0 && d->K >= 64 && d->K <= 192 &&
                   d->N % 64 == 0 && !d->a_rowsum && !(f & (VS_EPI_ATOMIC | VS_EPI_ACCUM)) && e.vec_ok;
  // Measured (scripts/microbench.py, ViT-Tiny shapes): faster than the per-tile kernels only for the
  // GELU' product (da: 43.2 -> 38.7 us); the per-tile whole-K kernel wins on the others (its
  // 2352 short tiles balance better than 512 persistent workgroups that each load a 48-KB A panel
  // before their first MFMA).  VSPIKE_PANEL=1 forces it for every eligible shape.
  const bool pick = (f & VS_EPI_GELU_BWD) || knob(VS_KNOB_PANEL);
  // knob: VSPIKE_NO_PANEL
  return can && pick && knob(VS_KNOB_NO_PANEL) == 0;
}

void launch_panel(const vs_gemm_desc* d, const EpiParams& e, hipStream_t s) {
  const bf16_t* a = (const bf16_t*)d->a;
  const bf16_t* b = (const bf16_t*)d->b;
  const int64_t items = cdiv(d->M, 128) * (d->N / 64);
  const int gcap = knob(VS_KNOB_PANEL_GRID) > 0 ? knob(VS_KNOB_PANEL_GRID) : 512;
  const unsigned grid = (unsigned)(items < gcap ? items : gcap);
  auto go = [&](auto kt) {
    with_epilogue(e.flags, [&](auto ef) {
      with_layout(d->b_kcontig, [&](auto bkc) {
        hipLaunchKernelGGL((gemm_bf16_panel_kernel<decltype(kt)::value, decltype(bkc)::value, decltype(ef)::value>),
                           dim3(grid), dim3(256), 0, s, a, d->lda, b, d->ldb, items, e);
      });
    });
  };
  const int KT = (int)(d->K / 64);
  if (KT == 1) go(IC<1>{});
  else if (KT == 2) go(IC<2>{});
  else go(IC<3>{});
}

// whole-K-in-LDS path: K = 64..192 in 64-steps, no split, no fused row sums, 128 x 64 tiles
// (72 KB of LDS at K = 192: 2 blocks per CU)
bool fullk_ok(const vs_gemm_desc* d, const EpiParams& e, const GemmPlan& p) {
  // the kernel: bf16, every k-step of the tile in LDS at once, stored once (no split, no atomics), no
  // row sums; instantiated for 128-row tiles only
  const bool can = d->dtype == VS_BF16 && p.g.splits == 1 && d->K % 64 == 0 && d->K >= 64 && d->K <= 192 && p.BM == 128 &&
                   !d->a_rowsum && !(e.flags & VS_EPI_ATOMIC);
  // knob: VSPIKE_NO_FULLK
  return can && knob(VS_KNOB_NO_FULLK) == 0;
}

void launch_fullk(const vs_gemm_desc* d, const EpiParams& e, const GemmPlan& p, hipStream_t s) {
  const bf16_t* a = (const bf16_t*)d->a;
  const bf16_t* b = (const bf16_t*)d->b;
  GridMap gf = p.g;
  gf.tiles_n = (int)cdiv(d->N, 64);
  const unsigned nbf = (unsigned)((int64_t)gf.tiles_n * gf.tiles_m);
  auto go = [&](auto kt) {
    with_epilogue(e.flags, [&](auto ef) {
      with_layout(d->a_kcontig, d->b_kcontig, [&](auto akc, auto bkc) {
        hipLaunchKernelGGL((gemm_bf16_fullk_kernel<128, 64, decltype(kt)::value, decltype(akc)::value, decltype(bkc)::value,
                                                   decltype(ef)::value>),
                           dim3(nbf), dim3(256), 0, s, a, d->lda, b, d->ldb, gf, e);
      });
    });
  };
  const int KT = (int)(d->K / 64);
  if (KT == 1) go(IC<1>{});
  else if (KT == 2) go(IC<2>{});
  else go(IC<3>{});
}

}  // namespace vs

#ifdef VS_STAMP
extern "C" int vs_dbg_gstamps(unsigned long long* host, int n) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(vs::g_gstamp), (size_t)n * sizeof(unsigned long long), 0,
                                  hipMemcpyDeviceToHost);
}
#endif
