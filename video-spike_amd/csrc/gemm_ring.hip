// gemm_ring.hip — vs_gemm's long-K bf16 tile kernel, a 3-stage LDS-DMA ring (gemm.hip has the overview).
#include "common.h"
#include "gemm_common.h"
#include "gemm_paths.h"
#include "gemm_tiles.h"

namespace vs {

// ----------------------------------------------------------------------------------------------
// bf16, long K (K % 64 == 0): 3-stage LDS-DMA ring.  Step t+2 is DMA'd while step t computes, and
// a counted vmcnt keeps step t+1 in flight across each barrier (raw s_barrier: __syncthreads()
// would wait vmcnt(0) and drain it).  The three stages are separate __shared__ objects, the loop
// is unrolled by 3 so every stage index is a constant: alias analysis then keeps hipcc from
// draining the ring before each step's LDS reads.  gemm_bf16_kernel (gemm_tile.hip) had one
// global-load latency exposed per 64-deep step.  Epilogue staged in two row halves (72 KB of LDS
// for 128 x 64: 2 blocks per CU).
// ----------------------------------------------------------------------------------------------
template <int BM, int BN, bool AKC, bool BKC, uint32_t EF>
__global__ __launch_bounds__(256, 2) void gemm_bf16_ring_kernel(const bf16_t* __restrict__ A, int64_t lda,
                                                                const bf16_t* __restrict__ B, int64_t ldb, int64_t K,
                                                                GridMap g, EpiParams e) {
  using OA = OperandBf16<BM, AKC>;
  using OB = OperandBf16<BN, BKC>;
  constexpr int WM = BM / 2, WN = BN / 2, TM = WM / 16, TN = WN / 16;
  constexpr int STAGE = OA::BYTES + OB::BYTES;
  constexpr int S0 = CMax<STAGE, (BM / 2) * (BN + 4) * 4>::v;
  constexpr int PER = OA::PPW + OB::PPW;  // DMA wave-instructions per k-step
  __shared__ __attribute__((aligned(16))) char st0[S0];
  __shared__ __attribute__((aligned(16))) char st1[STAGE];
  __shared__ __attribute__((aligned(16))) char st2[STAGE];

  int nt, mt, split;
  map_block(g, nt, mt, split);
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;
  const int64_t m0 = (int64_t)mt * BM, n0 = (int64_t)nt * BN;
  const int64_t k_begin = (int64_t)split * g.k_per_split;
  const int64_t k_end = k_begin + g.k_per_split < K ? k_begin + g.k_per_split : K;
  const int nk = (int)((k_end - k_begin) / 64);

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bool rowsum_on = e.a_rowsum != nullptr && nt == 0 && wc == 0;
  float rs[TM];
#pragma unroll
  for (int i = 0; i < TM; ++i) rs[i] = 0.f;

  auto issue = [&](int t, char* st) {
    const int64_t k0 = k_begin + (int64_t)t * 64;
    OA::template dma<true>(st, A, lda, m0, e.M, k0, wid, lane);
    OB::template dma<true>(st + OA::BYTES, B, ldb, n0, e.N, k0, wid, lane);
  };
  auto compute = [&](const char* sa) {
    const char* sb = sa + OA::BYTES;
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
  };
  auto step = [&](int t, auto sc) {
    constexpr int S = decltype(sc)::value;
    const char* cur = S == 0 ? st0 : (S == 1 ? st1 : st2);
    char* far = S == 0 ? st2 : (S == 1 ? st0 : st1);  // stage of step t + 2
    if (t + 1 < nk) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(PER) : "memory");  // step t landed
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // every wave's step-t pieces landed; step t-1's stage is free
    asm volatile("" ::: "memory");
    if (t + 2 < nk) issue(t + 2, far);
    compute(cur);
  };
  if (nk > 0) issue(0, st0);
  if (nk > 1) issue(1, st1);
  for (int t = 0; t < nk; t += 3) {
    step(t, IC<0>{});
    if (t + 1 < nk) step(t + 1, IC<1>{});
    if (t + 2 < nk) step(t + 2, IC<2>{});
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (the asm DMA is invisible to hipcc's own waits)
  if (rowsum_on) flush_rowsum<TM>(e.a_rowsum, rs, m0 + wr * WM, e.M, lane);
  store_tile<BM, BN, TM, TN, EF, 2>(e, (float*)st0, acc, m0, n0, split);
}

// ----------------------------------------------------------------------------------------------
// host
// ----------------------------------------------------------------------------------------------
bool ring_ok(const vs_gemm_desc* d, const EpiParams&, const GemmPlan&) {
  // the kernel: bf16, whole 64-deep DMA steps (it takes every layout, epilogue and split of the plan)
  const bool can = d->dtype == VS_BF16 && d->K % 64 == 0;
  // knob: VSPIKE_NO_RING
  return can && knob(VS_KNOB_NO_RING) == 0;
}

// long K: 3-stage DMA ring, BN = 64 tiles (72 KB of LDS at BM = 128: 2 blocks per CU)
void launch_ring(const vs_gemm_desc* d, const EpiParams& e, const GemmPlan& p, hipStream_t s) {
  const bf16_t* a = (const bf16_t*)d->a;
  const bf16_t* b = (const bf16_t*)d->b;
  // the same K split re-planned for 64-wide column tiles; splits as in the 128-wide plan, re-capped
  // by the workspace (its size was computed for the plan's split count)
  GridMap gr = p.g;
  gr.tiles_n = (int)cdiv(d->N, 64);
  const unsigned nbr = (unsigned)((int64_t)gr.tiles_n * gr.tiles_m * gr.splits);
  auto go = [&](auto bm) {
    with_epilogue(e.flags, [&](auto ef) {
      with_layout(d->a_kcontig, d->b_kcontig, [&](auto akc, auto bkc) {
        hipLaunchKernelGGL((gemm_bf16_ring_kernel<decltype(bm)::value, 64, decltype(akc)::value, decltype(bkc)::value,
                                                  decltype(ef)::value>),
                           dim3(nbr), dim3(256), 0, s, a, d->lda, b, d->ldb, d->K, gr, e);
      });
    });
  };
  if (p.BM == 128) go(IC<128>{});
  else go(IC<64>{});
}

}  // namespace vs
