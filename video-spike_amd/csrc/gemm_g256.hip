// gemm_g256.hip — vs_gemm's two large-tile kernels for the MFMA-heavy ViT-Base products (gemm.hip has
// the overview): the 256 x 128 "big" tile and the 256 x 256 persistent kernel.
#include "common.h"
#include "gemm_common.h"
#include "gemm_paths.h"
#include "gemm_tiles.h"

namespace vs {

// ----------------------------------------------------------------------------------------------
// bf16 big-tile kernel for the MFMA-heavy products (K >= 512, N >= 512: ViT-Base's D = 768 /
// F = 3072 projections and their dX, 2-4 TFLOP/s-scale work per launch): 256 x 128 output tile per
// workgroup of 8 waves (4 x 2, 64 x 64 per wave: 16 accumulator tiles, 32 MFMAs per 64-deep k-step
// against 16 fragment reads), 2-stage LDS-DMA ring of 48-KB stages (asm DMA, vmcnt(0) + raw barrier;
// step t+1 in flight under step t's MFMAs; guide §5 "glds vs register staging": at ~1 block per CU
// this ties a register pipeline), one workgroup per CU; the per-tile kernels of the generic plan (128 x 64, 4
// waves) re-read 4x more operand bytes per MFMA and ran these shapes at 0.1-0.2 of the MFMA roof.
// Epilogue: the f32 tile staged through the ring in two 128-row halves, 8-column groups per thread.
// ----------------------------------------------------------------------------------------------
template <bool BKC, uint32_t EF>
__global__ __launch_bounds__(512, 1) void gemm_bf16_big_kernel(const bf16_t* __restrict__ A, int64_t lda,
                                                               const bf16_t* __restrict__ B, int64_t ldb, int64_t K,
                                                               GridMap g, EpiParams e) {
  using OA = OperandBf16<256, true>;
  using OB = OperandBf16<128, BKC>;
  constexpr int STAGE = OA::BYTES + OB::BYTES;  // 48 KB
  constexpr int LDT = 128 + 4;
  constexpr int SMEM = CMax<3 * STAGE, 128 * LDT * 4>::v;  // 3-stage ring: 144 KB
  // DMA pieces (1 KB wave-instructions) one wave issues per stage: the counted wait of a step
  constexpr int PPW = OA::PIECES / 8 + OB::PIECES / 8;
  static_assert(PPW == 6, "vmcnt below assumes 6 pieces per wave and stage");
  __shared__ __attribute__((aligned(16))) char smem[SMEM];

  int nt, mt, split;
  map_block(g, nt, mt, split);
  (void)split;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wr = wid >> 1, wc = wid & 1;
  const int64_t m0 = (int64_t)mt * 256, n0 = (int64_t)nt * 128;
  const int nk = (int)(K / 64);
  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  auto issue = [&](int t, char* st) {
    const int64_t k0 = (int64_t)t * 64;
    OA::template dma_nw<8>(st, A, lda, m0, e.M, k0, wid, lane);
    OB::template dma_nw<8>(st + OA::BYTES, B, ldb, n0, e.N, k0, wid, lane);
  };
  auto compute = [&](const char* sa) {
    const char* sb = sa + OA::BYTES;
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 af[4], bfr[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i] = OA::frag(sa, wr * 64 + i * 16, kk, lane);
#pragma unroll
      for (int j = 0; j < 4; ++j) bfr[j] = OB::frag(sb, wc * 64 + j * 16, kk, lane);
#ifdef VS_GEMM_PRIO  // diagnostic builds: the MFMA cluster at raised wave priority
      __builtin_amdgcn_s_setprio(1);
#endif
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
#ifdef VS_GEMM_PRIO
      __builtin_amdgcn_s_setprio(0);
#endif
    }
  };
  // 3-stage ring, two steps in flight (guide §5 "Pipelining across barriers": a stage stays in flight
  // across the barrier): step t waits for ITS pieces only (vmcnt(6) leaves step t+1's 6 in flight),
  // then the raw barrier makes every wave's pieces of t visible and every wave's reads of t-1 done,
  // so step t+2 may refill t-1's stage.
  auto step = [&](int t, auto sc) {
    constexpr int S = decltype(sc)::value;  // == t % 3
    if (t + 1 < nk) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (t + 2 < nk) issue(t + 2, smem + ((S + 2) % 3) * STAGE);
    compute(smem + S * STAGE);
  };
  issue(0, smem);
  if (nk > 1) issue(1, smem + STAGE);
  for (int t = 0; t < nk; t += 3) {
    step(t, IC<0>{});
    if (t + 1 < nk) step(t + 1, IC<1>{});
    if (t + 2 < nk) step(t + 2, IC<2>{});
  }
  float* stg = (float*)smem;
  constexpr int CPR = 128 / 8;  // 8-column groups per row: 32 rows per pass of 512 threads
#pragma unroll
  for (int part = 0; part < 2; ++part) {
    __syncthreads();  // every wave's last operand reads / the previous half's epilogue reads are done
    if ((wr >> 1) == part) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            stg[((wr & 1) * 64 + i * 16 + (lane >> 4) * 4 + r) * LDT + wc * 64 + j * 16 + (lane & 15)] =
                acc[i][j][r] * e.alpha;
    }
    __syncthreads();
    // the 4 passes' operands are fetched before the first store (epi_eight_fetch: one store round
    // trip per half-tile instead of one per pass)
    EpiOps8 ops[EF == kEpiRuntime ? 1 : 4];
    if constexpr (EF != kEpiRuntime) {
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const int64_t m = m0 + part * 128 + p * 32 + tid / CPR, n = n0 + (tid % CPR) * 8;
        epi_eight_fetch<EF>(e, m < e.M ? m : e.M - 1, n, ops[p], false);
      }
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int rr = p * 32 + tid / CPR, cg = tid % CPR;
      const int64_t m = m0 + part * 128 + rr, n = n0 + cg * 8;
      if (m < e.M) {
        const float* src = stg + rr * LDT + cg * 8;
        float v[8];
        const float4 a = *(const float4*)src;
        const float4 b = *(const float4*)(src + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        if constexpr (EF != kEpiRuntime) epi_eight_finish<EF>(e, m, n, v, ops[p], false);
        else epi_eight<EF>(e, m, n, v, false);
      }
    }
  }
}

// ----------------------------------------------------------------------------------------------
// 256 x 256 persistent bf16 GEMM for the long-M block products of ViT-Base (C3: M = 200,704 token
// rows, N in {768, 2304, 3072}, K in {768, 2304, 3072}) where it beats the 256 x 128 big tile (VS_KNOB_G256).
//   * one persistent workgroup per CU (8 waves, 2 x 4, 128 x 64 outputs per wave: 4 x 4 16x16x32
//     MFMAs per 8 fragment reads), tiles dealt XCD-contiguously (a tile's A row-panel and the
//     weights stay in that XCD's L2);
//   * 64-deep k stages (2 x 32 KB: A and B images with 128-B rows), two LDS slots: the stage after
//     the current one is issued at its start and waited for at its last phase; the ring runs ACROSS
//     tiles, so the next tile's first stage loads under this tile's last stage and epilogue.  Full
//     128-B row segments per DMA piece (8 rows x 128 B): round 5's first version used 32-deep stages
//     whose pieces were 16 rows x 64 B, half-line requests that doubled the address path's work
//     (cdna_hip_programming.md: fragment-shaped 64-B loads +18-45 %);
//   * four phases per stage (k half x row half), the next phase's fragments read before the current
//     phase's MFMAs; one vmcnt(0) + raw barrier per stage;
//   * the product is computed transposed (C^T = B^T A^T on the MFMA), so a lane's accumulator quad is
//     4 consecutive output columns of one row: the epilogue works straight from registers with 8-B
//     (bf16) / 16-B (f32) vector loads and stores, no LDS staging, ring untouched.
// Operand images (per stage): A K-contiguous [256 rows][64 k] (128-B rows, 16-B chunk ^= (r >> 1) & 7:
// conflict-free ds_read_b128 over each 16-lane group); B K-contiguous likewise, or N-contiguous
// [64 k][256 n] (512-B rows, chunk ^= swz_mc(k): conflict-free ds_read_tr16_b64 pairs).
// ----------------------------------------------------------------------------------------------
// chunk key of the 256 x 256 kernel's K-contiguous B image: bits 1, 3, 4 of the row
__device__ __forceinline__ int g256_swzb(int r) { return ((r >> 1) & 1) | ((r >> 2) & 6); }
// a wave-uniform pointer pinned to SGPRs (the saddr operand of the asm DMA)
__device__ __forceinline__ const char* sgpr_ptr(const char* p) {
  const uint64_t v = (uint64_t)p;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return (const char*)(((uint64_t)hi << 32) | lo);
}

struct G256Map {
  int tiles_n, tiles, per_xcd, nk;  // nk = K / 64 stages per tile
  int dbg;      // VS_DEBUG_KNOBS builds: VS_KNOB_G256_DBG
  int stagger;  // odd-slot workgroups start this many s_sleep(127) (~4 us each) late (VS_KNOB_G256_STAGGER)
  int ed_ok;    // the early-DMA counted wait may be used: set by the host only when the instance has no
                // private (scratch) segment, i.e. its epilogue issues exactly `est` vector-memory ops
                // (a spill would add scratch loads / stores the count does not include)
  int a3;       // A (the streamed token-row operand) in THREE 32-KB slots, B in two: A's DMA is issued two
                // stages ahead and the stage wait is counted (vmcnt(4 + stores)), never 0 (VS_KNOB_G256_A3)
};

template <bool BKC, bool P8, uint32_t EF>
__global__ __launch_bounds__(512, 1) void gemm_bf16_g256_kernel(const bf16_t* __restrict__ A, int64_t lda,
                                                                const bf16_t* __restrict__ B, int64_t ldb,
                                                                G256Map g, EpiParams e) {
  static_assert(!BKC || P8, "K-contiguous B fragments are always column-permuted (8-column vectors)");
  constexpr int AB = 256 * 64 * 2, STAGE = 2 * AB;  // 2 slots x 64 KB (a3: A 3 x 32 KB + B 2 x 32 KB)
  __shared__ __attribute__((aligned(16))) char smem[5 * AB];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wr = wid >> 2, wc = wid & 3;
  // this workgroup's tiles: XCD x = blockIdx % 8 owns logical tiles [x * per_xcd, (x+1) * per_xcd)
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, slots = gridDim.x >> 3;
  const int t_lo = xcd * g.per_xcd;
  const int t_hi = t_lo + g.per_xcd < g.tiles ? t_lo + g.per_xcd : g.tiles;
  const int my_tiles = t_lo + slot < t_hi ? (t_hi - t_lo - slot + slots - 1) / slots : 0;
  const int total = my_tiles * g.nk;  // stages of this workgroup
  if (total == 0) return;
#ifdef VS_DEBUG_KNOBS
  // diagnostic builds only (VS_KNOB_G256_DBG): bit 0 skips the operand DMA (MFMAs on stale LDS), bit
  // 1 the epilogue's stores -- the k-loop, the memory stream and the epilogue timed apart
  const int dbg = g.dbg;
#else
  constexpr int dbg = 0;
#endif
  auto tile_of = [&](int k, int& m0, int& n0) __attribute__((always_inline)) {
    const int L = t_lo + slot + k * slots;
    m0 = (L / g.tiles_n) * 256;
    n0 = (L % g.tiles_n) * 256;
  };
  // Staggered start: every CU runs the same tile schedule, so without it all 256 store their epilogue
  // at the same moment and then all stream operands at once; half of them starting late interleaves
  // the two phases across the chip.
  if (slot & 1)
    for (int i = 0; i < g.stagger; ++i) __builtin_amdgcn_s_sleep(127);

  // ---- DMA: stage s -> slot s & 1; wave w fills rows 32w .. 32w+31 of the A image (4 pieces of
  // 8 rows x 128 B) and the same of B (or k rows 8w .. 8w+7 of an N-contiguous B: 4 pieces of
  // 2 k-rows x 512 B).  Per-lane byte offsets are stage-invariant (the tile / k base is an SGPR).
  uint32_t a_off[4], b_off[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int r = wid * 32 + p * 8 + (lane >> 3);
    a_off[p] = (uint32_t)(r * lda * 2 + ((((lane & 7) ^ ((r >> 1) & 7))) << 4));
    if constexpr (BKC) {  // B image chunk key g256_swzb(r) (fragment rows are permuted, see below)
      b_off[p] = (uint32_t)(r * ldb * 2 + ((((lane & 7) ^ g256_swzb(r))) << 4));
    } else {
      const int k = wid * 8 + 2 * p + (lane >> 5);
      b_off[p] = (uint32_t)(k * ldb * 2 + ((((lane & 31) ^ swz_mc<128>(k))) << 4));
    }
  }
  // Slot byte offsets: A of stage s at a_at(slot), B at b_at(slot) + AB (the B read offsets include + AB);
  // slots cycle 0, 1 (A and B together) or, a3, A 0, 1, 2 and B 0, 1
  const bool a3 = g.a3 != 0;
  auto a_at = [&](int sl) __attribute__((always_inline)) { return a3 ? sl * AB : sl * STAGE; };
  auto b_at = [&](int sl) __attribute__((always_inline)) { return a3 ? 2 * AB + sl * AB : sl * STAGE; };
  auto a_nxt = [&](int sl) __attribute__((always_inline)) { return a3 ? (sl == 2 ? 0 : sl + 1) : (sl ^ 1); };
  // The A and B DMA streams each issue stages 0, 1, 2, ... in order: scalar state advanced per stage
  // (global base + 64 k, the tile's rows and bases recomputed once per tile), LDS destinations as
  // wave-uniform 32-bit addresses (the round-5 form recomputed the tile by two divisions and converted
  // each piece's generic LDS pointer -- ~300 scalar / vector instructions per stage and wave)
  const uint32_t lds_w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uintptr_t)(VS_LDS char*)smem) +
                         (uint32_t)__builtin_amdgcn_readfirstlane(wid) * 4096u;
  const int64_t b_step = BKC ? 128 : (int64_t)128 * ldb;  // bytes per 64-deep stage of B
  int sa_k = 0, sa_t = 0, sa_sl = 0, sb_k = 0, sb_t = 0, sb_sl = 0;
  int64_t sa_rows = 0;
  const char* sa_ptr = nullptr;
  const char* sb_ptr = nullptr;
  auto a_tile = [&]() __attribute__((always_inline)) {
    int m0, n0;
    tile_of(sa_k, m0, n0);
    (void)n0;
    sa_rows = e.M - m0;  // rows past M re-read row M-1 (never stored)
    sa_ptr = (const char*)(A + (int64_t)m0 * lda);
  };
  auto b_tile = [&]() __attribute__((always_inline)) {
    int m0, n0;
    tile_of(sb_k, m0, n0);
    (void)m0;
    sb_ptr = BKC ? (const char*)(B + (int64_t)n0 * ldb) : (const char*)(B + n0);
  };
  a_tile();
  b_tile();
  auto issue_a = [&]() __attribute__((always_inline)) {
    if (!(dbg & 1)) {
      const uint32_t l = lds_w + (uint32_t)a_at(sa_sl);
      if (sa_rows >= 256) {
        glds16x4_m0(sa_ptr, a_off[0], a_off[1], a_off[2], a_off[3], l, l + 1024, l + 2048, l + 3072);
      } else {
        uint32_t o[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) {
          const int r = wid * 32 + p * 8 + (lane >> 3), rc = r < sa_rows ? r : (int)sa_rows - 1;
          o[p] = (uint32_t)(rc * lda * 2 + ((((lane & 7) ^ ((r >> 1) & 7))) << 4));
        }
        glds16x4_m0(sa_ptr, o[0], o[1], o[2], o[3], l, l + 1024, l + 2048, l + 3072);
      }
    }
    if (++sa_t == g.nk) {
      sa_t = 0;
      ++sa_k;
      a_tile();
    } else {
      sa_ptr += 128;
    }
    sa_sl = a_nxt(sa_sl);
  };
  auto issue_b = [&]() __attribute__((always_inline)) {
    if (!(dbg & 1)) {
      const uint32_t l = lds_w + (uint32_t)(b_at(sb_sl) + AB);
      glds16x4_m0(sb_ptr, b_off[0], b_off[1], b_off[2], b_off[3], l, l + 1024, l + 2048, l + 3072);
    }
    if (++sb_t == g.nk) {
      sb_t = 0;
      ++sb_k;
      b_tile();
    } else {
      sb_ptr += b_step;
    }
    sb_sl ^= 1;
  };
  auto issue = [&]() __attribute__((always_inline)) {
    issue_a();
    issue_b();
  };

  // ---- fragments (per lane, stage-invariant byte offsets; kk = 32-deep half of the stage)
  // K-contiguous B (the forward products, bf16 out): fragment j = 2p + e, row r holds output column
  // wc*64 + 32p + 8(r >> 2) + 4e + (r & 3), so the accumulator quads of fragments 2p and 2p+1 in one
  // lane are 8 CONSECUTIVE columns (8fc .. 8fc+7 of the 32-column half p) and the epilogue moves 16-B
  // bf16 vectors.  The image's chunk key g256_swzb(n) reads bits 1, 3, 4 of n -- unchanged by 4e and
  // 32p, so every fragment is the lane address + an immediate -- and keeps the ds_read_b128 groups
  // conflict-free (checked by enumeration).  N-contiguous B (read transposed, ds_read_tr16_b64) takes
  // the same permutation when the output is bf16 (P8: its quads then conflict 2-way) and keeps plain
  // 4-column quads for f32 outputs (16-B vectors already).
  const int fr = lane & 15, fc = lane >> 4;
  int a_rd[2], b_rd[4][2];
#pragma unroll
  for (int kk = 0; kk < 2; ++kk) a_rd[kk] = (wr * 128 + fr) * 128 + (((kk * 4 + fc) ^ ((fr >> 1) & 7)) << 4);
  if constexpr (BKC) {
    // image row n = R0 + 32p + 4e, R0 = wc*64 + 8(fr >> 2) + (fr & 3): key(n) = key(R0)
    const int R0 = wc * 64 + 8 * (fr >> 2) + (fr & 3);
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) b_rd[kk][0] = AB + R0 * 128 + (((kk * 4 + fc) ^ g256_swzb(R0)) << 4);
  } else {  // k rows kr0 / kr1 of a 32-deep half (swz_mc has period 16 in k: the second half is + 16 KB)
    const int q = fr >> 2, kr0 = 8 * fc + q, kr1 = kr0 + 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int col = P8 ? wc * 64 + 32 * (j >> 1) + 8 * (lane & 3) + 4 * (j & 1) : wc * 64 + j * 16 + (lane & 3) * 4;
      b_rd[j][0] = AB + kr0 * 512 + (((col >> 3) ^ swz_mc<128>(kr0)) << 4) + (col & 7) * 2;
      b_rd[j][1] = AB + kr1 * 512 + (((col >> 3) ^ swz_mc<128>(kr1)) << 4) + (col & 7) * 2;
    }
  }
  auto read_a = [&](const char* st, int kk, int rh, bf16x8 (&af)[4]) __attribute__((always_inline)) {
#pragma unroll
    for (int f = 0; f < 4; ++f) af[f] = *(const bf16x8*)(st + a_rd[kk] + (rh * 64 + f * 16) * 128);
  };
  auto read_b = [&](const char* st, int kk, bf16x8 (&bf)[4]) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if constexpr (BKC) {
        bf[j] = *(const bf16x8*)(st + b_rd[kk][0] + (32 * (j >> 1) + 4 * (j & 1)) * 128);
      } else {
        short4v t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((VS_LDS short4v*)(st + b_rd[j][0] + kk * 16384));
        short4v t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((VS_LDS short4v*)(st + b_rd[j][1] + kk * 16384));
        typedef __attribute__((ext_vector_type(8))) short short8v;
        short8v v = {t0[0], t0[1], t0[2], t0[3], t1[0], t1[1], t1[2], t1[3]};
        bf[j] = __builtin_bit_cast(bf16x8, v);
      }
    }
  };

  f32x4 acc[8][4];  // each tile's first k-step overwrites them (mfma16z); zeroed once so no path reads undef
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // epilogue geometry (see below) and the bias, which the early-DMA variants load one stage ahead
  constexpr int EW = P8 ? 8 : 4, ENV = 16 / EW, EVS = P8 ? 32 : 16;
  constexpr bool EBIAS = (EF & VS_EPI_BIAS) != 0;
  // ED (early DMA): the variants whose epilogue loads nothing per row (bias at most) issue each stage's
  // successor DMA right after the barrier that frees its slot -- before a tile's epilogue stores --
  // and wait for it with vmcnt(<stores issued since>), so the stores drain under the next tile's first
  // stage instead of stalling it (vmcnt retires loads, DMA and stores in order)
  constexpr bool ED = (EF & (VS_EPI_RESIDUAL | VS_EPI_MUL_AUX | VS_EPI_GELU_BWD)) == 0;
  // The early-DMA variants' bias by SCALAR loads (constant address space, wave-uniform base): counted by
  // lgkmcnt, so hipcc's wait for them never drains the in-flight DMA (a vector load's vmcnt wait does:
  // vmcnt retires in order); each lane then picks its EW columns of the wave's 4 x EW by fc
  float ebias[ENV][EW];
  auto load_bias = [&](int k) __attribute__((always_inline)) {
    int m0, n0;
    tile_of(k, m0, n0);
    (void)m0;
    if constexpr (ED) {
      typedef const __attribute__((address_space(4))) float* cfp;
      const cfp bp = (cfp)e.bias + __builtin_amdgcn_readfirstlane(n0 + wc * 64);
#pragma unroll
      for (int vv = 0; vv < ENV; ++vv) {
        float sb[4 * EW];
#pragma unroll
        for (int q = 0; q < 4 * EW; ++q) sb[q] = bp[EVS * vv + q];
#pragma unroll
        for (int r = 0; r < EW; ++r)
          ebias[vv][r] = fc == 0 ? sb[r] : fc == 1 ? sb[EW + r] : fc == 2 ? sb[2 * EW + r] : sb[3 * EW + r];
      }
    } else {
      // the residual / GELU' variants drain vmcnt every stage anyway; scalar loads there cost SGPRs that
      // their epilogue's operand addressing needs (fc2: SGPR spills to VGPR lanes at 256 VGPRs, 974 -> 1,177 us)
#pragma unroll
      for (int vv = 0; vv < ENV; ++vv) {
        if constexpr (EW == 8) ld8(e.bias, n0 + wc * 64 + EW * fc + EVS * vv, 0, ebias[vv]);
        else ld4(e.bias, n0 + wc * 64 + EW * fc + EVS * vv, 0, ebias[vv]);
      }
    }
  };
  // epilogue store instructions per lane (vmcnt units), all issued after the early DMA
  const int est_c = 8 * ENV * ((EW == 8 && !e.out_bf16) ? 2 : 1);
  const int est = est_c + ((EF & VS_EPI_GELU) ? 8 * ENV : 0);

  // Epilogue straight from the accumulators (C^T layout: lane (fr, fc) holds row m0+...+fr and W = 8
  // consecutive columns per 32-column half v (K-contiguous B: acc[i][2v] | acc[i][2v+1], columns 8fc ..)
  // or W = 4 per 16-column block v (acc[i][v], columns 4fc ..)).  CDNA4's vmcnt counts stores as well
  // as loads and retires them in order, so a "load operand -> use -> store" sequence per vector would
  // wait for every earlier store; every operand a group of rows needs is loaded before its first
  // store: the bias once per tile, the residual / GELU' factor per 32 rows of the wave.
  auto epilogue = [&](int k) __attribute__((always_inline)) {
    int m0, n0;
    tile_of(k, m0, n0);
    constexpr uint32_t F = EF;
    constexpr bool BIAS = (F & VS_EPI_BIAS) != 0, RES = (F & VS_EPI_RESIDUAL) != 0;
    constexpr bool AUXIN = (F & (VS_EPI_MUL_AUX | VS_EPI_GELU_BWD)) != 0, GELU = (F & VS_EPI_GELU) != 0;
    constexpr int W = EW, NV = ENV;  // columns per vector, vectors per row fragment
    constexpr int VS = EVS;          // column step between a lane's vectors
    const int ncol = n0 + wc * 64 + W * fc;
    auto stv = [&](void* p, int64_t i, int bf, const float (&v)[W]) __attribute__((always_inline)) {
      if constexpr (W == 8) st8(p, i, bf, v);
      else st4(p, i, bf, v);
    };
    if constexpr (BIAS && !ED) load_bias(k);  // ED: loaded at the start of the tile's last stage
    // Operand rows (residual f32, GELU' factor bf16: g256 runs bf16 operands only) as raw 16-B vectors,
    // row fragment i+1's loads issued before fragment i's stores (round 6).  vmcnt retires in order, so
    // a load issued after a fragment's stores waited for all of them: round 5 loaded per 32 rows, and
    // each later group of the epilogue stalled on the previous group's store completion.
    struct Raw {
      float4 f[NV][W / 4];
      uint4 h8[NV];
      uint2 h4[NV];
    };
    auto ld_raw = [&](int i, Raw& rw) __attribute__((always_inline)) {
      const int64_t m = m0 + wr * 128 + i * 16 + fr;
      const int64_t mc = m < e.M ? m : e.M - 1;  // rows past M: any valid row (not stored)
#pragma unroll
      for (int vv = 0; vv < NV; ++vv) {
        if constexpr (RES) {
#pragma unroll
          for (int q = 0; q < W / 4; ++q) rw.f[vv][q] = *(const float4*)(e.residual + mc * e.ldr + ncol + VS * vv + 4 * q);
        } else if constexpr (W == 8) {
          rw.h8[vv] = *(const uint4*)((const bf16_t*)e.aux_in + mc * e.ld_aux_in + ncol + VS * vv);
        } else {
          rw.h4[vv] = *(const uint2*)((const bf16_t*)e.aux_in + mc * e.ld_aux_in + ncol + VS * vv);
        }
      }
    };
    auto unpack = [&](const Raw& rw, int vv, float (&o)[W]) __attribute__((always_inline)) {
      if constexpr (RES) {
#pragma unroll
        for (int q = 0; q < W / 4; ++q) {
          o[4 * q] = rw.f[vv][q].x;
          o[4 * q + 1] = rw.f[vv][q].y;
          o[4 * q + 2] = rw.f[vv][q].z;
          o[4 * q + 3] = rw.f[vv][q].w;
        }
      } else {
        uint32_t w4[W / 2];
        if constexpr (W == 8) {
          w4[0] = rw.h8[vv].x; w4[1] = rw.h8[vv].y; w4[2] = rw.h8[vv].z; w4[3] = rw.h8[vv].w;
        } else {
          w4[0] = rw.h4[vv].x; w4[1] = rw.h4[vv].y;
        }
#pragma unroll
        for (int q = 0; q < W / 2; ++q) {
          o[2 * q] = __uint_as_float(w4[q] << 16);
          o[2 * q + 1] = __uint_as_float(w4[q] & 0xffff0000u);
        }
      }
    };
    Raw rbuf[2];
    if constexpr (RES || AUXIN) ld_raw(0, rbuf[0]);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if constexpr (RES || AUXIN) {
        if (i + 1 < 8) ld_raw(i + 1, rbuf[(i + 1) & 1]);
      }
      {
        const int64_t m = m0 + wr * 128 + i * 16 + fr;
        const bool live = m < e.M;
#pragma unroll
        for (int vv = 0; vv < NV; ++vv) {
          float opv[W];
          if constexpr (RES || AUXIN) unpack(rbuf[i & 1], vv, opv);
          float v[W], t[W];
#pragma unroll
          for (int r = 0; r < W; ++r) {
            v[r] = acc[i][(W / 4) * vv + (r >> 2)][r & 3] * e.alpha;
            if constexpr (BIAS) v[r] += ebias[vv][r];
          }
          if constexpr ((F & VS_EPI_GELU_BWD) != 0) {
#pragma unroll
            for (int r = 0; r < W; ++r) v[r] *= gelu_fast_grad(opv[r]);
          }
          if constexpr ((F & VS_EPI_MUL_AUX) != 0) {
#pragma unroll
            for (int r = 0; r < W; ++r) v[r] *= opv[r];
          }
          const int64_t n = ncol + VS * vv;
          if constexpr (GELU) {
            if constexpr ((F & VS_EPI_GELU_GRAD) != 0) {  // packed pairs (the epilogue's dominant VALU)
#pragma unroll
              for (int r = 0; r < W; r += 2) {
                const f32x2v x = {bf2f(f2bf(v[r])), bf2f(f2bf(v[r + 1]))};
                f32x2v gr;
                const f32x2v y = gelu_fast_both2(x, gr);
                v[r] = y.x;
                v[r + 1] = y.y;
                t[r] = gr.x;
                t[r + 1] = gr.y;
              }
            } else {
#pragma unroll
              for (int r = 0; r < W; ++r) {
                const float x = bf2f(f2bf(v[r]));
                t[r] = v[r];
                v[r] = gelu_fast(x);
              }
            }
            if (live && !(dbg & 2)) stv(e.aux_out, m * e.ld_aux_out + n, e.op_bf16, t);
          }
          if constexpr (RES) {
#pragma unroll
            for (int r = 0; r < W; ++r) v[r] += opv[r];
          }
          if (live && !(dbg & 2)) stv(e.c, m * e.ldc + n, e.out_bf16, v);
          // ED: no re-zeroing (the next tile's first k-step MFMAs take a zero C operand); the residual /
          // GELU' variants keep the zeroing pass: with the zero-C copy of the MFMA block fc2 (256 VGPRs)
          // measured 974 -> 1,236 us
          if constexpr (!ED) {
#pragma unroll
            for (int q = 0; q < W / 4; ++q) acc[i][(W / 4) * vv + q] = f32x4{0.f, 0.f, 0.f, 0.f};
          }
        }
      }
    }
  };

  auto mfma16 = [&](const bf16x8 (&bc)[4], const bf16x8 (&af)[4], int rh) __attribute__((always_inline)) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[rh * 4 + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bc[j], af[i], acc[rh * 4 + i][j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
  };
  // a tile's first k-step: C = 0 (an inline constant), so the accumulators need no zeroing pass
  // (128 v_mov per wave and tile)
  auto mfma16z = [&](const bf16x8 (&bc)[4], const bf16x8 (&af)[4], int rh) __attribute__((always_inline)) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[rh * 4 + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bc[j], af[i], f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
  };

  // prologue: stage 0 landed, its first fragments in registers
  bf16x8 a0[4], a1[4], b0[4], b1[4];
  issue();  // stage 0
  if (a3 && total > 1) {
    issue_a();  // A(1)
    asm volatile("s_waitcnt vmcnt(4)" ::: "memory");  // A(0), B(0) landed; A(1) in flight
  } else {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  read_b(smem + b_at(0), 0, b0);
  read_a(smem + a_at(0), 0, 0, a0);

  // Stage s (slot s & 1), four phases; fragments of the next phase are read before this phase's MFMAs:
  //   P0: DMA stage s+1 into the other slot (every wave's reads of stage s-1 retired before the
  //       barrier of s-1's P3) | A(kk0, rh1) | MFMA B0 x A(kk0, rh0)
  //   P1: B(kk1), A(kk1, rh0) | MFMA B0 x A(kk0, rh1)
  //   P2: A(kk1, rh1) | MFMA B1 x A(kk1, rh0)
  //   P3: vmcnt(0) + lgkmcnt(0) + barrier (stage s+1 landed everywhere; stage s's reads retired) |
  //       B(kk0), A(kk0, rh0) of stage s+1 | MFMA B1 x A(kk1, rh1) | epilogue at a tile's last stage
  // a3: A(s+2) is issued with B(s+1) at P0 (ED: B(s+2) and A(s+3) after the barrier of stage s, into the
  // slots stage s just freed); the P3 wait keeps the youngest A stage (4 pieces per wave) and the stores in
  // flight.  Spreading A's pieces over the phases instead (one per phase, the guide's 8-phase interleave)
  // measured 1-11 % SLOWER on every dX product (profiles/r06_g256_a3s_ab.json)
  if (ED && total > 1) {
    if (a3) {
      issue_b();                  // B(1)
      if (total > 2) issue_a();   // A(2)
    } else {
      issue();                    // stage 1
    }
  }
  int nst = 0;  // ED: store instructions issued after the DMA in flight (the previous tile's epilogue)
  int ra = 0, rb = 0, tk = 0, tt = 0;  // compute side: slots of stage s, its tile and k-step
  for (int s = 0; s < total; ++s) {
    const char* cur = smem + a_at(ra);
    const char* curb = smem + b_at(rb);
    const bool last = tt == g.nk - 1;
    const bool a_next = a3 && s + 2 < total;  // A(s+2) in flight at this stage's wait
    if (!ED) {
      if (a3) {
        if (s + 1 < total) issue_b();  // B(s+1)
        if (a_next) issue_a();         // A(s+2)
      } else if (s + 1 < total) {
        issue();                       // stage s+1
      }
    }
    if (ED && EBIAS && last) load_bias(tk);
    read_a(cur, 0, 1, a1);
    __builtin_amdgcn_sched_barrier(0);
    if (ED && tt == 0) mfma16z(b0, a0, 0);
    else mfma16(b0, a0, 0);
    read_b(curb, 1, b1);
    read_a(cur, 1, 0, a0);
    __builtin_amdgcn_sched_barrier(0);
    if (ED && tt == 0) mfma16z(b0, a1, 1);
    else mfma16(b0, a1, 1);
    read_a(cur, 1, 1, a1);
    __builtin_amdgcn_sched_barrier(0);
    mfma16(b1, a0, 0);
    // stage s+1 landed: vmcnt(0), or all but the youngest `allow` ops -- (ED) the nst stores issued after
    // its DMA, (a3) the 4 pieces of A(s+2) -- as the largest encodable count <= allow (waiting for more
    // than needed is always safe)
    const int allow = (ED ? nst : 0) + (a_next ? 4 : 0);
    if (allow < 4) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    else if (allow < 16) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else if (allow < 20) asm volatile("s_waitcnt vmcnt(16)" ::: "memory");
    else if (allow < 32) asm volatile("s_waitcnt vmcnt(20)" ::: "memory");
    else if (allow < 36) asm volatile("s_waitcnt vmcnt(32)" ::: "memory");
    else if (allow < 48) asm volatile("s_waitcnt vmcnt(36)" ::: "memory");
    else if (allow < 52) asm volatile("s_waitcnt vmcnt(48)" ::: "memory");
    else if (allow < 63) asm volatile("s_waitcnt vmcnt(52)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(63)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if constexpr (ED) {
      if (EBIAS && last) {  // the bias (scalar loads at this stage's start) in registers before the next DMA
#pragma unroll
        for (int vv = 0; vv < ENV; ++vv)
#pragma unroll
          for (int r = 0; r < EW; ++r) asm volatile("" : "+v"(ebias[vv][r]));
      }
      // into the slots of stage s: every wave's reads of stage s retired
      if (a3) {
        if (s + 2 < total) issue_b();  // B(s+2)
        if (s + 3 < total) issue_a();  // A(s+3)
      } else if (s + 2 < total) {
        issue();                       // stage s+2
      }
    }
    ra = a_nxt(ra);
    rb ^= 1;
    if (s + 1 < total) {
      read_b(smem + b_at(rb), 0, b0);
      read_a(smem + a_at(ra), 0, 0, a0);
    }
    __builtin_amdgcn_sched_barrier(0);
    mfma16(b1, a1, 1);
    nst = 0;
    if (last) {
      epilogue(tk);
      if constexpr (ED) {
        int m0, n0;
        tile_of(tk, m0, n0);
        (void)n0;
        // exact count only for a full tile (a ragged one skips the stores of all-dead rows) and real stores
        nst = (g.ed_ok && m0 + 256 <= e.M && !(dbg & 2)) ? (est < 63 ? est : 63) : 0;
      }
      tt = 0;
      ++tk;
    } else {
      ++tt;
    }
  }
}

// ----------------------------------------------------------------------------------------------
// host: the 256 x 128 big tile
// ----------------------------------------------------------------------------------------------
// big-tile path: MFMA-heavy products (K >= 512, N >= 512, N % 128 == 0: the ViT-Base block)
bool big_ok(const vs_gemm_desc* d, const EpiParams& e) {
  // the kernel: bf16, K-contiguous A, whole 128-column tiles and 64-deep DMA steps, 16-B epilogue
  // accesses, one pass (no split, no row sums, no read-modify-write of C)
  const bool can = d->dtype == VS_BF16 && d->a_kcontig && d->N % 128 == 0 && d->K % 64 == 0 && d->split_k <= 1 &&
                   !d->a_rowsum && e.vec_ok && !(e.flags & (VS_EPI_ATOMIC | VS_EPI_ACCUM));
  // where it pays: enough 256 x 128 tiles and k-steps to amortise the 144-KB ring (one workgroup per CU)
  const bool pick = d->M >= 4096 && d->N >= 512 && d->K >= 512;
  // knob: VSPIKE_NO_BIG
  return can && pick && !knob(VS_KNOB_NO_BIG);
}

int launch_big(const vs_gemm_desc* d, const EpiParams& e, hipStream_t s) {
  const bf16_t* a = (const bf16_t*)d->a;
  const bf16_t* b = (const bf16_t*)d->b;
  GridMap g;
  g.tiles_m = (int)cdiv(d->M, 256);
  g.tiles_n = (int)(d->N / 128);
  g.splits = 1;
  g.k_per_split = d->K;
  const unsigned nblk = (unsigned)((int64_t)g.tiles_m * g.tiles_n);
  with_epilogue(e.flags, [&](auto ef) {
    with_layout(d->b_kcontig, [&](auto bkc) {
      hipLaunchKernelGGL((gemm_bf16_big_kernel<decltype(bkc)::value, decltype(ef)::value>), dim3(nblk), dim3(512), 0, s, a,
                         d->lda, b, d->ldb, d->K, g, e);
    });
  });
  VS_LAUNCH_CHECK();
  return VS_OK;
}

// ----------------------------------------------------------------------------------------------
// host: the 256 x 256 persistent kernel
// ----------------------------------------------------------------------------------------------
// 256 x 256 persistent path: long-M ViT-Base block products (N % 256 == 0, K % 64 == 0, rows
// and leading dims addressable with 32-bit per-lane DMA offsets)
bool g256_ok(const vs_gemm_desc* d, const EpiParams& e) {
  const uint32_t f = e.flags;
  // the kernel: the seven compile-time epilogues (it has no all-runtime one), bf16 operands and aux, K-contiguous A,
  // whole 256-column tiles, at least 4 whole 64-deep stages, one pass (no split, no row sums, no atomics),
  // 16-B epilogue accesses, a tile's rows of A and the whole of B within 32-bit per-lane DMA offsets
  const bool g256_ef = f == 0 || f == VS_EPI_BIAS || f == (VS_EPI_BIAS | VS_EPI_RESIDUAL) ||
                       f == (VS_EPI_BIAS | VS_EPI_GELU) || f == VS_EPI_GELU_BWD ||
                       f == (VS_EPI_BIAS | VS_EPI_GELU | VS_EPI_GELU_GRAD) || f == VS_EPI_MUL_AUX;
  const bool can = g256_ef && d->dtype == VS_BF16 && e.op_bf16 && d->a_kcontig && d->N % 256 == 0 && d->K >= 256 &&
                   d->K % 64 == 0 && d->split_k <= 1 && !d->a_rowsum && e.vec_ok && d->ldc % 4 == 0 &&
                   !(f & (VS_EPI_ATOMIC)) && 256 * d->lda * 2 < (1ll << 31) &&
                   (d->b_kcontig ? d->N * d->ldb : d->K * d->ldb) * 2 < (1ll << 31);
  // measured per C3 product: the 256 x 256 kernel wins where N or K >= 2304 and
  // on the bf16-output dX products (fc2's GELU' product, proj); the 768 x 768 forward proj stays on the
  // 256 x 128 tile.  Long M: one persistent workgroup per CU needs tiles to deal.
  const bool measured = (d->N >= 2304 || d->K >= 2304) || (!d->b_kcontig && e.out_bf16);
  // knob: VSPIKE_G256 = 1 takes every shape the kernel can, 0 (default) the measured ones, else none
  const int g256k = knob(VS_KNOB_G256);
  const bool pick = g256k == 1 || (g256k == 0 && measured);
  return can && d->M >= 16384 && pick;
}

template <uint32_t EF>
static void launch_g256_ef(const vs_gemm_desc* d, const G256Map& g, unsigned grid, const EpiParams& e, hipStream_t s) {
  const bf16_t* a = (const bf16_t*)d->a;
  const bf16_t* b = (const bf16_t*)d->b;
  // P8 (8-column epilogue vectors): always with K-contiguous B; with N-contiguous B only for bf16
  // outputs (its transposed B reads conflict 2-way, which the f32 outputs' 16-B quads do not repay:
  // dX fc2 1,603 -> 1,463 us, dX proj 310 -> 281; dX fc1 989 -> 1,011)
  G256Map gm = g;
  auto go = [&](auto kern) {
    // the early-DMA wait counts the epilogue's stores exactly (`est`); an instance that spills to scratch
    // issues more vector-memory ops than that, so it falls back to vmcnt(0) (checked once per instance)
    static const int ok = [&] {
      hipFuncAttributes fa{};
      return hipFuncGetAttributes(&fa, (const void*)kern) == hipSuccess && fa.localSizeBytes == 0 ? 1 : 0;
    }();
    gm.ed_ok = ok;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(512), 0, s, a, d->lda, b, d->ldb, gm, e);
  };
  if (d->b_kcontig)
    go(gemm_bf16_g256_kernel<true, true, EF>);
  else if (e.out_bf16)
    go(gemm_bf16_g256_kernel<false, true, EF>);
  else
    go(gemm_bf16_g256_kernel<false, false, EF>);
}

int launch_g256(const vs_gemm_desc* d, const EpiParams& e, hipStream_t s) {
  G256Map g;
  g.tiles_n = (int)(d->N / 256);
  g.tiles = (int)(cdiv(d->M, 256) * g.tiles_n);
  g.nk = (int)(d->K / 64);
  const int gcap = knob(VS_KNOB_G256_GRID) > 0 ? knob(VS_KNOB_G256_GRID) : 256;
  int grid = g.tiles < gcap ? (g.tiles + 7) / 8 * 8 : gcap;
  grid = grid < 8 ? 8 : grid / 8 * 8;
  g.per_xcd = (int)cdiv(g.tiles, 8);
#ifdef VS_DEBUG_KNOBS
  g.dbg = knob(VS_KNOB_G256_DBG);
#else
  g.dbg = 0;
#endif
  g.stagger = knob(VS_KNOB_G256_STAGGER);
  g.ed_ok = 1;  // launch_g256_ef clears it for an instance with a private segment
  g.a3 = knob(VS_KNOB_G256_A3) != 2;  // default on (round 6: every forward / dX product faster)
  // g256_ok admits the seven compile-time epilogues only: the default case is never taken, but keeps
  // the all-runtime instances compiled
  with_epilogue(e.flags, [&](auto ef) { launch_g256_ef<decltype(ef)::value>(d, g, (unsigned)grid, e, s); });
  VS_LAUNCH_CHECK();
  return VS_OK;
}

// G256 early-DMA guard, for tests: 1 when every compiled 256 x 256 forward / dX instance has no private
// segment (the counted vmcnt of the early DMA is then exact), else 0
template <bool BKC, bool P8>
static int g256_no_scratch_all() {
  int ok = 1;
#define CHK_(EF)                                                                                    \
  {                                                                                                 \
    hipFuncAttributes fa{};                                                                          \
    if (hipFuncGetAttributes(&fa, (const void*)gemm_bf16_g256_kernel<BKC, P8, EF>) != hipSuccess || \
        fa.localSizeBytes != 0)                                                                     \
      ok = 0;                                                                                       \
  }
  CHK_(0u) CHK_((uint32_t)VS_EPI_BIAS) CHK_((uint32_t)(VS_EPI_BIAS | VS_EPI_RESIDUAL))
  CHK_((uint32_t)(VS_EPI_BIAS | VS_EPI_GELU)) CHK_((uint32_t)VS_EPI_GELU_BWD)
  CHK_((uint32_t)(VS_EPI_BIAS | VS_EPI_GELU | VS_EPI_GELU_GRAD)) CHK_((uint32_t)VS_EPI_MUL_AUX)
#undef CHK_
  return ok;
}

}  // namespace vs

extern "C" int vs_g256_scratch_free(void) {
  using namespace vs;
  return g256_no_scratch_all<true, true>() & g256_no_scratch_all<false, true>() & g256_no_scratch_all<false, false>();
}
