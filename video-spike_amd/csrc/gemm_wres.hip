// gemm_wres.hip — vs_gemm's W-resident kernel for the wide K = 192 products (gemm.hip has the overview).
#include <initializer_list>

#include "common.h"
#include "gemm_common.h"
#include "gemm_paths.h"

namespace vs {

// ----------------------------------------------------------------------------------------------
// bf16 W-resident kernel for the wide K = 192 products of the ViT block: qkv (N = 576), fc1 + GELU
// (N = 768, two bf16 outputs) and the GELU' dX product da = (dx' W2) * gelu'(a_pre) (N = 768).
// Outputs are 3-4x the input, so the bound is the output stream; the per-tile kernels re-read
// their A tile once per 64-column tile and spend a barrier per tile.  Here:
//   * the N columns are cut in parts of 192; a workgroup copies its part of W (192 x 192 bf16,
//     76.8 KB with padded rows) into LDS ONCE and keeps it for its whole row range (2 workgroups
//     per CU, persistent: grid = 512, workgroup = (row range, part), XCD-grouped so the parts of
//     a range share an L2);
//   * no barrier after the fill: each wave walks its own (16-token block, 64-column chunk) units;
//     the token block's operand rows come straight from HBM as MFMA B fragments (8 consecutive k of
//     one token per lane: the K-contiguous layout), loaded once per block;
//   * the product is computed transposed, C^T = W X^T (W rows as the MFMA A operand), with the W
//     rows permuted in LDS so that a lane's two accumulator quads are 8 CONSECUTIVE output columns
//     of one token: the epilogue (bias, GELU / GELU', bf16 casts) runs on registers and writes
//     16-B vectors, no staging.  The GELU' operand of a chunk is loaded before its MFMAs.
// ----------------------------------------------------------------------------------------------
constexpr int kWresNH = 192;                  // columns per part
// LDS bytes per W row: K = 192 plus 32 B.  A ds_read_b128 of the MFMA A fragment (row = lane & 15,
// 16-B chunk 4 ks + lane / 16) is serviced in four 16-lane groups; a row stride of 104 dwords puts the
// 16 chunks of every group on distinct 4-bank quads (the 400-B stride collided in half of them:
// SQ_LDS_BANK_CONFLICT 46 % of the LDS cycles at 128 clips).  2 x (192 x 416 + 768) B fits 160 KiB.
constexpr int kWresRow = 192 * 2 + 32;

// LDS row of part-local column n: chunk ch = n / 64; within it MFMA tile jj = 2 (r / 32) + (r % 8) / 4
// and tile row i = 4 ((r % 32) / 8) + r % 4 (r = n % 64), so that accumulator rows 4g..4g+3 of
// tiles 2p and 2p+1 are the columns 32p + 8g .. 32p + 8g + 7 of the chunk.
__device__ __forceinline__ int wres_lds_row(int n) {
  const int ch = n >> 6, r = n & 63, p = r >> 5, q = r & 31;
  return ch * 64 + (2 * p + ((q >> 2) & 1)) * 16 + 4 * (q >> 3) + (q & 3);
}

template <bool BKC, uint32_t EF, int WV = 4>
__global__ __launch_bounds__(64 * WV, 2) void gemm_bf16_wres_kernel(const bf16_t* __restrict__ A, int64_t lda,
                                                                const bf16_t* __restrict__ B, int64_t ldb,
                                                                EpiParams e, int dbg) {
  constexpr int K = 192, KS = K / 32, NCH = kWresNH / 64;
  constexpr bool MULA = (EF & VS_EPI_MUL_AUX) != 0;             // v *= aux (the stored gelu')
  constexpr bool GBWD = (EF & VS_EPI_GELU_BWD) != 0 || MULA;    // an aux operand per output
  __shared__ __attribute__((aligned(16))) char wl[kWresNH * kWresRow];
  __shared__ __attribute__((aligned(16))) float bl[kWresNH];
  // wave-uniform work bounds (readfirstlane): the block and chunk loops run on scalar counters
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int parts = (int)(e.N / kWresNH);
  const int G = gridDim.x, ranges = G / parts;
  const int logical = xcd_remap(blockIdx.x, G);
  const int part = logical % parts, range = logical / parts;
  if (range >= ranges) return;  // workgroup-uniform (at most parts - 1 idle workgroups)
  const int64_t r_begin = (int64_t)range * e.M / ranges, r_end = ((int64_t)range + 1) * e.M / ranges;
  const int64_t n_part = (int64_t)part * kWresNH;

  // ---- W part -> LDS (permuted rows), once: every thread issues all 18 of its 16-B loads before
  // its first LDS write (a load -> write chain per chunk serialises 18 HBM latencies)
  constexpr int NTH = 64 * WV;
  constexpr int FILL = kWresNH * K / 8 / NTH;  // 16-B chunks per thread
  static_assert(FILL * NTH * 8 == kWresNH * K, "fill split");
  uint4 fv[FILL];
  if constexpr (BKC) {  // W[n][k]: 24 16-B chunks per row
#pragma unroll
    for (int i = 0; i < FILL; ++i) {
      const int c = tid + NTH * i, n = c / (K / 8), kc = c % (K / 8);
      fv[i] = *(const uint4*)(B + (n_part + n) * ldb + kc * 8);
    }
#pragma unroll
    for (int i = 0; i < FILL; ++i) {
      const int c = tid + NTH * i, n = c / (K / 8), kc = c % (K / 8);
      *(uint4*)(wl + wres_lds_row(n) * kWresRow + kc * 16) = fv[i];
    }
  } else {  // W[k][n] (N-contiguous): 8 columns per 16-B load, scattered into 8 LDS rows
#pragma unroll
    for (int i = 0; i < FILL; ++i) {
      const int c = tid + NTH * i, k = c / (kWresNH / 8), nc = c % (kWresNH / 8);
      fv[i] = *(const uint4*)(B + (int64_t)k * ldb + n_part + nc * 8);
    }
#pragma unroll
    for (int i = 0; i < FILL; ++i) {
      const int c = tid + NTH * i, k = c / (kWresNH / 8), nc = c % (kWresNH / 8);
      const uint32_t w[4] = {fv[i].x, fv[i].y, fv[i].z, fv[i].w};
#pragma unroll
      for (int t = 0; t < 8; ++t)
        *(uint16_t*)(wl + wres_lds_row(nc * 8 + t) * kWresRow + k * 2) = (uint16_t)(w[t >> 1] >> (16 * (t & 1)));
    }
  }
  // the part's bias in LDS: the epilogue then issues no global load behind its own stores (on CDNA4
  // vmcnt counts stores too, so a load after the previous unit's stores would wait for all of them)
  if constexpr ((EF & VS_EPI_BIAS) != 0) {
    if (tid < kWresNH) bl[tid] = e.bias[n_part + tid];
  }
  __syncthreads();

  // ---- this wave's 16-token blocks (all NCH 64-column chunks of each); the next block's operand
  // rows are loaded while this block's chunks run
  const int64_t rows = r_end - r_begin;
  const int tb_n = (int)((rows + 15) / 16);
  const int tb0 = wid * tb_n / WV, tb1 = (wid + 1) * tb_n / WV - 1;
  const int g = lane >> 4, tok = lane & 15;
  const char* wbase = wl + tok * kWresRow + g * 16;  // + (tile row block) * kWresRow, + ks * 64
  if (tb0 > tb1) return;
  // Every global access goes through a buffer descriptor whose base is the token block's first row
  // (wave-uniform: the per-block address arithmetic is scalar) and whose extent ends at r_end: loads
  // of rows past the range return 0 and their stores are dropped by the range check, so no lane
  // predicate or branch remains, and hipcc sees one fixed sequence of loads and stores per block
  // (counted vmcnt waits).  Per lane only constant 32-bit offsets (+ immediates).  The host keeps
  // M x ld x 2 bytes below 2^31 for every operand.
  const uint32_t xoff = (uint32_t)(tok * lda + 8 * g) * 2u;
  const uint32_t coff = (uint32_t)(tok * e.ldc + n_part + 8 * g) * 2u;
  const uint32_t aooff = (uint32_t)(tok * e.ld_aux_out + n_part + 8 * g) * 2u;
  const uint32_t aioff = (uint32_t)(tok * e.ld_aux_in + n_part + 8 * g) * 2u;
  auto rsrc = [&](const void* base, int64_t row0, int64_t ld, bool live = true) {
    // a dead block (or one starting past the range): an empty descriptor, loads give 0, stores dropped
    const int64_t left = live && r_end > row0 ? r_end - row0 : 0;
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, (int)(left * ld * 2), 0x00020000);
  };
  // x fragments held as 32-bit vectors (bf16 vector copies were re-packed lane half by lane half)
  auto load_x = [&](int tb, u32x4v (&dst)[KS]) {
    const int64_t row0 = r_begin + (int64_t)(dbg & 2 ? 0 : tb) * 16;  // dbg & 2 (timing): L2-resident reads
    const auto rx = rsrc(A + row0 * lda, row0, lda);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) dst[ks] = __builtin_amdgcn_raw_buffer_load_b128(rx, xoff + 64 * ks, 0, 0);
  };
  auto pack8 = [](const float (&v)[8]) {
    u32x4v u;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      u[q] = __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2){v[2 * q], v[2 * q + 1]}, bf16x2v));
    return u;
  };
  // three fragment sets, prefetch two token blocks ahead (one block of MFMA work, ~0.5 us, hid too
  // little of the loaded HBM latency), the loop unrolled by three blocks: no register copies
  u32x4v xa[KS], xb[KS], xc[KS];
  load_x(tb0, xa);
  load_x(tb0 < tb1 ? tb0 + 1 : tb1, xb);
  auto block = [&](int tb, const u32x4v (&xf)[KS], u32x4v (&xn)[KS], bool live) {
    // compiler barrier: the W fragment reads are loop-invariant, and hoisted out of the block loop
    // they need 288 VGPRs (spills); re-read per block from LDS instead
    asm volatile("" ::: "memory");
    // unconditional (the last block re-loads itself): with a conditional prefetch the path without
    // it made hipcc wait vmcnt(0) for this block's fragments, i.e. for the prefetch just issued too
    load_x(tb + 2 <= tb1 ? tb + 2 : tb1, xn);
    __builtin_amdgcn_sched_barrier(0);  // the prefetch goes out first, ahead of this block's work
    const int64_t row0 = r_begin + (int64_t)tb * 16;
    // dbg & 1 (timing only): every block's stores rewrite the range's first two blocks (L2-resident)
    const int64_t srow0 = dbg & 1 ? r_begin + (int64_t)(tb & 1) * 16 : row0;
    const auto rc = rsrc((const bf16_t*)e.c + srow0 * e.ldc, srow0, e.ldc, live);
    const auto rao = rsrc((const bf16_t*)e.aux_out + srow0 * e.ld_aux_out, srow0, e.ld_aux_out, live);
    const auto rai = rsrc((const bf16_t*)e.aux_in + row0 * e.ld_aux_in, row0, e.ld_aux_in);
    // GELU' operand: chunk c + 1's is loaded before chunk c's stores (a counted wait then skips them)
    u32x4v aux[2][2];
    auto load_aux = [&](int ch, u32x4v (&dst)[2]) {
      if constexpr (GBWD) {
#pragma unroll
        for (int p = 0; p < 2; ++p) dst[p] = __builtin_amdgcn_raw_buffer_load_b128(rai, aioff + 2 * (ch * 64 + 32 * p), 0, 0);
      }
    };
    auto chunk = [&](int ch, u32x4v (&ax)[2], u32x4v (&axn)[2]) {
      if (ch + 1 < NCH) load_aux(ch + 1, axn);
      f32x4 acc[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        bf16x8 wf[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) wf[j] = *(const bf16x8*)(wbase + (ch * 64 + j * 16) * kWresRow + ks * 64);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], __builtin_bit_cast(bf16x8, xf[ks]), acc[j], 0, 0, 0);
      }
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        // this lane's 8 columns: n_part + ch * 64 + 32 p + 8 g .. + 7 of token row row0 + tok
        const uint32_t cb = 2 * (ch * 64 + 32 * p);
        float v[8];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          v[r] = acc[2 * p][r] * e.alpha;
          v[4 + r] = acc[2 * p + 1][r] * e.alpha;
        }
        if constexpr (GBWD) {
          const u32x4v w = ax[p];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const float lo = __uint_as_float(w[q] << 16), hi = __uint_as_float(w[q] & 0xffff0000u);
            v[2 * q] *= MULA ? lo : gelu_fast_grad(lo);
            v[2 * q + 1] *= MULA ? hi : gelu_fast_grad(hi);
          }
        } else {
          if constexpr ((EF & VS_EPI_BIAS) != 0) {
            const float4 b0 = *(const float4*)&bl[ch * 64 + 32 * p + 8 * g];
            const float4 b1 = *(const float4*)&bl[ch * 64 + 32 * p + 8 * g + 4];
            v[0] += b0.x; v[1] += b0.y; v[2] += b0.z; v[3] += b0.w;
            v[4] += b1.x; v[5] += b1.y; v[6] += b1.z; v[7] += b1.w;
          }
          if constexpr ((EF & VS_EPI_GELU) != 0 && (EF & VS_EPI_GELU_GRAD) != 0) {
            float gr[8];  // gelu' of the bf16-rounded pre-activation: what the backward multiplies by
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = gelu_fast_both(bf2f(f2bf(v[k])), gr[k]);
            __builtin_amdgcn_raw_buffer_store_b128(pack8(gr), rao, aooff + cb, 0, 0);
          } else if constexpr ((EF & VS_EPI_GELU) != 0) {
            __builtin_amdgcn_raw_buffer_store_b128(pack8(v), rao, aooff + cb, 0, 0);
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = gelu_fast(bf2f(f2bf(v[k])));  // GELU of the stored value
          }
        }
        __builtin_amdgcn_raw_buffer_store_b128(pack8(v), rc, coff + cb, 0, 0);
      }
    };
    // the chunks unrolled and unconditional (no inner loop: hipcc waits vmcnt(0) before a loop that
    // reads a pending load, i.e. for the next block's prefetch too), so every block issues the same
    // loads and stores and the waits before its MFMAs count past the previous block's stores
    load_aux(0, aux[0]);
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) chunk(ch, aux[ch & 1], aux[(ch + 1) & 1]);
  };
  // The first block peeled (every entry into the loop then follows a block's stores), then triples
  // of blocks, all unconditional: a conditional block let hipcc sink the previous blocks' prefetch
  // into it (its only user), i.e. issue it right before its use.  A count that is not a multiple of
  // three ends with dead blocks (their stores dropped by an empty descriptor).
  block(tb0, xa, xc, true);
  for (int tb = tb0 + 1; tb <= tb1; tb += 3) {
    block(tb, xb, xa, true);
    block(tb + 1, xc, xb, tb + 1 <= tb1);
    block(tb + 2, xa, xc, tb + 2 <= tb1);
  }
}

// ----------------------------------------------------------------------------------------------
// host
// ----------------------------------------------------------------------------------------------
// the W-resident kernel addresses every operand through 32-bit buffer descriptors
static inline bool wres_extent_ok(int64_t M, std::initializer_list<int64_t> lds) {
  for (int64_t ld : lds)
    if (M * ld * 2 >= ((int64_t)1 << 31)) return false;
  return true;
}

// W-resident path: K = 192, N a multiple of 192 (>= 384): qkv, fc1 + GELU, the GELU' product
bool wres_ok(const vs_gemm_desc* d, const EpiParams& e) {
  const uint32_t f = e.flags;
  // the kernel: bf16 operands and outputs, K-contiguous A rows of K = 192 read as 16-B fragments, N
  // in parts of 192 columns (at least two, at most 64 over the 512-workgroup grid), one pass (no split,
  // no row sums), 16-B rows and epilogue accesses, every operand within a 32-bit buffer descriptor
  const bool can = e.op_bf16 && e.out_bf16 && d->dtype == VS_BF16 && d->a_kcontig && d->K == 192 && d->N % kWresNH == 0 &&
                   d->N >= 2 * kWresNH && d->N <= 64 * kWresNH && d->split_k <= 1 && !d->a_rowsum && e.vec_ok &&
                   d->lda % 8 == 0 && d->ldb % 8 == 0 && aligned16(d->a) && aligned16(d->b) &&
                   wres_extent_ok(d->M, {d->lda, d->ldc, e.aux_out ? e.ld_aux_out : 0, e.aux_in ? e.ld_aux_in : 0});
  // the GELU' product (GELU_BWD, or MUL_AUX on the stored gelu') stays on the wide row-slab kernel
  // unless VSPIKE_WRES_GBWD=1: 35.7 vs 41.2 us (GELU_BWD), 27.8 vs 32.6 us (MUL_AUX) there — its
  // operand stream (a 16-B aux read per 8 outputs) overlaps better with the row-slab schedule.
  // Large M: the persistent grid's row ranges.
  const bool gbwd = knob(VS_KNOB_WRES_GBWD) != 0;
  const bool pick = d->M >= 8192 &&
                    (f == VS_EPI_BIAS || f == (VS_EPI_BIAS | VS_EPI_GELU) || f == 0 ||
                     f == (VS_EPI_BIAS | VS_EPI_GELU | VS_EPI_GELU_GRAD) ||
                     (gbwd && (f == VS_EPI_GELU_BWD || f == VS_EPI_MUL_AUX)));
  // knob: VSPIKE_NO_WRES
  return can && pick && knob(VS_KNOB_NO_WRES) == 0;
}

template <uint32_t EF>
static void launch_wres_ef(const vs_gemm_desc* d, const EpiParams& e, hipStream_t s) {
  const bf16_t* a = (const bf16_t*)d->a;
  const bf16_t* b = (const bf16_t*)d->b;
  // VSPIKE_WRES_WV=8: 8 waves per workgroup (16 per CU sharing 2 W parts; the GELU' / aux-product
  // instantiations need > 128 VGPRs, so one workgroup per CU there).  Measured at 128 clips: qkv
  // 94.3 -> 95.2 us, fc1 + GELU 216 -> 225 us (more waves do not raise the store-bound rate): 4 waves.
  const bool wide = knob(VS_KNOB_WRES_WV) == 8;
  void (*kern)(const bf16_t*, int64_t, const bf16_t*, int64_t, EpiParams, int);
  if (d->b_kcontig) kern = wide ? gemm_bf16_wres_kernel<true, EF, 8> : gemm_bf16_wres_kernel<true, EF, 4>;
  else kern = wide ? gemm_bf16_wres_kernel<false, EF, 8> : gemm_bf16_wres_kernel<false, EF, 4>;
#ifdef VS_DEBUG_KNOBS
  // diagnostic builds only: VS_KNOB_WRES_DBG makes the kernel re-read / re-write L2-resident blocks
  // (timing isolation; the results are WRONG)
  const int dbg = knob(VS_KNOB_WRES_DBG);
#else
  const int dbg = 0;
#endif
  hipLaunchKernelGGL(kern, dim3(512), dim3(wide ? 512 : 256), 0, s, a, d->lda, b, d->ldb, e, dbg);
}

int launch_wres(const vs_gemm_desc* d, const EpiParams& e, hipStream_t s) {
  const uint32_t f = e.flags;  // one of the six epilogues the kernel is instantiated for
  if (f == VS_EPI_BIAS) launch_wres_ef<(uint32_t)VS_EPI_BIAS>(d, e, s);
  else if (f == (VS_EPI_BIAS | VS_EPI_GELU)) launch_wres_ef<(uint32_t)(VS_EPI_BIAS | VS_EPI_GELU)>(d, e, s);
  else if (f == 0) launch_wres_ef<0u>(d, e, s);
  else if (f == (VS_EPI_BIAS | VS_EPI_GELU | VS_EPI_GELU_GRAD))
    launch_wres_ef<(uint32_t)(VS_EPI_BIAS | VS_EPI_GELU | VS_EPI_GELU_GRAD)>(d, e, s);
  else if (f == VS_EPI_MUL_AUX) launch_wres_ef<(uint32_t)VS_EPI_MUL_AUX>(d, e, s);
  else launch_wres_ef<(uint32_t)VS_EPI_GELU_BWD>(d, e, s);
  VS_LAUNCH_CHECK();
  return VS_OK;
}

}  // namespace vs
