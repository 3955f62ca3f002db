// attn_fwd.hip — the bf16 MFMA forward kernels of head-dim-64 attention and the entry vs_attn_fwd
// (attn_common.h has the overview).
#include "attn_common.h"

namespace vs {

// Per 64-key tile and wave (32 queries): 8 MFMAs for S^T = K (c Q)^T and 8 for O^T += V^T P^T.
// VALU per score is minimised:
//   * Q is pre-scaled by c = log2(e)/sqrt(64) when loaded, so the accumulator IS log2(p):
//     p = v_exp_f32(acc) with no per-score FMA;
//   * the fast pass has no running maximum at all; the safe pass raises its reference lazily (only
//     when a lane's scores exceed it by 2^kRefBand, guide T13): the O/l rescale is a wave-uniform
//     branch that is skipped in steady state;
//   * max via v_max3 (asm: hipcc canonicalises fmaxf operands), xor-32 exchange via
//     v_permlane32_swap (no LDS), staging loads unconditional (clamped row + select);
//   * the tile loop is unrolled over the two LDS buffers so every LDS address is a per-lane base
//     plus an immediate offset.
// Softmax VALU of sub-block j overlaps the MFMAs of sub-block j+1 (issue order QK1, SM0, PV0,
// SM1, PV1).
constexpr float kRefBand = 32.0f;  // forward: p <= 2^32 relative to the reference (f32/bf16-safe)

#ifdef VS_STAMP
// Diagnostic build only (-DVS_STAMP): per wave {start, end} realtime ticks (100 MHz), HW ids, and
// shader-clock cycles accumulated in the forward's barrier and vmcnt waits; read back with
// vs_dbg_stamps().  Not part of the product library.
__device__ unsigned long long g_stamp[8 * 8192];
__device__ __forceinline__ void stamp(int slot, bool end) {
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if ((threadIdx.x & 63) == 0 && w < 8192) {
    const unsigned long long t = __builtin_amdgcn_s_memrealtime();
    if (!end) {
      g_stamp[8 * w] = t;
      g_stamp[8 * w + 2] = __builtin_amdgcn_s_getreg((31 << 11) | 4);   // HW_ID
      g_stamp[8 * w + 3] = __builtin_amdgcn_s_getreg((31 << 11) | 20);  // XCC_ID
    } else {
      g_stamp[8 * w + 1] = t;
    }
  }
  (void)slot;
}
__device__ __forceinline__ void stamp_acc(int slot, unsigned long long v) {
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if ((threadIdx.x & 63) == 0 && w < 8192) g_stamp[8 * w + slot] = v;
}
#define VS_CLK() __builtin_amdgcn_s_memtime()
#define VS_STAMP_AT(end) stamp(0, end)
#else
#define VS_STAMP_AT(end)
#define VS_CLK() 0ull
#endif

// Row sums of P on the matrix pipe.  For v_mfma_f32_16x16x32_bf16 with P's packed half (pa or pb,
// this lane's 8 keys of query lane&31) as the B operand, column n = lane&15 collects lanes n, n+16,
// n+32, n+48 = queries n, n+16, n, n+16 in k-slot groups g = lane>>4 = 0..3.  The constant A
// operand `sel` has row 0 = ones over groups {0, 2} and row 1 = ones over groups {1, 3}, so row 0
// of the product is query n's sum over the block's keys and row 1 query n+16's.  Two 16-cycle
// MFMAs per 32-key block replace 15 v_add_f32 per lane (60 VALU issue cycles).
__device__ __forceinline__ bf16x8 rowsum_selector(int lane) {
  const int row = lane & 15, g = lane >> 4;
  const float one = (row == 0 && (g & 1) == 0) || (row == 1 && (g & 1) == 1) ? 1.f : 0.f;
  const f32x8 v = {one, one, one, one, one, one, one, one};
  return __builtin_convertvector(v, bf16x8);
}

// workgroups of the bf16 forward that re-ran their tile under the safe softmax (a query's scores
// left the fast pass's band): read / reset by vs_attn_redo_count
__device__ unsigned long long g_attn_redo = 0;

// ---- what the 32x32x16 and the 16x16x32 forward share ------------------------------------------
constexpr int kFwdTile = 64 * 128;  // bytes of one 64-key x 64-dh bf16 tile; a stage is K then V

// the V image's swizzle: swz_half for the 32x32x16 kernels; the 16x16x32 kernel's 16 rows x 32 B per
// tr read cover the 64 banks twice under 16-B chunk ^ 2((row >> 1) & 3)
__device__ __forceinline__ int swz_v16(int r) { return ((r >> 1) & 3) << 1; }
struct VSwzHalf {
  static __device__ __forceinline__ int swz(int r) { return swz_half(r); }
};
struct VSwz16 {
  static __device__ __forceinline__ int swz(int r) { return swz_v16(r); }
};

// K/V tiles arrive by LDS-DMA (global_load_lds_dwordx4): one wave-instruction fills a 1-KiB
// piece = 8 rows x 128 B, lane L writing position L*16.  The LDS images keep their XOR swizzles
// (K: swz_row, V: VSwz) because each lane loads the SOURCE chunk that belongs at its position:
// (L&7) ^ swz(row).  Wave w fills K pieces 2w, 2w+1 and V pieces 2w, 2w+1.  The asm DMA (SGPR tile
// base + per-lane offset) is invisible to hipcc's waitcnt insertion, which would otherwise drain the
// in-flight tile before LDS reads of the other stage; ordering is the loop's explicit vmcnt(0) +
// barrier.
template <class VSwz>
struct FwdTileLoader {
  const char* kp;
  int64_t ldq, tile_bytes, vdelta;
  int N, wid, prow0, ppos;  // this lane's rows prow0 and prow0 + 8 of a tile
  uint32_t gk0, gk1, gv0, gv1;
  __device__ __forceinline__ FwdTileLoader(const bf16_t* Kp, int64_t ldq_, int D, int N_, int wid_, int lane)
      : kp((const char*)Kp), ldq(ldq_), tile_bytes(64 * 2 * ldq_), vdelta(2 * (int64_t)D), N(N_), wid(wid_),
        prow0(wid_ * 16 + (lane >> 3)), ppos(lane & 7) {
    gk0 = (uint32_t)(prow0 * 2 * ldq + ((ppos ^ swz_row(prow0)) << 4));
    gk1 = (uint32_t)((prow0 + 8) * 2 * ldq + ((ppos ^ swz_row(prow0 + 8)) << 4));
    gv0 = (uint32_t)(prow0 * 2 * ldq + ((ppos ^ VSwz::swz(prow0)) << 4));
    gv1 = (uint32_t)((prow0 + 8) * 2 * ldq + ((ppos ^ VSwz::swz(prow0 + 8)) << 4));
  }
  __device__ __forceinline__ void operator()(int kt, char* buf) const {
    const char* kb = kp + kt * tile_bytes;
    const char* vb = kb + vdelta;
    char* dk = buf + wid * 2048;
    char* dv = buf + kFwdTile + wid * 2048;
    if ((kt + 1) * 64 <= N) {
      glds16_asm_so(kb, gk0, dk);
      glds16_asm_so(kb, gk1, dk + 1024);
      glds16_asm_so(vb, gv0, dv);
      glds16_asm_so(vb, gv1, dv + 1024);
    } else {  // partial last tile: rows past N re-read row N-1 (finite data; its scores are masked)
      const int r0 = kt * 64 + prow0, r1 = r0 + 8;
      const uint32_t c0 = (uint32_t)((r0 < N ? r0 : N - 1) - kt * 64) * (uint32_t)(2 * ldq);
      const uint32_t c1 = (uint32_t)((r1 < N ? r1 : N - 1) - kt * 64) * (uint32_t)(2 * ldq);
      glds16_asm_so(kb, c0 + ((ppos ^ swz_row(prow0)) << 4), dk);
      glds16_asm_so(kb, c1 + ((ppos ^ swz_row(prow0 + 8)) << 4), dk + 1024);
      glds16_asm_so(vb, c0 + ((ppos ^ VSwz::swz(prow0)) << 4), dv);
      glds16_asm_so(vb, c1 + ((ppos ^ VSwz::swz(prow0 + 8)) << 4), dv + 1024);
    }
  }
};

// Fast-pass validity of one query: its row sum l within [2^-100, 2^96] (false for NaN/inf) and its O
// accumulators finite (ofin).  p = exp2(s) is a normal bf16 / f32 number from 2^-126 to 2^127, so
// the band only guards the sums: l <= 2^96 keeps every p and the O sums (<= l * max|v|) finite for
// |v| < 2^31, and l >= 2^-100 keeps the largest p normal.  (Round 4's [2^-60, 2^60] re-ran every
// workgroup with a score above ~41 natural-log units: 1.9-2.2x the forward's time, which
// pretrained attention sinks reach; profiles/r05_attn_logit_scale.txt.)  (Arguments by reference: by
// value, the 16x16x32 kernel spills a fifth VGPR.)
__device__ __forceinline__ bool fast_pass_ok(const float& l, const bool& ofin) {
  return l >= 0x1p-100f && l <= 0x1p96f && ofin;
}

// The redo vote.  `bad`: this lane holds a real query that failed fast_pass_ok.  Returns (workgroup-
// uniform) whether any did: the whole workgroup then streams K/V again under the safe softmax.
// redo_flag was zeroed by thread 0 before the fast pass.
__device__ __forceinline__ bool fwd_redo_vote(bool bad, int& redo_flag) {
  __syncthreads();  // every wave is done with the last K/V tile; redo_flag = 0 is visible
  if (__any(bad) && (threadIdx.x & 63) == 0) redo_flag = 1;
  __syncthreads();
  if (!redo_flag) return false;
  if (threadIdx.x == 0) atomicAdd(&g_attn_redo, 1ull);
  return true;
}

// Epilogue: O^T accumulators -> normalised bf16 rows staged through LDS (wave-private 4 KB of the K/V
// stages, XOR-swizzled 16-B chunks), then written as whole 128-B rows (8 lanes per row).
__device__ __forceinline__ char* fwd_o_stage(char* smem0, char* smem1, int wid) {
  return (wid < 2 ? smem0 : smem1) + (wid & 1) * 4096;
}
// four consecutive dims of the wave's query q: 8-B half `half` of 16-B chunk `chunk`
__device__ __forceinline__ void fwd_o_put4(char* so, int q, int chunk, int half, float a, float b, float c, float d) {
  *(uint2*)(so + q * 128 + ((chunk ^ (q & 7)) << 4) + 8 * half) = pack4(a, b, c, d);
}
// rows of the wave's queries q0w .. q0w + 31 of head h (row0: the batch element's first row of o)
__device__ __forceinline__ void fwd_o_store(const char* so, bf16_t* __restrict__ o, int64_t ldo, int64_t row0, int h,
                                            int q0w, int N, int lane) {
  __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): this wave's LDS writes landed (wave-private)
#pragma unroll
  for (int pss = 0; pss < 4; ++pss) {
    const int r = pss * 8 + (lane >> 3), ch = lane & 7;
    const uint4 v = *(const uint4*)(so + r * 128 + ((ch ^ (r & 7)) << 4));
    if (q0w + r < N) *(uint4*)(o + (row0 + q0w + r) * ldo + h * 64 + ch * 8) = v;
  }
}

// ------------------------------------------------------------------ forward on 32x32x16 MFMAs
// ORD: the order of a 64-key tile's work (blocks a = keys 0..31, b = 32..63)
//   0: QK(a), softmax(a), PV(a), QK(b), softmax(b), PV(b)                (round 2)
//   1: QK(b) issued before PV(a), so softmax(b) waits on a chain that ran under PV(a)'s MFMAs (round 3)
//   2: software-pipelined across tiles: every softmax runs under the NEXT block's QK MFMAs, including
//      softmax(b) under QK(a) of tile kt + 1 (ORD 1 leaves softmax(b) with only its two row-sum
//      MFMAs to hide under): per tile  [QK(b) | softmax(a)] [PV(a) | V(b) reads] barrier
//      [QK(a') | softmax(b)] [PV(b) | V(a'), K(b') reads]  (round 6, VS_KNOB_ATTN_VARIANT 7).  Its two
//      blocks' live state needs ~206 VGPRs: 2 waves per SIMD, measured 9 % SLOWER than ORD 1's 3 waves
//      (at 3 waves / 168 VGPRs it spills 81); bitwise the same outputs
//   ORD 1 with the last tile peeled (no tail branch in the steady loop, so QK(b)'s MFMAs and softmax(a)
//   share one basic block) spilled 52 VGPRs at 168 and was dropped (round 6)
template <int ORD = 1>
__global__ __launch_bounds__(256, ORD == 2 ? 2 : 3) void attn_fwd_bf16_kernel(const bf16_t* __restrict__ qkv, int64_t ldq,
                                                               bf16_t* __restrict__ o, int64_t ldo,
                                                               float* __restrict__ lse, int N, int H,
                                                               float scale_log2) {
  constexpr int TILE = kFwdTile;
  // Two K/V stages as separate __shared__ objects (DMA into one while the other is read).
  __shared__ __attribute__((aligned(16))) char smem0[2 * TILE];
  __shared__ __attribute__((aligned(16))) char smem1[2 * TILE];
  __shared__ int redo_flag;
  VS_STAMP_AT(false);
  const int tid = threadIdx.x, lane = tid & 63, hh = lane >> 5;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const AttnBlock ab = attn_block(xcd_remap(blockIdx.x, gridDim.x), N, H);
  const int h = ab.h, b = ab.b;
  const int64_t row0 = ab.row0;
  const bf16_t* Qp = qkv + row0 * ldq + h * 64;
  const bf16_t* Kp = Qp + ab.D;
  const int q0w = ab.xb * 128 + wid * 32;  // this wave's first query
  const int qi = q0w + (lane & 31);
  if (tid == 0) redo_flag = 0;

  bf16x8 qf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int qr = qi < N ? qi : N - 1;
    qf[s] = scaled_frag(Qp + (int64_t)qr * ldq + 16 * s + 8 * hh, scale_log2);
  }
  const bf16x8 sel = rowsum_selector(lane);
  f32x16 oacc[2], zero16;
  f32x4 lacc;
  float m_run, l_half;

  // Per-lane LDS byte offsets, tile-invariant.  Every read is a lane base plus an immediate:
  //  K rows key = kb*32 + (lane&31): swz_row(key + 32) == swz_row(key), so kb adds 32*128 B;
  //  the 4 k-chunks XOR (2s+hh) into the swizzled chunk index -> one base per s.
  //  V^T reads rows k0 = kb*32 + 16s + 4hh + q4 (+8): swz_half(k0) depends on q4 bit 1 only, so
  //  kb/s/+8 are immediates and dt (64-B half) just selects one of two bases.
  const int q4 = (lane & 15) >> 2, p4 = (lane & 3) * 4, g16 = ((lane >> 4) & 1) * 16;
  int kbase[4];
  {
    const int key = lane & 31;
#pragma unroll
    for (int s = 0; s < 4; ++s) kbase[s] = key * 128 + (((2 * s + hh) ^ swz_row(key)) << 4);
  }
  int vbase[2];
  {
    const int k0 = 4 * hh + q4;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) vbase[dt] = TILE + off_halfswz(k0, dt * 32 + g16 + p4);
  }
  const FwdTileLoader<VSwzHalf> load_tile(Kp, ldq, ab.D, N, wid, lane);
  struct KFrag {
    bf16x8 k[4];
  };
  struct VFrag {
    bf16x8 v[4];
  };
  auto kread = [&](const char* base, int kb) {
    KFrag f;
#pragma unroll
    for (int s = 0; s < 4; ++s) f.k[s] = *(const bf16x8*)(base + kb * 4096 + kbase[s]);
    return f;
  };
  auto vread = [&](const char* base, int kb) {
    VFrag f;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        const char* vb = base + kb * 4096 + s * 2048;
        f.v[2 * s + dt] = tr_pair(vb, vbase[dt], vbase[dt] + 1024);
      }
    return f;
  };
  auto pv = [&](const VFrag& f, const bf16x8& pa, const bf16x8& pb) {
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
        oacc[dt] = mfma32p(f.v[2 * s + dt], s == 0 ? pa : pb, oacc[dt]);
  };

  // Softmax of one 32-key block.  acc = log2-domain scores s (Q pre-scaled by c; the MFMA chain
  // starts from 0).
  //  FAST pass (SAFE = 0): p = exp2(s) against a fixed reference 0 — no row maximum, no rescale,
  //    no per-score subtraction; row sums on the matrix pipe (lacc).  Exact whenever every query's
  //    scores stay within about [-100, 85] (log2 units); the epilogue checks the row sums and, if
  //    any query of the workgroup is outside that band (or overflowed), the workgroup re-runs
  //  SAFE pass (SAFE = 1): online softmax against a running reference that is raised lazily (a
  //    wave-uniform rare branch when a score exceeds it by 2^kRefBand, guide T13) and is set from
  //    the first block's maximum; p = exp2(s - m); VALU row sums.
  // maskc: IC<1> where the block may hold keys past N (the last tile), IC<0> in the pipelined loop's
  // full tiles (no tail branch there: a branch between QK(b)'s MFMAs and softmax(a)'s VALU splits the
  // basic block and the in-order wave then issues the two back to back instead of interleaved)
  auto softmax_m = [&](auto safec, auto maskc, f32x16& acc, int key0, bool first_blk, bf16x8& pa, bf16x8& pb) {
    constexpr bool SAFE = decltype(safec)::value;
    if (decltype(maskc)::value && key0 + 32 > N) mask_keys_past_n(acc, key0, hh, N);
    float p[16];
    if constexpr (!SAFE) {
#pragma unroll
      for (int r = 0; r < 16; ++r) p[r] = __builtin_amdgcn_exp2f(acc[r]);
    } else {
      const float mx = max16(acc);
      if (__any(first_blk || mx > m_run + kRefBand)) {
        const float mxp = pair_max(mx);  // the query's maximum over this block's 32 keys
        const bool move = first_blk || mxp > m_run + kRefBand;
        const float m_new = move ? mxp : m_run;  // identical in both lanes of a query
        const float alpha = first_blk ? 1.f : __builtin_amdgcn_exp2f(m_run - m_new);
        m_run = m_new;
        l_half *= alpha;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          oacc[0][r] *= alpha;
          oacc[1][r] *= alpha;
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) p[r] = __builtin_amdgcn_exp2f(acc[r] - m_run);
      l_half += ((((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]))) +
                 (((p[8] + p[9]) + (p[10] + p[11])) + ((p[12] + p[13]) + (p[14] + p[15]))));
    }
    pa = pack8f(p);
    pb = pack8f(p + 8);
    if constexpr (!SAFE) {
      lacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sel, pa, lacc, 0, 0, 0);
      lacc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(sel, pb, lacc, 0, 0, 0);
    }
  };

  // Software pipeline over 64-key tiles (halves a, b).  Fragments are read one phase before their
  // MFMAs; sched_barriers pin the reads where they are issued (left alone, the scheduler sinks each
  // read next to its MFMA behind an lgkmcnt(0)):
  //   QK(a) [V(a) reads] | K(b) reads, softmax(a) | PV(a) | QK(b) [V(b) reads] | softmax(b) |
  //   vmcnt(0) + barrier: tile kt+1 landed, every wave's reads of this tile retired |
  //   DMA tile kt+2 into this buffer, K(a) reads of tile kt+1 | PV(b) (registers only)
  const int nkt = (N + 63) / 64;
  const bool active = q0w < N;  // wave-uniform: a wave whose queries are all past N only stages K/V
  unsigned long long t_vm = 0, t_bar = 0;
  const unsigned long long t_begin = VS_CLK();
  auto pass = [&](auto safec) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      oacc[0][r] = 0.f;
      oacc[1][r] = 0.f;
      zero16[r] = 0.f;
    }
    lacc = f32x4{0.f, 0.f, 0.f, 0.f};
    m_run = 0.f;
    l_half = 0.f;
    load_tile(0, smem0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (nkt > 1) load_tile(1, smem1);
    KFrag ka = kread(smem0, 0);
    auto iter = [&](int kt, auto bufc) {
      constexpr int BUF = decltype(bufc)::value;
      using MaskC = IC<1>;
      const bool has_next = kt + 1 < nkt;
      char* cur = BUF ? smem1 : smem0;
      const char* nxt = BUF ? smem0 : smem1;
      bf16x8 b0, b1;
      if (active) {
        f32x16 sa = mfma32p(ka.k[0], qf[0], zero16);
        __builtin_amdgcn_sched_barrier(0);
        const VFrag va = vread(cur, 0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 1; s < 4; ++s) sa = mfma32p(ka.k[s], qf[s], sa);
        const KFrag kb = kread(cur, 1);
        __builtin_amdgcn_sched_barrier(0);
        bf16x8 a0, a1;
        softmax_m(safec, MaskC{}, sa, kt * 64, kt == 0, a0, a1);
        f32x16 sb;
        VFrag vb;
        if constexpr (ORD == 1) {
          sb = mfma32p(kb.k[0], qf[0], zero16);
#pragma unroll
          for (int s = 1; s < 4; ++s) sb = mfma32p(kb.k[s], qf[s], sb);
          __builtin_amdgcn_sched_barrier(0);
          vb = vread(cur, 1);
          __builtin_amdgcn_sched_barrier(0);
          pv(va, a0, a1);
          __builtin_amdgcn_sched_barrier(0);
        } else {
          pv(va, a0, a1);
          sb = mfma32p(kb.k[0], qf[0], zero16);
          __builtin_amdgcn_sched_barrier(0);
          vb = vread(cur, 1);
          __builtin_amdgcn_sched_barrier(0);
#pragma unroll
          for (int s = 1; s < 4; ++s) sb = mfma32p(kb.k[s], qf[s], sb);
        }
        softmax_m(safec, MaskC{}, sb, kt * 64 + 32, false, b0, b1);
        __builtin_amdgcn_sched_barrier(0);
        if (has_next) {
#ifdef VS_STAMP
          const unsigned long long c0 = VS_CLK();
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          const unsigned long long c1 = VS_CLK();
          __syncthreads();
          t_vm += c1 - c0;
          t_bar += VS_CLK() - c1;
#else
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMA pieces of tile kt+1 landed
          __syncthreads();                                  // ... every wave's; all reads of `cur` retired
#endif
          if (kt + 2 < nkt && !(VS_ATTN_DIAG & 1)) load_tile(kt + 2, cur);
          ka = kread(nxt, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        pv(vb, b0, b1);
      } else if (has_next) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (kt + 2 < nkt && !(VS_ATTN_DIAG & 1)) load_tile(kt + 2, cur);
      }
    };
    if constexpr (ORD != 2) {
      for (int kt = 0; kt < nkt; kt += 2) {
        iter(kt, IC<0>{});
        if (kt + 1 < nkt) iter(kt + 1, IC<1>{});
      }
    } else {
      // ORD 2: S(a), V(a) and K(b) of tile kt are in registers when iteration kt starts
      f32x16 sa_c;
      VFrag va_c;
      KFrag kb_c;
      if (active) {
        sa_c = mfma32p(ka.k[0], qf[0], zero16);
#pragma unroll
        for (int s = 1; s < 4; ++s) sa_c = mfma32p(ka.k[s], qf[s], sa_c);
        __builtin_amdgcn_sched_barrier(0);
        va_c = vread(smem0, 0);
        kb_c = kread(smem0, 1);
        __builtin_amdgcn_sched_barrier(0);
      }
      // LAST: the final tile (its blocks may hold keys past N: masked softmax; no next tile)
      auto iter2 = [&](int kt, auto bufc, auto lastc) {
        constexpr int BUF = decltype(bufc)::value;
        constexpr bool LAST = decltype(lastc)::value;
        char* cur = BUF ? smem1 : smem0;
        const char* nxt = BUF ? smem0 : smem1;
        if (active) {
          // [QK(b) | softmax(a)]
          f32x16 sb = mfma32p(kb_c.k[0], qf[0], zero16);
#pragma unroll
          for (int s = 1; s < 4; ++s) sb = mfma32p(kb_c.k[s], qf[s], sb);
          bf16x8 a0, a1;
          softmax_m(safec, lastc, sa_c, kt * 64, kt == 0, a0, a1);
          __builtin_amdgcn_sched_barrier(0);
          // [PV(a) | V(b) reads]
          const VFrag vb = vread(cur, 1);
          pv(va_c, a0, a1);
          __builtin_amdgcn_sched_barrier(0);
          bf16x8 b0, b1;
          if constexpr (!LAST) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMA pieces of tile kt+1 landed
            __syncthreads();                                  // ... every wave's; all reads of `cur` retired
            if (kt + 2 < nkt && !(VS_ATTN_DIAG & 1)) load_tile(kt + 2, cur);
            // [QK(a') | softmax(b)]
            const KFrag ka2 = kread(nxt, 0);
            sa_c = mfma32p(ka2.k[0], qf[0], zero16);
#pragma unroll
            for (int s = 1; s < 4; ++s) sa_c = mfma32p(ka2.k[s], qf[s], sa_c);
            softmax_m(safec, IC<0>{}, sb, kt * 64 + 32, false, b0, b1);
            __builtin_amdgcn_sched_barrier(0);
            // [PV(b) | V(a'), K(b') reads]
            va_c = vread(nxt, 0);
            kb_c = kread(nxt, 1);
            pv(vb, b0, b1);
            __builtin_amdgcn_sched_barrier(0);
          } else {
            softmax_m(safec, IC<1>{}, sb, kt * 64 + 32, false, b0, b1);
            pv(vb, b0, b1);
          }
        } else if (!LAST) {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          __syncthreads();
          if (kt + 2 < nkt && !(VS_ATTN_DIAG & 1)) load_tile(kt + 2, cur);
        }
      };
      int kt = 0;
      for (; kt + 2 < nkt; kt += 2) {
        iter2(kt, IC<0>{}, IC<0>{});
        iter2(kt + 1, IC<1>{}, IC<0>{});
      }
      if (kt + 1 < nkt) {
        iter2(kt, IC<0>{}, IC<0>{});
        iter2(kt + 1, IC<1>{}, IC<1>{});
      } else {
        iter2(kt, IC<0>{}, IC<1>{});
      }
    }
  };

  pass(IC<0>{});
  // Row sum of this lane's query (lane & 31): row (q >> 4) of lacc in lane (q & 15).
  float l;
  {
    const int q = lane & 31, src = (q & 15) << 2;
    // asm: hipcc folds "q < 16 ? bpermute(x0) : bpermute(x1)" into bpermute(q < 16 ? x0 : x1),
    // evaluating the select in the SOURCE lane (always x0 there) — wrong for queries 16..31.
    float l0, l1;
    asm volatile(
        "ds_bpermute_b32 %0, %2, %3\n\t"
        "ds_bpermute_b32 %1, %2, %4\n\t"
        "s_waitcnt lgkmcnt(0)"
        : "=&v"(l0), "=&v"(l1)
        : "v"(src), "v"(lacc[0]), "v"(lacc[1])
        : "memory");
    l = q < 16 ? l0 : l1;
  }
  bool ofin = true;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) ofin = ofin && __builtin_isfinite(oacc[dt][r]);
  const bool bad = active && qi < N && !fast_pass_ok(l, ofin);
  if (fwd_redo_vote(bad, redo_flag)) {
    pass(IC<1>{});
    l = pair_sum(l_half);
    __syncthreads();
  }

  const float inv = 1.f / l;
  char* so = fwd_o_stage(smem0, smem1, wid);
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g)  // chunk dt * 4 + g holds 8 dims; this lane holds its 4hh half
      fwd_o_put4(so, lane & 31, dt * 4 + g, hh, oacc[dt][4 * g] * inv, oacc[dt][4 * g + 1] * inv,
                 oacc[dt][4 * g + 2] * inv, oacc[dt][4 * g + 3] * inv);
  if (hh == 0 && qi < N) lse[((int64_t)b * H + h) * N + qi] = (m_run + __log2f(l)) * kLn2;
  fwd_o_store(so, o, ldo, row0, h, q0w, N, lane);
  VS_STAMP_AT(true);
#ifdef VS_STAMP
  stamp_acc(4, t_vm);
  stamp_acc(5, t_bar);
  stamp_acc(6, VS_CLK() - t_begin);
#else
  (void)t_vm;
  (void)t_bar;
  (void)t_begin;
#endif
}

// ------------------------------------------------------------------ forward on 16x16x32 MFMAs
// The same wave tile as attn_fwd_bf16_kernel (32 queries x 64 dims of O, 64-key K/V tiles by LDS-DMA,
// fast pass with the safe-pass redo) on v_mfma_f32_16x16x32_bf16 (VS_KNOB_ATTN_VARIANT 8, round 6):
// same MFMA cycles per FLOP in twice the instructions; MI355X_MICROARCH.md "DVFS give-back" item 7
// measures this shape holding a higher clock on random data.  Lane l = (c, g) = (l & 15, l >> 4):
//   S^T tile (ks, qt) = K[16 keys] (cQ)^T[16 queries]: A = K rows (key c, dims 8g..8g+7, ds_read_b128),
//     B = this lane's Q fragment (query qt*16 + c); the lane holds query qt*16+c, keys 16ks + 4g + i;
//   P (qt) = {p(ks 0)[0..3], p(ks 1)[0..3]} is the B operand of O^T += V^T P^T with k-slot 8g + j <->
//     key 4g + j (j < 4) or 16 + 4g + j - 4; the V^T A operand (dim c, those keys) is two
//     ds_read_tr16_b64 of rows 4g..4g+3 and 16+4g..: a 16-lane group reads 4 rows x 16 dims;
//   row sums: A = all ones, so every lane's 4 accumulators hold its query's sum (no broadcast);
//   V image swizzle: swz_v16 (the K image keeps swz_row: 16 rows x 16 B per group, conflict-free).
// A lane holds two queries (qt = 0, 1): the safe pass keeps two running references and reduces a
// query's max / sum over its four lanes (xor 16, xor 32).
__device__ __forceinline__ f32x4 mfma16(const bf16x8& a, const bf16x8& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

__global__ __launch_bounds__(256, 3) void attn_fwd16_bf16_kernel(const bf16_t* __restrict__ qkv, int64_t ldq,
                                                                bf16_t* __restrict__ o, int64_t ldo,
                                                                float* __restrict__ lse, int N, int H,
                                                                float scale_log2) {
  constexpr int TILE = kFwdTile;
  __shared__ __attribute__((aligned(16))) char smem0[2 * TILE];
  __shared__ __attribute__((aligned(16))) char smem1[2 * TILE];
  __shared__ int redo_flag;
  const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, g = lane >> 4;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const AttnBlock ab = attn_block(xcd_remap(blockIdx.x, gridDim.x), N, H);
  const int h = ab.h, b = ab.b;
  const int64_t row0 = ab.row0;
  const bf16_t* Qp = qkv + row0 * ldq + h * 64;
  const bf16_t* Kp = Qp + ab.D;
  const int q0w = ab.xb * 128 + wid * 32;
  if (tid == 0) redo_flag = 0;

  bf16x8 qf[2][2];  // [query tile][32-dim chunk]
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const int qi = q0w + qt * 16 + c, qr = qi < N ? qi : N - 1;
#pragma unroll
    for (int dc = 0; dc < 2; ++dc) qf[qt][dc] = scaled_frag(Qp + (int64_t)qr * ldq + dc * 32 + 8 * g, scale_log2);
  }
  const bf16x8 ones = __builtin_convertvector((f32x8){1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f}, bf16x8);
  f32x4 oacc[4][2], lacc[2];
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  float m_run[2], l_half[2];

  int kbase[2], vbase[4];
#pragma unroll
  for (int dc = 0; dc < 2; ++dc) kbase[dc] = c * 128 + (((dc * 4 + g) ^ swz_row(c)) << 4);
  {
    const int r = 4 * g + (c >> 2), sw = swz_v16(r);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) vbase[dt] = TILE + r * 128 + (((dt * 2 + ((c & 3) >> 1)) ^ sw) << 4) + (c & 1) * 8;
  }
  const FwdTileLoader<VSwz16> load_tile(Kp, ldq, ab.D, N, wid, lane);
  struct KFrag {
    bf16x8 k[2][2];  // [16-key subtile][32-dim chunk]
  };
  struct VFrag {
    bf16x8 v[4];  // [16-dim tile]
  };
  struct SAcc {
    f32x4 s[2][2];  // [16-key subtile][query tile]
  };
  auto kread = [&](const char* base, int kb) {
    KFrag f;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int dc = 0; dc < 2; ++dc) f.k[ks][dc] = *(const bf16x8*)(base + kb * 4096 + ks * 2048 + kbase[dc]);
    return f;
  };
  auto vread = [&](const char* base, int kb) {
    VFrag f;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) f.v[dt] = tr_pair(base + kb * 4096, vbase[dt], vbase[dt] + 2048);
    return f;
  };
  auto qk_first = [&](const KFrag& f, SAcc& a) { a.s[0][0] = mfma16(f.k[0][0], qf[0][0], zero4); };
  auto qk_rest = [&](const KFrag& f, SAcc& a) {
    a.s[0][1] = mfma16(f.k[0][0], qf[1][0], zero4);
    a.s[1][0] = mfma16(f.k[1][0], qf[0][0], zero4);
    a.s[1][1] = mfma16(f.k[1][0], qf[1][0], zero4);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) a.s[ks][qt] = mfma16(f.k[ks][1], qf[qt][1], a.s[ks][qt]);
  };
  auto pv = [&](const VFrag& f, const bf16x8 (&p)[2]) {
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) oacc[dt][qt] = mfma16(f.v[dt], p[qt], oacc[dt][qt]);
  };
  auto qmax4 = [&](float v) {  // max over the query's four lanes (c, g = 0..3)
    v = fmaxf(v, __shfl_xor(v, 16));
    return fmaxf(v, __shfl_xor(v, 32));
  };
  auto softmax = [&](auto safec, SAcc& a, int key0, bool first_blk, bf16x8 (&p)[2]) {
    constexpr bool SAFE = decltype(safec)::value;
    if (key0 + 32 > N) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int qt = 0; qt < 2; ++qt)
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (key0 + 16 * ks + 4 * g + i >= N) a.s[ks][qt][i] = -INFINITY;
    }
    float e[2][2][4];
    if constexpr (!SAFE) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int qt = 0; qt < 2; ++qt)
#pragma unroll
          for (int i = 0; i < 4; ++i) e[ks][qt][i] = __builtin_amdgcn_exp2f(a.s[ks][qt][i]);
    } else {
      float mx[2];
#pragma unroll
      for (int qt = 0; qt < 2; ++qt)
        mx[qt] = max3f(max3f(a.s[0][qt][0], a.s[0][qt][1], a.s[0][qt][2]),
                       max3f(a.s[0][qt][3], a.s[1][qt][0], a.s[1][qt][1]), max3f(a.s[1][qt][2], a.s[1][qt][3], -INFINITY));
      if (__any(first_blk || mx[0] > m_run[0] + kRefBand || mx[1] > m_run[1] + kRefBand)) {
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
          const float mq = qmax4(mx[qt]);
          const bool move = first_blk || mq > m_run[qt] + kRefBand;
          const float m_new = move ? mq : m_run[qt];
          const float alpha = first_blk ? 1.f : __builtin_amdgcn_exp2f(m_run[qt] - m_new);
          m_run[qt] = m_new;
          l_half[qt] *= alpha;
#pragma unroll
          for (int dt = 0; dt < 4; ++dt)
#pragma unroll
            for (int i = 0; i < 4; ++i) oacc[dt][qt][i] *= alpha;
        }
      }
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        float sum = 0.f;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            e[ks][qt][i] = __builtin_amdgcn_exp2f(a.s[ks][qt][i] - m_run[qt]);
            sum += e[ks][qt][i];
          }
        l_half[qt] += sum;
      }
    }
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      const f32x8 v = {e[0][qt][0], e[0][qt][1], e[0][qt][2], e[0][qt][3],
                       e[1][qt][0], e[1][qt][1], e[1][qt][2], e[1][qt][3]};
      p[qt] = __builtin_convertvector(v, bf16x8);
    }
    if constexpr (!SAFE) {
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) lacc[qt] = mfma16(ones, p[qt], lacc[qt]);
    }
  };

  // the tile order of attn_fwd_bf16_kernel<1>: QK(a) [V(a) reads] | K(b) reads, softmax(a) |
  // QK(b) | V(b) reads | PV(a) | softmax(b) | vmcnt(0) + barrier, DMA tile kt+2, K(a') reads | PV(b)
  const int nkt = (N + 63) / 64;
  const bool active = q0w < N;
  auto pass = [&](auto safec) {
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) oacc[dt][qt] = zero4;
    lacc[0] = zero4;
    lacc[1] = zero4;
    m_run[0] = m_run[1] = 0.f;
    l_half[0] = l_half[1] = 0.f;
    load_tile(0, smem0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (nkt > 1) load_tile(1, smem1);
    KFrag ka = kread(smem0, 0);
    auto iter = [&](int kt, auto bufc) {
      constexpr int BUF = decltype(bufc)::value;
      const bool has_next = kt + 1 < nkt;
      char* cur = BUF ? smem1 : smem0;
      const char* nxt = BUF ? smem0 : smem1;
      if (active) {
        SAcc sa, sb;
        qk_first(ka, sa);
        __builtin_amdgcn_sched_barrier(0);
        const VFrag va = vread(cur, 0);
        __builtin_amdgcn_sched_barrier(0);
        qk_rest(ka, sa);
        const KFrag kb = kread(cur, 1);
        __builtin_amdgcn_sched_barrier(0);
        bf16x8 pa[2], pb[2];
        softmax(safec, sa, kt * 64, kt == 0, pa);
        qk_first(kb, sb);
        qk_rest(kb, sb);
        __builtin_amdgcn_sched_barrier(0);
        const VFrag vb = vread(cur, 1);
        __builtin_amdgcn_sched_barrier(0);
        pv(va, pa);
        __builtin_amdgcn_sched_barrier(0);
        softmax(safec, sb, kt * 64 + 32, false, pb);
        __builtin_amdgcn_sched_barrier(0);
        if (has_next) {
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          __syncthreads();
          if (kt + 2 < nkt) load_tile(kt + 2, cur);
          ka = kread(nxt, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        pv(vb, pb);
      } else if (has_next) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (kt + 2 < nkt) load_tile(kt + 2, cur);
      }
    };
    for (int kt = 0; kt < nkt; kt += 2) {
      iter(kt, IC<0>{});
      if (kt + 1 < nkt) iter(kt + 1, IC<1>{});
    }
  };

  pass(IC<0>{});
  float l[2] = {lacc[0][0], lacc[1][0]};  // every accumulator row holds the query's sum
  bool ofin = true;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
#pragma unroll
      for (int i = 0; i < 4; ++i) ofin = ofin && __builtin_isfinite(oacc[dt][qt][i]);
  bool bad = false;
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) bad = bad || (q0w + qt * 16 + c < N && !fast_pass_ok(l[qt], ofin));
  bad = active && bad;
  if (fwd_redo_vote(bad, redo_flag)) {
    pass(IC<1>{});
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      float v = l_half[qt];
      v += __shfl_xor(v, 16);
      l[qt] = v + __shfl_xor(v, 32);
    }
    __syncthreads();
  }

  // lane (c, g) holds query qt*16 + c, dims 16dt + 4g .. +3
  char* so = fwd_o_stage(smem0, smem1, wid);
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const float inv = 1.f / l[qt];
    const int qr = qt * 16 + c;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
      fwd_o_put4(so, qr, dt * 2 + (g >> 1), g & 1, oacc[dt][qt][0] * inv, oacc[dt][qt][1] * inv, oacc[dt][qt][2] * inv,
                 oacc[dt][qt][3] * inv);
    if (g == 0 && q0w + qr < N) lse[((int64_t)b * H + h) * N + q0w + qr] = (m_run[qt] + __log2f(l[qt])) * kLn2;
  }
  fwd_o_store(so, o, ldo, row0, h, q0w, N, lane);
}

}  // namespace vs

using namespace vs;

extern "C" int vs_attn_fwd(int32_t dtype, int64_t B, int64_t N, int64_t H, int64_t Dh, const void* qkv, int64_t ld_qkv,
                           void* o, int64_t ld_o, float* lse, float scale, void* stream) {
  VS_CALL(attn_check(B, N, H, Dh));
  VS_REQUIRE(qkv && o && lse, "vs_attn_fwd: null pointer");
  VS_REQUIRE(ld_qkv >= 3 * H * 64 && ld_o >= H * 64, "vs_attn_fwd: leading dims too small");
  hipStream_t s = (hipStream_t)stream;
  const double es = dtype == VS_BF16 ? 2.0 : 4.0;
  ScopedTimer timer(VS_TIMER_ATTN_FWD, s, (double)(B * N * H * 64) * 4.0 * es + (double)(B * H * N) * 4.0);
  if (dtype == VS_BF16) {
    // Q rows are read and K/V tiles DMA'd as 16-byte chunks, and every forward kernel stores O rows as
    // 16-byte vectors (the uint4 stores of the epilogues): both operands need 16-byte rows
    VS_REQUIRE(ld_qkv % 8 == 0 && ld_o % 8 == 0 && aligned16(qkv) && aligned16(o),
               "vs_attn_fwd: bf16 rows must be 16-byte aligned");
    count_path(VS_PATH_ATTN_FWD);
    // VS_KNOB_ATTN_VARIANT low nibble: 0 the default kernel (QK(b) issued ahead of PV(a): 299 -> 252 us
    // back to back at 128 clips, neutral inside the step); 6: the round-2 order (PV(a) before QK(b)),
    // the one experimental slot kept.  The one-wave-per-SIMD kernels of round 3 (slower: DESIGN.md
    // section 5) were removed.
    const int fv = knob(VS_KNOB_ATTN_VARIANT) & 15;
    dim3 grid((unsigned)(cdiv(N, 128) * H * B));  // 1D: xcd_remap groups a (b, h)'s blocks on one XCD
    // 7: the cross-tile software pipeline (ORD 2, round 6)
    // (round-6 A/B, profiles/r06_attn_ab_c2.json: 283.6 vs 260.7 us at C2, 1,100 vs 1,019 at C3 -- slower)
    // 8: the 16x16x32-MFMA forward (round 6)
    auto kern = fv == 6   ? attn_fwd_bf16_kernel<0>
                : fv == 7 ? attn_fwd_bf16_kernel<2>
                : fv == 8 ? attn_fwd16_bf16_kernel
                          : attn_fwd_bf16_kernel<1>;
    hipLaunchKernelGGL(kern, grid, dim3(256), 0, s, (const bf16_t*)qkv, ld_qkv, (bf16_t*)o, ld_o, lse, (int)N, (int)H,
                       scale * kLog2e);
  } else if (dtype == VS_F32) {
    count_path(VS_PATH_ATTN_F32);
    attn_fwd_f32_launch(s, B, N, H, (const float*)qkv, ld_qkv, (float*)o, ld_o, lse, scale);
  } else {
    VS_REQUIRE(false, "vs_attn_fwd: bad dtype");
  }
  VS_LAUNCH_CHECK();
  return VS_OK;
}

extern "C" int vs_attn_redo_count(int64_t* out, int32_t reset) {
  VS_REQUIRE(out, "vs_attn_redo_count: null pointer");
  unsigned long long v = 0;
  // synchronising (as the header says): forward launches on any stream (torch's side streams are
  // not ordered against the null-stream symbol copies) have finished their atomicAdd before the
  // read, and none is in flight when the counter is reset
  hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) return (int)e;
  e = hipMemcpyFromSymbol(&v, HIP_SYMBOL(vs::g_attn_redo), sizeof(v), 0, hipMemcpyDeviceToHost);
  if (e != hipSuccess) return (int)e;
  *out = (int64_t)v;
  if (reset) {
    const unsigned long long z = 0;
    e = hipMemcpyToSymbol(HIP_SYMBOL(vs::g_attn_redo), &z, sizeof(z), 0, hipMemcpyHostToDevice);
    if (e != hipSuccess) return (int)e;
  }
  return VS_OK;
}

#ifdef VS_STAMP
extern "C" int vs_dbg_stamps(unsigned long long* host, int n) {
  return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(vs::g_stamp), (size_t)n * sizeof(unsigned long long), 0,
                                  hipMemcpyDeviceToHost);
}
#endif
