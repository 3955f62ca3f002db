// attn_bwd.hip — the bf16 MFMA backward of head-dim-64 attention: the row-constant kernel, the dK/dV
// and dQ passes (each with a 3-wave and a pipelined-pair schedule) as one launch, and the entry
// vs_attn_bwd (attn_common.h has the overview).
#include "attn_common.h"

namespace vs {

// ------------------------------------------------------------------ backward: row constants
// Per (batch, head, query): nlse2 = -LSE * log2(e) and ndel = -delta (delta = rowsum(dO * O)),
// stored [B*H][Npad] with Npad = N rounded up to 64 and the padding set to (-inf, 0): the dK/dV
// kernel DMAs 64-query slices of them straight into LDS and seeds its S / dP accumulators with
// them, and a padded query then contributes exactly P = 0, dS = 0.  Four lanes per (row, head),
// two 16-B loads of O and of dO each, then a 2-step shuffle (one thread per (row, head) with 16
// loads in its chain was latency-bound: 14 us for 19 MB).
__global__ __launch_bounds__(256) void attn_rowprep_kernel(const bf16_t* __restrict__ o, int64_t ldo,
                                                           const bf16_t* __restrict__ dout, int64_t lddo,
                                                           const float* __restrict__ lse, float* __restrict__ nlse2,
                                                           float* __restrict__ ndel, int64_t B, int N, int H,
                                                           int Npad) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * 256;
  const int64_t pair = t >> 2;          // (row, head)
  const int q = (int)(t & 3);           // 16-column quarter of the head
  float acc = 0.f;
  const bool live = pair < B * N * H;
  int64_t row = 0;
  int h = 0;
  if (live) {
    row = pair / H;
    h = (int)(pair % H);
    const bf16x8* op = (const bf16x8*)(o + row * ldo + h * 64 + q * 16);
    const bf16x8* dp = (const bf16x8*)(dout + row * lddo + h * 64 + q * 16);
    const bf16x8 a0 = op[0], a1 = op[1], g0 = dp[0], g1 = dp[1];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc = fmaf((float)a0[k], (float)g0[k], acc);
#pragma unroll
    for (int k = 0; k < 8; ++k) acc = fmaf((float)a1[k], (float)g1[k], acc);
  }
  acc += __shfl_xor(acc, 1, 64);
  acc += __shfl_xor(acc, 2, 64);
  if (live && q == 0) {
    const int64_t b = row / N, n = row % N;
    const int64_t w = (b * H + h) * Npad + n;
    ndel[w] = -acc;
    nlse2[w] = -lse[(b * H + h) * N + n] * kLog2e;
  }
  const int pad = Npad - N;
  for (int64_t i = t; i < B * H * pad; i += nthreads) {
    const int64_t w = (i / pad) * Npad + N + i % pad;
    nlse2[w] = -INFINITY;
    ndel[w] = 0.f;
  }
}

// ------------------------------------------------------------------ backward: what the passes share
// Both passes sweep 64-row stages of two swz_rt images (dK/dV: Q and dO slices, then nlse2[64] and
// ndel[64]; dQ: K and V tiles) that arrive by LDS-DMA into two buffers, one barrier per stage.
constexpr int kBwdQT = 64 * 128;             // one 64-row x 64-dh bf16 image
constexpr int kBwdStage = 2 * kBwdQT + 512;  // two images + the dK/dV pass's row constants

// Per-lane LDS offsets into a 32-row half of an image (+4096 B for the second half: an immediate):
// roff[s]: the row read (ds_read_b128) of row lane & 31, chunk 2s + hh; toff[dt]: the transposed
// reads (ds_read_tr16_b64) of rows t and t + 8, t = 4hh + q4 (+16 rows per s2 = +2048 B: immediate).
// The same arithmetic for Q/dO rows (dK/dV) and K/V rows (dQ).
struct BwdLdsOff {
  int roff[4];
  int toff[2][2];
};
__device__ __forceinline__ BwdLdsOff bwd_lds_off(int lane) {
  const int hh = lane >> 5, row = lane & 31;
  BwdLdsOff o;
#pragma unroll
  for (int s = 0; s < 4; ++s) o.roff[s] = row * 128 + (((2 * s + hh) ^ swz_rt(row)) << 4);
  const int q4 = (lane & 15) >> 2, p4 = (lane & 3) * 4, g16 = ((lane >> 4) & 1) * 16, t = 4 * hh + q4;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt) {
    o.toff[dt][0] = off_rtswz(t, dt * 32 + g16 + p4);
    o.toff[dt][1] = off_rtswz(t + 8, dt * 32 + g16 + p4);
  }
  return o;
}
// the transposed A operand of dims 32dt .. 32dt+31 x the 16 rows at byte offset o of an image
__device__ __forceinline__ bf16x8 tr_frag(const char* img, int o, const BwdLdsOff& lo, int dt) {
  return tr_pair(img, o + lo.toff[dt][0], o + lo.toff[dt][1]);
}
// ... of all 32 rows of half `sub`: f[2 s2 + dt]
__device__ __forceinline__ void tr4(const char* img, int sub, const BwdLdsOff& lo, bf16x8 (&f)[4]) {
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) f[2 * s2 + dt] = tr_frag(img, sub * 4096 + s2 * 2048, lo, dt);
}

// dQ's product of one 32-key block: dS^T = exp2(S^T) * dP^T (the chains started from nlse2 / ndel),
// packed to bf16, is the B operand of dQ^T += K^T dS^T; frag(s2, dt) supplies the K^T fragments
template <class Frag>
__device__ __forceinline__ void ds_mma(const f32x16& sacc, const f32x16& dpacc, f32x16 (&dqacc)[2], Frag&& frag) {
#pragma unroll
  for (int s2 = 0; s2 < 2; ++s2) {
    float ds[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) ds[r] = __builtin_amdgcn_exp2f(sacc[8 * s2 + r]) * dpacc[8 * s2 + r];
    const bf16x8 db = pack8f(ds);
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) dqacc[dt] = mfma32p(frag(s2, dt), db, dqacc[dt]);
  }
}

// The stage loaders.  Wave w fills pieces 2w, 2w+1 (8 rows x 128 B each) of both images; lane L loads
// the source chunk that belongs at position L & 7 of its row.  Rows past N re-read row N-1 (finite
// data: their nlse2 = -inf, or the key mask, zeroes them).  Every DMA is the asm form (SGPR base +
// 32-bit lane offset): a compiler-visible one in flight makes hipcc wait vmcnt(0) before the next LDS
// read, draining the prefetch of stage it + 1 under stage it.
// HOIST: the form the 3-wave schedules were tuned with -- the full-stage lane offsets are computed
// once (the per-stage 64-bit address arithmetic and the rows-past-N selects cost ~40 VALU per stage)
// and the partial last stage clamps in a branch of its own; !HOIST: the pairs' form -- offsets from
// the clamped rows at every call, no branch.  Both fill identical LDS images.
template <bool HOIST>
struct QdoStageLoader {  // dK/dV: Q and dO slices + nlse2 / ndel
  const bf16_t *Qp, *Dp;
  const float *NL, *ND;
  int64_t ldq, lddo;
  int N, wid, lane;
  uint32_t gq0, gq1, gd0, gd1;  // HOIST: the lane's offsets into a full Q / dO slice
  __device__ __forceinline__ QdoStageLoader(const bf16_t* Qp_, int64_t ldq_, const bf16_t* Dp_, int64_t lddo_,
                                            const float* NL_, const float* ND_, int N_, int wid_, int lane_)
      : Qp(Qp_), Dp(Dp_), NL(NL_), ND(ND_), ldq(ldq_), lddo(lddo_), N(N_), wid(wid_), lane(lane_) {
    const int prow = wid * 16 + (lane >> 3), ppos = lane & 7;
    const uint32_t cq0 = (uint32_t)((ppos ^ swz_rt(prow)) << 4), cq1 = (uint32_t)((ppos ^ swz_rt(prow + 8)) << 4);
    gq0 = (uint32_t)(prow * 2 * ldq) + cq0, gq1 = (uint32_t)((prow + 8) * 2 * ldq) + cq1;
    gd0 = (uint32_t)(prow * 2 * lddo) + cq0, gd1 = (uint32_t)((prow + 8) * 2 * lddo) + cq1;
  }
  __device__ __forceinline__ void operator()(int it, char* dst) const {
    const int prow = wid * 16 + (lane >> 3), ppos = lane & 7;  // this lane's rows prow, prow + 8 of a slice
    const uint32_t cq0 = (uint32_t)((ppos ^ swz_rt(prow)) << 4), cq1 = (uint32_t)((ppos ^ swz_rt(prow + 8)) << 4);
    const int q0 = it * 64;
    const char* qs = (const char*)(Qp + (int64_t)q0 * ldq);
    const char* ds = (const char*)(Dp + (int64_t)q0 * lddo);
    char* dq_ = dst + wid * 2048;
    char* dd_ = dst + kBwdQT + wid * 2048;
    auto dma = [&](uint32_t oq0, uint32_t oq1, uint32_t od0, uint32_t od1) {
      glds16_asm_so(qs, oq0, dq_);
      glds16_asm_so(qs, oq1, dq_ + 1024);
      glds16_asm_so(ds, od0, dd_);
      glds16_asm_so(ds, od1, dd_ + 1024);
    };
    if constexpr (HOIST) {
      if (q0 + 64 <= N) {
        dma(gq0, gq1, gd0, gd1);
      } else {
        const int r0 = q0 + prow < N ? prow : N - 1 - q0, r1 = q0 + prow + 8 < N ? prow + 8 : N - 1 - q0;
        dma((uint32_t)(r0 * 2 * ldq) + cq0, (uint32_t)(r1 * 2 * ldq) + cq1, (uint32_t)(r0 * 2 * lddo) + cq0,
            (uint32_t)(r1 * 2 * lddo) + cq1);
      }
      // nlse2 by wave 0, ndel by wave 1: 64 lanes x 4 B each
      if (wid == 0) glds4_asm_so(NL + q0, 4 * lane, dst + 2 * kBwdQT);
      else if (wid == 1) glds4_asm_so(ND + q0, 4 * lane, dst + 2 * kBwdQT + 256);
    } else {
      int r0 = prow, r1 = prow + 8;
      if (q0 + 64 > N) {
        r0 = q0 + r0 < N ? r0 : N - 1 - q0;
        r1 = q0 + r1 < N ? r1 : N - 1 - q0;
      }
      dma((uint32_t)r0 * (uint32_t)(2 * ldq) + cq0, (uint32_t)r1 * (uint32_t)(2 * ldq) + cq1,
          (uint32_t)r0 * (uint32_t)(2 * lddo) + cq0, (uint32_t)r1 * (uint32_t)(2 * lddo) + cq1);
      // the same 512 B as four waves x 32 lanes: waves 0, 1 the halves of nlse2, waves 2, 3 of ndel
      const float* src = (wid < 2 ? NL : ND) + q0 + (wid & 1) * 32;
      if (lane < 32) glds4_asm_so(src, (uint32_t)(lane & 31) * 4, dst + 2 * kBwdQT + (wid >> 1) * 256 + (wid & 1) * 128);
    }
  }
};

template <bool HOIST>
struct KvStageLoader {  // dQ: K and V tiles (V = K + vdelta bytes)
  const char* kp;
  int64_t ldq, tile_bytes, vdelta;
  int N, wid, lane;
  uint32_t ko0, ko1;  // HOIST: the lane's offsets into a full tile
  __device__ __forceinline__ KvStageLoader(const bf16_t* Kp, int64_t ldq_, int D, int N_, int wid_, int lane_)
      : kp((const char*)Kp), ldq(ldq_), tile_bytes(64 * 2 * ldq_), vdelta(2 * (int64_t)D), N(N_), wid(wid_),
        lane(lane_) {
    const int prow = wid * 16 + (lane >> 3), ppos = lane & 7;
    ko0 = (uint32_t)(prow * 2 * ldq + ((ppos ^ swz_rt(prow)) << 4));
    ko1 = (uint32_t)((prow + 8) * 2 * ldq + ((ppos ^ swz_rt(prow + 8)) << 4));
  }
  __device__ __forceinline__ void operator()(int kt, char* buf) const {
    const int prow = wid * 16 + (lane >> 3), ppos = lane & 7;
    const char* kb = kp + kt * tile_bytes;
    char* dk = buf + wid * 2048;
    char* dv = buf + kBwdQT + wid * 2048;
    auto dma = [&](uint32_t o0, uint32_t o1) {
      glds16_asm_so(kb, o0, dk);
      glds16_asm_so(kb, o1, dk + 1024);
      glds16_asm_so(kb + vdelta, o0, dv);
      glds16_asm_so(kb + vdelta, o1, dv + 1024);
    };
    if constexpr (HOIST) {
      if ((kt + 1) * 64 <= N) {
        dma(ko0, ko1);
      } else {
        const int r0 = kt * 64 + prow < N ? prow : N - 1 - kt * 64;
        const int r1 = kt * 64 + prow + 8 < N ? prow + 8 : N - 1 - kt * 64;
        dma((uint32_t)(r0 * 2 * ldq + ((ppos ^ swz_rt(prow)) << 4)),
            (uint32_t)(r1 * 2 * ldq + ((ppos ^ swz_rt(prow + 8)) << 4)));
      }
    } else {
      const uint32_t cc0 = (uint32_t)((ppos ^ swz_rt(prow)) << 4), cc1 = (uint32_t)((ppos ^ swz_rt(prow + 8)) << 4);
      int r0 = prow, r1 = prow + 8;
      if ((kt + 1) * 64 > N) {
        r0 = kt * 64 + r0 < N ? r0 : N - 1 - kt * 64;
        r1 = kt * 64 + r1 < N ? r1 : N - 1 - kt * 64;
      }
      dma((uint32_t)r0 * (uint32_t)(2 * ldq) + cc0, (uint32_t)r1 * (uint32_t)(2 * ldq) + cc1);
    }
  }
};

// The double-buffered sweep of a pass: stage it + 1 is in flight while fn(stage, it) computes stage it.
template <class Loader, class Fn>
__device__ __forceinline__ void bwd_sweep(int N, char* st0, char* st1, const Loader& load, Fn&& fn) {
  const int nit = (N + 63) / 64;
  load(0, st0);
  auto iter = [&](int it, auto bufc) {
    constexpr int BUF = decltype(bufc)::value;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's DMA pieces of stage it landed
    __syncthreads();                                  // ... and every wave's; buffer BUF^1 is free
    if (it + 1 < nit && !((VS_ATTN_DIAG & 2) && it >= 1)) load(it + 1, BUF ? st0 : st1);
    fn(BUF ? st1 : st0, it);
  };
  for (int it = 0; it < nit; it += 2) {
    iter(it, IC<0>{});
    if (it + 1 < nit) iter(it + 1, IC<1>{});
  }
}

// ------------------------------------------------------------------ backward: dK, dV
// Key-major.  Workgroup = 4 waves x 32 keys; each wave holds its keys' K (pre-scaled by
// c = scale * log2 e, one bf16 rounding as the forward's Q) and V as MFMA B operands and dK^T,
// dV^T in accumulators while the workgroup sweeps 64-query slices.  S and dP are produced with the
// key on the lane and the query on the accumulator row; their chains start from nlse2 / ndel
// (4 ds_read_b128 each), so p = exp2(acc) and dS = p * acc with no other VALU, and P, dS are
// directly the B operands of dV^T += dO^T P and dK^T += Q^T dS (A operands: ds_read_tr16_b64).
struct DkdvWave {
  int lane, hh, wid, ki;  // ki: this lane's key
  const bf16_t *Qp, *Dp;  // the (batch, head)'s Q and dO rows
  const float *NL, *ND;   // ... and its nlse2 / ndel
  bf16x8 kf[4], vf[4];
  f32x16 dkacc[2], dvacc[2];
  int h, D;
  int64_t row0;  // the batch element's first row
};
__device__ __forceinline__ DkdvWave dkdv_prologue(int blk, const bf16_t* __restrict__ qkv, int64_t ldq,
                                                  const bf16_t* __restrict__ dout, int64_t lddo,
                                                  const float* __restrict__ nlse2, const float* __restrict__ ndel,
                                                  int N, int H, int Npad, float scale) {
  DkdvWave w;
  const int tid = threadIdx.x;
  w.lane = tid & 63, w.hh = w.lane >> 5, w.wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const AttnBlock ab = attn_block(blk, N, H);
  w.h = ab.h, w.D = ab.D, w.row0 = ab.row0;
  w.Qp = qkv + ab.row0 * ldq + ab.h * 64;
  const bf16_t* Kp = w.Qp + ab.D;
  const bf16_t* Vp = w.Qp + 2 * ab.D;
  w.Dp = dout + ab.row0 * lddo + ab.h * 64;
  w.NL = nlse2 + ((int64_t)ab.b * H + ab.h) * Npad;
  w.ND = ndel + ((int64_t)ab.b * H + ab.h) * Npad;
  w.ki = ab.xb * 128 + w.wid * 32 + (w.lane & 31);
  const float c2 = scale * kLog2e;
  const int kr = w.ki < N ? w.ki : N - 1;  // rows past N: finite data, their dK/dV are not stored
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    w.kf[s] = scaled_frag(Kp + (int64_t)kr * ldq + 16 * s + 8 * w.hh, c2);
    w.vf[s] = *(const bf16x8*)(Vp + (int64_t)kr * ldq + 16 * s + 8 * w.hh);
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    w.dkacc[0][r] = 0.f;
    w.dkacc[1][r] = 0.f;
    w.dvacc[0][r] = 0.f;
    w.dvacc[1][r] = 0.f;
  }
  return w;
}
__device__ __forceinline__ void dkdv_epilogue(const DkdvWave& w, bf16_t* __restrict__ dqkv, int64_t ldd, int N,
                                              float scale) {
  if (w.ki < N) {
    bf16_t* krow = dqkv + (w.row0 + w.ki) * ldd + w.D + w.h * 64;
    bf16_t* vrow = krow + w.D;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d = dt * 32 + 8 * g + 4 * w.hh;
        *(uint2*)(krow + d) = pack4(w.dkacc[dt][4 * g] * scale, w.dkacc[dt][4 * g + 1] * scale,
                                    w.dkacc[dt][4 * g + 2] * scale, w.dkacc[dt][4 * g + 3] * scale);
        *(uint2*)(vrow + d) =
            pack4(w.dvacc[dt][4 * g], w.dvacc[dt][4 * g + 1], w.dvacc[dt][4 * g + 2], w.dvacc[dt][4 * g + 3]);
      }
  }
}

// PIPE = false, the 3-wave schedule: one 32-query sub-slice at a time; the other waves of the SIMD fill
// the gap between a chain's MFMAs and the VALU that consumes them (exp after S, dS after dP).
// PIPE = true, the pipelined pair (2 waves per SIMD: the register file of two units): a 64-query slice
// runs as S(a), S(b) (interleaved chains) -> P(a) under S(b)'s MFMAs -> dV(a), dP(a) -> P(b) under
// them -> dV(b), dP(b) -> dS(a) under them -> dK(a) -> dS(b) under dK(a) -> dK(b).  P stays f32 between
// the dV and dK products (no bf16 unpack).  Same LDS images, DMA and numerics.
template <bool PIPE>
__device__ __forceinline__ void attn_bwd_dkdv(char* __restrict__ stg0, char* __restrict__ stg1, int blk,
                                              const bf16_t* __restrict__ qkv, int64_t ldq,
                                              const bf16_t* __restrict__ dout, int64_t lddo,
                                              const float* __restrict__ nlse2, const float* __restrict__ ndel,
                                              bf16_t* __restrict__ dqkv, int64_t ldd, int N, int H, int Npad,
                                              float scale) {
  constexpr int QT = kBwdQT;
  DkdvWave w = dkdv_prologue(blk, qkv, ldq, dout, lddo, nlse2, ndel, N, H, Npad, scale);
  const int hh = w.hh;
  const BwdLdsOff lo = bwd_lds_off(w.lane);
  const QdoStageLoader<!PIPE> load_stage(w.Qp, ldq, w.Dp, lddo, w.NL, w.ND, N, w.wid, w.lane);

  if constexpr (!PIPE) {
    // Phased so that S and dP are never live together (fits 3 waves/SIMD): S -> P -> dV += dO^T P,
    // then dP -> dS = P * dP -> dK += Q^T dS.  sched_barriers keep the scheduler from merging the
    // phases back (it hoists the second chain's LDS reads and MFMAs otherwise: 212 VGPRs).
    auto slice = [&](const char* st, int sub) {
      const char* sQ = st;
      const char* sD = st + QT;
      const float* sL = (const float*)(st + 2 * QT) + sub * 32 + 4 * hh;
      const float* sE = (const float*)(st + 2 * QT + 256) + sub * 32 + 4 * hh;
      // dP first, then S: both accumulators live together (the 158-VGPR body has the room since the
      // DMA offsets were hoisted), so dS = P * dP takes P in f32 straight from the exp2 instead of
      // unpacking the bf16 P of the dV product (16 fewer VALU per 32 x 32 unit)
      f32x16 dpa, acc;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 e4 = *(const float4*)(sE + 8 * g);
        dpa[4 * g] = e4.x; dpa[4 * g + 1] = e4.y; dpa[4 * g + 2] = e4.z; dpa[4 * g + 3] = e4.w;
        const float4 l4 = *(const float4*)(sL + 8 * g);
        acc[4 * g] = l4.x; acc[4 * g + 1] = l4.y; acc[4 * g + 2] = l4.z; acc[4 * g + 3] = l4.w;
      }
#pragma unroll
      for (int s = 0; s < 4; ++s)
        dpa = mfma32p(*(const bf16x8*)(sD + sub * 4096 + lo.roff[s]), w.vf[s], dpa);
#pragma unroll
      for (int s = 0; s < 4; ++s)
        acc = mfma32p(*(const bf16x8*)(sQ + sub * 4096 + lo.roff[s]), w.kf[s], acc);
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        float p[8], ds[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          p[r] = __builtin_amdgcn_exp2f(acc[8 * s2 + r]);
          ds[r] = p[r] * dpa[8 * s2 + r];  // dS = P * (dP - delta)
        }
        const bf16x8 pb = pack8f(p), db = pack8f(ds);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
          w.dvacc[dt] = mfma32p(tr_frag(sD, sub * 4096 + s2 * 2048, lo, dt), pb, w.dvacc[dt]);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
          w.dkacc[dt] = mfma32p(tr_frag(sQ, sub * 4096 + s2 * 2048, lo, dt), db, w.dkacc[dt]);
      }
      __builtin_amdgcn_sched_barrier(0);
    };
    bwd_sweep(N, stg0, stg1, load_stage, [&](const char* st, int it) {
      slice(st, 0);
      __builtin_amdgcn_sched_barrier(0);  // keep the two slices' S/dP accumulators from overlapping
      if (it * 64 + 32 < N) slice(st, 1);
      __builtin_amdgcn_sched_barrier(0);
    });
  } else {
    auto rowc = [&](const float* base, int sub, f32x16& acc) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 l4 = *(const float4*)(base + sub * 32 + 4 * hh + 8 * g);
        acc[4 * g] = l4.x; acc[4 * g + 1] = l4.y; acc[4 * g + 2] = l4.z; acc[4 * g + 3] = l4.w;
      }
    };
    auto rows4 = [&](const char* img, int sub, bf16x8 (&f)[4]) {
#pragma unroll
      for (int s = 0; s < 4; ++s) f[s] = *(const bf16x8*)(img + sub * 4096 + lo.roff[s]);
    };
    auto mma_p = [&](const bf16x8 (&f)[4], const float (&pv)[16], f32x16 (&acc)[2]) {
#pragma unroll
      for (int s2 = 0; s2 < 2; ++s2) {
        const bf16x8 pb = pack8f(pv + 8 * s2);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) acc[dt] = mfma32p(f[2 * s2 + dt], pb, acc[dt]);
      }
    };
    // one 64-query slice: sub-slices a (queries 0..31) and b (32..63).  A sub-slice past N runs on
    // padded rows (nlse2 = -inf: P = 0, dS = 0), so every slice is branch-free.  Each phase's LDS
    // operand reads are issued ahead of its MFMAs (pinned by sched_barriers; the compiler otherwise
    // sinks every read next to its MFMA behind an lgkmcnt(0)).
    bwd_sweep(N, stg0, stg1, load_stage, [&](const char* st, int) {
      const char* sQ = st;
      const char* sD = st + QT;
      const float* sL = (const float*)(st + 2 * QT);
      const float* sE = (const float*)(st + 2 * QT + 256);
      f32x16 xa, xb;
      bf16x8 fa[4], fb[4];
      rowc(sL, 0, xa);
      rows4(sQ, 0, fa);
      rowc(sL, 1, xb);
      rows4(sQ, 1, fb);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int s = 0; s < 4; ++s) {  // S(a), S(b): two independent chains, interleaved
        xa = mfma32p(fa[s], w.kf[s], xa);
        xb = mfma32p(fb[s], w.kf[s], xb);
      }
      __builtin_amdgcn_sched_barrier(0);
      tr4(sD, 0, lo, fa);  // dO(a)^T for dV(a)
      rows4(sD, 0, fb);    // dO(a) rows for dP(a)
      __builtin_amdgcn_sched_barrier(0);
      float pa[16], pb[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) pa[r] = __builtin_amdgcn_exp2f(xa[r]);
      rowc(sE, 0, xa);
      mma_p(fa, pa, w.dvacc);
#pragma unroll
      for (int s = 0; s < 4; ++s) xa = mfma32p(fb[s], w.vf[s], xa);
      __builtin_amdgcn_sched_barrier(0);
      tr4(sD, 1, lo, fa);  // dO(b)^T
      rows4(sD, 1, fb);    // dO(b) rows
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int r = 0; r < 16; ++r) pb[r] = __builtin_amdgcn_exp2f(xb[r]);
      rowc(sE, 1, xb);
      mma_p(fa, pb, w.dvacc);
#pragma unroll
      for (int s = 0; s < 4; ++s) xb = mfma32p(fb[s], w.vf[s], xb);
      __builtin_amdgcn_sched_barrier(0);
      tr4(sQ, 0, lo, fa);  // Q(a)^T, Q(b)^T for dK
      tr4(sQ, 1, lo, fb);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int r = 0; r < 16; ++r) pa[r] *= xa[r];
      mma_p(fa, pa, w.dkacc);
#pragma unroll
      for (int r = 0; r < 16; ++r) pb[r] *= xb[r];
      mma_p(fb, pb, w.dkacc);
      __builtin_amdgcn_sched_barrier(0);
    });
  }
  dkdv_epilogue(w, dqkv, ldd, N, scale);
}

// ------------------------------------------------------------------ backward: dQ
// Query-major, the forward's structure: workgroup = 4 waves x 32 queries sweeping 64-key K/V tiles.
// Q is pre-scaled by c = scale * log2 e exactly as in the forward (same bf16 rounding, so P is the
// forward's P).  S^T = K Q^T and dP^T = V dO^T put the QUERY on the lane; their chains start from
// per-lane splats of nlse2 and ndel, so p = exp2(acc) and dS^T = p * acc, which is directly the B
// operand of dQ^T += K^T dS^T (K^T via ds_read_tr16_b64).  No atomics.
struct DqWave {
  int lane, hh, wid, qi;  // qi: this lane's query
  const bf16_t* Kp;       // the (batch, head)'s K rows
  int h, D;
  int64_t row0;  // the batch element's first row
  bf16x8 qf[4], df[4];
  f32x16 sinit, dinit, dqacc[2];
};
__device__ __forceinline__ DqWave dq_prologue(int blk, const bf16_t* __restrict__ qkv, int64_t ldq,
                                              const bf16_t* __restrict__ dout, int64_t lddo,
                                              const float* __restrict__ nlse2, const float* __restrict__ ndel,
                                              int N, int H, int Npad, float scale) {
  DqWave w;
  const int tid = threadIdx.x;
  w.lane = tid & 63, w.hh = w.lane >> 5, w.wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const AttnBlock ab = attn_block(blk, N, H);
  w.h = ab.h, w.D = ab.D, w.row0 = ab.row0;
  const bf16_t* Qp = qkv + ab.row0 * ldq + ab.h * 64;
  w.Kp = Qp + ab.D;
  const bf16_t* Dp = dout + ab.row0 * lddo + ab.h * 64;
  w.qi = ab.xb * 128 + w.wid * 32 + (w.lane & 31);
  const float c2 = scale * kLog2e;
  const int qr = w.qi < N ? w.qi : N - 1;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    w.qf[s] = scaled_frag(Qp + (int64_t)qr * ldq + 16 * s + 8 * w.hh, c2);
    w.df[s] = *(const bf16x8*)(Dp + (int64_t)qr * lddo + 16 * s + 8 * w.hh);
  }
  const int64_t i = ((int64_t)ab.b * H + ab.h) * Npad + w.qi;
  const float nl = w.qi < N ? nlse2[i] : -INFINITY;  // a padded query: p = 0
  const float nd = w.qi < N ? ndel[i] : 0.f;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    w.sinit[r] = nl;
    w.dinit[r] = nd;
    w.dqacc[0][r] = 0.f;
    w.dqacc[1][r] = 0.f;
  }
  return w;
}
__device__ __forceinline__ void dq_epilogue(const DqWave& w, bf16_t* __restrict__ dqkv, int64_t ldd, int N,
                                            float scale) {
  if (w.qi < N) {
    bf16_t* qrow = dqkv + (w.row0 + w.qi) * ldd + w.h * 64;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int d = dt * 32 + 8 * g + 4 * w.hh;
        *(uint2*)(qrow + d) = pack4(w.dqacc[dt][4 * g] * scale, w.dqacc[dt][4 * g + 1] * scale,
                                      w.dqacc[dt][4 * g + 2] * scale, w.dqacc[dt][4 * g + 3] * scale);
      }
  }
}

// PIPE = false: one 32-key block at a time (3 waves per SIMD).  PIPE = true: a 64-key tile runs as
// S, dP of keys a and b (interleaved chains) -> dS(a) under b's MFMAs -> dQ(a) -> dS(b) under dQ(a)
// -> dQ(b) (2 waves per SIMD).
template <bool PIPE>
__device__ __forceinline__ void attn_bwd_dq(char* __restrict__ kv0, char* __restrict__ kv1, int blk,
                                            const bf16_t* __restrict__ qkv, int64_t ldq,
                                            const bf16_t* __restrict__ dout, int64_t lddo,
                                            const float* __restrict__ nlse2, const float* __restrict__ ndel,
                                            bf16_t* __restrict__ dqkv, int64_t ldd, int N, int H, int Npad,
                                            float scale) {
  constexpr int TILE = kBwdQT;
  DqWave w = dq_prologue(blk, qkv, ldq, dout, lddo, nlse2, ndel, N, H, Npad, scale);
  const int hh = w.hh;
  const BwdLdsOff lo = bwd_lds_off(w.lane);
  const KvStageLoader<!PIPE> load_tile(w.Kp, ldq, w.D, N, w.wid, w.lane);

  if constexpr (!PIPE) {
    auto sub = [&](const char* sK, int kb, int key0) {
      const char* sV = sK + TILE;
      f32x16 sacc = w.sinit, dpacc = w.dinit;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const bf16x8 ka = *(const bf16x8*)(sK + kb * 4096 + lo.roff[s]);
        const bf16x8 va = *(const bf16x8*)(sV + kb * 4096 + lo.roff[s]);
        sacc = mfma32p(ka, w.qf[s], sacc);
        dpacc = mfma32p(va, w.df[s], dpacc);
      }
      if (key0 + 32 > N) mask_keys_past_n(sacc, key0, hh, N);
      ds_mma(sacc, dpacc, w.dqacc, [&](int s2, int dt) { return tr_frag(sK, kb * 4096 + s2 * 2048, lo, dt); });
    };
    bwd_sweep(N, kv0, kv1, load_tile, [&](const char* cur, int kt) {
      sub(cur, 0, kt * 64);
      if (kt * 64 + 32 < N) sub(cur, 1, kt * 64 + 32);
    });
  } else {
    // one 64-key tile: key blocks a (0..31) and b (32..63; keys past N masked to p = 0, so every tile
    // is branch-free but the last one's mask).  Operand reads one phase ahead of their MFMAs.
    bwd_sweep(N, kv0, kv1, load_tile, [&](const char* sK, int kt) {
      const int key0 = kt * 64;
      const char* sV = sK + TILE;
      f32x16 sa, da, sb, db;
      bf16x8 ka[4], va[4], kb_[4], vb[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        ka[s] = *(const bf16x8*)(sK + lo.roff[s]);
        va[s] = *(const bf16x8*)(sV + lo.roff[s]);
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        kb_[s] = *(const bf16x8*)(sK + 4096 + lo.roff[s]);
        vb[s] = *(const bf16x8*)(sV + 4096 + lo.roff[s]);
      }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        sa = mfma32p(ka[s], w.qf[s], s == 0 ? w.sinit : sa);
        da = mfma32p(va[s], w.df[s], s == 0 ? w.dinit : da);
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        sb = mfma32p(kb_[s], w.qf[s], s == 0 ? w.sinit : sb);
        db = mfma32p(vb[s], w.df[s], s == 0 ? w.dinit : db);
      }
      __builtin_amdgcn_sched_barrier(0);
      tr4(sK, 0, lo, ka);
      tr4(sK, 1, lo, kb_);
      __builtin_amdgcn_sched_barrier(0);
      if (key0 + 64 > N) {
        if (key0 + 32 > N) mask_keys_past_n(sa, key0, hh, N);
        mask_keys_past_n(sb, key0 + 32, hh, N);
      }
      ds_mma(sa, da, w.dqacc, [&](int s2, int dt) { return ka[2 * s2 + dt]; });
      ds_mma(sb, db, w.dqacc, [&](int s2, int dt) { return kb_[2 * s2 + dt]; });
      __builtin_amdgcn_sched_barrier(0);
    });
  }
  dq_epilogue(w, dqkv, ldd, N, scale);
}

// ------------------------------------------------------------------ backward: one launch
// The dK/dV and dQ passes run as ONE grid: blocks [0, nblk) are dK/dV workgroups, [nblk, 2 nblk)
// dQ workgroups, sharing the same two LDS stages.  Each pass alone puts 2496 waves on 3072 wave
// slots (B = 16, N = 1568, H = 3), so a third of the SIMDs carry 3 waves and the rest 2 and the
// launch lasts as long as the 3-wave SIMDs; one grid of both lets the dispatcher backfill slots
// freed by the (longer, dispatched first) dK/dV workgroups with dQ workgroups.
// <3, false>: the 3-wave schedules; <2, true>: the pipelined pairs.
template <int WPS, bool PIPE>
__global__ __launch_bounds__(256, WPS) void attn_bwd_bf16_kernel(const bf16_t* __restrict__ qkv, int64_t ldq,
                                                                 const bf16_t* __restrict__ dout, int64_t lddo,
                                                                 const float* __restrict__ nlse2,
                                                                 const float* __restrict__ ndel,
                                                                 bf16_t* __restrict__ dqkv, int64_t ldd, int N, int H,
                                                                 int Npad, float scale, int nblk, int skip) {
  __shared__ __attribute__((aligned(16))) char st0[kBwdStage];  // two objects: see attn_fwd_bf16_kernel
  __shared__ __attribute__((aligned(16))) char st1[kBwdStage];
  const int id = blockIdx.x;
  if (skip & (id < nblk ? 1 : 2)) return;  // diagnostic builds only: one pass timed alone (VS_DEBUG_KNOBS)
  if (id < nblk)
    attn_bwd_dkdv<PIPE>(st0, st1, xcd_remap(id, nblk), qkv, ldq, dout, lddo, nlse2, ndel, dqkv, ldd, N, H, Npad, scale);
  else
    attn_bwd_dq<PIPE>(st0, st1, xcd_remap(id - nblk, nblk), qkv, ldq, dout, lddo, nlse2, ndel, dqkv, ldd, N, H, Npad,
                      scale);
}

}  // namespace vs

using namespace vs;

static inline int64_t attn_npad(int64_t N) { return (N + 63) / 64 * 64; }

extern "C" size_t vs_attn_bwd_workspace_bytes(int64_t B, int64_t N, int64_t H, int64_t Dh) {
  (void)Dh;
  // bf16: nlse2 and ndel [B*H][Npad] f32; f32: delta [B,H,N] (smaller); 256-B padded
  return ((size_t)(2 * B * H * attn_npad(N)) * 4 + 255) / 256 * 256;
}

extern "C" int vs_attn_bwd(int32_t dtype, int64_t B, int64_t N, int64_t H, int64_t Dh, const void* qkv, int64_t ld_qkv,
                           const void* o, int64_t ld_o, const void* dout, int64_t ld_do, const float* lse, void* dqkv,
                           int64_t ld_dqkv, void* workspace, float scale, void* stream) {
  VS_CALL(attn_check(B, N, H, Dh));
  VS_REQUIRE(qkv && o && dout && lse && dqkv && workspace, "vs_attn_bwd: null pointer");
  VS_REQUIRE(ld_qkv >= 3 * H * 64 && ld_dqkv >= 3 * H * 64 && ld_o >= H * 64 && ld_do >= H * 64,
             "vs_attn_bwd: leading dims too small");
  hipStream_t s = (hipStream_t)stream;
  const double es = dtype == VS_BF16 ? 2.0 : 4.0;
  ScopedTimer timer(VS_TIMER_ATTN_BWD, s, (double)(B * N * H * 64) * 8.0 * es + (double)(B * H * N) * 4.0);
  if (dtype == VS_BF16) {
    VS_REQUIRE(ld_qkv % 8 == 0 && ld_dqkv % 4 == 0 && ld_do % 8 == 0 && aligned16(qkv) && aligned16(dout) &&
                   (((uintptr_t)dqkv) & 7) == 0,
               "vs_attn_bwd: bf16 rows must be 16-byte aligned");
    VS_REQUIRE(ld_o % 8 == 0 && aligned16(o) && aligned16(workspace), "vs_attn_bwd: o / workspace alignment");
    const int64_t npad = attn_npad(N), rows = B * N;
    float* nlse2 = (float*)workspace;
    float* ndel = nlse2 + B * H * npad;
    count_path(VS_PATH_ATTN_BWD);
    hipLaunchKernelGGL(attn_rowprep_kernel, dim3((unsigned)cdiv(rows * H * 4, 256)), dim3(256), 0, s, (const bf16_t*)o,
                       ld_o, (const bf16_t*)dout, ld_do, lse, nlse2, ndel, B, (int)N, (int)H, (int)npad);
    // VS_KNOB_ATTN_VARIANT bits 4..7: 0 (default) picks 6 or 9 by grid size; 6 the software-pipelined
    // pair kernel (2 waves per SIMD), 9 the 3-wave kernel (3 waves per SIMD, one 32-row unit per wave)
    int bv = (knob(VS_KNOB_ATTN_VARIANT) >> 4) & 15;
    if (bv == 0) {
      // default by grid size: the pipelined pairs (2 waves/SIMD) when both passes fit in about two
      // rounds of the 3-wave kernel's slots (C2 at 16 clips: 624 + 624 workgroups, 122.3 -> 116.6 us),
      // the 3-wave kernel beyond (128 clips: 4,992 + 4,992 workgroups, 1,026 vs 924 us in
      // profiles/r03_v5_microbench_b128.txt)
      static const int slots = [] {
        int dev = 0, cus = 256;
        if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        return 3 * cus;
      }();
      bv = cdiv(N, 128) * H * B <= slots ? 6 : 9;
    }
#ifdef VS_DEBUG_KNOBS
    // diagnostic builds only (build.build(variant=..., defines=["VS_DEBUG_KNOBS"])): bits 8, 9 skip the
    // dK/dV or the dQ pass, so one pass can be timed alone -- the gradients are then WRONG
    const int skip = (knob(VS_KNOB_ATTN_VARIANT) >> 8) & 3;
#else
    const int skip = 0;
#endif
    const unsigned g = (unsigned)(cdiv(N, 128) * H * B);  // 1D: xcd_remap groups a (b, h)'s blocks on one XCD
    // 6: the pipelined pairs; anything else is 9, the 3-wave kernel (round-2 default)
    auto kern = bv == 6 ? attn_bwd_bf16_kernel<2, true> : attn_bwd_bf16_kernel<3, false>;
    hipLaunchKernelGGL(kern, dim3(2 * g), dim3(256), 0, s, (const bf16_t*)qkv, ld_qkv, (const bf16_t*)dout, ld_do, nlse2,
                       ndel, (bf16_t*)dqkv, ld_dqkv, (int)N, (int)H, (int)npad, scale, (int)g, skip);
  } else if (dtype == VS_F32) {
    count_path(VS_PATH_ATTN_F32);
    attn_bwd_f32_launch(s, B, N, H, (const float*)qkv, ld_qkv, (const float*)o, ld_o, (const float*)dout, ld_do, lse,
                        (float*)dqkv, ld_dqkv, (float*)workspace, scale);
  } else {
    VS_REQUIRE(false, "vs_attn_bwd: bad dtype");
  }
  VS_LAUNCH_CHECK();
  return VS_OK;
}
