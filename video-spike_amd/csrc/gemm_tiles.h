// gemm_tiles.h — what more than one GEMM kernel family (gemm_*.hip, patch_embed.hip) uses: the staged
// tile epilogue, the swizzled bf16 LDS operand images, and the host helpers that turn a call's runtime
// layout / epilogue flags into template arguments.
#pragma once

#include <type_traits>

#include "common.h"
#include "gemm_common.h"

namespace vs {

// Stage a BM x BN f32 tile (16x16-MFMA C layout in `acc`) through LDS and apply the epilogue in
// row order.  PARTS = 2 stages the two 64-row halves one after the other (the waves of row block
// wr write in pass wr), halving the staging LDS; `lds` must hold (BM/PARTS)*(BN+4) floats.
template <int BM, int BN, int TM, int TN, uint32_t EF, int PARTS = 1>
__device__ __forceinline__ void store_tile(const EpiParams& e, float* lds, const f32x4 (&acc)[TM][TN], int64_t m0,
                                           int64_t n0, int split) {
  static_assert(PARTS == 1 || (PARTS == 2 && BM / 2 == BM / 2 / 16 * 16), "row halves");
  const bool first_split = split == 0;
  const uint32_t F = epi_flags<EF>(e);
  constexpr int LDT = BN + 4;  // +4 floats: 16-B aligned rows, conflict-free scalar writes
  constexpr int WM = BM / 2, WN = BN / 2, RB = BM / PARTS;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wr = wid >> 1, wc = wid & 1;
  constexpr int CPR = BN / 8;        // 8-column groups per row
  constexpr int RPP = 256 / CPR;     // rows per pass
  const int cg = tid % CPR;
  const int64_t n = n0 + cg * 8;     // a thread keeps its column group in every pass
  const bool vec = e.vec_ok && n + 8 <= e.N;
  float bias8[8];
  if ((F & VS_EPI_BIAS) && vec && !(F & VS_EPI_ATOMIC) && !e.part) ld8(e.bias, n, 0, bias8);
#pragma unroll
  for (int part = 0; part < PARTS; ++part) {
    const int64_t mp = m0 + part * RB;  // first output row of this pass
    __syncthreads();
    if (PARTS == 1 || wr == part) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            lds[(wr * WM - part * RB + i * 16 + (lane >> 4) * 4 + r) * LDT + wc * WN + j * 16 + (lane & 15)] =
                acc[i][j][r] * e.alpha;
    }
    __syncthreads();
    if (e.part) {
      // split-K partial: plain 16-B stores of this split's tile (gemm_splitk_reduce adds the splits)
      float* pbase = e.part + (int64_t)split * e.M * e.N;
      constexpr int C4 = BN / 4;
      for (int idx = tid; idx < RB * C4; idx += 256) {
        const int rr = idx / C4, c4 = idx % C4;
        const int64_t m = mp + rr, nn = n0 + 4 * c4;
        if (m < e.M && nn < e.N) {
          const float* src = lds + rr * LDT + 4 * c4;
          if (nn + 4 <= e.N && (e.N & 3) == 0) {
            *(float4*)(pbase + m * e.N + nn) = *(const float4*)src;
          } else {
            for (int k = 0; k < 4 && nn + k < e.N; ++k) pbase[m * e.N + nn + k] = src[k];
          }
        }
      }
      continue;
    }
    if (F & VS_EPI_ATOMIC) {
      // one column per lane: a wave adds 64 consecutive floats (256 B) of a row per instruction
      for (int idx = tid; idx < RB * BN; idx += 256) {
        const int rr = idx / BN, cc = idx % BN;
        const int64_t m = mp + rr, nn = n0 + cc;
        if (m < e.M && nn < e.N) {
          float v = lds[rr * LDT + cc];
          if ((F & VS_EPI_BIAS) && first_split) v += e.bias[nn];
          unsafeAtomicAdd((float*)e.c + m * e.ldc + nn, v);
        }
      }
      continue;
    }
    if (n >= e.N) continue;
    if (vec) {
      // per-column constants loaded once, all row passes unrolled: their LDS reads, operand loads
      // and stores overlap (the rolled loop paid one global-load latency per pass: ~5.5k of a
      // ~10k-cycle K = 192 tile, scripts/stamp_gemm.py)
#pragma unroll
      for (int p = 0; p < RB / RPP; ++p) {
        const int rr = tid / CPR + p * RPP;
        const int64_t m = mp + rr;
        if (m < e.M) {
          const float* src = lds + rr * LDT + cg * 8;
          float v[8];
          const float4 a = *(const float4*)src;
          const float4 b = *(const float4*)(src + 4);
          v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
          if (F & VS_EPI_BIAS) {
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] += bias8[k];
          }
          epi_eight<EF>(e, m, n, v, true);
        }
      }
    } else {
      for (int rr = tid / CPR; rr < RB; rr += RPP) {
        const int64_t m = mp + rr;
        if (m >= e.M) break;
        const float* src = lds + rr * LDT + cg * 8;
        for (int k = 0; k < 8 && n + k < e.N; ++k) epi_one<EF>(e, m, n + k, src[k]);
      }
    }
  }
}

template <int R>
__device__ __forceinline__ int swz_mc(int k) {  // chunk XOR for [k][R] images (R = 128 or 64)
  if constexpr (R == 128) return 2 * ((k & 3) | (((k >> 3) & 1) << 2));
  else return 2 * (((k >> 1) & 1) | (((k >> 3) & 1) << 1));
}
__device__ __forceinline__ int swz_kc(int r) { return (r >> 1) & 7; }

template <int R, bool KC>
struct OperandBf16 {
  static constexpr int BK = 64;
  static constexpr int BYTES = R * BK * 2;
  static constexpr int CHUNKS = R * BK / 8 / 256;  // 16-B chunks per thread per tile

  __device__ __forceinline__ static void load(uint4 (&reg)[CHUNKS], const bf16_t* __restrict__ p, int64_t ld,
                                              int64_t r0, int64_t rows, int64_t k0, int64_t k_end, int tid) {
#pragma unroll
    for (int s = 0; s < CHUNKS; ++s) {
      const int i = tid + 256 * s;
      int64_t gr, gk;
      if constexpr (KC) {
        gr = r0 + (i >> 3);
        gk = k0 + (i & 7) * 8;
      } else {
        gk = k0 + i / (R / 8);
        gr = r0 + (i % (R / 8)) * 8;
      }
      const bool ok = gr < rows && gk < k_end;
      const bf16_t* src = KC ? p + gr * ld + gk : p + gk * ld + gr;
      reg[s] = ok ? *(const uint4*)src : make_uint4(0, 0, 0, 0);
    }
  }
  __device__ __forceinline__ static void store(char* lds, const uint4 (&reg)[CHUNKS], int tid) {
#pragma unroll
    for (int s = 0; s < CHUNKS; ++s) {
      const int i = tid + 256 * s;
      int off;
      if constexpr (KC) {
        const int r = i >> 3, c = i & 7;
        off = r * 128 + ((c ^ swz_kc(r)) << 4);
      } else {
        const int k = i / (R / 8), c = i % (R / 8);
        off = k * (R * 2) + ((c ^ swz_mc<R>(k)) << 4);
      }
      *(uint4*)(lds + off) = reg[s];
    }
  }
  // LDS-DMA fill of the same image (global_load_lds_dwordx4, 1-KiB pieces, the XOR swizzle moved
  // to the per-lane source chunk): wave `wid` issues pieces wid*PPW .. +PPW.  Rows / columns past
  // `rows` re-read the last valid ones (their outputs are never stored); k must be in range.
  static constexpr int PIECES = BYTES / 1024, PPW = PIECES / 4;
  template <bool ASM = false>
  __device__ __forceinline__ static void dma(char* lds, const bf16_t* __restrict__ p, int64_t ld, int64_t r0,
                                             int64_t rows, int64_t k0, int wid, int lane) {
#pragma unroll
    for (int j = 0; j < PPW; ++j) {
      const int pi = wid * PPW + j;
      const bf16_t* src;
      if constexpr (KC) {
        const int r = pi * 8 + (lane >> 3), c = (lane & 7) ^ swz_kc(r);
        const int64_t gr = r0 + r < rows ? r0 + r : rows - 1;
        src = p + gr * ld + k0 + c * 8;
      } else if constexpr (R == 128) {
        const int k = pi * 4 + (lane >> 4), c = (lane & 15) ^ swz_mc<R>(k);
        const int64_t gc = r0 + c * 8 <= rows - 8 ? r0 + c * 8 : rows - 8;
        src = p + (k0 + k) * ld + gc;
      } else {
        const int k = pi * 8 + (lane >> 3), c = (lane & 7) ^ swz_mc<R>(k);
        const int64_t gc = r0 + c * 8 <= rows - 8 ? r0 + c * 8 : rows - 8;
        src = p + (k0 + k) * ld + gc;
      }
      if constexpr (ASM) glds16_asm(src, lds + pi * 1024);
      else glds16(src, lds + pi * 1024);
    }
  }
  // the same fill issued by NW waves (8-wave kernels)
  template <int NW>
  __device__ __forceinline__ static void dma_nw(char* lds, const bf16_t* __restrict__ p, int64_t ld, int64_t r0,
                                                int64_t rows, int64_t k0, int wid, int lane) {
    static_assert(PIECES % NW == 0, "whole pieces per wave");
#pragma unroll
    for (int j = 0; j < PIECES / NW; ++j) {
      const int pi = wid * (PIECES / NW) + j;
      const bf16_t* src;
      if constexpr (KC) {
        const int r = pi * 8 + (lane >> 3), c = (lane & 7) ^ swz_kc(r);
        const int64_t gr = r0 + r < rows ? r0 + r : rows - 1;
        src = p + gr * ld + k0 + c * 8;
      } else if constexpr (R == 128) {
        const int k = pi * 4 + (lane >> 4), c = (lane & 15) ^ swz_mc<R>(k);
        const int64_t gc = r0 + c * 8 <= rows - 8 ? r0 + c * 8 : rows - 8;
        src = p + (k0 + k) * ld + gc;
      } else {
        const int k = pi * 8 + (lane >> 3), c = (lane & 7) ^ swz_mc<R>(k);
        const int64_t gc = r0 + c * 8 <= rows - 8 ? r0 + c * 8 : rows - 8;
        src = p + (k0 + k) * ld + gc;
      }
      glds16_asm(src, lds + pi * 1024);
    }
  }
  // fragment of rows [rb, rb+16) for the 32-deep k step kk (0/1): lane holds rows rb+(lane&15),
  // k = 32kk + 8(lane>>4) + 0..7.
  __device__ __forceinline__ static bf16x8 frag(const char* lds, int rb, int kk, int lane) {
    if constexpr (KC) {
      const int r = rb + (lane & 15);
      const int c = kk * 4 + (lane >> 4);
      return *(const bf16x8*)(lds + r * 128 + ((c ^ swz_kc(r)) << 4));
    } else {
      const int q = (lane & 15) >> 2, p4 = (lane & 3) * 4;
      const int col = rb + p4;
      const int k0 = kk * 32 + 8 * (lane >> 4) + q;
      const int k1 = k0 + 4;
      const int off0 = k0 * (R * 2) + (((col >> 3) ^ swz_mc<R>(k0)) << 4) + (col & 7) * 2;
      const int off1 = k1 * (R * 2) + (((col >> 3) ^ swz_mc<R>(k1)) << 4) + (col & 7) * 2;
      short4v t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((VS_LDS short4v*)(lds + off0));
      short4v t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((VS_LDS short4v*)(lds + off1));
      typedef __attribute__((ext_vector_type(8))) short short8v;
      short8v s = {t0[0], t0[1], t0[2], t0[3], t1[0], t1[1], t1[2], t1[3]};
      return __builtin_bit_cast(bf16x8, s);
    }
  }
};

template <int A, int B>
struct CMax {
  static constexpr int v = A > B ? A : B;
};

// ---- host: a call's runtime flags as template arguments ---------------------------------------
// call(a_kcontig, b_kcontig) or call(b_kcontig) with std::bool_constant arguments: a launcher then
// names its kernel once, `kernel<decltype(akc)::value, ...>`, and every layout is instantiated
template <class Fn>
inline void with_layout(bool a_kcontig, bool b_kcontig, Fn&& call) {
  if (a_kcontig && b_kcontig) call(std::true_type{}, std::true_type{});
  else if (a_kcontig) call(std::true_type{}, std::false_type{});
  else if (b_kcontig) call(std::false_type{}, std::true_type{});
  else call(std::false_type{}, std::false_type{});
}
template <class Fn>
inline void with_layout(bool b_kcontig, Fn&& call) {
  if (b_kcontig) call(std::true_type{});
  else call(std::false_type{});
}

// compile-time epilogue variants: the flag sets of the ViT block (vit_exec.hip) and patch embed; any
// other set runs the all-runtime epilogue.  call(EpiC<EF>{})
template <uint32_t EF>
using EpiC = std::integral_constant<uint32_t, EF>;
template <class Fn>
inline void with_epilogue(uint32_t flags, Fn&& call) {
  switch (flags) {
    case 0: call(EpiC<0u>{}); break;
    case VS_EPI_BIAS: call(EpiC<(uint32_t)VS_EPI_BIAS>{}); break;
    case VS_EPI_BIAS | VS_EPI_RESIDUAL: call(EpiC<(uint32_t)(VS_EPI_BIAS | VS_EPI_RESIDUAL)>{}); break;
    case VS_EPI_BIAS | VS_EPI_GELU: call(EpiC<(uint32_t)(VS_EPI_BIAS | VS_EPI_GELU)>{}); break;
    case VS_EPI_GELU_BWD: call(EpiC<(uint32_t)VS_EPI_GELU_BWD>{}); break;
    case VS_EPI_BIAS | VS_EPI_GELU | VS_EPI_GELU_GRAD:
      call(EpiC<(uint32_t)(VS_EPI_BIAS | VS_EPI_GELU | VS_EPI_GELU_GRAD)>{}); break;
    case VS_EPI_MUL_AUX: call(EpiC<(uint32_t)VS_EPI_MUL_AUX>{}); break;
    default: call(EpiC<kEpiRuntime>{}); break;
  }
}

}  // namespace vs
