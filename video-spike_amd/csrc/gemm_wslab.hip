// gemm_wslab.hip — vs_gemm's wide row-slab kernel for K <= 192, N > 192 (gemm.hip has the overview).
#include "common.h"
#include "gemm_common.h"
#include "gemm_paths.h"
#include "gemm_tiles.h"

namespace vs {

// ----------------------------------------------------------------------------------------------
// bf16 wide row-slab kernel for K <= 192 and N > 192 (the ViT block's qkv, fc1 + GELU and the
// GELU' dX product: outputs 3-4x the size of the input, so they are bound by their stores).  Same
// balanced row ownership as the slab kernel (workgroup g owns rows [g M / G, (g+1) M / G), one
// 64-row tile), walking the N columns in 64-wide chunks:
//   * A: each wave keeps its 32 rows x K as MFMA fragments in registers, loaded once;
//   * W chunk c+1 (64 x K, L2-resident) is register-staged: loads in flight under chunk c's MFMAs,
//     written into the one LDS image between two barriers (guide T14);
//   * the GELU' operand of chunk c+1 is loaded under chunk c too, so the epilogue never waits on
//     HBM; epilogue stores are compiler-visible, so no wait ever drains them;
//   * epilogue per wave from a wave-private LDS staging tile (32 x 32 f32), 16-B accesses.
// 2 workgroups per CU (4 waves each).
// ----------------------------------------------------------------------------------------------
template <int KT, bool BKC, uint32_t EF>
__global__ __launch_bounds__(256, 2) void gemm_bf16_wslab_kernel(const bf16_t* __restrict__ A, int64_t lda,
                                                                 const bf16_t* __restrict__ B, int64_t ldb,
                                                                 EpiParams e) {
  using OB = OperandBf16<64, BKC>;
  constexpr int KS = 2 * KT;   // 32-deep MFMA k-steps
  constexpr int LDS_T = 68;    // staging row stride (floats)
  constexpr bool MULA = (EF & VS_EPI_MUL_AUX) != 0;           // v *= aux (the stored gelu')
  constexpr bool GBWD = (EF & VS_EPI_GELU_BWD) != 0 || MULA;  // an aux operand per output
  __shared__ __attribute__((aligned(16))) char wimg[KT * OB::BYTES];
  __shared__ __attribute__((aligned(16))) float stage[4][16 * LDS_T];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int64_t G = gridDim.x;
  const int64_t r_begin = (int64_t)blockIdx.x * e.M / G, r_end = ((int64_t)blockIdx.x + 1) * e.M / G;
  const int nch = (int)(e.N / 64);
  float* st = stage[wid];
  // wave w: rows 16w .. 16w+15 of the tile, all 64 columns of a chunk (whole 128-B output rows);
  // epilogue: lane -> rows erow, erow + 8, 8-column group ecg
  const int erow = lane >> 3, ecg = lane & 7;

  for (int64_t m0 = r_begin; m0 < r_end; m0 += 64) {
    const int64_t m_end = m0 + 64 < r_end ? m0 + 64 : r_end;
    bf16x8 af[KS];
    {
      int64_t r = m0 + wid * 16 + (lane & 15);
      r = r < m_end ? r : m_end - 1;  // rows past the slab: its last row again (never stored)
      const bf16_t* p = A + r * lda + 8 * (lane >> 4);
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) af[ks] = *(const bf16x8*)(p + 32 * ks);
    }
    uint4 wreg[KT][OB::CHUNKS];
    auto load_w = [&](int c) {
#pragma unroll
      for (int t = 0; t < KT; ++t) OB::load(wreg[t], B, ldb, (int64_t)c * 64, e.N, t * 64, KT * 64, tid);
    };
    // GELU' operand of this lane's two epilogue rows of chunk c (rows past the slab: clamped), in
    // two named register sets (the chunk loop is unrolled by 2) so no copy waits on a load
    uint4 auxA[2], auxB[2];
    auto load_aux = [&](int c, uint4 (&dst)[2]) {
      if constexpr (GBWD) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          int64_t m = m0 + wid * 16 + erow + 8 * k;
          m = m < m_end ? m : m_end - 1;
          dst[k] = *(const uint4*)((const bf16_t*)e.aux_in + m * e.ld_aux_in + (int64_t)c * 64 + ecg * 8);
        }
      }
    };
    auto chunk = [&](int c, uint4 (&cur)[2], uint4 (&nxt)[2]) {
      __syncthreads();  // every wave is done reading chunk c-1's W image
#pragma unroll
      for (int t = 0; t < KT; ++t) OB::store(wimg + t * OB::BYTES, wreg[t], tid);
      __syncthreads();  // chunk c's W image complete
      if (c + 1 < nch) {
        load_w(c + 1);  // in flight under this chunk's MFMAs and epilogue
        load_aux(c + 1, nxt);
      }
      f32x4 acc[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        bf16x8 bfr[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) bfr[j] = OB::frag(wimg + (ks >> 1) * OB::BYTES, j * 16, ks & 1, lane);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[ks], bfr[j], acc[j], 0, 0, 0);
      }
      // wave-private staging: the previous chunk's epilogue reads of `st` come earlier in this
      // wave's program order, and LDS executes one wave's operations in order
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) st[((lane >> 4) * 4 + r) * LDS_T + j * 16 + (lane & 15)] = acc[j][r] * e.alpha;
      const int64_t n = (int64_t)c * 64 + ecg * 8;
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int rr = erow + 8 * k;
        const int64_t m = m0 + wid * 16 + rr;
        const float* src = st + rr * LDS_T + ecg * 8;
        float v[8];
        const float4 a = *(const float4*)src;
        const float4 b = *(const float4*)(src + 4);
        v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        if (m < m_end) {
          if constexpr (GBWD) {
            const uint32_t w[4] = {cur[k].x, cur[k].y, cur[k].z, cur[k].w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const float lo = __uint_as_float(w[q] << 16), hi = __uint_as_float(w[q] & 0xffff0000u);
              v[2 * q] *= MULA ? lo : gelu_fast_grad(lo);
              v[2 * q + 1] *= MULA ? hi : gelu_fast_grad(hi);
            }
            st8(e.c, m * e.ldc + n, e.out_bf16, v);
          } else {
            epi_eight<EF>(e, m, n, v, false);
          }
        }
      }
    };
    __syncthreads();  // the previous tile's readers of wimg are done
    load_w(0);
    load_aux(0, auxA);
    for (int c = 0; c < nch; c += 2) {
      chunk(c, auxA, auxB);
      if (c + 1 < nch) chunk(c + 1, auxB, auxA);
    }
  }
}

// ----------------------------------------------------------------------------------------------
// host
// ----------------------------------------------------------------------------------------------
// wide row-slab path: K <= 192, N > 192 (qkv, fc1 + GELU, the GELU' dX product)
bool wslab_ok(const vs_gemm_desc* d, const EpiParams& e) {
  const uint32_t f = e.flags;
  // the kernel: bf16, K-contiguous A rows held as fragments (K = 64, 128, 192), whole 64-column chunks
  // past the slab kernel's N <= 192, 16-B epilogue accesses, one pass (no split, no row sums); the
  // GELU' / aux product reads its aux operand as bf16
  const bool can = d->dtype == VS_BF16 && d->a_kcontig && d->N % 64 == 0 && d->N > 192 &&
                   (d->K == 64 || d->K == 128 || d->K == 192) && d->split_k <= 1 && !d->a_rowsum && e.vec_ok;
  // Measured (scripts/microbench.py, bench shapes): faster than the panel kernel for the GELU'
  // product (39.7 -> 36.8 us), slower than the whole-K tile kernel for the store-bound forward
  // products (qkv 19.0 -> 22.2, fc1 + GELU 37.9 -> 41.2 us), which therefore stay on it unless
  // VSPIKE_WSLAB=1 forces this path for every eligible epilogue.  Large M: the balanced slabs.
  const int all_wslab = knob(VS_KNOB_WSLAB);
  const bool pick = d->M >= 8192 &&
                    (f == VS_EPI_GELU_BWD || (f == VS_EPI_MUL_AUX && e.op_bf16) ||
                     (all_wslab && (f == 0 || f == VS_EPI_BIAS || f == (VS_EPI_BIAS | VS_EPI_GELU))));
  // knob: VSPIKE_NO_WSLAB
  return can && pick && !knob(VS_KNOB_NO_WSLAB);
}

int launch_wslab(const vs_gemm_desc* d, const EpiParams& e, hipStream_t s) {
  const bf16_t* a = (const bf16_t*)d->a;
  const bf16_t* b = (const bf16_t*)d->b;
  const int gw = knob(VS_KNOB_WSLAB_G) > 0 ? knob(VS_KNOB_WSLAB_G) : 512;
  const unsigned grid = (unsigned)(d->M / 16 < gw ? d->M / 16 : gw);
  auto go = [&](auto kt, auto ef) {
    with_layout(d->b_kcontig, [&](auto bkc) {
      hipLaunchKernelGGL((gemm_bf16_wslab_kernel<decltype(kt)::value, decltype(bkc)::value, decltype(ef)::value>), dim3(grid),
                         dim3(256), 0, s, a, d->lda, b, d->ldb, e);
    });
  };
  auto ef_switch = [&](auto kt) {  // the five epilogues the kernel is instantiated for
    switch (e.flags) {
      case 0: go(kt, EpiC<0u>{}); break;
      case VS_EPI_BIAS: go(kt, EpiC<(uint32_t)VS_EPI_BIAS>{}); break;
      case VS_EPI_BIAS | VS_EPI_GELU: go(kt, EpiC<(uint32_t)(VS_EPI_BIAS | VS_EPI_GELU)>{}); break;
      case VS_EPI_MUL_AUX: go(kt, EpiC<(uint32_t)VS_EPI_MUL_AUX>{}); break;
      default: go(kt, EpiC<(uint32_t)VS_EPI_GELU_BWD>{}); break;
    }
  };
  if (d->K == 64) ef_switch(IC<1>{});
  else if (d->K == 128) ef_switch(IC<2>{});
  else ef_switch(IC<3>{});
  VS_LAUNCH_CHECK();
  return VS_OK;
}

}  // namespace vs
