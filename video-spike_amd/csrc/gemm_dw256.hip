// gemm_dw256.hip — vs_gemm's 256 x 256 persistent weight-gradient kernel and its reduce (gemm.hip has
// the overview; the split-K dW kernel for the other shapes is gemm_dw.hip).
#include "common.h"
#include "gemm_common.h"
#include "gemm_paths.h"
#include "gemm_tiles.h"

namespace vs {

// ----------------------------------------------------------------------------------------------
// 256 x 256 persistent weight-gradient GEMM: dW[M][N] += dY^T X over the token axis for the long-K
// products of ViT-Base (C3: K = 200,704 tokens; M, N in {768, 2304, 3072}), VERDICT r4 item 3 ("a
// true long-K GEMM with few splits and large tiles").  Same engine as gemm_bf16_g256_kernel (8 waves,
// 128 x 64 per wave, C^T on the MFMA, 64-deep stages of 2 x 32 KB, two slots, one barrier per
// stage), with both operands token-major: A = dY [K][M] and B = X [K][N] are staged as [64 k][256]
// images (512-B rows, chunk ^= swz_mc(k)) and BOTH are read by ds_read_tr16_b64.  The token axis is
// cut into `splits` equal slabs; an item = (split, tile) is processed by one workgroup and its f32
// 256 x 256 partial goes to the workspace, which gemm_dw256_reduce sums IN SPLIT ORDER into C (C +=
// sum: bitwise reproducible, no atomics).  Items are dealt XCD-contiguously, split-major: the
// workgroups of one XCD share one token slab's A and B rows in its L2.  The bias gradient (row sums
// of dY) is summed from the staged A image by VALU, spread over the tile's N-column items (item
// (mt, nt) takes the k rows r % tiles_n == nt), into per-item partial rows reduced the same way.
// A tile's A fragment offsets differ per 16-row fragment only in chunk bits 1-3, which the k-row
// swizzle also uses: the read address is a lane constant XOR an immediate (one v_xor per read).
// ----------------------------------------------------------------------------------------------
struct Dw256Map {
  int tiles_n, tiles, items, per_xcd, kps, nk;
};

template <bool SUMS>
__global__ __launch_bounds__(512, 1) void gemm_dw256_kernel(const bf16_t* __restrict__ A, int64_t lda,
                                                            const bf16_t* __restrict__ B, int64_t ldb, Dw256Map g,
                                                            float* __restrict__ part, float* __restrict__ sums) {
  constexpr int AB = 64 * 256 * 2, STAGE = 2 * AB;  // 2 slots x 64 KB (+ 16 KB of bias partials)
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wr = wid >> 2, wc = wid & 3;
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, slots = gridDim.x >> 3;
  const int i_lo = xcd * g.per_xcd;
  const int i_hi = i_lo + g.per_xcd < g.items ? i_lo + g.per_xcd : g.items;
  const int my_items = i_lo + slot < i_hi ? (i_hi - i_lo - slot + slots - 1) / slots : 0;
  if (my_items == 0) return;
  auto item_of = [&](int k) __attribute__((always_inline)) { return i_lo + slot + k * slots; };
  auto steps_of = [&](int item) __attribute__((always_inline)) {
    const int k0 = (item / g.tiles) * g.kps;
    return g.nk - k0 < g.kps ? g.nk - k0 : g.kps;
  };

  // ---- DMA: wave w fills k rows 8w .. 8w+7 of both images (4 pieces of 2 k-rows x 512 B each)
  uint32_t a_off[4], b_off[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int k = wid * 8 + 2 * p + (lane >> 5), c = ((lane & 31) ^ swz_mc<128>(k)) << 4;
    a_off[p] = (uint32_t)(k * lda * 2 + c);
    b_off[p] = (uint32_t)(k * ldb * 2 + c);
  }
  // The DMA stream's global bases are recomputed (two divisions) only when it moves to a new item and
  // advanced by 64 token rows per stage otherwise; LDS destinations are wave-uniform 32-bit addresses
  // (glds16x4_m0: no per-piece generic -> LDS conversion)
  const uint32_t lds_w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(uintptr_t)(VS_LDS char*)smem) +
                         (uint32_t)__builtin_amdgcn_readfirstlane(wid) * 4096u;
  const char* dA = nullptr;
  const char* dB = nullptr;
  auto item_bases = [&](int item, int t) __attribute__((always_inline)) {
    const int sp = item / g.tiles, tile = item - sp * g.tiles, mt = tile / g.tiles_n, nt = tile - mt * g.tiles_n;
    const int64_t k0 = (int64_t)(sp * g.kps + t) * 64;
    dA = (const char*)(A + k0 * lda + (int64_t)mt * 256);
    dB = (const char*)(B + k0 * ldb + (int64_t)nt * 256);
  };
  auto issue = [&](int item, int t, int slot_s) __attribute__((always_inline)) {
    if (t == 0) item_bases(item, 0);
    else {
      dA += (int64_t)128 * lda;  // 64 token rows
      dB += (int64_t)128 * ldb;
    }
    const uint32_t l = lds_w + (uint32_t)(slot_s * STAGE);
    glds16x4_m0(dA, a_off[0], a_off[1], a_off[2], a_off[3], l, l + 1024, l + 2048, l + 3072);
    glds16x4_m0(dB, b_off[0], b_off[1], b_off[2], b_off[3], l + AB, l + AB + 1024, l + AB + 2048, l + AB + 3072);
  };

  // ---- fragments: lane (fr, fc) reads k rows kr0 = 8 fc + (fr >> 2) and kr0 + 4, columns p4 .. p4+3
  // of each 16-column block (ds_read_tr16_b64 pairs: the MFMA operand layout row = lane & 15,
  // k = 8 (lane >> 4) + 0..7).  A: block base wr*128 + rh*64 + f*16 -> address = xa ^ ((rh*8 + f*2) << 4).
  const int fr = lane & 15, fc = lane >> 4;
  const int q = fr >> 2, p4 = (lane & 3) * 4, kr0 = 8 * fc + q, kr1 = kr0 + 4;
  const int lc = wr * 16 + (p4 >> 3);
  const int xa0 = kr0 * 512 + ((lc ^ swz_mc<128>(kr0)) << 4) + (p4 & 7) * 2;
  const int xa1 = kr1 * 512 + ((lc ^ swz_mc<128>(kr1)) << 4) + (p4 & 7) * 2;
  int b_rd[4][2];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int col = wc * 64 + j * 16 + p4;
    b_rd[j][0] = AB + kr0 * 512 + (((col >> 3) ^ swz_mc<128>(kr0)) << 4) + (col & 7) * 2;
    b_rd[j][1] = AB + kr1 * 512 + (((col >> 3) ^ swz_mc<128>(kr1)) << 4) + (col & 7) * 2;
  }
  typedef __attribute__((ext_vector_type(8))) short short8v;
  auto tr_frag = [&](const char* p0, const char* p1) __attribute__((always_inline)) {
    short4v t0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((VS_LDS short4v*)p0);
    short4v t1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((VS_LDS short4v*)p1);
    short8v v = {t0[0], t0[1], t0[2], t0[3], t1[0], t1[1], t1[2], t1[3]};
    return __builtin_bit_cast(bf16x8, v);
  };
  auto read_a = [&](const char* st, int kk, int rh, bf16x8 (&af)[4]) __attribute__((always_inline)) {
#pragma unroll
    for (int f = 0; f < 4; ++f) {
      const int x = (rh * 8 + f * 2) << 4;
      af[f] = tr_frag(st + kk * 16384 + (xa0 ^ x), st + kk * 16384 + (xa1 ^ x));
    }
  };
  auto read_b = [&](const char* st, int kk, bf16x8 (&bf)[4]) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < 4; ++j) bf[j] = tr_frag(st + b_rd[j][0] + kk * 16384, st + b_rd[j][1] + kk * 16384);
  };

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // bias-gradient partials: thread -> 4-column group sg = tid & 63 of the A image, k rows
  // (tid >> 6) + 8 i whose index is = nt (mod tiles_n), 4 running sums in registers (8-column groups
  // in registers spilled 13 VGPRs; in a thread-private LDS slot they cost a read-modify-write per
  // stage: dW qkv 918 us with, 826 without the sums)
  const int sg = tid & 63, sr = tid >> 6;
  float bsum[4] = {0.f, 0.f, 0.f, 0.f};
  int bmask = 0;  // bit ii: k row sr + 8 ii belongs to this item's share (recomputed per item)
  auto set_bmask = [&](int it) __attribute__((always_inline)) {
    const int nt = (it % g.tiles) % g.tiles_n;
    bmask = 0;
#pragma unroll
    for (int ii = 0; ii < 8; ++ii) bmask |= ((sr + 8 * ii) % g.tiles_n == nt) << ii;
  };
  auto bias_rows = [&](const char* st) __attribute__((always_inline)) {
#pragma unroll
    for (int ii = 0; ii < 8; ++ii) {
      const int r = sr + 8 * ii;
      if ((bmask >> ii) & 1) {
        const uint2 u = *(const uint2*)(st + r * 512 + (((sg >> 1) ^ swz_mc<128>(r)) << 4) + (sg & 1) * 8);
        bsum[0] += __uint_as_float(u.x << 16);
        bsum[1] += __uint_as_float(u.x & 0xffff0000u);
        bsum[2] += __uint_as_float(u.y << 16);
        bsum[3] += __uint_as_float(u.y & 0xffff0000u);
      }
    }
  };
  auto epilogue = [&](int item) __attribute__((always_inline)) {
    float* pt = part + (int64_t)item * 65536;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const float v[4] = {acc[i][jj][0], acc[i][jj][1], acc[i][jj][2], acc[i][jj][3]};
        st4(pt, (wr * 128 + i * 16 + fr) * 256 + wc * 64 + jj * 16 + 4 * fc, 0, v);
        acc[i][jj] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
    if constexpr (SUMS) {
      *(float4*)(sums + ((int64_t)item * 8 + sr) * 256 + sg * 4) = make_float4(bsum[0], bsum[1], bsum[2], bsum[3]);
#pragma unroll
      for (int c = 0; c < 4; ++c) bsum[c] = 0.f;
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

  bf16x8 a0[4], a1[4], b0[4], b1[4];
  int item = item_of(0), nsteps = steps_of(item), k = 0, t = 0, s = 0;
  if constexpr (SUMS) set_bmask(item);
  issue(item, 0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
  read_b(smem, 0, b0);
  read_a(smem, 0, 0, a0);
  // the four phases of gemm_bf16_g256_kernel's stage loop; (k, t) walks this workgroup's items and
  // their k-steps, the ring continues across items
  while (true) {
    const char* cur = smem + (s & 1) * STAGE;
    int nk_item = k, nt_step = t + 1;
    if (nt_step == nsteps) {
      nk_item = k + 1;
      nt_step = 0;
    }
    const bool more = nk_item < my_items;
    const int nitem = nk_item == k ? item : (more ? item_of(nk_item) : item);
    if (more) issue(nitem, nt_step, (s + 1) & 1);
    read_a(cur, 0, 1, a1);
    __builtin_amdgcn_sched_barrier(0);
    mfma16(b0, a0, 0);
    read_b(cur, 1, b1);
    read_a(cur, 1, 0, a0);
    __builtin_amdgcn_sched_barrier(0);
    mfma16(b0, a1, 1);
    read_a(cur, 1, 1, a1);
    __builtin_amdgcn_sched_barrier(0);
    mfma16(b1, a0, 0);
    if constexpr (SUMS) bias_rows(cur);  // behind the queued MFMAs (a0's registers are dead here)
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (more) {
      const char* nxt = smem + ((s + 1) & 1) * STAGE;
      read_b(nxt, 0, b0);
      read_a(nxt, 0, 0, a0);
    }
    __builtin_amdgcn_sched_barrier(0);
    mfma16(b1, a1, 1);
    if (nk_item != k) epilogue(item);
    if (!more) break;
    if (nk_item != k) {
      item = nitem;
      nsteps = steps_of(item);
      if constexpr (SUMS) set_bmask(item);
    }
    k = nk_item;
    t = nt_step;
    ++s;
  }
}

// C[m][n] += sum over splits (in order) of the items' partial tiles; bias[m] += the bias partials
// (splits, then the tile row's N-column items, then the 8 partial rows, in order).  One thread per
// output float4, then one per bias element.
__global__ __launch_bounds__(256) void gemm_dw256_reduce(const float* __restrict__ part, const float* __restrict__ sums,
                                                         Dw256Map g, int splits, int64_t M, int64_t N,
                                                         float* __restrict__ c, int64_t ldc, float* __restrict__ bias) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x, nc4 = M * N / 4;
  if (i < nc4) {
    const int64_t m = i / (N / 4), n = (i % (N / 4)) * 4;
    const int tile = (int)(m / 256) * g.tiles_n + (int)(n / 256);
    const int64_t off = (m % 256) * 256 + (n % 256);
    float4 acc = *(const float4*)(part + (int64_t)tile * 65536 + off);
    for (int sp = 1; sp < splits; ++sp) {
      const float4 v = *(const float4*)(part + ((int64_t)sp * g.tiles + tile) * 65536 + off);
      acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    float4* cp = (float4*)(c + m * ldc + n);
    float4 o = *cp;
    o.x += acc.x; o.y += acc.y; o.z += acc.z; o.w += acc.w;
    *cp = o;
  } else if (bias && i < nc4 + M) {
    const int64_t m = i - nc4;
    const int mt = (int)(m / 256), ml = (int)(m % 256);
    float a = 0.f;
    for (int sp = 0; sp < splits; ++sp)
      for (int nt = 0; nt < g.tiles_n; ++nt) {
        const float* p = sums + ((int64_t)(sp * g.tiles + mt * g.tiles_n + nt) * 8) * 256 + ml;
#pragma unroll
        for (int r = 0; r < 8; ++r) a += p[r * 256];
      }
    bias[m] += a;
  }
}

// the split count: every workgroup one item per round (256 slots), the busiest one's k-steps
// (plus ~4 steps' worth per item for its partial-tile store) minimised, partials <= 128 MB
struct Dw256Plan {
  bool valid;
  int splits;
  Dw256Map g;
};
static Dw256Plan plan_dw256(int64_t M, int64_t N, int64_t K) {
  Dw256Plan p = {};
  // 768 x 768 (the projection's dW) measured no faster than the split-K dW tiles: 326 vs 308 us
  if (M % 256 || N % 256 || K % 64 || K < 64 * 64 || (M * N <= 768 * 768 && knob(VS_KNOB_DW256_ALL) != 1)) return p;
  const int64_t tiles = (M / 256) * (N / 256), nk = K / 64;
  double best = 1e30;
  for (int64_t S0 = 1; S0 <= 256 && S0 * 8 <= nk; ++S0) {
    const int64_t kps = (nk + S0 - 1) / S0, S = (nk + kps - 1) / kps;  // no empty last split
    const int64_t items = tiles * S;
    if (items * 65536 * 4 > (128ll << 20)) break;
    const int64_t rounds = (items + 255) / 256;
    const double t = (double)rounds * (double)(kps + 4);
    if (t < best - 1e-9) {
      best = t;
      p.valid = true;
      p.splits = (int)S;
      p.g.kps = (int)kps;
    }
  }
  if (!p.valid) return p;
  p.g.tiles_n = (int)(N / 256);
  p.g.tiles = (int)tiles;
  p.g.items = (int)(tiles * p.splits);
  p.g.per_xcd = (p.g.items + 7) / 8;
  p.g.nk = (int)nk;
  return p;
}
size_t dw256_workspace_bytes(int64_t M, int64_t N, int64_t K) {
  const Dw256Plan p = plan_dw256(M, N, K);
  return p.valid ? (size_t)p.g.items * (65536 + 8 * 256) * 4 : 0;
}

// ----------------------------------------------------------------------------------------------
// host
// ----------------------------------------------------------------------------------------------
// token-reduction weight gradients (dW = dY^T X, both operands token-major): the long-K products
// with 256-multiple widths on this kernel, the rest on the split-K dW kernel (gemm_dw.hip); both
// reduce their partials in a fixed order
bool dw256_ok(const vs_gemm_desc* d, const EpiParams& e) {
  // the kernel: both bf16 operands token-major with 16-B rows, f32 C += the partials (16-B rows of C)
  // and nothing else -- it does not scale by alpha (alpha != 1 takes the generic split-K tiles, whose
  // store_tile multiplies every split's partial tile), and an explicit split_k is theirs too; a
  // 64-token stage within 32-bit per-lane DMA offsets; a plan (256-multiple widths, K % 64 == 0, >= 64
  // stages) whose partials fit the caller's workspace
  const bool can = d->alpha == 1.0f && d->dtype == VS_BF16 && d->out_dtype == VS_F32 && e.flags == VS_EPI_ATOMIC &&
                   !d->a_kcontig && !d->b_kcontig && d->split_k <= 0 && splitk_ws(d) && d->lda % 8 == 0 && d->ldb % 8 == 0 &&
                   d->ldc % 4 == 0 && aligned16(d->c) && 64 * d->lda * 2 < (1ll << 31) && 64 * d->ldb * 2 < (1ll << 31);
  if (!can) return false;
  // measured: plan_dw256 leaves 768 x 768 to the split-K dW tiles (unless VSPIKE_DW256_ALL=1)
  if (!plan_dw256(d->M, d->N, d->K).valid || (size_t)d->workspace_bytes < dw256_workspace_bytes(d->M, d->N, d->K)) return false;
  // knob: VSPIKE_NO_DW256
  return !knob(VS_KNOB_NO_DW256);
}

int launch_dw256(const vs_gemm_desc* d, const EpiParams&, hipStream_t s) {
  const Dw256Plan p = plan_dw256(d->M, d->N, d->K);
  float* part = (float*)d->workspace;
  float* sums = part + (int64_t)p.g.items * 65536;
  const unsigned grid = p.g.items < 256 ? (unsigned)((p.g.items + 7) / 8 * 8) : 256u;
  if (d->a_rowsum)
    hipLaunchKernelGGL((gemm_dw256_kernel<true>), dim3(grid), dim3(512), 0, s, (const bf16_t*)d->a, d->lda,
                       (const bf16_t*)d->b, d->ldb, p.g, part, sums);
  else
    hipLaunchKernelGGL((gemm_dw256_kernel<false>), dim3(grid), dim3(512), 0, s, (const bf16_t*)d->a, d->lda,
                       (const bf16_t*)d->b, d->ldb, p.g, part, sums);
  const int64_t n = d->M * d->N / 4 + (d->a_rowsum ? d->M : 0);
  hipLaunchKernelGGL(gemm_dw256_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part, sums, p.g, p.splits,
                     d->M, d->N, (float*)d->c, d->ldc, d->a_rowsum);
  VS_LAUNCH_CHECK();
  return VS_OK;
}

}  // namespace vs
