// conv_dw.hip — Conv3d weight gradient of the R3D-18 encoder (conv_common.h has the design notes):
// dw[o][k] (+)= sum_m dy[m][o] * gather(x)[m][k]
#include "conv_common.h"

namespace vs {

struct ConvDw {
  const float* x;
  int N, Di, Hi, Wi, C, cshift;
  int Do, Ho, Wo;             // output (row) grid
  int sd, sh, sw, pd, ph, pw;
  int kd, kh, kw;
  const float* dy;            // [M][Co]
  int Co, K;                  // K = kd*kh*kw*C
  int64_t M;
  int splits, steps_per_split;  // rows of a split: steps_per_split * 32
  float* part;                // [splits][Co][Kp], Kp = tiles_k * 64
  int Kp;
};

// One schedule: a 64 out channel x 64 k tile per workgroup, four v_mfma_f32_16x16x4_f32 chains per wave,
// two steps (of 32 voxel rows) of global loads in flight.  Two variants were measured slower at C4 and
// are gone (DESIGN.md has the record):
//   * 128 k columns per tile read the dy slab (the tile's A operand) half as often (the dy of one voxel
//     row slab is re-read by every k tile of the product): conv dW 40.9 vs 39.4 ms/step;
//   * v_mfma_f32_32x32x2_f32 on each wave's 32 x 32 output block: the same MACs and operand reads (one A
//     and one B dword per lane per 2 k) with half the MFMA instructions (half the issue slots the matrix
//     pipe takes from the gather's VALU / LDS work), but one dependent 64-cycle accumulation chain per
//     wave instead of four independent 32-cycle ones: conv dW 37.3 vs 32.5 ms/step
//     (profiles/r06_r3d_ab_mfma.json).
__global__ __launch_bounds__(256, 2) void conv_dw_kernel(ConvDw g) {
  constexpr int BO = 64, BK = 64, BM = 32, LDO = 80, LD = BK + 16;   // row strides % 32 == 16: conflict-free b32 reads
  constexpr int SO = BM * LDO, STAGE = SO + BM * LD;
  __shared__ __attribute__((aligned(16))) float smem[2 * STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wr = wid >> 1, wc = wid & 1;
  const int tiles_o = g.Co / BO, tiles_k = g.Kp / BK;  // Kp: K rounded up to BK
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int split = bid / (tiles_o * tiles_k), rem = bid % (tiles_o * tiles_k);
  const int ot = rem / tiles_k, kt = rem % tiles_k;
  const int o0 = ot * BO, k0 = kt * BK;
  const int64_t mb = (int64_t)split * g.steps_per_split * BM;
  int64_t me = mb + (int64_t)g.steps_per_split * BM;
  if (me > g.M) me = g.M;
  const int nsteps = me > mb ? (int)((me - mb + BM - 1) / BM) : 0;
  // both operand slabs are 32 rows x 16 float4 (BO = BK = 64): this thread loads and stores float4
  // `chunk` (along o of dy, along k of the gather) of rows `row` and `row + 16`
  const int chunk = tid & 15, row = tid >> 4;
  // the gather's k chunk: tap and channel are fixed for the whole launch of this thread
  const int k = k0 + chunk * 4;
  const bool kok = k < g.K;
  const int tap = k >> g.cshift, c = k & (g.C - 1);
  const int khw = g.kh * g.kw;
  const int td = tap / khw, tr = tap - td * khw, th = tr / g.kw, tw = tr - th * g.kw;
  const int oz = td - g.pd, oy = th - g.ph, ox = tw - g.pw;
  const float ihw = 1.0f / (float)g.Wo, ihh = 1.0f / (float)g.Ho, ihd = 1.0f / (float)g.Do;

  // Operand addresses as 32-bit element offsets (the host checks M < 2^24, M Co < 2^31 and the input
  // volume x C < 2^31).  The gather's voxel coordinates are advanced incrementally: each thread keeps
  // the (n, z0 = gd sd, y0 = gh sh, x0 = gw sw) of its row slots and adds the mixed-radix digits of
  // one step (32 rows) with one conditional carry per digit, instead of three divisions per row and
  // step (the int64 index chains with three float-reciprocal divisions per row were ~200 VALU per
  // step, VALU : MFMA 6.5 : 1 in the counters, profiles/r05_pmc_convdw.json)
  const int me32 = (int)me, mb32 = (int)mb;
  const auto rsx = conv_rsrc(g.x, (g.N * g.Di * g.Hi * g.Wi) << (g.cshift + 2));
  const auto rsdy = conv_rsrc(g.dy, (int)g.M * g.Co * 4);
  const int XW = g.Wo * g.sw, YH = g.Ho * g.sh, ZD = g.Do * g.sd;
  int cW, cH, cD, cN;  // the step's digits (x0, y0, z0 strides; n count)
  {
    int q = BM;
    cW = (q % g.Wo) * g.sw; q /= g.Wo;
    cH = (q % g.Ho) * g.sh; q /= g.Ho;
    cD = (q % g.Do) * g.sd; q /= g.Do;
    cN = q;
  }
  int sx0[2], sy0[2], sz0[2], sn[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int m = mb32 + row + 16 * s;
    // (a slot past the split end only ever loads zeros)
    const RowPos p = row_decode(m < me32 ? m : 0, g.Do, g.Ho, g.Wo, ihd, ihh, ihw);
    sx0[s] = p.gw * g.sw;
    sy0[s] = p.gh * g.sh;
    sz0[s] = p.gd * g.sd;
    sn[s] = p.n;
  }
  auto advance = [&]() {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      int x0 = sx0[s] + cW;
      const bool cw = x0 >= XW;
      x0 -= cw ? XW : 0;
      int y0 = sy0[s] + cH + (cw ? g.sh : 0);
      const bool ch = y0 >= YH;
      y0 -= ch ? YH : 0;
      int z0 = sz0[s] + cD + (ch ? g.sd : 0);
      const bool cd = z0 >= ZD;
      z0 -= cd ? ZD : 0;
      sx0[s] = x0;
      sy0[s] = y0;
      sz0[s] = z0;
      sn[s] += cN + (cd ? 1 : 0);
    }
  };
  // load(step) reads the slots' current coordinates: called for steps 0, 1, 2, ... in order, each
  // call followed by advance()
  auto load = [&](float4 (&rd)[2], float4 (&rx)[2], int step) {
    const int mstep = mb32 + step * BM;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int m = mstep + row + 16 * s;
      const bool ok = m < me32;
      rd[s] = bload4(rsdy, ok ? (uint32_t)(mul24(m, g.Co) + o0 + chunk * 4) * 4u : kOob);
    }
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int m = mstep + row + 16 * s;
      const int z = sz0[s] + oz, yy = sy0[s] + oy, xx = sx0[s] + ox;
      const bool in = m < me32 && kok && (unsigned)z < (unsigned)g.Di && (unsigned)yy < (unsigned)g.Hi &&
                      (unsigned)xx < (unsigned)g.Wi;
      const int vox = mul24(mul24(mul24(sn[s], g.Di) + z, g.Hi) + yy, g.Wi) + xx;
      rx[s] = bload4(rsx, in ? (uint32_t)((vox << g.cshift) + c) * 4u : kOob);
    }
    advance();
  };

  auto store = [&](float* st, const float4 (&rd)[2], const float4 (&rx)[2]) {
#pragma unroll
    for (int s = 0; s < 2; ++s) *(float4*)(st + (row + 16 * s) * LDO + chunk * 4) = rd[s];
#pragma unroll
    for (int s = 0; s < 2; ++s) *(float4*)(st + SO + (row + 16 * s) * LD + chunk * 4) = rx[s];
  };

  // blocked accumulation: the MFMA chain runs over 16 steps (512 voxels), then folds into tot —
  // one f32 chain over a whole split (up to ~40k voxels at 16 clips) lets rounding grow with its
  // length, and these sums cancel strongly (the gradient of a conv feeding a BatchNorm)
  f32x4 acc[2][2], tot[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = tot[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float4 rd[2], rx[2];
  if (nsteps > 0) {
    load(rd, rx, 0);
    store(smem, rd, rx);
  }
  // Two steps of global loads in flight (round 6): step t+2's dy / gather rows are loaded into the
  // register set not being stored this step, so a load has a whole step of MFMAs plus the next
  // step's to land before its LDS store (one step ahead, the stores waited on L2 / HBM latency:
  // wait_inst 0.62 of wave cycles, profiles/r05_pmc_convdw.json).  The two sets alternate by unrolling.
  float4 rdb[2], rxb[2];
  if (nsteps > 1) load(rd, rx, 1);
  __syncthreads();
  constexpr int NS = BM / 4, HS = NS / 2;
  auto body = [&](int t, float4 (&sd1)[2], float4 (&sx1)[2], float4 (&ld2)[2], float4 (&lx2)[2]) {
    const float* sd_ = smem + (t & 1) * STAGE;
    const float* sx = sd_ + SO;
    if (t + 2 < nsteps) load(ld2, lx2, t + 2);
    float af[NS][2], bfr[NS][2];
    auto rd_ops = [&](int sub) {
      const int mrow = 4 * sub + (lane >> 4);
#pragma unroll
      for (int i = 0; i < 2; ++i) af[sub][i] = sd_[mrow * LDO + wr * 32 + i * 16 + (lane & 15)];
#pragma unroll
      for (int j = 0; j < 2; ++j) bfr[sub][j] = sx[mrow * LD + wc * 32 + j * 16 + (lane & 15)];
    };
    auto mm_ops = [&](int sub) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[sub][i], bfr[sub][j], acc[i][j], 0, 0, 0);
    };
    // operand fragments read a half-step (4 sub-steps) ahead of their MFMAs: reading each sub-step's
    // 4 values right before its 4 MFMAs (hipcc's choice, reusing 4 registers) serialised every
    // sub-step behind an LDS round trip (conv dW 34.0 -> 32.5 ms/step at C4; the same change in
    // conv_igemm_kernel, 146 VGPRs, measured slower: fwd 25.1 -> 26.2, dX 26.0 -> 26.9)
#pragma unroll
    for (int sub = 0; sub < HS; ++sub) rd_ops(sub);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int sub = HS; sub < NS; ++sub) rd_ops(sub);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int sub = 0; sub < HS; ++sub) mm_ops(sub);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int sub = HS; sub < NS; ++sub) mm_ops(sub);
    if (t + 1 < nsteps) store(smem + ((t + 1) & 1) * STAGE, sd1, sx1);
    if ((t & 15) == 15) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          tot[i][j] += acc[i][j];
          acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    }
    __syncthreads();
  };
  for (int t = 0; t < nsteps; t += 2) {
    body(t, rd, rx, rdb, rxb);                     // stores step t+1 from (rd, rx), loads t+2 into (rdb, rxb)
    if (t + 1 < nsteps) body(t + 1, rdb, rxb, rd, rx);
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] += tot[i][j];
  // partial tile (plain stores; the reduce adds the splits in order)
  float* pt = g.part + (int64_t)split * g.Co * g.Kp;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = o0 + wr * 32 + i * 16 + 4 * (lane >> 4) + r;
        const int kk = k0 + wc * 32 + j * 16 + (lane & 15);
        pt[(int64_t)o * g.Kp + kk] = acc[i][j][r];
      }
}

// dw[o][k] (=|+=) sum_s part[s][o][k] for k < K (float4 over k when K % 4 == 0)
__global__ __launch_bounds__(256) void conv_dw_reduce(const float* __restrict__ part, int splits, int Co, int K,
                                                      int Kp, float* __restrict__ dw, int accumulate) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t n = (int64_t)Co * K;
  if (i >= n) return;
  const int o = (int)(i / K), k = (int)(i % K);
  const int64_t src = (int64_t)o * Kp + k, plane = (int64_t)Co * Kp;
  float s = 0.f;
  for (int sp = 0; sp < splits; ++sp) s += part[sp * plane + src];
  dw[i] = accumulate ? dw[i] + s : s;
}

struct DwPlanC {
  int tiles_o, tiles_k, Kp, splits, sps;
};
static DwPlanC plan_conv_dw(const vs_conv3d_desc* d) {
  DwPlanC p;
  const int K = d->kd * d->kh * d->kw * (int)d->Ci;
  p.tiles_o = (int)(d->Co / 64);
  p.tiles_k = (K + 63) / 64;
  p.Kp = p.tiles_k * 64;
  const int64_t M = d->N * d->Do * d->Ho * d->Wo;
  const int64_t steps = (M + 31) / 32;
  const int tiles = p.tiles_o * p.tiles_k;
  int64_t S = (1024 + tiles - 1) / tiles;        // ~4 workgroups per CU
  const int64_t smax = steps / 16 > 0 ? steps / 16 : 1;   // >= 16 row steps per split
  if (S > smax) S = smax;
  if (S < 1) S = 1;
  p.sps = (int)((steps + S - 1) / S);
  p.splits = (int)((steps + p.sps - 1) / p.sps);
  return p;
}
}  // namespace vs

using namespace vs;

extern "C" size_t vs_conv3d_dw_workspace_bytes(const vs_conv3d_desc* d) {
  if (!desc_ok(d) || d->Co % 64) return 0;
  const DwPlanC p = plan_conv_dw(d);
  return (size_t)p.splits * d->Co * p.Kp * 4 + 256;
}

extern "C" int vs_conv3d_dw(const vs_conv3d_desc* d, const float* x, const float* dy, float* dw, int32_t accumulate,
                            void* workspace, int64_t workspace_bytes, void* stream) {
  VS_REQUIRE(desc_ok(d), "vs_conv3d_dw: inconsistent geometry");
  VS_REQUIRE(x && dy && dw && workspace, "vs_conv3d_dw: null pointer");
  const int cs = ilog2(d->Ci);
  VS_REQUIRE(cs >= 2 && d->Co % 64 == 0, "vs_conv3d_dw: Ci must be a power of two >= 4, Co a multiple of 64");
  VS_REQUIRE((size_t)workspace_bytes >= vs_conv3d_dw_workspace_bytes(d), "vs_conv3d_dw: workspace too small");
  VS_REQUIRE(aligned16(x) && aligned16(dy) && aligned16(workspace), "vs_conv3d_dw: pointers must be 16-byte aligned");
  const int64_t M = d->N * d->Do * d->Ho * d->Wo;
  VS_REQUIRE(M < (1ll << 24) && M * d->Co < (1ll << 29) && d->N * d->Di * d->Hi * d->Wi < (1ll << 24) &&
                 d->N * d->Di * d->Hi * d->Wi * d->Ci < (1ll << 29),
             "vs_conv3d_dw: volume too large (operands must stay below 2^31 bytes)");
  hipStream_t s = (hipStream_t)stream;
  ScopedTimer timer(VS_TIMER_CONV_DW, s, conv_flops(d));
  const DwPlanC p = plan_conv_dw(d);
  ConvDw g = {};
  g.x = x; g.N = (int)d->N; g.Di = (int)d->Di; g.Hi = (int)d->Hi; g.Wi = (int)d->Wi; g.C = (int)d->Ci; g.cshift = cs;
  g.Do = (int)d->Do; g.Ho = (int)d->Ho; g.Wo = (int)d->Wo;
  g.sd = d->sd; g.sh = d->sh; g.sw = d->sw; g.pd = d->pd; g.ph = d->ph; g.pw = d->pw;
  g.kd = d->kd; g.kh = d->kh; g.kw = d->kw;
  g.dy = dy; g.Co = (int)d->Co; g.K = d->kd * d->kh * d->kw * (int)d->Ci;
  g.M = M; g.splits = p.splits; g.steps_per_split = p.sps; g.part = (float*)workspace; g.Kp = p.Kp;
  count_path(VS_PATH_CONV_DW);
  const int64_t nwg = (int64_t)p.splits * p.tiles_o * p.tiles_k;
  hipLaunchKernelGGL(conv_dw_kernel, dim3((unsigned)nwg), dim3(256), 0, s, g);
  VS_LAUNCH_CHECK();
  const int64_t n = d->Co * (int64_t)g.K;
  hipLaunchKernelGGL(conv_dw_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float*)workspace,
                     p.splits, g.Co, g.K, p.Kp, dw, accumulate);
  VS_LAUNCH_CHECK();
  return VS_OK;
}
