// conv_igemm.hip — Conv3d forward and input gradient of the R3D-18 encoder: one implicit-GEMM kernel
// (conv_common.h has the design notes).  The forward gathers x; dX gathers dy with the flipped offsets,
// one launch per parity class of the input positions.
#include "conv_common.h"

namespace vs {

// ------------------------------------------------------------------------------------------------
// geometry of one implicit-GEMM launch
// ------------------------------------------------------------------------------------------------
struct Igemm {
  const float* x;             // gathered operand, channels-last [N][Di][Hi][Wi][C]
  int N, Di, Hi, Wi, C, cshift;
  int Gd, Gh, Gw;             // GEMM row grid: rows = N * Gd * Gh * Gw
  int sd, sh, sw;             // input step per grid step
  // taps: per dim j in [0, cnt): input offset o0 + ostep * j (added to g * s)
  int cd, ch, cw;
  int od0, oh0, ow0, ods, ohs, ows;
  const float* w;             // [Ng][K] K-contiguous, K = cd*ch*cw * C
  int Ng, K;
  float* y;                   // output, channels-last with Ng channels, storage grid Od x Oh x Ow
  int Od, Oh, Ow;
  int ysd, ysh, ysw, yod, yoh, yow;   // output voxel = g * ys + yo
  int accumulate;
  float* stats;               // [tiles_m][2][Ng] per 128-row tile: column sum of y, sum of (y - tile mean)^2; or null
  int64_t M;
};

// a gathered float4 into an operand image: rows of kLdA floats are only 8-byte aligned (two ds_write_b64)
__device__ __forceinline__ void lds_store4(float* d, const float4& v) {
  *(float2*)d = make_float2(v.x, v.y);
  *(float2*)(d + 2) = make_float2(v.z, v.w);
}

__global__ __launch_bounds__(256, 2) void conv_igemm_kernel(Igemm g) {
  constexpr int BM = 128, BN = 64, BK = 32, LD = kLdA;
  constexpr int SA = BM * LD, SB = BN * LD, STAGE = SA + SB;
  __shared__ __attribute__((aligned(16))) float smem[2 * STAGE];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, wr = wid >> 1, wc = wid & 1;
  const int tiles_n = g.Ng / BN;
  const int bid = xcd_remap(blockIdx.x, gridDim.x);
  const int mt = bid / tiles_n, nt = bid % tiles_n;
  const int64_t m0 = (int64_t)mt * BM;
  const int n0 = nt * BN;
  const int chunk = tid & 7;  // float4 index along k of this thread's operand loads
  const float ihw = 1.0f / (float)g.Gw, ihh = 1.0f / (float)g.Gh, ihd = 1.0f / (float)g.Gd;

  // the 4 A rows of this thread (rows tid/8 + 32 s): voxel coordinates of the gathered input and the
  // voxel index of the row's tap-(0,0,0) origin.  Operand offsets are 32-bit (the host checks the
  // gathered volume x C < 2^31): the int64 index chain and the two integer divisions of the tap
  // were 31 v_mul_lo_u32 + 12 64-bit multiply-adds (quarter rate) per k step
  int rz[4], ry[4], rx[4], rvb[4];
  bool rok[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int64_t m = m0 + (tid >> 3) + 32 * s;
    rok[s] = m < g.M;
    const RowPos p = row_decode(rok[s] ? (int)m : 0, g.Gd, g.Gh, g.Gw, ihd, ihh, ihw);
    rz[s] = p.gd * g.sd;
    ry[s] = p.gh * g.sh;
    rx[s] = p.gw * g.sw;
    rvb[s] = ((p.n * g.Di + rz[s]) * g.Hi + ry[s]) * g.Wi + rx[s];
  }
  const int chw = g.ch * g.cw;
  const float ichw = 1.0f / (float)chw, icw = 1.0f / (float)g.cw;
  const auto rsx = conv_rsrc(g.x, (g.N * g.Di * g.Hi * g.Wi) << (g.cshift + 2));
  const auto rsw = conv_rsrc(g.w, g.Ng * g.K * 4);
  auto load_a = [&](float4 (&ra)[4], int k0) {
    const int k = k0 + chunk * 4;
    const bool kok = k < g.K;
    const int tap = k >> g.cshift, c = k & (g.C - 1);
    const int jd = divq(tap, chw, ichw), jr = tap - mul24(jd, chw);
    const int jh = divq(jr, g.cw, icw), jw = jr - mul24(jh, g.cw);
    const int oz = g.od0 + __mul24(g.ods, jd), oy = g.oh0 + __mul24(g.ohs, jh), ox = g.ow0 + __mul24(g.ows, jw);
    const int toff = __mul24(__mul24(oz, g.Hi) + oy, g.Wi) + ox;  // voxel offset of the tap (may be < 0)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int z = rz[s] + oz, yy = ry[s] + oy, xx = rx[s] + ox;
      const bool ok = kok && rok[s] && (unsigned)z < (unsigned)g.Di && (unsigned)yy < (unsigned)g.Hi &&
                      (unsigned)xx < (unsigned)g.Wi;
      ra[s] = bload4(rsx, ok ? (uint32_t)(((rvb[s] + toff) << g.cshift) + c) * 4u : kOob);
    }
  };
  auto load_b = [&](float4 (&rb)[2], int k0) {
    const int k = k0 + chunk * 4;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int n = n0 + (tid >> 3) + 32 * s;
      rb[s] = bload4(rsw, k < g.K ? (uint32_t)(n * g.K + k) * 4u : kOob);
    }
  };
  auto store = [&](float* st, const float4 (&ra)[4], const float4 (&rb)[2]) {
#pragma unroll
    for (int s = 0; s < 4; ++s) lds_store4(st + ((tid >> 3) + 32 * s) * LD + chunk * 4, ra[s]);
#pragma unroll
    for (int s = 0; s < 2; ++s) lds_store4(st + SA + ((tid >> 3) + 32 * s) * LD + chunk * 4, rb[s]);
  };

  f32x4 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nk = (g.K + BK - 1) / BK;
  float4 ra[4], rb[2];
  load_a(ra, 0);
  load_b(rb, 0);
  store(smem, ra, rb);
  __syncthreads();
  for (int t = 0; t < nk; ++t) {
    const float* sa = smem + (t & 1) * STAGE;
    const float* sb = sa + SA;
    const bool more = t + 1 < nk;
    if (more) {
      load_a(ra, (t + 1) * BK);
      load_b(rb, (t + 1) * BK);
    }
#pragma unroll
    for (int sub = 0; sub < BK / 4; ++sub) {
      const int kk = 4 * sub + (lane >> 4);
      float af[4], bfr[2];
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i] = sa[(wr * 64 + i * 16 + (lane & 15)) * LD + kk];
#pragma unroll
      for (int j = 0; j < 2; ++j) bfr[j] = sb[(wc * 32 + j * 16 + (lane & 15)) * LD + kk];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
    if (more) store(smem + ((t + 1) & 1) * STAGE, ra, rb);
    __syncthreads();
  }

  // epilogue: acc[i][j][r] = C[wr*64 + i*16 + 4*(lane>>4) + r][wc*32 + j*16 + (lane&15)]
  float csum[2] = {0.f, 0.f};
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t m = m0 + wr * 64 + i * 16 + 4 * (lane >> 4) + r;
      if (m >= g.M) continue;
      const RowPos p = row_decode((int)m, g.Gd, g.Gh, g.Gw, ihd, ihh, ihw);
      const int64_t vox = (((int64_t)p.n * g.Od + p.gd * g.ysd + g.yod) * g.Oh + p.gh * g.ysh + g.yoh) * g.Ow +
                          p.gw * g.ysw + g.yow;
      float* dst = g.y + vox * g.Ng + n0 + wc * 32 + (lane & 15);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        float v = acc[i][j][r];
        if (g.accumulate) v += dst[j * 16];
        dst[j * 16] = v;
        acc[i][j][r] = v;  // the stored value, for the tile's second statistics pass
        csum[j] += v;
      }
    }
  if (g.stats) {
    // BatchNorm partials per 128-row tile: the column sum S and the sum of squared deviations from
    // the TILE's own column mean, M2 = sum (y - S/n)^2 (two passes over the registers), merged later
    // with Chan's formula in f64.  A single-pass sum of y^2 loses the variance to cancellation in f32
    // when |mean| >> std (trained weights): E[y^2] - mean^2.
    __shared__ float red[2][2][64];
    __syncthreads();  // (smem reads done; red is a separate array written once)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float v = csum[j];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      if (lane < 16) red[wr][0][wc * 32 + j * 16 + lane] = v;
    }
    __syncthreads();
    const int64_t nrows = g.M - m0 < BM ? g.M - m0 : BM;
    const float inv_n = 1.0f / (float)nrows;
    float csq[2] = {0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = wc * 32 + j * 16 + (lane & 15);
      const float mu = (red[0][0][col] + red[1][0][col]) * inv_n;
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int64_t m = m0 + wr * 64 + i * 16 + 4 * (lane >> 4) + r;
          const float dv = acc[i][j][r] - mu;
          csq[j] += m < g.M ? dv * dv : 0.f;
        }
      float q = csq[j];
      q += __shfl_xor(q, 16, 64);
      q += __shfl_xor(q, 32, 64);
      if (lane < 16) red[wr][1][wc * 32 + j * 16 + lane] = q;
    }
    __syncthreads();
    if (tid < 128) {
      const int which = tid >> 6, col = tid & 63;
      g.stats[((int64_t)mt * 2 + which) * g.Ng + n0 + col] = red[0][which][col] + red[1][which][col];
    }
  }
}

// dX weights of one parity class: wd[ci][(jd, jh, jw)][co] = w[co][td][th][tw][ci], t = t0 + tstep j
__global__ __launch_bounds__(256) void conv_dx_weights(const float* __restrict__ w, int Co, int Ci, int kd, int kh,
                                                       int kw, int cd, int ch, int cw, int t0d, int t0h, int t0w,
                                                       int tsd, int tsh, int tsw, float* __restrict__ wd) {
  const int T = cd * ch * cw;
  const int64_t n = (int64_t)Ci * T * Co;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int co = (int)(i % Co);
  const int64_t q = i / Co;
  const int j = (int)(q % T), ci = (int)(q / T);
  const int jd = j / (ch * cw), jr = j % (ch * cw), jh = jr / cw, jw = jr % cw;
  const int td = t0d + tsd * jd, th = t0h + tsh * jh, tw = t0w + tsw * jw;
  wd[i] = w[((((int64_t)co * kd + td) * kh + th) * kw + tw) * Ci + ci];
}

static int launch_igemm(const Igemm& g, hipStream_t s) {
  VS_REQUIRE((int64_t)g.N * g.Di * g.Hi * g.Wi * g.C < (1ll << 29) && (int64_t)g.Ng * g.K < (1ll << 29) &&
                 g.M < (1ll << 24) && g.K < (1 << 24),
             "conv3d: gathered volume too large (operands must stay below 2^31 bytes)");
  const int64_t tiles_m = (g.M + 127) / 128;
  const int64_t nwg = tiles_m * (g.Ng / 64);
  VS_REQUIRE(nwg < (1ll << 31), "conv3d: grid too large");
  count_path(VS_PATH_CONV_IGEMM);
  hipLaunchKernelGGL(conv_igemm_kernel, dim3((unsigned)nwg), dim3(256), 0, s, g);
  VS_LAUNCH_CHECK();
  return VS_OK;
}

// the parity classes of a dX launch: per dim the first tap, tap step, class count and the offsets
struct DxDim {
  int ncls;            // 1 (stride 1) or 2 (stride 2)
  int cnt[2], t0[2], ts[2], o0[2], os[2], start[2], step;
};
static DxDim dx_dim(int k, int s, int p) {
  DxDim r = {};
  if (s == 1) {    // dX[i] = sum_t dy[i + p - t] w[t]
    r.ncls = 1;
    r.cnt[0] = k; r.t0[0] = 0; r.ts[0] = 1; r.o0[0] = p; r.os[0] = -1; r.start[0] = 0;
    r.step = 1;
    return r;
  }
  // stride 2: i = 2 j + par; taps t with (par + p - t) even; dy index j + (par + p - t) / 2
  r.ncls = 2;
  r.step = 2;
  for (int par = 0; par < 2; ++par) {
    const int t0 = (par + p) & 1;
    r.t0[par] = t0;
    r.ts[par] = 2;
    r.cnt[par] = t0 < k ? (k - 1 - t0) / 2 + 1 : 0;
    r.o0[par] = (par + p - t0) / 2;
    r.os[par] = -1;
    r.start[par] = par;
  }
  return r;
}

// the implicit GEMM of parity class (a, b, c): rows = the class's input positions i = start + step * j,
// j < G; gathered operand dy; weights the class's regrouped taps in wd
static Igemm dx_class_igemm(const vs_conv3d_desc* d, int cshift, const float* dy, const float* wd, float* dx,
                            int accumulate, const DxDim& zd, const DxDim& yd, const DxDim& xd, int a, int b, int c) {
  Igemm g = {};
  g.x = dy; g.N = (int)d->N; g.Di = (int)d->Do; g.Hi = (int)d->Ho; g.Wi = (int)d->Wo; g.C = (int)d->Co;
  g.cshift = cshift;
  g.Gd = (int)((d->Di - zd.start[a] + zd.step - 1) / zd.step);
  g.Gh = (int)((d->Hi - yd.start[b] + yd.step - 1) / yd.step);
  g.Gw = (int)((d->Wi - xd.start[c] + xd.step - 1) / xd.step);
  g.sd = g.sh = g.sw = 1;
  g.cd = zd.cnt[a]; g.ch = yd.cnt[b]; g.cw = xd.cnt[c];
  g.od0 = zd.o0[a]; g.oh0 = yd.o0[b]; g.ow0 = xd.o0[c];
  g.ods = zd.os[a]; g.ohs = yd.os[b]; g.ows = xd.os[c];
  g.w = wd; g.Ng = (int)d->Ci; g.K = g.cd * g.ch * g.cw * (int)d->Co;
  g.y = dx; g.Od = (int)d->Di; g.Oh = (int)d->Hi; g.Ow = (int)d->Wi;
  g.ysd = zd.step; g.ysh = yd.step; g.ysw = xd.step;
  g.yod = zd.start[a]; g.yoh = yd.start[b]; g.yow = xd.start[c];
  g.accumulate = accumulate;
  g.M = d->N * (int64_t)g.Gd * g.Gh * g.Gw;
  return g;
}

}  // namespace vs

using namespace vs;

extern "C" size_t vs_conv3d_stats_rows(const vs_conv3d_desc* d) {
  if (!desc_ok(d)) return 0;
  return (size_t)((d->N * d->Do * d->Ho * d->Wo + 127) / 128);
}

extern "C" int vs_conv3d_fwd(const vs_conv3d_desc* d, const float* x, const float* w, float* y, float* stats,
                             void* stream) {
  VS_REQUIRE(desc_ok(d), "vs_conv3d_fwd: inconsistent geometry (Do = (Di + 2 pd - kd) / sd + 1, ...)");
  VS_REQUIRE(x && w && y, "vs_conv3d_fwd: null pointer");
  const int cs = ilog2(d->Ci);
  VS_REQUIRE(cs >= 2 && d->Co % 64 == 0, "vs_conv3d_fwd: Ci must be a power of two >= 4, Co a multiple of 64");
  VS_REQUIRE(aligned16(x) && aligned16(w) && aligned16(y), "vs_conv3d_fwd: pointers must be 16-byte aligned");
  const int64_t M = d->N * d->Do * d->Ho * d->Wo;
  VS_REQUIRE(M < (1ll << 24) && d->N * d->Di * d->Hi * d->Wi < (1ll << 31), "vs_conv3d_fwd: volume too large");
  hipStream_t s = (hipStream_t)stream;
  ScopedTimer timer(VS_TIMER_CONV_FWD, s, conv_flops(d));
  Igemm g = {};
  g.x = x; g.N = (int)d->N; g.Di = (int)d->Di; g.Hi = (int)d->Hi; g.Wi = (int)d->Wi; g.C = (int)d->Ci; g.cshift = cs;
  g.Gd = (int)d->Do; g.Gh = (int)d->Ho; g.Gw = (int)d->Wo;
  g.sd = d->sd; g.sh = d->sh; g.sw = d->sw;
  g.cd = d->kd; g.ch = d->kh; g.cw = d->kw;
  g.od0 = -d->pd; g.oh0 = -d->ph; g.ow0 = -d->pw; g.ods = 1; g.ohs = 1; g.ows = 1;
  g.w = w; g.Ng = (int)d->Co; g.K = d->kd * d->kh * d->kw * (int)d->Ci;
  g.y = y; g.Od = (int)d->Do; g.Oh = (int)d->Ho; g.Ow = (int)d->Wo;
  g.ysd = g.ysh = g.ysw = 1;
  g.accumulate = 0;
  g.stats = stats;
  g.M = M;
  return launch_igemm(g, s);
}

extern "C" size_t vs_conv3d_dx_workspace_bytes(const vs_conv3d_desc* d) {
  if (!desc_ok(d)) return 0;
  return (size_t)d->Ci * d->kd * d->kh * d->kw * d->Co * 4 + 256;
}

extern "C" int vs_conv3d_dx(const vs_conv3d_desc* d, const float* dy, const float* w, float* dx, int32_t accumulate,
                            void* workspace, int64_t workspace_bytes, void* stream) {
  VS_REQUIRE(desc_ok(d), "vs_conv3d_dx: inconsistent geometry");
  VS_REQUIRE(dy && w && dx && workspace, "vs_conv3d_dx: null pointer");
  const int cs = ilog2(d->Co);
  VS_REQUIRE(cs >= 2 && d->Ci % 64 == 0, "vs_conv3d_dx: Co must be a power of two >= 4, Ci a multiple of 64");
  VS_REQUIRE(d->sd <= 2 && d->sh <= 2 && d->sw <= 2, "vs_conv3d_dx: stride 1 or 2");
  VS_REQUIRE((size_t)workspace_bytes >= vs_conv3d_dx_workspace_bytes(d), "vs_conv3d_dx: workspace too small");
  VS_REQUIRE(aligned16(dy) && aligned16(w) && aligned16(dx) && aligned16(workspace),
             "vs_conv3d_dx: pointers must be 16-byte aligned");
  VS_REQUIRE(d->N * d->Di * d->Hi * d->Wi < (1ll << 24), "vs_conv3d_dx: volume too large");
  hipStream_t s = (hipStream_t)stream;
  ScopedTimer timer(VS_TIMER_CONV_DX, s, conv_flops(d));
  const DxDim zd = dx_dim(d->kd, d->sd, d->pd), yd = dx_dim(d->kh, d->sh, d->ph), xd = dx_dim(d->kw, d->sw, d->pw);
  float* wd = (float*)workspace;
  for (int a = 0; a < zd.ncls; ++a)
    for (int b = 0; b < yd.ncls; ++b)
      for (int c = 0; c < xd.ncls; ++c) {
        Igemm g = dx_class_igemm(d, cs, dy, wd, dx, accumulate, zd, yd, xd, a, b, c);
        if (g.Gd <= 0 || g.Gh <= 0 || g.Gw <= 0) continue;
        if (g.K == 0) {   // no tap reaches these positions: their gradient is zero
          if (accumulate) continue;
          // a K = 0 GEMM writes zeros through the same epilogue; the tap counts stay 1 (the kernel forms
          // 1 / (ch * cw) before it knows K = 0)
          g.cd = g.ch = g.cw = 1;
        } else {
          const int64_t nw = d->Ci * (int64_t)g.K;
          hipLaunchKernelGGL(conv_dx_weights, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, s, w, (int)d->Co,
                             (int)d->Ci, d->kd, d->kh, d->kw, g.cd, g.ch, g.cw, zd.t0[a], yd.t0[b], xd.t0[c],
                             zd.ts[a], yd.ts[b], xd.ts[c], wd);
          VS_LAUNCH_CHECK();
        }
        VS_CALL(launch_igemm(g, s));
      }
  return VS_OK;
}
