// gemm.hip — MFMA GEMM with fused epilogues (vs_gemm): argument validation and the ordered list of
// kernel paths.  Each kernel family is a translation unit of its own (gemm_paths.h has the map of
// path -> file -> VS_PATH_* counter); the device helpers they share are in gemm_tiles.h.
//
// Replaces the nn.Linear / F.linear / Conv3d(as im2col) kernels of the reference hot path and
// their autograd backward (see include/vspike.h for the per-call-site citations).
//
// bf16 operands: v_mfma_f32_16x16x32_bf16, block tile BM x BN x 64, 4 waves in 2x2, each wave
//   (BM/2) x (BN/2).  Operands are staged global -> registers -> LDS (double-buffered, loads for
//   tile t+1 issued before the MFMAs of tile t).  LDS images:
//     K-contiguous operand:  [rows][64 k] 128-B rows, 16-B chunk XOR (row>>1)&7  -> ds_read_b128
//     M/N-contiguous operand: [64 k][rows] rows, chunk XOR f(k)                 -> ds_read_tr16_b64
//   so the transposed products of the backward (dW = dY^T X, dX = dY W) need no transpose pass.
// f32 operands: v_mfma_f32_16x16x4_f32 (exact f32 fma chain), tile 64x64x32, [k][rows] images.
// Epilogue: the accumulator tile is staged through LDS (f32, padded rows) and written back in
//   row order, 8 consecutive columns per thread: every bias/pos/residual/aux read and every output
//   store is a 16-B vector access (the shapes here — M = 25,088 tokens, K = 192..768 — are
//   HBM-bound on their outputs; the first version's 2-4 B scattered stores were 5-9x off that
//   bound, profiles/r01_v0_kernel_stats.csv).  Split-K (VS_EPI_ATOMIC) adds whole 256-B rows.
// Grid: 1-D, tiles remapped so that consecutive tiles of one XCD (blockIdx % 8 group) share the
//   A row-panel / the same K slice (bijective remap, cdna_hip_programming.md §5 T1).
#include "common.h"
#include "gemm_common.h"
#include "gemm_dw.h"
#include "gemm_paths.h"

namespace vs {

static bool vec_ok(const vs_gemm_desc* d) {
  const uint32_t f = d->epilogue;
  const int ovec = d->out_dtype == VS_BF16 ? 8 : 4;
  const int avec = d->dtype == VS_BF16 ? 8 : 4;
  bool ok = d->ldc % ovec == 0 && aligned16(d->c);
  if (f & VS_EPI_BIAS) ok = ok && aligned16(d->bias);
  if (f & VS_EPI_POS) ok = ok && aligned16(d->pos) && d->N % 4 == 0;
  if (f & VS_EPI_RESIDUAL) ok = ok && aligned16(d->residual) && d->ld_residual % 4 == 0;
  if (f & (VS_EPI_GELU_BWD | VS_EPI_RELU_BWD | VS_EPI_MUL_AUX)) ok = ok && aligned16(d->aux_in) && d->ld_aux_in % avec == 0;
  if (f & VS_EPI_GELU) ok = ok && aligned16(d->aux_out) && d->ld_aux_out % avec == 0;
  return ok;
}

// Bytes a perfect kernel moves for this call (the roofline numerator): A and B read once, C written
// once (read too when accumulated into), every epilogue operand read / written once.
static double gemm_algorithmic_bytes(const vs_gemm_desc* d) {
  const double ea = esize(d->dtype), ec = esize(d->out_dtype), mn = (double)d->M * (double)d->N;
  const uint32_t f = d->epilogue;
  double b = ((double)d->M + (double)d->N) * (double)d->K * ea + mn * ec;
  if (f & (VS_EPI_ATOMIC | VS_EPI_ACCUM)) b += mn * 4.0;
  if (f & VS_EPI_BIAS) b += (double)d->N * 4.0;
  if (f & VS_EPI_RESIDUAL) b += mn * 4.0;
  if (f & VS_EPI_POS) b += (double)(d->pos_rows < d->M ? d->pos_rows : d->M) * (double)d->N * 4.0;
  if (f & (VS_EPI_GELU_BWD | VS_EPI_RELU_BWD | VS_EPI_MUL_AUX)) b += mn * ea;
  if (f & VS_EPI_GELU) b += mn * ea;
  if (d->a_rowsum) b += (double)d->M * 8.0;
  return b;
}

}  // namespace vs

extern "C" int vs_gemm(const vs_gemm_desc* d, void* stream) {
  using namespace vs;
  VS_REQUIRE(d != nullptr, "vs_gemm: null descriptor");
  VS_REQUIRE(d->dtype == VS_F32 || d->dtype == VS_BF16, "vs_gemm: dtype must be VS_F32 or VS_BF16");
  VS_REQUIRE(d->out_dtype == VS_F32 || d->out_dtype == VS_BF16, "vs_gemm: bad out_dtype");
  VS_REQUIRE(d->M >= 0 && d->N >= 0 && d->K >= 0, "vs_gemm: negative extent");
  if (d->M == 0 || d->N == 0) return VS_OK;
  VS_REQUIRE(d->a && d->b && d->c, "vs_gemm: null operand");
  const uint32_t f = d->epilogue;
  const int vec = d->dtype == VS_BF16 ? 8 : 4;
  // contiguous extents and leading dims must allow 16-byte vector loads
  VS_REQUIRE(aligned16(d->a) && aligned16(d->b), "vs_gemm: operands must be 16-byte aligned");
  VS_REQUIRE(d->lda % vec == 0 && d->ldb % vec == 0, "vs_gemm: lda/ldb must be multiples of 16 bytes");
  VS_REQUIRE(d->a_kcontig ? (d->K % vec == 0 && d->lda >= d->K) : (d->M % vec == 0 && d->lda >= d->M),
             "vs_gemm: A contiguous extent must be a multiple of 16 bytes and <= lda");
  VS_REQUIRE(d->b_kcontig ? (d->K % vec == 0 && d->ldb >= d->K) : (d->N % vec == 0 && d->ldb >= d->N),
             "vs_gemm: B contiguous extent must be a multiple of 16 bytes and <= ldb");
  VS_REQUIRE(d->ldc >= d->N, "vs_gemm: ldc < N");
  VS_REQUIRE(!(f & VS_EPI_BIAS) || d->bias, "vs_gemm: BIAS needs bias");
  VS_REQUIRE(!(f & VS_EPI_RESIDUAL) || d->residual, "vs_gemm: RESIDUAL needs residual");
  VS_REQUIRE(!(f & VS_EPI_POS) || (d->pos && d->pos_rows > 0), "vs_gemm: POS needs pos/pos_rows");
  VS_REQUIRE(!(f & (VS_EPI_GELU_BWD | VS_EPI_RELU_BWD | VS_EPI_MUL_AUX)) || d->aux_in, "vs_gemm: *_BWD / MUL_AUX need aux_in");
  VS_REQUIRE(!(f & VS_EPI_GELU) || d->aux_out, "vs_gemm: GELU needs aux_out");
  VS_REQUIRE(!(f & (VS_EPI_ATOMIC | VS_EPI_ACCUM)) || d->out_dtype == VS_F32, "vs_gemm: ATOMIC/ACCUM need f32 C");
  VS_REQUIRE(!((f & VS_EPI_ATOMIC) && (f & ~(VS_EPI_ATOMIC | VS_EPI_BIAS | VS_EPI_RELU))),
             "vs_gemm: ATOMIC combines with BIAS (and RELU on the skinny split-K path) only");
  VS_REQUIRE(d->split_k <= 1 || (f & VS_EPI_ATOMIC), "vs_gemm: split_k > 1 needs VS_EPI_ATOMIC");

  EpiParams e;
  e.M = d->M; e.N = d->N; e.c = d->c; e.ldc = d->ldc;
  e.out_bf16 = d->out_dtype == VS_BF16; e.op_bf16 = d->dtype == VS_BF16;
  e.flags = f; e.alpha = d->alpha; e.bias = d->bias;
  e.residual = d->residual; e.ldr = d->ld_residual;
  e.pos = d->pos; e.pos_rows = d->pos_rows;
  e.aux_in = d->aux_in; e.ld_aux_in = d->ld_aux_in;
  e.aux_out = d->aux_out; e.ld_aux_out = d->ld_aux_out;
  e.vec_ok = vec_ok(d);
  e.a_rowsum = d->a_rowsum;
  e.part = nullptr;

  hipStream_t s = (hipStream_t)stream;
  ScopedTimer timer(g_timer_tag >= 0 ? g_timer_tag : (f & VS_EPI_ATOMIC) ? VS_TIMER_GEMM_DW : VS_TIMER_GEMM, s,
                    gemm_algorithmic_bytes(d));

  // The paths in order of preference: the first whose predicate holds takes the call.  A predicate is
  // the path's whole condition (what its kernel requires, where it was measured faster, its knob) and
  // is written beside the kernel.
  if (dw256_ok(d, e)) return count_path(VS_PATH_GEMM_DW256), launch_dw256(d, e, s);
  if (dw_ok(d)) return count_path(VS_PATH_GEMM_DW), launch_dw(d, s);
  const bool skinny = skinny_ok(d);
  VS_REQUIRE(skinny || !((f & VS_EPI_ATOMIC) && (f & VS_EPI_RELU)),
             "vs_gemm: ATOMIC|RELU needs the skinny split-K path (M <= 64, N <= 256, K-contiguous, workspace, alpha 1)");
  if (skinny) {
    int S = 0;
    count_path(VS_PATH_GEMM_SKINNY);
    VS_CALL(launch_skinny(d, s, &S));
    launch_splitk_reduce(d, (const float*)d->workspace, S, true, s);
    VS_LAUNCH_CHECK();
    return VS_OK;
  }
  if (slab_ok(d, e)) return count_path(VS_PATH_GEMM_SLAB), launch_slab(d, e, s);
  if (g256_ok(d, e)) return count_path(VS_PATH_GEMM_G256), launch_g256(d, e, s);
  if (big_ok(d, e)) return count_path(VS_PATH_GEMM_BIG), launch_big(d, e, s);
  if (wres_ok(d, e)) return count_path(VS_PATH_GEMM_WRES), launch_wres(d, e, s);
  if (wslab_ok(d, e)) return count_path(VS_PATH_GEMM_WSLAB), launch_wslab(d, e, s);

  // the generic plan: tiles of the whole output, K split (into the workspace when there is one) for the
  // token reductions; panel, then whole-K, then ring, then the register-staged tiles
  const bool use_ws = splitk_ws(d);
  const GemmPlan plan = plan_gemm(d->dtype, d->M, d->N, d->K, d->split_k, (f & VS_EPI_ATOMIC) != 0, use_ws ? d->workspace_bytes : 0);
  const GridMap& g = plan.g;
  if (use_ws && g.splits > 1) e.part = (float*)d->workspace;
  VS_REQUIRE((int64_t)g.tiles_n * g.tiles_m * g.splits < (1ll << 31), "vs_gemm: grid too large");
  if (panel_ok(d, e, plan)) {
    count_path(VS_PATH_GEMM_PANEL);
    launch_panel(d, e, s);
    VS_LAUNCH_CHECK();
    return VS_OK;
  }
  if (fullk_ok(d, e, plan)) count_path(VS_PATH_GEMM_FULLK), launch_fullk(d, e, plan, s);
  else if (ring_ok(d, e, plan)) count_path(VS_PATH_GEMM_RING), launch_ring(d, e, plan, s);
  else if (d->dtype == VS_BF16) count_path(VS_PATH_GEMM_TILE), launch_tile(d, e, plan, s);
  else count_path(VS_PATH_GEMM_F32), launch_f32(d, e, plan, s);
  if (e.part) launch_splitk_reduce(d, e.part, g.splits, false, s);
  VS_LAUNCH_CHECK();
  return VS_OK;
}

extern "C" size_t vs_gemm_splitk_workspace_bytes(int32_t dtype, int64_t M, int64_t N, int64_t K) {
  using namespace vs;
  if (M <= 0 || N <= 0 || K <= 0 || (dtype != VS_F32 && dtype != VS_BF16)) return 0;
  const GemmPlan p = plan_gemm(dtype, M, N, K, 0, true, 0);
  size_t b = p.g.splits > 1 ? (size_t)p.g.splits * (size_t)(M * N) * 4 : 0;
  if (dtype == VS_BF16) {  // the dW kernels' partial tiles + bias sums (if this shape is a dW product)
    const size_t dw = dw_workspace_bytes(M, N, K);
    if (dw > b) b = dw;
    const size_t dw256 = knob(VS_KNOB_NO_DW256) ? 0 : dw256_workspace_bytes(M, N, K);
    if (dw256 > b) b = dw256;
  }
  const size_t sk = skinny_workspace_bytes(dtype, M, N, K);   // skinny split-K (head / Linear layer 0)
  if (sk > b) b = sk;
  return b;
}
