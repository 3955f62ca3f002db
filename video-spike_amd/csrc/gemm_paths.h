// gemm_paths.h — what vs_gemm (gemm.hip) sees of the GEMM kernel families: per path a predicate
// `<path>_ok` (the path's whole condition, written beside its kernel) and a `launch_<path>`, plus the
// plans and workspace sizes.  The dW and skinny split-K paths are in gemm_dw.h.
//
//   path (in vs_gemm's order)   file              counter
//   dw256                       gemm_dw256.hip    VS_PATH_GEMM_DW256
//   dw, skinny                  gemm_dw.hip       VS_PATH_GEMM_DW, VS_PATH_GEMM_SKINNY
//   slab (+ fused LayerNorm)    gemm_slab.hip     VS_PATH_GEMM_SLAB, _LN_FWD, _LN_BWD
//   g256, big                   gemm_g256.hip     VS_PATH_GEMM_G256, VS_PATH_GEMM_BIG
//   wres                        gemm_wres.hip     VS_PATH_GEMM_WRES
//   wslab                       gemm_wslab.hip    VS_PATH_GEMM_WSLAB
//   panel, fullk                gemm_wholek.hip   VS_PATH_GEMM_PANEL, VS_PATH_GEMM_FULLK
//   ring                        gemm_ring.hip     VS_PATH_GEMM_RING
//   tile, f32, split-K reduce   gemm_tile.hip     VS_PATH_GEMM_TILE, VS_PATH_GEMM_F32
#pragma once

#include "common.h"
#include "gemm_common.h"
#include "gemm_dw.h"

namespace vs {

// ---- paths that take the call whole: `launch_*` returns VS_OK or the launch error -------------
bool dw256_ok(const vs_gemm_desc* d, const EpiParams& e);
int launch_dw256(const vs_gemm_desc* d, const EpiParams& e, hipStream_t s);
size_t dw256_workspace_bytes(int64_t M, int64_t N, int64_t K);

bool slab_ok(const vs_gemm_desc* d, const EpiParams& e);
int launch_slab(const vs_gemm_desc* d, const EpiParams& e, hipStream_t s);

bool g256_ok(const vs_gemm_desc* d, const EpiParams& e);
int launch_g256(const vs_gemm_desc* d, const EpiParams& e, hipStream_t s);

bool big_ok(const vs_gemm_desc* d, const EpiParams& e);
int launch_big(const vs_gemm_desc* d, const EpiParams& e, hipStream_t s);

bool wres_ok(const vs_gemm_desc* d, const EpiParams& e);
int launch_wres(const vs_gemm_desc* d, const EpiParams& e, hipStream_t s);

bool wslab_ok(const vs_gemm_desc* d, const EpiParams& e);
int launch_wslab(const vs_gemm_desc* d, const EpiParams& e, hipStream_t s);

// ---- the generic plan: tile / split geometry shared by vs_gemm and
// vs_gemm_splitk_workspace_bytes; its paths launch only (vs_gemm adds the split-K reduce and checks)
struct GemmPlan {
  int BM, BN, BK;
  GridMap g;
};
GemmPlan plan_gemm(int dtype, int64_t M, int64_t N, int64_t K, int want_split, bool atomic_ok, int64_t ws_bytes);

bool panel_ok(const vs_gemm_desc* d, const EpiParams& e, const GemmPlan& p);
void launch_panel(const vs_gemm_desc* d, const EpiParams& e, hipStream_t s);

bool fullk_ok(const vs_gemm_desc* d, const EpiParams& e, const GemmPlan& p);
void launch_fullk(const vs_gemm_desc* d, const EpiParams& e, const GemmPlan& p, hipStream_t s);

bool ring_ok(const vs_gemm_desc* d, const EpiParams& e, const GemmPlan& p);
void launch_ring(const vs_gemm_desc* d, const EpiParams& e, const GemmPlan& p, hipStream_t s);

void launch_tile(const vs_gemm_desc* d, const EpiParams& e, const GemmPlan& p, hipStream_t s);  // bf16
void launch_f32(const vs_gemm_desc* d, const EpiParams& e, const GemmPlan& p, hipStream_t s);

// C += (bias +) the sum over `splits` of part[split][M][N], in a fixed order.  `skinny`: the skinny
// split-K path's reduce (always the one-float4-per-workgroup kernel, with its optional RELU)
void launch_splitk_reduce(const vs_gemm_desc* d, const float* part, int splits, bool skinny, hipStream_t s);

}  // namespace vs
