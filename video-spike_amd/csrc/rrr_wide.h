// rrr_wide.h — what csrc/rrr_pixel.hip shares with csrc/rrr_wide.hip: the scoring of a standardised yhat.
#pragma once

#include "common.h"

namespace vs {

// Bytes of vs_rrr_wide_score's workspace: K T N doubles (the standardised yhat, at offset 0) + the statistics.
size_t rrw_score_workspace_bytes(int64_t K, int64_t T, int64_t N);
// rrw_score_kernel + rrw_score_final_kernel on the yhat [K][T][N] a forward product left at the start of
// `workspace`: pred (may be null), bps, r2 and out as vs_rrr_wide_score writes them.  gt_dtype VS_F32 or VS_F64.
int rrw_score_yhat(hipStream_t s, int64_t K, int64_t T, int64_t N, const double* mean_y, const double* std_y,
                   const void* gt, int32_t gt_dtype, double* pred, double* bps, double* r2, double* out,
                   void* workspace);

}  // namespace vs
