// mx8_api.h — what the engine launches of mx8.hip (the MXFP8 quantisers and the block-scaled MFMA GEMM, pgemm_mx8.h):
// plain host functions, so that translation unit keeps the one compiled copy of those kernels.
#pragma once
#include "common.h"

namespace sli {

// the LDS opt-in of every tiling of every epilogue; once, outside any stream capture
int mx8_prepare();
// codes [M][D], scales [M][D / 32] of RMSNorm(x row) * w (w null: of x), or of hi + lo
int mx8_norm_quant(const float* x, const float* w, void* codes, void* scales, int M, int D, float eps, hipStream_t s);
int mx8_pair_quant(const void* hi, const void* lo, void* codes, void* scales, int M, int D, hipStream_t s);
// one pgemm_mx8_kernel launch under the group table `segs` (read by role 0 alone); nothing is checked here
int mx8_gemm(const void* data, const void* scales, const void* acodes, const void* ascales, int N, int K, int M,
             const sli_pgemm_epilogue& e, const void* segs, sli_pgemm_tiling* tiling, hipStream_t s);

}  // namespace sli
