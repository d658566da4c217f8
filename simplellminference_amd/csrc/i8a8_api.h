// i8a8_api.h — what the engine launches of i8a8.hip (the per-token int8 quantisers and the integer-MFMA prefill GEMM of
// pgemm_i8a8.h): plain host functions, so that translation unit keeps the one compiled copy of those kernels.
#pragma once
#include "common.h"

namespace sli {

constexpr int kI8A8MaxK = 131072;  // 127^2 K stays below 2^31: the i32 accumulator holds the whole depth

// the LDS opt-in of every tiling of every epilogue; once, outside any stream capture
int i8a8_prepare();
// codes int8 [M][D], scales fp32 [M] of RMSNorm(x row) * w (w null: of x), or of hi + lo
int i8a8_norm_quant(const float* x, const float* w, void* codes, float* scales, int M, int D, float eps, hipStream_t s);
int i8a8_pair_quant(const void* hi, const void* lo, void* codes, float* scales, int M, int D, hipStream_t s);
// one pgemm_i8a8_kernel launch under the group table `segs` (read by role 0 alone); nothing is checked here
int i8a8_gemm(const void* w, const float* w_row_scale, const void* acodes, const float* ascales, int N, int K, int M,
              const sli_pgemm_epilogue& e, const void* segs, sli_pgemm_tiling* tiling, hipStream_t s);

}  // namespace sli
