// Pieces the decode GEMM kernels share (skinny_gemm.hip: <= 16 token rows; decode_gemm_mid.hip:
// 17-64 rows with fp8 / int4 weights): the MFMA step and the two weight dequantisations.
#pragma once

#include "attn_common.h"

namespace llmctl {

using attn::bf16x8_t;
using f32x4_t = __attribute__((ext_vector_type(4))) float;

constexpr int KBLK = 128;  // K per block: 4 MFMA steps of 32

__device__ __forceinline__ f32x4_t mfma16(bf16x8_t a, bf16x8_t b, f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// 8 fp8 (e4m3fn) -> 8 bf16, exact: the bf16 is the f32 image's high half
__device__ __forceinline__ bf16x8_t fp8x8_to_bf16x8(unsigned lo, unsigned hi) {
  float x[8];
  fp8x8_to_f32(make_uint2(lo, hi), x);
  bf16x8_t r;
  unsigned* w = reinterpret_cast<unsigned*>(&r);
#pragma unroll
  for (int j = 0; j < 4; ++j) w[j] = __builtin_amdgcn_perm(__float_as_uint(x[2 * j + 1]), __float_as_uint(x[2 * j]), 0x07060302u);
  return r;
}

// 8 nibbles u -> the bf16 integers 128 + u, in element order (0, 4, 1, 5, 2, 6, 3, 7)
__device__ __forceinline__ bf16x8_t u4x8_to_bf16x8(unsigned d, unsigned mask, unsigned one28) {
  bf16x8_t r;
  unsigned* w = reinterpret_cast<unsigned*>(&r);
#pragma unroll
  for (int t = 0; t < 4; ++t) w[t] = ((d >> (4 * t)) & mask) | one28;
  return r;
}

// decode_gemm_mid.hip: fp8 / int4 weights at 17-64 token rows.  Split-K slice count for the shape
// (knob decode_mid_splits > 0 forces it), and the launch that fills ws [KS][M][N].
int decode_mid_splits(int M, int N, int K, bool int4);
void launch_decode_mid(const at::Tensor& x, const at::Tensor& w, const at::Tensor& w_scale, float* ws, int KS);

}  // namespace llmctl
