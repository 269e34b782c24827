// Pieces the routed-expert decode GEMMs share (moe_decode.hip: bf16 experts behind a pointer table;
// moe_decode_wq.hip: stacked fp8 / int4 experts): the two finalize passes over the fp32 K-chunk
// partials ws[chunk][copy][n], and the argument checks; and the router kernel, which moe_grouped.hip
// launches for more than 64 rows.  The kernels have internal linkage: each translation unit
// launches its own copy.
#pragma once

#include "common.h"

namespace llmctl {
namespace {

__device__ __forceinline__ f32x4 sum_parts(const float* __restrict__ ws, long MN, int KS, long i) {
  f32x4 v = *reinterpret_cast<const f32x4*>(ws + i);
  for (int s = 1; s < KS; ++s) v += *reinterpret_cast<const f32x4*>(ws + s * MN + i);
  return v;
}

// gate/up partials [KS][MK][2F] -> act[c] = silu(g) * u, the projection rounded to bf16 first
// (as decode_fin_swiglu_kernel); thread = 4 columns of one copy
__global__ __launch_bounds__(256) void moe_fin_swiglu_kernel(const float* __restrict__ ws,
                                                             unsigned short* __restrict__ act, int MK, int F, int KS) {
  const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;  // index into act [MK][F]
  if (i >= (long)MK * F) return;
  const long m = i / F, n = i % F;
  const long N = 2L * F, MN = (long)MK * N;
  const f32x4 gs = sum_parts(ws, MN, KS, m * N + n), us = sum_parts(ws, MN, KS, m * N + F + n);
  ushort4 pk;
  unsigned short* pp = reinterpret_cast<unsigned short*>(&pk);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float gv = bf2f(f2bf(gs[j])), uv = bf2f(f2bf(us[j]));
    pp[j] = f2bf(gv * (1.f / (1.f + __expf(-gv))) * uv);
  }
  *reinterpret_cast<ushort4*>(act + i) = pk;
}

// down partials [KS][M k][N] -> per token t (one workgroup of 1024 threads):
//   d_j = bf16(sum_chunks), y = bf16(sum_j topw[t][j] d_j) (fp32, slot order j = 0 .. k-1),
//   s = bf16(y + res) -> res_out, xn = bf16(s rsqrt(mean(s^2) + eps) nw)
// the row is kept in LDS between the two passes (as decode_fin_add_rmsnorm_kernel)
__global__ __launch_bounds__(1024) void moe_fin_combine_add_rmsnorm_kernel(
    const float* __restrict__ ws, const float* __restrict__ topw, const unsigned short* __restrict__ res,
    const unsigned short* __restrict__ nw, unsigned short* __restrict__ y, unsigned short* __restrict__ res_out, int M,
    int k, int N, int KS, float eps) {
  extern __shared__ __attribute__((aligned(16))) float srow[];
  __shared__ float red[16];
  const int t = blockIdx.x;
  const long MN = (long)M * k * N, base = (long)t * N;
  float ss = 0.f;
  for (int n = threadIdx.x * 4; n < N; n += 4096) {
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    for (int j = 0; j < k; ++j) {
      const f32x4 v = sum_parts(ws, MN, KS, ((long)t * k + j) * N + n);
      const float w = topw[t * k + j];
#pragma unroll
      for (int q = 0; q < 4; ++q) o[q] += w * bf2f(f2bf(v[q]));
    }
    const ushort4 rv = *reinterpret_cast<const ushort4*>(res + base + n);
    const unsigned short r4[4] = {rv.x, rv.y, rv.z, rv.w};
    ushort4 pk;
    unsigned short* pp = reinterpret_cast<unsigned short*>(&pk);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      pp[q] = f2bf(bf2f(f2bf(o[q])) + bf2f(r4[q]));
      const float sv = bf2f(pp[q]);
      srow[n + q] = sv;
      ss += sv * sv;
    }
    *reinterpret_cast<ushort4*>(res_out + base + n) = pk;
  }
  const float rs = rsqrtf(block_sum<16>(ss, red) / (float)N + eps);  // (barrier: srow complete)
  for (int n = threadIdx.x * 4; n < N; n += 4096) {
    const ushort4 wv = *reinterpret_cast<const ushort4*>(nw + n);
    ushort4 pk;
    pk.x = f2bf(srow[n] * rs * bf2f(wv.x));
    pk.y = f2bf(srow[n + 1] * rs * bf2f(wv.y));
    pk.z = f2bf(srow[n + 2] * rs * bf2f(wv.z));
    pk.w = f2bf(srow[n + 3] * rs * bf2f(wv.w));
    *reinterpret_cast<ushort4*>(y + base + n) = pk;
  }
}

// ---- router: bf16-rounded logits -> fp32 softmax -> top-k by repeated arg-max (ties: the lowest
// expert index), weights renormalised over the picks.  One workgroup per token; wave w computes the
// logits of experts w, w + 4, ...; wave 0 then holds one expert per lane (E <= 64).
// The arg-max order is total (NaN compares as a tie, so the lower index wins) and an expert once
// picked is excluded, so the k indices are always distinct and in [0, E), whatever the inputs.
__global__ __launch_bounds__(256) void moe_route_kernel(const unsigned short* __restrict__ x,
                                                        const unsigned short* __restrict__ wr,
                                                        int* __restrict__ topi, float* __restrict__ topw, int E,
                                                        int k, int h) {
  __shared__ float lg[64];
  const int t = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned short* xr = x + (long)t * h;
  for (int e = wave; e < E; e += 4) {
    const unsigned short* w = wr + (long)e * h;
    float s = 0.f;
    for (int c = lane * 8; c < h; c += 512) {
      float a[8], b[8];
      load8(xr + c, a);
      load8(w + c, b);
#pragma unroll
      for (int j = 0; j < 8; ++j) s += a[j] * b[j];
    }
    s = wave_sum(s);
    if (lane == 0) lg[e] = bf2f(f2bf(s));  // linear() returns bf16 before the fp32 softmax
  }
  __syncthreads();
  if (wave != 0) return;
  const bool valid = lane < E;
  const float l = valid ? lg[lane] : -INFINITY;
  const float mx = wave_max(l);
  const float ex = valid ? __expf(l - mx) : 0.f;
  const float p = ex / wave_sum(ex);
  bool used = !valid;
  int myi = 0;
  float myw = 0.f;
  for (int j = 0; j < k; ++j) {
    float bp = p;
    int bi = used ? 64 : lane;  // 64: no candidate
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float op = __shfl_xor(bp, o);
      const int oi = __shfl_xor(bi, o);
      const bool take = oi < 64 && (bi >= 64 || op > bp || (!(bp > op) && oi < bi));
      bp = take ? op : bp;
      bi = take ? oi : bi;
    }
    bi = __shfl(bi, 0);
    bp = __shfl(bp, 0);
    if (lane == bi) used = true;
    if (lane == j) myi = bi, myw = bp;
  }
  const float tot = wave_sum(myw);  // lanes >= k hold 0
  if (lane < k) {
    topi[t * k + lane] = myi;
    topw[t * k + lane] = myw / tot;
  }
}

inline void check_routing(const at::Tensor& topi, int M, int k, int E, const char* who) {
  LLMCTL_CHECK(M >= 1 && M <= 64, who, ": 1 <= tokens <= 64 (got ", M, ")");
  LLMCTL_CHECK(E >= 1 && E <= 64, who, ": experts <= 64 (got ", E, ")");
  LLMCTL_CHECK(k >= 1 && k <= 8 && k <= E, who, ": 1 <= picks per token <= min(experts, 8) (got ", k, ")");
  LLMCTL_CHECK(topi.is_cuda() && topi.scalar_type() == at::kInt && topi.is_contiguous() && topi.dim() == 2 &&
                   topi.size(0) == M,
               who, ": topi int32 [M, k] on the GPU");
}

inline void check_act(const at::Tensor& t, const char* who) {
  LLMCTL_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16 && t.is_contiguous() && t.dim() == 2, who,
               ": bf16 contiguous 2-D GPU activations");
}

}  // namespace
}  // namespace llmctl
