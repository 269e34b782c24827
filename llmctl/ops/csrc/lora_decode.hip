// Multi-LoRA decode delta (gfx950): every token row picks its own adapter.
//
//   delta[m, n] = scale[s] * sum_j ( sum_k x[m, k] A[s, j, k] ) B[s, n, j],   s = lora_idx[m]
//
// x bf16 [M, K]; the adapters of one projection are resident as stacked tensors A_all [S, R, K],
// B_all [S, N, R] (bf16) and scale_all [S] (fp32) whose addresses never change, so a captured decode
// graph stays valid across adapter loads; lora_idx int32 [M], a slot or -1 (no adapter).  Both sums are
// fp32 and the inner one is not rounded.  R is 16, 32 or 64 (smaller ranks are zero-padded).
//   * shrink: t[m, j] as K-chunk pieces tp [KP][M][R]; workgroup = (row m, K chunk of 512, 16 values of
//     j), 16 lanes per j streaming 16 B of the A row each per trip, reduced with 4 shuffles.  One row's
//     A is R K 2 bytes (128 KB at K = 4096, R = 16): the op is launch-latency-bound, the K split is
//     there to put more than M workgroups on the device at 1-16 rows;
//   * expand: workgroup = (row m, 256 columns n); the pieces are summed into LDS once, a thread reads
//     its B row (R contiguous bf16) and writes one fp32.
// The fused decode projections (skinny_gemm.hip) let the expand kernel write one more slice of their
// fp32 K-chunk partials ws [KS + 1][M][N]; the finalize kernels sum it with the rest, ahead of the
// RoPE / SwiGLU / residual + RMSNorm epilogue.  A row without an adapter gets -0.0f: v + (-0.0f) == v
// bit for bit for every v (+0.0f would turn a -0.0f sum into +0.0f), so such rows are the rows of the
// call without adapters.  No atomics, no host sync, no data-dependent shapes: graph-capturable.
#include "common.h"

namespace llmctl {
namespace {

constexpr int kLoraKC = 512;  // K chunk of a shrink workgroup

__global__ __launch_bounds__(256) void lora_shrink_kernel(const unsigned short* __restrict__ x,
                                                          const int* __restrict__ idx,
                                                          const unsigned short* __restrict__ A,
                                                          float* __restrict__ tp, int M, int K, int R, int S) {
  const int m = blockIdx.x;
  const int s = idx[m];
  if (s < 0 || s >= S) return;  // (workgroup-uniform) the expand kernel never reads this row's pieces
  const int kc0 = blockIdx.y * kLoraKC;
  const int kc = min(kLoraKC, K - kc0);  // multiple of 64
  const int j = blockIdx.z * 16 + (threadIdx.x >> 4), l = threadIdx.x & 15;
  const unsigned short* arow = A + ((long)s * R + j) * K + kc0;
  const unsigned short* xrow = x + (long)m * K + kc0;
  float acc = 0.f;
  for (int c = l * 8; c < kc; c += 128) {
    const uint4 av = *reinterpret_cast<const uint4*>(arow + c);
    const uint4 xv = *reinterpret_cast<const uint4*>(xrow + c);
    const unsigned a4[4] = {av.x, av.y, av.z, av.w}, x4[4] = {xv.x, xv.y, xv.z, xv.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      acc += __uint_as_float(a4[e] << 16) * __uint_as_float(x4[e] << 16);
      acc += __uint_as_float(a4[e] & 0xFFFF0000u) * __uint_as_float(x4[e] & 0xFFFF0000u);
    }
  }
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
  if (l == 0) tp[((long)blockIdx.y * M + m) * R + j] = acc;
}

__global__ __launch_bounds__(256) void lora_expand_kernel(const float* __restrict__ tp, const int* __restrict__ idx,
                                                          const unsigned short* __restrict__ B,
                                                          const float* __restrict__ scale, float* __restrict__ out,
                                                          int M, int N, int R, int S, int KP) {
  __shared__ float ts[64];
  const int m = blockIdx.x;
  const int n = blockIdx.y * 256 + threadIdx.x;
  const int s = idx[m];
  if (s < 0 || s >= S) {  // workgroup-uniform
    if (n < N) out[(long)m * N + n] = -0.0f;
    return;
  }
  if (threadIdx.x < R) {
    float t = 0.f;
    for (int p = 0; p < KP; ++p) t += tp[((long)p * M + m) * R + threadIdx.x];
    ts[threadIdx.x] = t;
  }
  __syncthreads();
  if (n >= N) return;
  const unsigned short* brow = B + ((long)s * N + n) * R;
  float acc = 0.f;
  for (int j = 0; j < R; j += 8) {
    const uint4 bv = *reinterpret_cast<const uint4*>(brow + j);
    const unsigned b4[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      acc += ts[j + 2 * e] * __uint_as_float(b4[e] << 16);
      acc += ts[j + 2 * e + 1] * __uint_as_float(b4[e] & 0xFFFF0000u);
    }
  }
  out[(long)m * N + n] = scale[s] * acc;
}

}  // namespace

// delta [M, N] fp32 into ``out`` (M * N floats on x's device); ``who`` names the calling op
void lora_delta_into(const at::Tensor& x, const at::Tensor& idx, const at::Tensor& A, const at::Tensor& B,
                     const at::Tensor& scale, float* out, int64_t N, const char* who) {
  LLMCTL_CHECK(x.is_cuda() && idx.is_cuda() && A.is_cuda() && B.is_cuda() && scale.is_cuda(), who,
               ": LoRA operands must be GPU tensors");
  LLMCTL_CHECK(x.dim() == 2 && x.is_contiguous() && x.scalar_type() == at::kBFloat16, who,
               ": LoRA needs bf16 contiguous activations [M, K]");
  const int M = x.size(0), K = x.size(1);
  LLMCTL_CHECK(idx.scalar_type() == at::kInt && idx.is_contiguous() && idx.dim() == 1 && idx.numel() == M, who,
               ": lora_idx int32 [M]");
  LLMCTL_CHECK(A.dim() == 3 && B.dim() == 3 && A.is_contiguous() && B.is_contiguous() &&
                   A.scalar_type() == at::kBFloat16 && B.scalar_type() == at::kBFloat16,
               who, ": lora_a [slots, R, K] and lora_b [slots, N, R] bf16 contiguous");
  const int S = A.size(0), R = A.size(1);
  LLMCTL_CHECK(R == 16 || R == 32 || R == 64, who, ": LoRA rank (padded) must be 16, 32 or 64, got ", R);
  LLMCTL_CHECK(A.size(2) == K && B.size(0) == S && B.size(1) == N && B.size(2) == R, who,
               ": LoRA shapes: lora_a [slots, R, K], lora_b [slots, N, R] (got A ", A.sizes(), ", B ", B.sizes(),
               " for x ", x.sizes(), ", N = ", N, ")");
  LLMCTL_CHECK(scale.scalar_type() == at::kFloat && scale.is_contiguous() && scale.numel() == S, who,
               ": lora_scale fp32 [slots]");
  LLMCTL_CHECK(M >= 1 && S >= 1 && K % 64 == 0 && N % 64 == 0, who, ": LoRA needs M >= 1, K % 64 == 0, N % 64 == 0 (got ", M,
               "x", N, "x", K, ")");
  LLMCTL_CHECK(x.device() == idx.device() && x.device() == A.device() && x.device() == B.device() &&
                   x.device() == scale.device(),
               who, ": LoRA operands on one device");
  const int KP = (K + kLoraKC - 1) / kLoraKC;
  LLMCTL_CHECK(KP <= 65535 && (N + 255) / 256 <= 65535, who, ": LoRA K or N too large");
  auto tp = at::empty({(long)KP * M * R}, x.options().dtype(at::kFloat));
  hipLaunchKernelGGL(lora_shrink_kernel, dim3(M, KP, R / 16), dim3(256), 0, stream(), bf_ptr(x), idx.data_ptr<int>(),
                     bf_ptr(A), tp.data_ptr<float>(), M, K, R, S);
  hipLaunchKernelGGL(lora_expand_kernel, dim3(M, (unsigned)((N + 255) / 256)), dim3(256), 0, stream(),
                     tp.data_ptr<float>(), idx.data_ptr<int>(), bf_ptr(B), scale.data_ptr<float>(), out, M, (int)N, R, S,
                     KP);
}

at::Tensor lora_delta(const at::Tensor& x, const at::Tensor& idx, const at::Tensor& A, const at::Tensor& B,
                      const at::Tensor& scale) {
  LLMCTL_CHECK(B.dim() == 3, "lora_delta: lora_b [slots, N, R]");
  LLMCTL_CHECK(x.dim() == 2 && x.is_cuda(), "lora_delta: x must be a 2-D GPU tensor");
  const c10::DeviceGuard guard(x.device());
  auto out = at::empty({x.size(0), B.size(1)}, x.options().dtype(at::kFloat));
  lora_delta_into(x, idx, A, B, scale, out.data_ptr<float>(), B.size(1), "lora_delta");
  return out;
}

TORCH_LIBRARY_IMPL(llmctl, CUDA, m) { m.impl("lora_delta", &lora_delta); }

}  // namespace llmctl
