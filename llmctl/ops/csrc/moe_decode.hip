// Routed-expert decode MLP (gfx950): router top-k, gate/up + SwiGLU and down + combine + residual +
// RMSNorm of a Mixtral-style MoE layer for M <= 64 decode tokens, with no host synchronisation, no
// atomics and no data-dependent shapes, so the layer sits inside the captured decode hipGraph.
//
// A decode step is an HBM stream of weights, and at small batch most experts are not routed to
// (1 token, top-2 of 8: a quarter of the expert bytes).  The two GEMMs are skinny_gemm.hip's v3
// weight-streaming kernel with an expert axis on the grid:
//   * grid = (N / 64, K chunks of 1024, E); a workgroup of expert e first builds, in LDS, the list
//     of (token, slot) copies routed to e from topi (<= M k <= 512 entries, every wave counts them
//     with ballots, wave 0 writes them), and returns BEFORE issuing any weight load when the list is
//     empty: an unrouted expert costs no HBM traffic;
//   * otherwise the chunk's weight fragments (8 K blocks, 4 x 16 B per lane each) are issued first
//     and held in registers, the listed copies' x rows are gathered into LDS 16 at a time (row
//     stride KC + 8), and MFMA 16x16x32 runs with weight rows on the row axis and the copies on the
//     column axis; an expert with more than 16 copies loops over column tiles with the same weight
//     registers, so each weight byte is still read once;
//   * fp32 partials go to ws[chunk][t k + j][n]: every copy belongs to exactly one expert, so every
//     workspace row is written exactly once per chunk, and the finalize passes sum the chunks in a
//     fixed order (SwiGLU; weighted combine in slot order + residual + RMSNorm).
// Expert weights come as a device table of pointers (one Parameter per expert in the model; a
// stacked copy would double the model).
#include "moe_decode.h"

namespace llmctl {
namespace {

using bf16x8_t = __attribute__((ext_vector_type(8))) __bf16;
using f32x4_t = __attribute__((ext_vector_type(4))) float;

constexpr int KBLK = 128;        // K per block: 4 MFMA steps of 32
constexpr int kKC = 1024;        // K chunk per workgroup
constexpr int kMaxCopies = 512;  // M k <= 64 x 8

__device__ __forceinline__ f32x4_t mfma16(bf16x8_t a, bf16x8_t b, f32x4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ bf16x8_t ld16(const unsigned short* p) {
  return *reinterpret_cast<const bf16x8_t*>(p);
}

// ---- routed weight-streaming GEMM: ws[chunk][c][n] = x[row(c)] . W_e[n] over the chunk's K range,
// for every copy c = t k + j with topi[c] == e (e = blockIdx.z); row(c) = c / xdiv (gate/up: the
// token's row, xdiv = k; down: the copy's own activation row, xdiv = 1).
template <int NB>
__global__ __launch_bounds__(256) void moe_gemm_kernel(const unsigned short* __restrict__ x,
                                                       const int64_t* __restrict__ wptrs,
                                                       const int* __restrict__ topi, float* __restrict__ ws, int MK,
                                                       int xdiv, int N, int K) {
  constexpr int KC = NB * KBLK, XST = KC + 8;
  __shared__ __attribute__((aligned(16))) unsigned short xs[16 * XST];
  __shared__ int list[kMaxCopies];  // copy | x row << 16
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int e = blockIdx.z;
  // the copies routed to this expert, in copy order: every wave counts, wave 0 writes
  int cnt = 0;
  for (int i0 = 0; i0 < MK; i0 += 64) {
    const int i = i0 + lane;
    const bool hit = i < MK && topi[i] == e;
    const unsigned long long b = __ballot(hit);
    if (hit && wave == 0) list[cnt + __popcll(b & ((1ull << lane) - 1ull))] = i | ((i / xdiv) << 16);
    cnt += __popcll(b);
  }
  if (cnt == 0) return;  // unrouted expert: no weight load is issued
  const int r = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 64 + wave * 16;
  const int kc0 = blockIdx.y * KC;
  const int kc = min(KC, K - kc0);
  const int nb = kc / KBLK;
  const int ko = 8 * g, ks = 32;  // MFMA step s of lane group g reads k = 32 s + 8 g
  const unsigned short* wrow = reinterpret_cast<const unsigned short*>(wptrs[e]) + (long)(n0 + r) * K + kc0 + ko;
  bf16x8_t a[NB][4];
#pragma unroll
  for (int u = 0; u < NB; ++u) {
    const int bu = u < nb ? u : nb - 1;  // a short last chunk re-loads its last block
#pragma unroll
    for (int s = 0; s < 4; ++s) a[u][s] = ld16(wrow + bu * KBLK + ks * s);
  }
  __builtin_amdgcn_sched_barrier(0);
  lds_sync();  // list complete (LDS-only barrier: the weight loads stay in flight)
  const int c8 = kc >> 3;
  const unsigned short* xrow = xs + r * XST + ko;
  const int n = n0 + 4 * g;
  for (int c0 = 0; c0 < cnt; c0 += 16) {
    if (c0 > 0) __syncthreads();  // the previous tile's MFMA reads of xs
    for (int i = threadIdx.x; i < 16 * c8; i += 256) {
      const int m = i / c8, c = i - m * c8;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (c0 + m < cnt) v = *reinterpret_cast<const uint4*>(x + (long)(list[c0 + m] >> 16) * K + kc0 + c * 8);
      *reinterpret_cast<uint4*>(xs + m * XST + c * 8) = v;
    }
    __syncthreads();
    f32x4_t acc = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      if (u < nb) {
#pragma unroll
        for (int s = 0; s < 4; ++s) acc = mfma16(a[u][s], *reinterpret_cast<const bf16x8_t*>(xrow + u * KBLK + ks * s), acc);
      }
    }
    if (c0 + r < cnt) {
      const int copy = list[c0 + r] & 0xffff;
      *reinterpret_cast<f32x4_t*>(ws + ((long)blockIdx.y * MK + copy) * N + n) = acc;
    }
  }
}

void check_table(const at::Tensor& ptrs, int E, const char* who) {
  LLMCTL_CHECK(ptrs.is_cuda() && ptrs.scalar_type() == at::kLong && ptrs.is_contiguous() && ptrs.numel() == E, who,
               ": expert pointer table int64 [E] on the GPU");
}

// routed x W_e^T as fp32 K-chunk partials ws [KS][MK][N]; returns KS
int moe_partials(const at::Tensor& x, const at::Tensor& ptrs, const at::Tensor& topi, at::Tensor& ws, int MK, int xdiv,
                 int N, int K, int E) {
  const int KS = (K + kKC - 1) / kKC;
  ws = at::empty({(long)KS * MK * N}, x.options().dtype(at::kFloat));
  hipLaunchKernelGGL((moe_gemm_kernel<kKC / KBLK>), dim3(N / 64, KS, E), dim3(256), 0, stream(), bf_ptr(x),
                     ptrs.data_ptr<int64_t>(), topi.data_ptr<int>(), ws.data_ptr<float>(), MK, xdiv, N, K);
  return KS;
}

}  // namespace

// (topi int32 [M, k], topw fp32 [M, k]) of softmax(bf16(x w_router^T))
std::tuple<at::Tensor, at::Tensor> moe_route(const at::Tensor& x, const at::Tensor& w_router, int64_t k) {
  check_act(x, "moe_route");
  check_act(w_router, "moe_route");
  const int M = x.size(0), h = x.size(1), E = w_router.size(0);
  LLMCTL_CHECK(w_router.size(1) == h && h % 128 == 0, "moe_route: router [E, h], h % 128 == 0 (got h = ", h, ")");
  LLMCTL_CHECK(M >= 1 && M <= 64 && E >= 1 && E <= 64 && k >= 1 && k <= 8 && k <= E,
               "moe_route: 1 <= tokens <= 64, experts <= 64, 1 <= k <= min(experts, 8) (got ", M, ", ", E, ", ", k, ")");
  const c10::DeviceGuard guard(x.device());
  auto topi = at::empty({M, k}, x.options().dtype(at::kInt));
  auto topw = at::empty({M, k}, x.options().dtype(at::kFloat));
  hipLaunchKernelGGL(moe_route_kernel, dim3(M), dim3(256), 0, stream(), bf_ptr(x), bf_ptr(w_router),
                     topi.data_ptr<int>(), topw.data_ptr<float>(), E, (int)k, h);
  return {topi, topw};
}

// act [M k, F]: row t k + j = silu(g) * u of x[t] . W_up[topi[t, j]]^T  (W_up[e] = [2F, h], gate first)
at::Tensor moe_decode_up_swiglu(const at::Tensor& x, const at::Tensor& up_ptrs, const at::Tensor& topi, int64_t E,
                                int64_t F) {
  check_act(x, "moe_decode_up_swiglu");
  const int M = x.size(0), h = x.size(1), k = topi.dim() == 2 ? topi.size(1) : 0;
  check_routing(topi, M, k, E, "moe_decode_up_swiglu");
  check_table(up_ptrs, E, "moe_decode_up_swiglu");
  LLMCTL_CHECK(h % 128 == 0 && F >= 128 && F % 128 == 0, "moe_decode_up_swiglu: h % 128 == 0, F % 128 == 0 (got ", h, ", ",
               F, ")");
  const c10::DeviceGuard guard(x.device());
  const int MK = M * k;
  at::Tensor ws;
  const int KS = moe_partials(x, up_ptrs, topi, ws, MK, k, 2 * F, h, E);
  auto act = at::empty({MK, F}, x.options());
  const long n4 = (long)MK * F / 4;
  hipLaunchKernelGGL(moe_fin_swiglu_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream(),
                     ws.data_ptr<float>(), bf_mut(act), MK, (int)F, KS);
  return act;
}

// (xn, res_out): res_out = sum_j topw[t, j] (act[t k + j] . W_down[topi[t, j]]^T) + residual,
// xn = rmsnorm(res_out) * norm_w
std::tuple<at::Tensor, at::Tensor> moe_decode_down_add_rmsnorm(const at::Tensor& act, const at::Tensor& down_ptrs,
                                                               const at::Tensor& topi, const at::Tensor& topw,
                                                               const at::Tensor& residual, const at::Tensor& norm_w,
                                                               double eps, int64_t E) {
  check_act(act, "moe_decode_down_add_rmsnorm");
  check_act(residual, "moe_decode_down_add_rmsnorm");
  const int M = residual.size(0), h = residual.size(1), F = act.size(1), k = topi.dim() == 2 ? topi.size(1) : 0;
  check_routing(topi, M, k, E, "moe_decode_down_add_rmsnorm");
  check_table(down_ptrs, E, "moe_decode_down_add_rmsnorm");
  LLMCTL_CHECK(act.size(0) == (long)M * k, "moe_decode_down_add_rmsnorm: act [M k, F]");
  LLMCTL_CHECK(topw.is_cuda() && topw.scalar_type() == at::kFloat && topw.is_contiguous() && topw.dim() == 2 &&
                   topw.size(0) == M && topw.size(1) == k,
               "moe_decode_down_add_rmsnorm: topw fp32 [M, k] on the GPU");
  LLMCTL_CHECK(h % 128 == 0 && F >= 128 && F % 128 == 0 && h <= 16384,
               "moe_decode_down_add_rmsnorm: h % 128 == 0, F % 128 == 0, h <= 16384 (row staged in LDS; got ", h, ", ", F,
               ")");
  LLMCTL_CHECK(norm_w.is_cuda() && norm_w.is_contiguous() && norm_w.scalar_type() == at::kBFloat16 && norm_w.numel() == h,
               "moe_decode_down_add_rmsnorm: norm weight bf16 [h]");
  const c10::DeviceGuard guard(act.device());
  const int MK = M * k;
  at::Tensor ws;
  const int KS = moe_partials(act, down_ptrs, topi, ws, MK, 1, h, F, E);
  auto y = at::empty({M, h}, act.options());
  auto res_out = at::empty({M, h}, act.options());
  hipLaunchKernelGGL(moe_fin_combine_add_rmsnorm_kernel, dim3(M), dim3(1024), (size_t)h * 4, stream(),
                     ws.data_ptr<float>(), topw.data_ptr<float>(), bf_ptr(residual), bf_ptr(norm_w), bf_mut(y),
                     bf_mut(res_out), M, k, h, KS, (float)eps);
  return {y, res_out};
}

TORCH_LIBRARY_IMPL(llmctl, CUDA, m) {
  m.impl("moe_route", &moe_route);
  m.impl("moe_decode_up_swiglu", &moe_decode_up_swiglu);
  m.impl("moe_decode_down_add_rmsnorm", &moe_decode_down_add_rmsnorm);
}

}  // namespace llmctl
