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
#include "common.h"

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

__device__ __forceinline__ f32x4_t sum_parts(const float* __restrict__ ws, long MN, int KS, long i) {
  f32x4_t v = *reinterpret_cast<const f32x4_t*>(ws + i);
  for (int s = 1; s < KS; ++s) v += *reinterpret_cast<const f32x4_t*>(ws + s * MN + i);
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
  const f32x4_t gs = sum_parts(ws, MN, KS, m * N + n), us = sum_parts(ws, MN, KS, m * N + F + n);
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
      const f32x4_t v = sum_parts(ws, MN, KS, ((long)t * k + j) * N + n);
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

void check_routing(const at::Tensor& topi, int M, int k, int E, const char* who) {
  LLMCTL_CHECK(M >= 1 && M <= 64, who, ": 1 <= tokens <= 64 (got ", M, ")");
  LLMCTL_CHECK(E >= 1 && E <= 64, who, ": experts <= 64 (got ", E, ")");
  LLMCTL_CHECK(k >= 1 && k <= 8 && k <= E, who, ": 1 <= picks per token <= min(experts, 8) (got ", k, ")");
  LLMCTL_CHECK(topi.is_cuda() && topi.scalar_type() == at::kInt && topi.is_contiguous() && topi.dim() == 2 &&
                   topi.size(0) == M,
               who, ": topi int32 [M, k] on the GPU");
}

void check_table(const at::Tensor& ptrs, int E, const char* who) {
  LLMCTL_CHECK(ptrs.is_cuda() && ptrs.scalar_type() == at::kLong && ptrs.is_contiguous() && ptrs.numel() == E, who,
               ": expert pointer table int64 [E] on the GPU");
}

void check_act(const at::Tensor& t, const char* who) {
  LLMCTL_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16 && t.is_contiguous() && t.dim() == 2, who,
               ": bf16 contiguous 2-D GPU activations");
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
