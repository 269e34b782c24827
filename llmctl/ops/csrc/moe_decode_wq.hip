// Routed-expert decode GEMMs over quantised experts (gfx950): the two projections of moe_decode.hip
// with the expert weights streamed as fp8 e4m3fn + fp32 row scales (W8A16) or packed int4 + fp32
// group-128 scales (W4A16) -- llmctl.plugins.quantizers' formats, dequantised as in decode_gemm.h.
// On an MoE model the experts are nearly all of a decode step's HBM stream; this halves / quarters it.
//
// The quantised copies are made by the engine, so they are stacked: qweight [E, N, K] fp8 or
// [E, N, K / 2] uint8, scale [E, N] or [E, N, K / 128]; blockIdx.z indexes them, no pointer table.
//   * grid = (N / WR, K chunks of 1024, E).  A workgroup builds its expert's copy list in LDS as
//     moe_gemm_kernel does and returns before any weight or scale load when it is empty.
//   * The chunk's weight fragments are issued first and held quantised in registers: per lane and
//     128-deep block two 16-B loads of 16 consecutive k (fp8, one 16-row tile per wave, WR = 64) or
//     one 16-B load of 32 consecutive k for each of two 16-row tiles (int4, WR = 128).  Either way
//     64 VGPRs hold the chunk and a workgroup has 64 KB in flight.
//   * The listed x rows are gathered into LDS 16 copies at a time, a whole chunk deep (fp8: k order;
//     int4: lane-group-major and elements (0, 4, 1, 5, 2, 6, 3, 7), with the per-(copy, group) sums of
//     x taken while staging).  int4: the workgroup's 128 x 8 group scales go through LDS; a K block
//     is one scale group, its 4 MFMAs run on the exact integers 128 + u into a fresh tile t, and
//     acc += scale (t - 136 sum x).  fp8: the row scale multiplies the partial once before the store.
//   * An expert with more than 16 copies takes them 32 per pass: two column tiles, so every
//     dequantised A fragment (the VALU cost) feeds two MFMAs.  The same 33 KB of LDS then holds 32
//     rows of half a chunk, and the pass walks the chunk in two halves into the same accumulators
//     (a 32-row whole-chunk image would be 66 KB and leave two workgroups per CU).  An odd last
//     tile runs alone.
//   * fp32 partials go to ws[chunk][copy][n], every row written exactly once per chunk, and the
//     finalize passes of moe_decode.h follow unchanged.
// No atomics, no host sync, no data-dependent shapes, no scratch (134 / 162 VGPRs: three workgroups
// per CU, as moe_gemm_kernel).
#include <type_traits>

#include "decode_gemm.h"
#include "moe_decode.h"

namespace llmctl {
namespace {

constexpr int kKC = 1024;        // K chunk per workgroup
constexpr int kMaxCopies = 512;  // M k <= 64 x 8

template <int N>
using int_c = std::integral_constant<int, N>;

// The weight registers of a chunk are dequantised once per pass over the copy list.  Left alone, the
// compiler hoists that loop-invariant work out of the pass loop and keeps (spills) the bf16 image of
// the whole chunk; an empty asm on the quantised registers, at their use, keeps it in the pass.
__device__ __forceinline__ void fresh(uint4& q) { asm volatile("" : "+v"(q.x), "+v"(q.y), "+v"(q.z), "+v"(q.w)); }

template <bool W4, int NB>
__global__ __launch_bounds__(256, 3) void moe_gemm_wq_kernel(const unsigned short* __restrict__ x,
                                                          const unsigned char* __restrict__ qw,
                                                          const float* __restrict__ scale,
                                                          const int* __restrict__ topi, float* __restrict__ ws, int MK,
                                                          int xdiv, int N, int K) {
  static_assert(NB % 8 == 0, "a paired pass walks the chunk in two halves of NB / 2 blocks");
  constexpr int KC = NB * KBLK;
  constexpr int NT = W4 ? 2 : 1;       // 16-row weight tiles per wave
  constexpr int WR = 64 * NT;          // weight rows per workgroup
  constexpr int AV = W4 ? NB : 2 * NB;  // 16-B weight loads per tile and chunk
  // 16 rows x (KC + 8), or 32 rows x (KC / 2 + 8)
  __shared__ __attribute__((aligned(16))) unsigned short xs[32 * (KC / 2 + 8)];
  __shared__ __attribute__((aligned(16))) float xsum[W4 ? 16 * NB : 4];  // int4: sum of x over [copy][K block]
  __shared__ __attribute__((aligned(16))) float ssc[W4 ? WR : 1][NB];    // int4: scale of [weight row][K block]
  __shared__ int list[kMaxCopies];  // copy | x row << 16
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
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
  if (cnt == 0) return;  // unrouted expert: no weight or scale load is issued
  const int r = lane & 15, g = lane >> 4;
  const int nw0 = blockIdx.x * WR, n0 = nw0 + wave * 16 * NT;
  const int kc0 = blockIdx.y * KC;
  const int kc = min(KC, K - kc0);
  const int nb = kc / KBLK;
  const long wrb = W4 ? (K >> 1) : K;  // bytes per weight row
  uint4 a[NT][AV];
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const unsigned char* wrow = qw + ((long)e * N + n0 + 16 * i + r) * wrb + (W4 ? kc0 >> 1 : kc0) + 16 * g;
#pragma unroll
    for (int u = 0; u < NB; ++u) {
      const int bu = u < nb ? u : nb - 1;  // a short last chunk re-loads its last block
      if constexpr (W4) {
        a[i][u] = *reinterpret_cast<const uint4*>(wrow + bu * (KBLK / 2));
      } else {
#pragma unroll
        for (int h = 0; h < 2; ++h) a[i][2 * u + h] = *reinterpret_cast<const uint4*>(wrow + bu * KBLK + 64 * h);
      }
    }
  }
  // fp8: the row scales of the lane's 4 output columns.  int4: thread -> NB / 4 group scales of
  // weight rows tid / 4 + 64 i
  float4 rsc = make_float4(1.f, 1.f, 1.f, 1.f);
  float sv[NT][NB / 4];
  if constexpr (W4) {
    const float* srow = scale + ((long)e * N + nw0 + (tid >> 2)) * (K / KBLK) + kc0 / KBLK;
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
      for (int q = 0; q < NB / 4; ++q) {
        const int u = (tid & 3) * (NB / 4) + q;
        sv[i][q] = srow[(long)64 * i * (K / KBLK) + (u < nb ? u : nb - 1)];
      }
  } else {
    rsc = *reinterpret_cast<const float4*>(scale + (long)e * N + n0 + 4 * g);
  }
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (W4) {
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
      for (int q = 0; q < NB / 4; ++q) ssc[64 * i + (tid >> 2)][(tid & 3) * (NB / 4) + q] = sv[i][q];
  }
  // the two unpack constants held in VGPRs (opaque to the optimiser): (d & mask) | c is then one v_and_or_b32
  unsigned mask = 0x000F000Fu, one28 = 0x43004300u;
  asm volatile("" : "+v"(mask), "+v"(one28));

  // one pass: T column tiles (the copies c0 .. c0 + 16 T - 1 of the list) against the chunk's weights
  auto pass = [&](auto tc, int c0) {
    constexpr int T = decltype(tc)::value;
    constexpr int KH = KC / T, NBH = KH / KBLK;  // K and blocks per staged part (T parts per chunk)
    constexpr int XST = KH + 8, GS = KH / 4, V = KH / 8;  // LDS row stride, int4 lane-group stride, 16-B vectors per row
    f32x4_t acc[NT][T];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
      for (int t = 0; t < T; ++t) acc[i][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int p = 0; p < T; ++p) {
      if (p * NBH >= nb) continue;  // a short last chunk may end in the first half
      lds_sync();  // the list (first pass) / the previous part's MFMA reads of xs (LDS only: loads stay in flight)
      // rows of part p -> LDS; the whole workgroup takes every trip (int4: 16 consecutive threads =
      // one (copy, K block)); copies past the list and k past the chunk are staged as zeros
#pragma unroll
      for (int j = 0; j < 16 * T * V / 256; ++j) {
        const int i = tid + 256 * j;
        const int m = i / V, c = i % V;
        const int kl = p * KH + c * 8;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (c0 + m < cnt && kl < kc) v = *reinterpret_cast<const uint4*>(x + (long)(list[c0 + m] >> 16) * K + kc0 + kl);
        if constexpr (W4) {
          float s = 0.f;
          const unsigned vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
          for (int q = 0; q < 4; ++q) s += __uint_as_float(vv[q] << 16) + __uint_as_float(vv[q] & 0xFFFF0000u);
          uint4 pk;  // elements (0, 4, 1, 5, 2, 6, 3, 7)
          pk.x = (v.x & 0xFFFFu) | (v.z << 16);
          pk.y = (v.x >> 16) | (v.z & 0xFFFF0000u);
          pk.z = (v.y & 0xFFFFu) | (v.w << 16);
          pk.w = (v.y >> 16) | (v.w & 0xFFFF0000u);
          const int ul = c >> 4, cg = (c >> 2) & 3, cs = c & 3;
          *reinterpret_cast<uint4*>(xs + m * XST + cg * GS + ul * 32 + cs * 8) = pk;
#pragma unroll
          for (int o = 1; o < 16; o <<= 1) s += __shfl_xor(s, o);
          if ((tid & 15) == 0) xsum[m * NBH + ul] = s;
        } else {
          *reinterpret_cast<uint4*>(xs + m * XST + c * 8) = v;
        }
      }
      lds_sync();
      const unsigned short* xrow = xs + r * XST + (W4 ? g * GS : 16 * g);
#pragma unroll
      for (int ul = 0; ul < NBH; ++ul) {
        const int u = p * NBH + ul;
        if (u >= nb) continue;
        __builtin_amdgcn_sched_barrier(0);  // a block's LDS reads stay with its MFMAs (registers)
        if constexpr (W4) {
          float off[T];
          f32x4_t tt[NT][T];
#pragma unroll
          for (int t = 0; t < T; ++t) {
            off[t] = -136.f * xsum[(16 * t + r) * NBH + ul];
#pragma unroll
            for (int i = 0; i < NT; ++i) tt[i][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
          }
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            bf16x8_t xb[T];
#pragma unroll
            for (int t = 0; t < T; ++t) xb[t] = *reinterpret_cast<const bf16x8_t*>(xrow + 16 * t * XST + ul * 32 + 8 * s);
#pragma unroll
            for (int i = 0; i < NT; ++i) {
              if (s == 0) fresh(a[i][u]);
              const uint4 q = a[i][u];
              const bf16x8_t af = u4x8_to_bf16x8(s == 0 ? q.x : s == 1 ? q.y : s == 2 ? q.z : q.w, mask, one28);
#pragma unroll
              for (int t = 0; t < T; ++t) tt[i][t] = mfma16(af, xb[t], tt[i][t]);
            }
          }
          // D: lane holds [weight row n0 + 16 i + 4 g + j][copy c0 + 16 t + r]
#pragma unroll
          for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const float sc = ssc[wave * 16 * NT + 16 * i + 4 * g + j][u];
#pragma unroll
              for (int t = 0; t < T; ++t) acc[i][t][j] += sc * (tt[i][t][j] + off[t]);
            }
        } else {
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            fresh(a[0][2 * u + h]);
            const uint4 q = a[0][2 * u + h];
            const bf16x8_t a0 = fp8x8_to_bf16x8(q.x, q.y), a1 = fp8x8_to_bf16x8(q.z, q.w);
#pragma unroll
            for (int t = 0; t < T; ++t) {
              const unsigned short* xp = xrow + 16 * t * XST + ul * KBLK + 64 * h;
              acc[0][t] = mfma16(a0, *reinterpret_cast<const bf16x8_t*>(xp), acc[0][t]);
              acc[0][t] = mfma16(a1, *reinterpret_cast<const bf16x8_t*>(xp + 8), acc[0][t]);
            }
          }
        }
      }
    }
#pragma unroll
    for (int t = 0; t < T; ++t) {
      if (c0 + 16 * t + r >= cnt) continue;
      const int copy = list[c0 + 16 * t + r] & 0xffff;
      float* out = ws + ((long)blockIdx.y * MK + copy) * N + n0 + 4 * g;
#pragma unroll
      for (int i = 0; i < NT; ++i) {
        f32x4_t v = acc[i][t];
        if constexpr (!W4) {
          v[0] *= rsc.x;
          v[1] *= rsc.y;
          v[2] *= rsc.z;
          v[3] *= rsc.w;
        }
        *reinterpret_cast<f32x4_t*>(out + 16 * i) = v;
      }
    }
  };

  int c0 = 0;
  for (; cnt - c0 > 16; c0 += 32) pass(int_c<2>{}, c0);
  if (c0 < cnt) pass(int_c<1>{}, c0);
}

bool is_int4(const at::Tensor& qw) { return qw.scalar_type() == at::kByte; }

// stacked experts: fp8 [E, N, K] + scales [E, N], or uint8 [E, N, K / 2] + scales [E, N, K / 128]
void check_experts(const at::Tensor& qw, const at::Tensor& scale, int N, int K, const char* who) {
  LLMCTL_CHECK(qw.is_cuda() && qw.is_contiguous() && qw.dim() == 3 &&
                   (qw.scalar_type() == at::kFloat8_e4m3fn || qw.scalar_type() == at::kByte),
               who, ": expert weights fp8 e4m3fn [E, N, K] or packed int4 uint8 [E, N, K / 2] on the GPU");
  const bool w4 = is_int4(qw);
  const long E = qw.size(0);
  LLMCTL_CHECK(qw.size(1) == N && qw.size(2) == (w4 ? K / 2 : K), who, ": expert weights must be [E, ", N, ", ",
               w4 ? K / 2 : K, "], got [", E, ", ", qw.size(1), ", ", qw.size(2), "]");
  LLMCTL_CHECK(N % (w4 ? 128 : 64) == 0, who, ": out features % ", w4 ? 128 : 64, " == 0 (got ", N, ")");
  LLMCTL_CHECK(scale.is_cuda() && scale.is_contiguous() && scale.scalar_type() == at::kFloat &&
                   scale.device() == qw.device() && scale.size(0) == E && scale.size(1) == N &&
                   (w4 ? scale.dim() == 3 && scale.size(2) == K / KBLK : scale.dim() == 2),
               who, w4 ? ": int4 experts need fp32 group scales [E, N, K / 128] on the GPU"
                       : ": fp8 experts need fp32 row scales [E, N] on the GPU");
  LLMCTL_CHECK(reinterpret_cast<uintptr_t>(qw.data_ptr()) % 16 == 0 && reinterpret_cast<uintptr_t>(scale.data_ptr()) % 16 == 0,
               who, ": expert weights and scales must be 16-byte aligned");
}

// routed x dequant(W_e)^T as fp32 K-chunk partials ws [KS][MK][N]; returns KS
int moe_partials_wq(const at::Tensor& x, const at::Tensor& qw, const at::Tensor& scale, const at::Tensor& topi,
                    at::Tensor& ws, int MK, int xdiv, int N, int K) {
  const int KS = (K + kKC - 1) / kKC, E = qw.size(0);
  ws = at::empty({(long)KS * MK * N}, x.options().dtype(at::kFloat));
  const unsigned char* wp = static_cast<const unsigned char*>(qw.data_ptr());
  if (is_int4(qw))
    hipLaunchKernelGGL((moe_gemm_wq_kernel<true, kKC / KBLK>), dim3(N / 128, KS, E), dim3(256), 0, stream(), bf_ptr(x),
                       wp, scale.data_ptr<float>(), topi.data_ptr<int>(), ws.data_ptr<float>(), MK, xdiv, N, K);
  else
    hipLaunchKernelGGL((moe_gemm_wq_kernel<false, kKC / KBLK>), dim3(N / 64, KS, E), dim3(256), 0, stream(), bf_ptr(x),
                       wp, scale.data_ptr<float>(), topi.data_ptr<int>(), ws.data_ptr<float>(), MK, xdiv, N, K);
  return KS;
}

}  // namespace

// moe_decode_up_swiglu over quantised experts: qweight = W_up stacked [E, 2F, h] (gate rows first)
at::Tensor moe_decode_up_swiglu_wq(const at::Tensor& x, const at::Tensor& qweight, const at::Tensor& scale,
                                   const at::Tensor& topi) {
  const char* who = "moe_decode_up_swiglu_wq";
  check_act(x, who);
  LLMCTL_CHECK(qweight.dim() == 3, who, ": stacked expert weights [E, 2F, h]");
  const int M = x.size(0), h = x.size(1), k = topi.dim() == 2 ? topi.size(1) : 0;
  const int E = qweight.size(0), F = qweight.size(1) / 2;
  check_routing(topi, M, k, E, who);
  LLMCTL_CHECK(h % 128 == 0 && F >= 128 && F % 128 == 0, who, ": h % 128 == 0, F % 128 == 0 (got ", h, ", ", F, ")");
  check_experts(qweight, scale, 2 * F, h, who);
  LLMCTL_CHECK(qweight.device() == x.device() && topi.device() == x.device(), who, ": operands on one device");
  const c10::DeviceGuard guard(x.device());
  const int MK = M * k;
  at::Tensor ws;
  const int KS = moe_partials_wq(x, qweight, scale, topi, ws, MK, k, 2 * F, h);
  auto act = at::empty({MK, F}, x.options());
  const long n4 = (long)MK * F / 4;
  hipLaunchKernelGGL(moe_fin_swiglu_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, stream(),
                     ws.data_ptr<float>(), bf_mut(act), MK, F, KS);
  return act;
}

// moe_decode_down_add_rmsnorm over quantised experts: qweight = W_down stacked [E, h, F]
std::tuple<at::Tensor, at::Tensor> moe_decode_down_add_rmsnorm_wq(const at::Tensor& act, const at::Tensor& qweight,
                                                                  const at::Tensor& scale, const at::Tensor& topi,
                                                                  const at::Tensor& topw, const at::Tensor& residual,
                                                                  const at::Tensor& norm_w, double eps) {
  const char* who = "moe_decode_down_add_rmsnorm_wq";
  check_act(act, who);
  check_act(residual, who);
  LLMCTL_CHECK(qweight.dim() == 3, who, ": stacked expert weights [E, h, F]");
  const int M = residual.size(0), h = residual.size(1), F = act.size(1), k = topi.dim() == 2 ? topi.size(1) : 0;
  const int E = qweight.size(0);
  check_routing(topi, M, k, E, who);
  LLMCTL_CHECK(act.size(0) == (long)M * k, who, ": act [M k, F]");
  LLMCTL_CHECK(topw.is_cuda() && topw.scalar_type() == at::kFloat && topw.is_contiguous() && topw.dim() == 2 &&
                   topw.size(0) == M && topw.size(1) == k,
               who, ": topw fp32 [M, k] on the GPU");
  LLMCTL_CHECK(h % 128 == 0 && F >= 128 && F % 128 == 0 && h <= 16384, who,
               ": h % 128 == 0, F % 128 == 0, h <= 16384 (row staged in LDS; got ", h, ", ", F, ")");
  check_experts(qweight, scale, h, F, who);
  LLMCTL_CHECK(norm_w.is_cuda() && norm_w.is_contiguous() && norm_w.scalar_type() == at::kBFloat16 && norm_w.numel() == h,
               who, ": norm weight bf16 [h]");
  LLMCTL_CHECK(qweight.device() == act.device() && topi.device() == act.device() && topw.device() == act.device() &&
                   residual.device() == act.device() && norm_w.device() == act.device(),
               who, ": operands on one device");
  const c10::DeviceGuard guard(act.device());
  const int MK = M * k;
  at::Tensor ws;
  const int KS = moe_partials_wq(act, qweight, scale, topi, ws, MK, 1, h, F);
  auto y = at::empty({M, h}, act.options());
  auto res_out = at::empty({M, h}, act.options());
  hipLaunchKernelGGL(moe_fin_combine_add_rmsnorm_kernel, dim3(M), dim3(1024), (size_t)h * 4, stream(),
                     ws.data_ptr<float>(), topw.data_ptr<float>(), bf_ptr(residual), bf_ptr(norm_w), bf_mut(y),
                     bf_mut(res_out), M, k, h, KS, (float)eps);
  return {y, res_out};
}

TORCH_LIBRARY_IMPL(llmctl, CUDA, m) {
  m.impl("moe_decode_up_swiglu_wq", &moe_decode_up_swiglu_wq);
  m.impl("moe_decode_down_add_rmsnorm_wq", &moe_decode_down_add_rmsnorm_wq);
}

}  // namespace llmctl
