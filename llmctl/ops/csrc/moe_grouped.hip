// Routed-expert MLP for 1..8192 token rows (gfx950): the compute-shaped sibling of moe_decode.hip.
// Prefill chunks, mixed steps and decode steps above 64 rows are GEMM-bound, so the routed copies
// are sorted by expert on the device and the two projections run as grouped GEMMs over row tiles.
// No host synchronisation, no atomics, no data-dependent launch shapes: the layer can be captured.
//
//   plan      one workgroup of 16 waves.  Wave w owns a contiguous range of the copies c = t k + j;
//             a wave finds the lanes that hold the same expert with 6 ballots (one per index bit),
//             the lowest such lane adds their number to the wave's LDS counter of that expert.
//             Wave 0 turns the totals into tiles of BM rows per expert (exclusive scan over lanes)
//             and the counters into each wave's first row per expert; a second walk writes
//             perm[sorted row] = c (copy order within an expert) and tile_expert[tile] = e.  Rows
//             and tiles that stay unused hold -1.  ntile = M k / BM + E bounds the tiles from shapes.
//   gate/up   grid (ntile, F / 64), row tile fastest: the tiles of one expert are neighbours, so
//             the workgroups resident together read one weight panel.  A tile with expert -1 returns
//             before any load.  256 threads; the weight tile is 64 gate rows n0.. and the 64 matching
//             up rows F + n0.., the A tile BM rows gathered from x[perm / k] (zero rows for padding).
//             Both are K-contiguous and go global -> registers -> LDS in K steps of 64, two LDS
//             buffers, rows padded to 72 elements, the next step's loads issued before the current
//             step's MFMAs.  Wave (wn, wm) multiplies weight blocks wn (gate) and wn + 2 (up) of 32
//             rows with the 32-row token blocks wm, wm + 2, .. (MFMA 32x32x16 bf16, weights on the
//             row axis), so a lane holds gate and up of the same elements: the epilogue rounds both
//             to bf16, applies silu(g) u and stores 4 bf16 per row group to act_sorted[row][F].
//   down      the same loop over A = act_sorted (contiguous: the point of the sorted layout) and
//             128 rows of W_down[e]; the epilogue stores row perm[row] of y_copy [M k, h] in bf16.
//             A row of A only reaches its own row of C; padding rows (zeros) are not stored.
//   combine   y[t] = bf16(sum_j topw[t, j] y_copy[t k + j]) in fp32, slot order.
// BM = 128 when the experts average 128 copies or more (M k >= 128 E), else 64.
#include "moe_decode.h"

namespace llmctl {
namespace {

using bf16x8_t = __attribute__((ext_vector_type(8))) __bf16;
using f32x16_t = __attribute__((ext_vector_type(16))) float;
using u32x4_t = __attribute__((ext_vector_type(4))) unsigned;  // 16 B in flight (a plain vector: stays in registers)

constexpr int kBN = 128;      // weight rows per tile
constexpr int kBK = 64;       // K per step
constexpr int kLd = kBK + 8;  // LDS row stride in elements (144 B: 16 rows cover the 64 banks once)
constexpr int kPlanWaves = 16;
constexpr int kMaxRows = 8192, kMaxCopies = 65536;

// ---- plan
// the lanes of this wave that hold the same expert as this lane (v in [0, 64), ok lanes only)
__device__ __forceinline__ unsigned long long same_expert(int v, bool ok) {
  unsigned long long m = __ballot(ok);
#pragma unroll
  for (int b = 0; b < 6; ++b) {
    const bool bit = (v >> b) & 1;
    const unsigned long long bb = __ballot(bit);
    m &= bit ? bb : ~bb;
  }
  return m;
}

template <int BM>
__global__ __launch_bounds__(1024) void moe_plan_kernel(const int* __restrict__ topi, int* __restrict__ perm,
                                                        int* __restrict__ tile_expert, int MK, int E, int ntile) {
  __shared__ int cnt_s[kPlanWaves][64];  // pass 1: copies of expert e in wave w's range; pass 2: its next row
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  volatile int* cnt = cnt_s[wave];
  for (int i = threadIdx.x; i < ntile * BM; i += 1024) perm[i] = -1;
  for (int i = threadIdx.x; i < ntile; i += 1024) tile_expert[i] = -1;
  cnt[lane] = 0;
  const int seg = (MK + kPlanWaves * 64 - 1) / (kPlanWaves * 64) * 64;
  const int i0 = min(MK, wave * seg), i1 = min(MK, i0 + seg);
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int c = i0; c < i1; c += 64) {
    const int i = c + lane;
    const int v = i < i1 ? topi[i] : -1;
    const bool ok = (unsigned)v < (unsigned)E;  // an index out of range is left out (its copy counts as 0)
    const unsigned long long m = same_expert(v, ok);
    if (ok && (m & below) == 0) cnt[v] += __popcll(m);  // one leader per expert: no two lanes share a counter
  }
  __syncthreads();
  if (wave == 0) {
    int tot = 0;
    for (int w = 0; w < kPlanWaves; ++w) tot += cnt_s[w][lane];  // lanes >= E: 0
    const int nt = (tot + BM - 1) / BM;
    int inc = nt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(inc, o);
      if (lane >= o) inc += up;
    }
    const int t0 = inc - nt;  // sum over experts of nt <= M k / BM + E = ntile
    for (int t = 0; t < nt; ++t) tile_expert[t0 + t] = lane;
    int row = t0 * BM;
    for (int w = 0; w < kPlanWaves; ++w) {
      const int c = cnt_s[w][lane];
      cnt_s[w][lane] = row;
      row += c;
    }
  }
  __syncthreads();
  for (int c = i0; c < i1; c += 64) {
    const int i = c + lane;
    const int v = i < i1 ? topi[i] : -1;
    const bool ok = (unsigned)v < (unsigned)E;
    const unsigned long long m = same_expert(v, ok);
    const int row = ok ? cnt[v] : 0;  // every lane reads before the leader advances the counter
    if (ok) perm[row + __popcll(m & below)] = i;
    if (ok && (m & below) == 0) cnt[v] = row + __popcll(m);
  }
}

// ---- grouped GEMM: C[n][row] = W_e[n] . A[row] over one (row tile, weight tile)
// UP:  A rows gathered from a = x [M, K] by perm / k; weights W_up[e] [2 N, K], the tile's rows are
//      n0 .. n0 + 63 (gate) and N + n0 .. (up), n0 = 64 blockIdx.y; out = act_sorted [rows, N].
// !UP: A rows tile BM .. of a = act_sorted [rows, K]; weights W_down[e] [N, K], rows n0 .. n0 + 127,
//      n0 = 128 blockIdx.y; out = y_copy [M k, N], row perm[row].
template <int BM, bool UP>
__global__ __launch_bounds__(256) void moe_grouped_gemm_kernel(const unsigned short* __restrict__ a,
                                                               const int64_t* __restrict__ wptrs,
                                                               const int* __restrict__ perm,
                                                               const int* __restrict__ tile_expert,
                                                               unsigned short* __restrict__ out, int k, int N, int K) {
  constexpr int MB = BM / 64;  // 32-row token blocks per wave
  constexpr int AQ = BM / 32;  // 16-byte A chunks per thread and K step
  __shared__ __attribute__((aligned(16))) unsigned short wl[2][kBN * kLd];
  __shared__ __attribute__((aligned(16))) unsigned short al[2][BM * kLd];
  const int tile = blockIdx.x;
  const int e = tile_expert[tile];
  if (e < 0) return;  // unused tile: nothing is loaded
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wn = wave & 1, wm = wave >> 1, l32 = lane & 31, hi = lane >> 5;
  const int n0 = blockIdx.y * (UP ? 64 : kBN);
  const unsigned short* wbase = reinterpret_cast<const unsigned short*>(wptrs[e]);

  // this thread's chunks of a K step: chunk q is row (tid + 256 q) / 8, elements 8 ((tid + 256 q) % 8) ..
  const int cr = tid >> 3, cc = (tid & 7) * 8;
  const unsigned short* wp[4];
  const unsigned short* ap[AQ];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int r = cr + 32 * q;
    const long wrow = UP ? (r < 64 ? n0 + r : N + n0 + r - 64) : n0 + r;
    wp[q] = wbase + wrow * K + cc;
  }
#pragma unroll
  for (int q = 0; q < AQ; ++q) {
    const long srow = (long)tile * BM + cr + 32 * q;
    if (UP) {
      const int p = perm[srow];
      ap[q] = p < 0 ? nullptr : a + (long)(p / k) * K + cc;
    } else {
      ap[q] = a + srow * K + cc;
    }
  }
  u32x4_t wv[4], av[AQ];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) wv[q] = *reinterpret_cast<const u32x4_t*>(wp[q] + k0);
#pragma unroll
    for (int q = 0; q < AQ; ++q)
      av[q] = ap[q] != nullptr ? *reinterpret_cast<const u32x4_t*>(ap[q] + k0) : u32x4_t{0u, 0u, 0u, 0u};
  };
  auto stage = [&](int buf) {
#pragma unroll
    for (int q = 0; q < 4; ++q) *reinterpret_cast<u32x4_t*>(&wl[buf][(cr + 32 * q) * kLd + cc]) = wv[q];
#pragma unroll
    for (int q = 0; q < AQ; ++q) *reinterpret_cast<u32x4_t*>(&al[buf][(cr + 32 * q) * kLd + cc]) = av[q];
  };

  f32x16_t acc[2][MB];
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int mi = 0; mi < MB; ++mi)
#pragma unroll
      for (int i = 0; i < 16; ++i) acc[nb][mi][i] = 0.f;

  fetch(0);
  stage(0);
  __syncthreads();
  const int nk = K / kBK;
  const int foff = l32 * kLd + 8 * hi;  // MFMA 32x32x16: lane = row l32, k = 8 hi .. 8 hi + 7
  for (int ks = 0; ks < nk; ++ks) {
    const int buf = ks & 1;
    if (ks + 1 < nk) fetch((ks + 1) * kBK);  // in flight under this step's MFMAs
#pragma unroll
    for (int kk = 0; kk < kBK / 16; ++kk) {
      bf16x8_t fw[2], fa[MB];
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
        fw[nb] = *reinterpret_cast<const bf16x8_t*>(&wl[buf][(wn + 2 * nb) * 32 * kLd + foff + 16 * kk]);
#pragma unroll
      for (int mi = 0; mi < MB; ++mi)
        fa[mi] = *reinterpret_cast<const bf16x8_t*>(&al[buf][(wm + 2 * mi) * 32 * kLd + foff + 16 * kk]);
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int mi = 0; mi < MB; ++mi)
          acc[nb][mi] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fw[nb], fa[mi], acc[nb][mi], 0, 0, 0);
    }
    if (ks + 1 < nk) stage(buf ^ 1);  // last read in step ks - 1, before that step's barrier
    __syncthreads();
  }

  // C layout: lane holds column (token row) l32, element i is weight row 8 (i / 4) + 4 hi + i % 4
#pragma unroll
  for (int mi = 0; mi < MB; ++mi) {
    const long srow = (long)tile * BM + (wm + 2 * mi) * 32 + l32;
    if (UP) {
      unsigned short* dst = out + srow * N + n0 + wn * 32 + 4 * hi;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        ushort4 pk;
        unsigned short* pp = reinterpret_cast<unsigned short*>(&pk);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float gv = bf2f(f2bf(acc[0][mi][4 * g + j])), uv = bf2f(f2bf(acc[1][mi][4 * g + j]));
          pp[j] = f2bf(gv * (1.f / (1.f + __expf(-gv))) * uv);
        }
        *reinterpret_cast<ushort4*>(dst + 8 * g) = pk;
      }
    } else {
      const int p = perm[srow];
      if (p < 0) continue;
      unsigned short* dst = out + (long)p * N + n0 + wn * 32 + 4 * hi;
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          ushort4 pk;
          pk.x = f2bf(acc[nb][mi][4 * g]), pk.y = f2bf(acc[nb][mi][4 * g + 1]);
          pk.z = f2bf(acc[nb][mi][4 * g + 2]), pk.w = f2bf(acc[nb][mi][4 * g + 3]);
          *reinterpret_cast<ushort4*>(dst + 64 * nb + 8 * g) = pk;
        }
    }
  }
}

// ---- combine: thread = 8 columns of one token; a copy whose expert index is out of range counts as 0
__global__ __launch_bounds__(256) void moe_grouped_combine_kernel(const unsigned short* __restrict__ yc,
                                                                  const int* __restrict__ topi,
                                                                  const float* __restrict__ topw,
                                                                  unsigned short* __restrict__ y, int M, int k, int h,
                                                                  int E) {
  const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 8;
  if (i >= (long)M * h) return;
  const long t = i / h, n = i % h;
  float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < k; ++j) {
    if ((unsigned)topi[t * k + j] >= (unsigned)E) continue;
    const float w = topw[t * k + j];
    float v[8];
    load8(yc + (t * k + j) * h + n, v);
#pragma unroll
    for (int q = 0; q < 8; ++q) o[q] += w * v[q];
  }
  store8(y + i, o);
}

template <int BM>
void launch_grouped(const at::Tensor& x, const at::Tensor& up_ptrs, const at::Tensor& down_ptrs, const at::Tensor& topi,
                    const at::Tensor& topw, at::Tensor& y, int M, int k, int h, int F, int E) {
  const int MK = M * k, ntile = MK / BM + E;
  auto iopt = x.options().dtype(at::kInt);
  auto perm = at::empty({(long)ntile * BM}, iopt);
  auto tile_expert = at::empty({ntile}, iopt);
  auto act = at::empty({(long)ntile * BM, F}, x.options());  // sorted rows; unused tiles are never touched
  auto yc = at::empty({MK, h}, x.options());
  hipLaunchKernelGGL(moe_plan_kernel<BM>, dim3(1), dim3(1024), 0, stream(), topi.data_ptr<int>(), perm.data_ptr<int>(),
                     tile_expert.data_ptr<int>(), MK, E, ntile);
  hipLaunchKernelGGL((moe_grouped_gemm_kernel<BM, true>), dim3(ntile, F / 64), dim3(256), 0, stream(), bf_ptr(x),
                     up_ptrs.data_ptr<int64_t>(), perm.data_ptr<int>(), tile_expert.data_ptr<int>(), bf_mut(act), k, F, h);
  hipLaunchKernelGGL((moe_grouped_gemm_kernel<BM, false>), dim3(ntile, h / kBN), dim3(256), 0, stream(), bf_ptr(act),
                     down_ptrs.data_ptr<int64_t>(), perm.data_ptr<int>(), tile_expert.data_ptr<int>(), bf_mut(yc), k, h, F);
  const long n8 = (long)M * h / 8;
  hipLaunchKernelGGL(moe_grouped_combine_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, stream(), bf_ptr(yc),
                     topi.data_ptr<int>(), topw.data_ptr<float>(), bf_mut(y), M, k, h, E);
}

void check_limits(int M, int k, int E, int h, const char* who) {
  LLMCTL_CHECK(M >= 1 && M <= kMaxRows && (long)M * k <= kMaxCopies, who, ": 1 <= tokens <= 8192, tokens x picks <= 65536 (got ",
               M, " x ", k, ")");
  LLMCTL_CHECK(E >= 1 && E <= 64 && k >= 1 && k <= 8 && k <= E, who,
               ": experts <= 64, 1 <= picks per token <= min(experts, 8) (got ", E, ", ", k, ")");
  LLMCTL_CHECK(h % 128 == 0, who, ": hidden % 128 == 0 (got ", h, ")");
}

}  // namespace

// moe_route for any row count up to 8192: the same kernel, one workgroup per token
std::tuple<at::Tensor, at::Tensor> moe_route_rows(const at::Tensor& x, const at::Tensor& w_router, int64_t k) {
  check_act(x, "moe_route_rows");
  check_act(w_router, "moe_route_rows");
  const int M = x.size(0), h = x.size(1), E = w_router.size(0);
  LLMCTL_CHECK(w_router.size(1) == h, "moe_route_rows: router [E, h]");
  check_limits(M, (int)k, E, h, "moe_route_rows");
  const c10::DeviceGuard guard(x.device());
  auto topi = at::empty({M, k}, x.options().dtype(at::kInt));
  auto topw = at::empty({M, k}, x.options().dtype(at::kFloat));
  hipLaunchKernelGGL(moe_route_kernel, dim3(M), dim3(256), 0, stream(), bf_ptr(x), bf_ptr(w_router),
                     topi.data_ptr<int>(), topw.data_ptr<float>(), E, (int)k, h);
  return {topi, topw};
}

// y [M, h] = sum_j topw[t, j] W_down[e] (silu(g) u of W_up[e] x[t]), e = topi[t, j]
at::Tensor moe_grouped_mlp(const at::Tensor& x, const at::Tensor& up_ptrs, const at::Tensor& down_ptrs,
                           const at::Tensor& topi, const at::Tensor& topw, int64_t F) {
  check_act(x, "moe_grouped_mlp");
  const int M = x.size(0), h = x.size(1), E = up_ptrs.numel(), k = topi.dim() == 2 ? topi.size(1) : 0;
  check_limits(M, k, E, h, "moe_grouped_mlp");
  LLMCTL_CHECK(F >= 128 && F % 128 == 0 && F <= (1 << 20), "moe_grouped_mlp: F % 128 == 0, F >= 128 (got ", F, ")");
  for (const at::Tensor* p : {&up_ptrs, &down_ptrs})
    LLMCTL_CHECK(p->is_cuda() && p->scalar_type() == at::kLong && p->is_contiguous() && p->numel() == E,
                 "moe_grouped_mlp: expert pointer tables int64 [E] on the GPU");
  LLMCTL_CHECK(topi.is_cuda() && topi.scalar_type() == at::kInt && topi.is_contiguous() && topi.dim() == 2 &&
                   topi.size(0) == M,
               "moe_grouped_mlp: topi int32 [M, k] on the GPU");
  LLMCTL_CHECK(topw.is_cuda() && topw.scalar_type() == at::kFloat && topw.is_contiguous() && topw.dim() == 2 &&
                   topw.size(0) == M && topw.size(1) == k,
               "moe_grouped_mlp: topw fp32 [M, k] on the GPU");
  const c10::DeviceGuard guard(x.device());
  auto y = at::empty({M, h}, x.options());
  if ((long)M * k >= 128L * E) launch_grouped<128>(x, up_ptrs, down_ptrs, topi, topw, y, M, k, h, (int)F, E);
  else launch_grouped<64>(x, up_ptrs, down_ptrs, topi, topw, y, M, k, h, (int)F, E);
  return y;
}

TORCH_LIBRARY_IMPL(llmctl, CUDA, m) {
  m.impl("moe_route_rows", &moe_route_rows);
  m.impl("moe_grouped_mlp", &moe_grouped_mlp);
}

}  // namespace llmctl
