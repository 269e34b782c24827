// Mid-batch decode GEMM (gfx950): fp32 partials ws[KS][M][N] of x[M,K] · W[N,K]^T for 17 <= M <= 64
// token rows and quantised weights -- fp8 e4m3fn with fp32 row scales (W8A16), or packed int4
// (uint8 [N, K/2]) with fp32 group-128 scales [N, K/128] (W4A16).  The finalize passes of
// skinny_gemm.hip sum the partials, as they do for the <= 16-row kernels.
//
// At 32-64 rows the projection is still bound by the weight stream, but the two costs that the
// 16-row kernels could ignore now rival it: the staged token rows (64 rows of a K chunk are 4x the
// bytes of 64 int4 weight rows) and the fp32 partials (at KS = 4, M = 64 as many bytes as the int4
// weight).  Hence:
//   * MFMA 16x16x32 bf16, weight rows on the MFMA row axis, tokens on the column axis.  A wave
//     owns NT = 2 16-row weight tiles and MT = ceil(M / 16) token tiles (NT x MT fp32 accumulators);
//     a workgroup = NW waves = 32 NW weight rows: 128 (4 waves, two workgroups per CU), or 256 (8
//     waves, one per CU) for int4 at 33-64 rows on the wide projections, so that the token bytes
//     staged per chunk do not exceed the int4 weight bytes they meet.  Rows >= M are staged as zeros and never stored; a last workgroup past N clamps its
//     loads to row N - 1 and skips those tiles' stores.
//   * every dequantised A fragment is built once in registers and feeds MT MFMAs: the fp8 -> bf16
//     conversion and the int4 v_and_or_b32 unpack are amortised over the token tiles.
//   * K is walked inside the workgroup in chunks of 256 through a double-buffered LDS ring: chunk
//     c + 1's weight loads (and int4 scales) are issued before chunk c's MFMAs, its token rows are
//     loaded behind them and written to the other buffer after the MFMAs; one LDS barrier per
//     chunk.  A slice of cps chunks per blockIdx.y; the host picks the fewest slices that fill the
//     machine (decode_mid_splits).
//   * LDS token layout (both kinds): lane-group-major, [g][block][MFMA step][8], g at multiples of
//     128 B and rows 16 B past a multiple of 512 B, so the ds_read_b128 of a 16-lane group hits 16
//     distinct 16-B slots.  int4: lane group g's 16-B load holds k = 32 g + [0, 32) of a block, step
//     s = dword s, elements in the unpack's order (0, 4, 1, 5, 2, 6, 3, 7).  fp8: its two 16-B loads
//     hold k = 64 h + 16 g + [0, 16), step s = 2 h + half.
//   * int4 scaling as in decode_gemm_w4_kernel: a block is one scale group, its MFMAs run on the
//     exact integers 128 + u into fresh tiles t, and acc += scale[row][group] (t - 136 sum_k x); the
//     sums of x per (token, group) are taken while the token rows are staged, `off` differs per
//     token tile.  fp8: the row scale multiplies the accumulators once, before the store.
// No atomics, no host sync, no data-dependent shapes, no scratch (profiles/decode_wq_mid.txt has
// the registers, LDS and occupancy of every instantiation).
#include <algorithm>

#include "decode_gemm.h"

namespace llmctl {
namespace {

constexpr int KCH = 256;          // K per chunk
constexpr int NBC = KCH / KBLK;   // blocks (int4 scale groups) per chunk
constexpr int XST = KCH + 8;      // LDS token row stride (elements)
constexpr int GS = KCH / 4;       // lane-group stride within an LDS row
constexpr int NT = 2;             // 16-row weight tiles per wave

template <bool W4, int MT, int NW>
__global__ __launch_bounds__(64 * NW, 2) void decode_gemm_mid_kernel(const unsigned short* __restrict__ x,
                                                                     const unsigned char* __restrict__ w,
                                                                     const float* __restrict__ wscale,
                                                                     float* __restrict__ ws, int M, int N, int K,
                                                                     int cps) {
  constexpr int NTH = 64 * NW, ROWS = 16 * MT, WR = 16 * NT * NW;
  constexpr int AV = W4 ? NBC : 2 * NBC;       // 16-B weight loads per tile and chunk
  constexpr int TV = ROWS * (KCH / 8) / NTH;   // 16-B token loads per thread and chunk
  static_assert(WR * NBC == NTH, "one int4 scale per thread and chunk");
  __shared__ __attribute__((aligned(16))) unsigned short xs[2][ROWS * XST];
  __shared__ float xsum[2][W4 ? ROWS : 1][NBC];  // int4: sum of x over [token][block]
  __shared__ float ssc[2][W4 ? WR : 1][NBC];     // int4: scale of [weight row][block]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int nw0 = blockIdx.x * WR, n0 = nw0 + wave * 16 * NT;
  const int chunks = (K + KCH - 1) / KCH;
  const int c0 = blockIdx.y * cps;
  const int nch = min(cps, chunks - c0);
  const long wrb = W4 ? (K >> 1) : K;  // bytes per weight row

  const unsigned char* wrow[NT];
#pragma unroll
  for (int i = 0; i < NT; ++i) wrow[i] = w + (long)min(n0 + 16 * i + r, N - 1) * wrb + 16 * g;
  // int4: thread -> the scale of weight row tid / 2, block tid % 2
  const float* srow = wscale + (long)min(nw0 + (tid >> 1), N - 1) * (K / KBLK);

  uint4 a[2][NT][AV];  // weights of the chunk in work and of the next one
  uint4 tv[TV];        // token rows of the next chunk
  float sv = 0.f;      // int4 scale of the next chunk

  // valid blocks of local chunk c (the last chunk of K may hold one)
  auto blocks = [&](int c) { return min(NBC, (K - (c0 + c) * KCH) / KBLK); };
  // issue the global loads of local chunk c: weights, scales, then token rows (past-the-end blocks
  // re-read the last valid one and are not used)
  auto load = [&](uint4 (&aw)[NT][AV], int c) {
    const int k0 = (c0 + c) * KCH, nb = blocks(c);
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
      for (int u = 0; u < NBC; ++u) {
        const int bu = u < nb ? u : nb - 1;
        if constexpr (W4) {
          aw[i][u] = *reinterpret_cast<const uint4*>(wrow[i] + (k0 >> 1) + bu * (KBLK / 2));
        } else {
#pragma unroll
          for (int h = 0; h < 2; ++h) aw[i][2 * u + h] = *reinterpret_cast<const uint4*>(wrow[i] + k0 + bu * KBLK + 64 * h);
        }
      }
    if constexpr (W4) sv = srow[k0 / KBLK + min(tid & 1, nb - 1)];
    // thread -> 16-B vector tid % 32 of token rows tid / 32 + 2 NW j
    const int cv = tid & 31;
#pragma unroll
    for (int j = 0; j < TV; ++j) {
      const int m = (tid >> 5) + 2 * NW * j;
      tv[j] = make_uint4(0, 0, 0, 0);
      if (m < M && cv * 8 < nb * KBLK) tv[j] = *reinterpret_cast<const uint4*>(x + (long)m * K + k0 + cv * 8);
    }
  };
  // the loaded token rows (and int4 group sums, scales) -> LDS buffer b
  auto stage = [&](int b) {
    const int cv = tid & 31, u = cv >> 4;
#pragma unroll
    for (int j = 0; j < TV; ++j) {
      const int m = (tid >> 5) + 2 * NW * j;
      const uint4 v = tv[j];
      if constexpr (W4) {
        float s = 0.f;
        const unsigned vv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) s += __uint_as_float(vv[e] << 16) + __uint_as_float(vv[e] & 0xFFFF0000u);
        uint4 p;  // elements (0, 4, 1, 5, 2, 6, 3, 7)
        p.x = (v.x & 0xFFFFu) | (v.z << 16);
        p.y = (v.x >> 16) | (v.z & 0xFFFF0000u);
        p.z = (v.y & 0xFFFFu) | (v.w << 16);
        p.w = (v.y >> 16) | (v.w & 0xFFFF0000u);
        *reinterpret_cast<uint4*>(&xs[b][m * XST + ((cv >> 2) & 3) * GS + u * 32 + (cv & 3) * 8]) = p;
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) s += __shfl_xor(s, o);  // 16 consecutive threads = one (token, block)
        if ((tid & 15) == 0) xsum[b][m][u] = s;
      } else {
        // k = 8 cv = 128 u + 64 h + 16 g + 8 half -> step 2 h + half of lane group g
        const int st = ((cv >> 2) & 2) | (cv & 1);
        *reinterpret_cast<uint4*>(&xs[b][m * XST + ((cv >> 1) & 3) * GS + u * 32 + st * 8]) = v;
      }
    }
    if constexpr (W4) ssc[b][tid >> 1][tid & 1] = sv;
  };

  f32x4_t acc[NT][MT];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[i][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  // the two unpack constants held in VGPRs (opaque to the optimiser): (d & mask) | c is then one v_and_or_b32
  unsigned mask = 0x000F000Fu, one28 = 0x43004300u;
  asm volatile("" : "+v"(mask), "+v"(one28));

  auto compute = [&](const uint4 (&aw)[NT][AV], int b, int nb) {
    const unsigned short* xrow = &xs[b][r * XST + g * GS];
#pragma unroll
    for (int u = 0; u < NBC; ++u) {
      if (u >= nb) continue;
      if constexpr (W4) {
        float off[MT];
#pragma unroll
        for (int t = 0; t < MT; ++t) off[t] = -136.f * xsum[b][16 * t + r][u];
        {
          f32x4_t tt[NT][MT];
#pragma unroll
          for (int ii = 0; ii < NT; ++ii)
#pragma unroll
            for (int t = 0; t < MT; ++t) tt[ii][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int s = 0; s < 4; ++s) {
            bf16x8_t xb[MT];
#pragma unroll
            for (int t = 0; t < MT; ++t) xb[t] = *reinterpret_cast<const bf16x8_t*>(xrow + t * 16 * XST + u * 32 + 8 * s);
#pragma unroll
            for (int ii = 0; ii < NT; ++ii) {
              const uint4 q = aw[ii][u];
              const bf16x8_t af = u4x8_to_bf16x8(s == 0 ? q.x : s == 1 ? q.y : s == 2 ? q.z : q.w, mask, one28);
#pragma unroll
              for (int t = 0; t < MT; ++t) tt[ii][t] = mfma16(af, xb[t], tt[ii][t]);
            }
          }
          // D: lane holds [weight row n0 + 16 i + 4 g + j][token 16 t + r]
#pragma unroll
          for (int ii = 0; ii < NT; ++ii)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const float sc = ssc[b][wave * 16 * NT + 16 * ii + 4 * g + j][u];
#pragma unroll
              for (int t = 0; t < MT; ++t) acc[ii][t][j] += sc * (tt[ii][t][j] + off[t]);
            }
        }
      } else {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          bf16x8_t xb[MT];
#pragma unroll
          for (int t = 0; t < MT; ++t) xb[t] = *reinterpret_cast<const bf16x8_t*>(xrow + t * 16 * XST + u * 32 + 8 * s);
#pragma unroll
          for (int i = 0; i < NT; ++i) {
            const uint4 q = aw[i][2 * u + (s >> 1)];
            const bf16x8_t af = (s & 1) ? fp8x8_to_bf16x8(q.z, q.w) : fp8x8_to_bf16x8(q.x, q.y);
#pragma unroll
            for (int t = 0; t < MT; ++t) acc[i][t] = mfma16(af, xb[t], acc[i][t]);
          }
        }
      }
    }
  };

  load(a[0], 0);
  stage(0);
  lds_sync();
  for (int c = 0; c < nch; c += 2) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int cc = c + p;
      if (cc >= nch) break;
      const bool more = cc + 1 < nch;
      if (more) load(a[p ^ 1], cc + 1);
      __builtin_amdgcn_sched_barrier(0);
      compute(a[p], p, blocks(cc));
      if (more) stage(p ^ 1);
      lds_sync();  // buffer p read by all, buffer p ^ 1 written
    }
  }

#pragma unroll
  for (int i = 0; i < NT; ++i) {
    if (n0 + 16 * i >= N) break;  // wave-uniform: tiles past N
    const int n = n0 + 16 * i + 4 * g;
    float4 sc = make_float4(1.f, 1.f, 1.f, 1.f);
    if constexpr (!W4) sc = *reinterpret_cast<const float4*>(wscale + n);
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      const int m = 16 * t + r;
      if (m >= M) continue;
      f32x4_t v = acc[i][t];
      if constexpr (!W4) {
        v[0] *= sc.x;
        v[1] *= sc.y;
        v[2] *= sc.z;
        v[3] *= sc.w;
      }
      *reinterpret_cast<f32x4_t*>(ws + ((long)blockIdx.y * M + m) * N + n) = v;
    }
  }
}

// waves per workgroup (32 weight rows each).  4: 128 rows, two workgroups per CU; fp8 rows of a chunk
// are then as many bytes as the 64 token rows staged for them.  8: 256 rows, one workgroup per CU,
// for int4 at 33-64 token rows where the projection is wide enough to leave a grid.
int mid_nw(int M, int N, bool int4) { return int4 && M > 32 && N >= 8192 ? 8 : 4; }

template <bool W4, int MT, int NW>
void launch_mid(const at::Tensor& x, const at::Tensor& w, const at::Tensor& w_scale, float* ws, int M, int N, int K,
                int KS) {
  constexpr int WR = 16 * NT * NW;
  const int chunks = (K + KCH - 1) / KCH;
  const int cps = (chunks + KS - 1) / KS;
  LLMCTL_CHECK(KS >= 1 && (long)(KS - 1) * cps < chunks, "decode_gemm_mid: empty split-K slice");
  hipLaunchKernelGGL((decode_gemm_mid_kernel<W4, MT, NW>), dim3((N + WR - 1) / WR, KS), dim3(64 * NW), 0, stream(),
                     bf_ptr(x), static_cast<const unsigned char*>(w.data_ptr()), w_scale.data_ptr<float>(), ws, M, N, K,
                     cps);
}

template <bool W4, int NW>
void launch_mid_mt(const at::Tensor& x, const at::Tensor& w, const at::Tensor& w_scale, float* ws, int M, int N, int K,
                   int KS) {
  switch ((M + 15) / 16) {
    case 2:  // (8-wave workgroups are taken from 33 token rows on: mid_nw)
      if constexpr (NW == 4) launch_mid<W4, 2, NW>(x, w, w_scale, ws, M, N, K, KS);
      break;
    case 3: launch_mid<W4, 3, NW>(x, w, w_scale, ws, M, N, K, KS); break;
    case 4: launch_mid<W4, 4, NW>(x, w, w_scale, ws, M, N, K, KS); break;
    default: LLMCTL_CHECK(false, "decode_gemm_mid: 17 <= M <= 64, got ", M);
  }
}

}  // namespace

// Split-K slices, from the shape only (a captured decode graph stays valid): the fewest that put
// 8 waves (two 4-wave workgroups, or one of 8) on every CU, each at least two chunks deep and at most 8 (the partials
// ws[KS][M][N] are written and read once more per slice).  Normalised so that no slice is empty.
int decode_mid_splits(int M, int N, int K, bool int4) {
  const int chunks = (K + KCH - 1) / KCH;
  int want = (int)knob("decode_mid_splits", 0);
  if (want <= 0) {
    const int nw = mid_nw(M, N, int4), wr = 16 * NT * nw;
    const int nwg = (N + wr - 1) / wr;
    want = std::min({(8 / nw * num_cus() + nwg - 1) / nwg, std::max(1, chunks / 2), 8});
  }
  want = std::max(1, std::min(want, chunks));
  const int cps = (chunks + want - 1) / want;
  return (chunks + cps - 1) / cps;
}

void launch_decode_mid(const at::Tensor& x, const at::Tensor& w, const at::Tensor& w_scale, float* ws, int KS) {
  const int M = x.size(0), K = x.size(1), N = w.size(0);
  const bool int4 = w.scalar_type() == at::kByte;
  if (!int4) launch_mid_mt<false, 4>(x, w, w_scale, ws, M, N, K, KS);
  else if (mid_nw(M, N, true) == 8) launch_mid_mt<true, 8>(x, w, w_scale, ws, M, N, K, KS);
  else launch_mid_mt<true, 4>(x, w, w_scale, ws, M, N, K, KS);
}

}  // namespace llmctl
