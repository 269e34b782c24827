// Batched token sampling: temperature / top-k / top-p / greedy in one launch (gfx950).
//
// Replaces the reference's per-request Python loop with a host sync per token
// (``server.py:209-235``).  One 256-thread workgroup per sequence row; no sort: the top-k
// and top-p cut-offs are found by bisection on the logit threshold (count / probability
// mass of logits >= T are monotone in T), then an inverse-CDF draw over the kept tokens in
// index order using a caller-provided uniform (so results are reproducible and the whole
// step is hipGraph-capturable: no RNG state, no allocation, no host sync).
#include <type_traits>

#include "common.h"

namespace llmctl {
namespace {

template <typename T>
__device__ __forceinline__ float ld(const T* p, long i);
template <>
__device__ __forceinline__ float ld<unsigned short>(const unsigned short* p, long i) { return bf2f(p[i]); }
template <>
__device__ __forceinline__ float ld<float>(const float* p, long i) { return p[i]; }

__device__ __forceinline__ float bmax(float v, float* sm) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sm[w] = v;
  __syncthreads();
  float r = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
  __syncthreads();
  return r;
}

// kMasked (``sample_guided`` only): the row may hold -inf entries (tokens a guide does not allow).
// They are never kept: the bisections start from the smallest *finite* entry (from -inf every
// midpoint is -inf and top-k / top-p stop cutting), the inverse CDF skips them, and the rounding
// fallback returns the last kept finite entry.  On a row without -inf both instantiations compute
// the same values.
template <typename T, bool kMasked = false>
__global__ __launch_bounds__(256) void sample_kernel(const T* __restrict__ logits, const float* __restrict__ temp,
                                                      const int* __restrict__ topk, const float* __restrict__ topp,
                                                      const float* __restrict__ uni, int64_t* __restrict__ out, int V) {
  __shared__ float sm[8];
  __shared__ float scan[256];
  __shared__ int found;
  const long row = blockIdx.x;
  const T* lr = logits + row * (long)V;
  const int tid = threadIdx.x;
  const float t = temp[row];
  if (t <= 0.f) {  // greedy: argmax, lowest index on ties
    float best = -INFINITY;
    int bi = 0x7fffffff;
    int i0 = 0;
    if constexpr (sizeof(T) == 2) {
      // 16-B vectors (8 logits per lane, 4 loads in flight per unrolled step): a 32k-vocab row
      // is 16 vector steps per thread instead of 125 dependent scalar loads (37 -> a few us)
      if ((V & 7) == 0 && (reinterpret_cast<uintptr_t>(lr) & 15) == 0) {
        const bf16x8* lv = reinterpret_cast<const bf16x8*>(lr);
        const int V8 = V >> 3;
#pragma unroll 4
        for (int c = tid; c < V8; c += 256) {
          const bf16x8 v = lv[c];
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float x = bf2f(v[e]);
            if (x > best) {  // in index order within the thread: strict > keeps the lowest index
              best = x;
              bi = c * 8 + e;
            }
          }
        }
        i0 = V;
      }
    }
    for (int i = i0 + tid; i < V; i += 256) {
      const float x = ld(lr, i);
      if (x > best) {
        best = x;
        bi = i;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ob = __shfl_xor(best, o);
      const int oi = __shfl_xor(bi, o);
      if (ob > best || (ob == best && oi < bi)) {
        best = ob;
        bi = oi;
      }
    }
    __shared__ float wb[4];
    __shared__ int wi[4];
    if ((tid & 63) == 0) {
      wb[tid >> 6] = best;
      wi[tid >> 6] = bi;
    }
    __syncthreads();
    if (tid == 0) {
      float B = wb[0];
      int I = wi[0];
      for (int w = 1; w < 4; ++w)
        if (wb[w] > B || (wb[w] == B && wi[w] < I)) {
          B = wb[w];
          I = wi[w];
        }
      out[row] = I;
    }
    return;
  }
  const float inv_t = 1.f / t;
  // max / min of scaled logits
  float mx = -INFINITY, mn = INFINITY;
  for (int i = tid; i < V; i += 256) {
    const float x = ld(lr, i) * inv_t;
    mx = fmaxf(mx, x);
    if (!kMasked || x > -INFINITY) mn = fminf(mn, x);
  }
  mx = bmax(mx, sm);
  mn = -bmax(-mn, sm);
  float z = 0.f;
  for (int i = tid; i < V; i += 256) z += __expf(ld(lr, i) * inv_t - mx);
  z = block_sum<4>(z, sm);
  float thr = -INFINITY;
  const int k = topk[row];
  if (k > 0 && k < V) {  // largest T with count(x >= T) >= k
    float lo = mn, hi = mx + 1e-6f;
    for (int it = 0; it < 40; ++it) {
      const float mid = 0.5f * (lo + hi);
      float c = 0.f;
      for (int i = tid; i < V; i += 256) c += (ld(lr, i) * inv_t >= mid) ? 1.f : 0.f;
      c = block_sum<4>(c, sm);
      if (c >= (float)k) lo = mid;
      else hi = mid;
    }
    thr = lo;
  }
  const float p = topp[row];
  if (p < 1.f) {  // largest T with mass(x >= T) >= p
    float lo = mn, hi = mx + 1e-6f;
    const float target = p * z;
    for (int it = 0; it < 40; ++it) {
      const float mid = 0.5f * (lo + hi);
      float s = 0.f;
      for (int i = tid; i < V; i += 256) {
        const float x = ld(lr, i) * inv_t;
        if (x >= mid) s += __expf(x - mx);
      }
      s = block_sum<4>(s, sm);
      if (s >= target) lo = mid;
      else hi = mid;
    }
    thr = fmaxf(thr, lo);
  }
  // inverse CDF over kept tokens in index order: contiguous chunk per thread
  const int chunk = (V + 255) / 256;
  const int c0 = tid * chunk, c1 = min(V, c0 + chunk);
  float cs = 0.f;
  for (int i = c0; i < c1; ++i) {
    const float x = ld(lr, i) * inv_t;
    if (x >= thr && (!kMasked || x > -INFINITY)) cs += __expf(x - mx);
  }
  scan[tid] = cs;
  if (tid == 0) found = -1;
  __syncthreads();
  if (tid == 0) {  // exclusive scan (256 elements, serial: negligible vs the passes above)
    float acc = 0.f;
    for (int i = 0; i < 256; ++i) {
      const float v = scan[i];
      scan[i] = acc;
      acc += v;
    }
    sm[4] = acc;
  }
  __syncthreads();
  const float r = uni[row] * sm[4];
  float acc = scan[tid];
  if (acc <= r && acc + cs > r) {
    for (int i = c0; i < c1; ++i) {
      const float x = ld(lr, i) * inv_t;
      if (x >= thr && (!kMasked || x > -INFINITY)) {
        acc += __expf(x - mx);
        if (acc > r) {  // chunks are disjoint and ordered: exactly one thread gets here
          found = i;
          break;
        }
      }
    }
  }
  __syncthreads();
  if (tid == 0) {
    int f = found;
    if (f < 0) {  // r at the very top (rounding): last kept token
      for (int i = V - 1; i >= 0; --i) {
        const float x = ld(lr, i) * inv_t;
        if (x >= thr && (!kMasked || x > -INFINITY)) {
          f = i;
          break;
        }
      }
    }
    out[row] = f < 0 ? 0 : f;
  }
}

// ---- sample_ext: repetition / frequency / presence penalties, logprobs, device-resident state.
//
// Three launches, one 256-thread workgroup per row each: (1) the penalized fp32 row into a
// scratch buffer, (2) sample_kernel<float> on that scratch (so the draw is bit-for-bit what
// ``sample`` gives on the penalized row), (3) log-sum-exp, the chosen token's logprob, the nlp
// largest entries and the count increment.  Per row: state slot s (-1: no state), counts
// int32 [S, V] = occurrences among generated tokens, prompt_mask uint8 [S, V].

constexpr int kTopLp = 8;  // width of the top-logprob outputs

// 4-wide row accesses (a 32k-vocab row is 32 vector steps per thread instead of 125 scalar ones);
// taken when V % 4 == 0 and the row pointers are aligned, else the scalar loop covers the row
using f32x4 = __attribute__((ext_vector_type(4))) float;
using i32x4 = __attribute__((ext_vector_type(4))) int;
using u8x4 = __attribute__((ext_vector_type(4))) unsigned char;
using bf16x4 = __attribute__((ext_vector_type(4))) unsigned short;

__device__ __forceinline__ f32x4 ld4(const unsigned short* p, int c) {
  const bf16x4 v = reinterpret_cast<const bf16x4*>(p)[c];
  return f32x4{bf2f(v[0]), bf2f(v[1]), bf2f(v[2]), bf2f(v[3])};
}
__device__ __forceinline__ f32x4 ld4(const float* p, int c) { return reinterpret_cast<const f32x4*>(p)[c]; }

template <typename P>
__device__ __forceinline__ bool aligned(const P* p, int bytes) {
  return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0;
}

// fixed order, every step rounded on its own (no FMA contraction): repetition over prompt and
// output, then frequency, then presence over the output only
__device__ __forceinline__ float penalized(float x, int c, unsigned char m, float r, float f, float p) {
  if (m || c > 0) x = x > 0.f ? x / r : __fmul_rn(x, r);
  x = __fsub_rn(x, __fmul_rn(f, (float)c));
  return __fsub_rn(x, c > 0 ? p : 0.f);
}

template <typename T>
__global__ __launch_bounds__(256) void penalize_kernel(const T* __restrict__ logits, const int* __restrict__ slot,
                                                        const float* __restrict__ rep, const float* __restrict__ freq,
                                                        const float* __restrict__ pres, const int* __restrict__ counts,
                                                        const unsigned char* __restrict__ pmask,
                                                        float* __restrict__ out, int V, int S) {
  const long row = blockIdx.x;
  const T* lr = logits + row * (long)V;
  float* xr = out + row * (long)V;
  const int s = slot[row];
  const bool vec = (V & 3) == 0 && aligned(lr, 4 * (int)sizeof(T)) && aligned(xr, 16);
  if (s < 0 || s >= S) {  // stateless row: the fp32 image of the logits
    const int V4 = vec ? V >> 2 : 0;
#pragma unroll 4
    for (int c = threadIdx.x; c < V4; c += 256) reinterpret_cast<f32x4*>(xr)[c] = ld4(lr, c);
    for (int i = V4 * 4 + threadIdx.x; i < V; i += 256) xr[i] = ld(lr, i);
    return;
  }
  const int* cr = counts + s * (long)V;
  const unsigned char* mr = pmask + s * (long)V;
  const float r = rep[row], f = freq[row], p = pres[row];
  const int V4 = vec && aligned(cr, 16) && aligned(mr, 4) ? V >> 2 : 0;
#pragma unroll 4
  for (int c = threadIdx.x; c < V4; c += 256) {
    f32x4 x = ld4(lr, c);
    const i32x4 cn = reinterpret_cast<const i32x4*>(cr)[c];
    const u8x4 m = reinterpret_cast<const u8x4*>(mr)[c];
#pragma unroll
    for (int e = 0; e < 4; ++e) x[e] = penalized(x[e], cn[e], m[e], r, f, p);
    reinterpret_cast<f32x4*>(xr)[c] = x;
  }
  for (int i = V4 * 4 + threadIdx.x; i < V; i += 256) xr[i] = penalized(ld(lr, i), cr[i], mr[i], r, f, p);
}

// ---- sample_guided: sample_ext plus a token-class automaton per guided row.
//
// A guide (table slot g) is cls int32 [V] (class of every token), next int32 [S_g, C_g] (-1: not
// allowed) and meta (S_g, C_g); a guided row owns one word of guide_state (index gslot): its
// current automaton state.  The pre-pass writes -inf over the tokens the state does not allow,
// the draw and the logprobs run on that row (kMasked / kGuided instantiations), and the logprob
// kernel's thread 0 advances the state.  Launches of one stream order the state's read (pre-pass)
// and its write (logprob kernel); rows of a launch never share a gslot.

constexpr int kGuideMaxClasses = 8192;  // one state's row of ``next`` in 32 KB of static LDS

struct GuideArgs {
  const int* guide;  // [N] table slot, -1: unguided row
  const int* gslot;  // [N] index into state
  const int* cls;    // [G, V]
  const int* next;   // [G, W], slot g holds next[s * C_g + c]
  const int* meta;   // [G, 2] = (S_g, C_g)
  int* state;        // [Sg]
  int G, W, Sg;
};

// The row's guide, if it has a well-formed one: table slot, state word and the automaton state are
// all range-checked here, so no later index can leave the arena.  Block-uniform.
__device__ __forceinline__ bool guide_of(const GuideArgs& ga, long row, int& g, int& gs, int& st, int& C) {
  g = ga.guide[row];
  if (g < 0 || g >= ga.G) return false;
  gs = ga.gslot[row];
  if (gs < 0 || gs >= ga.Sg) return false;
  const int S = ga.meta[2 * g];
  C = ga.meta[2 * g + 1];
  if (S < 1 || C < 1 || C > kGuideMaxClasses || (long)S * C > (long)ga.W) return false;
  st = ga.state[gs];
  return st >= 0 && st < S;
}

template <typename T>
__global__ __launch_bounds__(256) void penalize_mask_kernel(const T* __restrict__ logits, const int* __restrict__ slot,
                                                             const float* __restrict__ rep,
                                                             const float* __restrict__ freq,
                                                             const float* __restrict__ pres,
                                                             const int* __restrict__ counts,
                                                             const unsigned char* __restrict__ pmask,
                                                             float* __restrict__ out, int V, int S, GuideArgs ga) {
  __shared__ int nx[kGuideMaxClasses];
  const long row = blockIdx.x;
  const T* lr = logits + row * (long)V;
  float* xr = out + row * (long)V;
  int g, gs, st, C = 0;
  const bool guided = guide_of(ga, row, g, gs, st, C);
  const int* cl = nullptr;
  if (guided) {  // this state's row of next into LDS
    const int* nr = ga.next + (long)g * ga.W + (long)st * C;
    for (int j = threadIdx.x; j < C; j += 256) nx[j] = nr[j];
    cl = ga.cls + (long)g * V;
  }
  __syncthreads();
  const int s = slot[row];
  const bool state = s >= 0 && s < S;
  const int* cr = state ? counts + s * (long)V : nullptr;
  const unsigned char* mr = state ? pmask + s * (long)V : nullptr;
  const float r = state ? rep[row] : 1.f, f = state ? freq[row] : 0.f, p = state ? pres[row] : 0.f;
  const bool vec = (V & 3) == 0 && aligned(lr, 4 * (int)sizeof(T)) && aligned(xr, 16) &&
                   (!state || (aligned(cr, 16) && aligned(mr, 4))) && (!guided || aligned(cl, 16));
  const int V4 = vec ? V >> 2 : 0;
  // one branch-free loop per (state, guided) combination; the values of a row with a state are
  // those of penalize_kernel, bit for bit
  auto run = [&](auto st_, auto gd_) {
    constexpr bool kState = decltype(st_)::value, kGuide = decltype(gd_)::value;
#pragma unroll 4
    for (int c = threadIdx.x; c < V4; c += 256) {
      f32x4 x = ld4(lr, c);
      if constexpr (kState) {
        const i32x4 cn = reinterpret_cast<const i32x4*>(cr)[c];
        const u8x4 m = reinterpret_cast<const u8x4*>(mr)[c];
#pragma unroll
        for (int e = 0; e < 4; ++e) x[e] = penalized(x[e], cn[e], m[e], r, f, p);
      }
      if constexpr (kGuide) {
        const i32x4 k = reinterpret_cast<const i32x4*>(cl)[c];
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if ((unsigned)k[e] >= (unsigned)C || nx[k[e]] < 0) x[e] = -INFINITY;
      }
      reinterpret_cast<f32x4*>(xr)[c] = x;
    }
    for (int i = V4 * 4 + threadIdx.x; i < V; i += 256) {
      float x = ld(lr, i);
      if constexpr (kState) x = penalized(x, cr[i], mr[i], r, f, p);
      if constexpr (kGuide) {
        const int k = cl[i];
        if ((unsigned)k >= (unsigned)C || nx[k] < 0) x = -INFINITY;
      }
      xr[i] = x;
    }
  };
  using yes = std::true_type;
  using no = std::false_type;
  if (state) {
    if (guided) run(yes{}, yes{});
    else run(yes{}, no{});
  } else {
    if (guided) run(no{}, yes{});
    else run(no{}, no{});
  }
}

// (value, index) arg-max over the workgroup in the order "larger value first, lower index on
// ties"; an index of INT_MAX means no candidate.  All threads get the result.
__device__ __forceinline__ void bargmax(float& v, int& idx, float* smv, int* smi) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o);
    const int oi = __shfl_xor(idx, o);
    if (oi != 0x7fffffff && (idx == 0x7fffffff || ov > v || (ov == v && oi < idx))) {
      v = ov;
      idx = oi;
    }
  }
  if ((threadIdx.x & 63) == 0) {
    smv[threadIdx.x >> 6] = v;
    smi[threadIdx.x >> 6] = idx;
  }
  __syncthreads();
  v = smv[0];
  idx = smi[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) {
    const float ov = smv[w];
    const int oi = smi[w];
    if (oi != 0x7fffffff && (idx == 0x7fffffff || ov > v || (ov == v && oi < idx))) {
      v = ov;
      idx = oi;
    }
  }
  __syncthreads();
}

// kGuided (``sample_guided`` only): -inf entries (masked tokens) are never listed (the scan is the
// unflagged one; a round whose best entry is -inf ends the list), and thread 0 advances the row's
// automaton state after the count increment.
template <bool kGuided = false>
__global__ __launch_bounds__(256) void logprob_topk_kernel(const float* __restrict__ x, const int64_t* __restrict__ toks,
                                                            const int* __restrict__ slot, const int* __restrict__ nlp,
                                                            int* __restrict__ counts, float* __restrict__ logprob,
                                                            int* __restrict__ top_ids, float* __restrict__ top_lp,
                                                            int V, int S, GuideArgs ga = GuideArgs{}) {
  __shared__ float sm[8];
  __shared__ float smv[4];
  __shared__ int smi[4];
  const long row = blockIdx.x;
  const float* xr = x + row * (long)V;
  const int tid = threadIdx.x;
  const int V4 = (V & 3) == 0 && aligned(xr, 16) ? V >> 2 : 0;  // vector steps; the scalar loops take the rest
  const f32x4* x4 = reinterpret_cast<const f32x4*>(xr);
  float mx = -INFINITY;
#pragma unroll 4
  for (int c = tid; c < V4; c += 256) {
    const f32x4 v = x4[c];
    mx = fmaxf(fmaxf(mx, fmaxf(v[0], v[1])), fmaxf(v[2], v[3]));
  }
  for (int i = V4 * 4 + tid; i < V; i += 256) mx = fmaxf(mx, xr[i]);
  mx = bmax(mx, sm);
  float z = 0.f;
#pragma unroll 4
  for (int c = tid; c < V4; c += 256) {
    const f32x4 v = x4[c];
    z += (__expf(v[0] - mx) + __expf(v[1] - mx)) + (__expf(v[2] - mx) + __expf(v[3] - mx));
  }
  for (int i = V4 * 4 + tid; i < V; i += 256) z += __expf(xr[i] - mx);
  z = block_sum<4>(z, sm);
  const float lz = logf(z);  // logsumexp = mx + lz; x - logsumexp is taken as (x - mx) - lz
  const int tok = (int)toks[row];
  if (tid == 0) logprob[row] = (xr[tok] - mx) - lz;
  // the nlp largest entries by repeated arg-max: round j takes the best entry that comes after
  // round j - 1's pick in (value descending, index ascending) order
  const int n = min(max(nlp[row], 0), kTopLp);
  float pv = INFINITY;
  int pi = -1;
  for (int j = 0; j < kTopLp; ++j) {
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    if (j < n && pi != 0x7fffffff) {  // uniform over the workgroup
      // index order within the thread: strict > keeps the lowest index
      auto take = [&](float v, int i) {
        if ((v < pv || (v == pv && i > pi)) && (bi == 0x7fffffff || v > bv)) {
          bv = v;
          bi = i;
        }
      };
#pragma unroll 4
      for (int c = tid; c < V4; c += 256) {
        const f32x4 v = x4[c];
#pragma unroll
        for (int e = 0; e < 4; ++e) take(v[e], c * 4 + e);
      }
      for (int i = V4 * 4 + tid; i < V; i += 256) take(xr[i], i);
      bargmax(bv, bi, smv, smi);
      // the best entry left is masked: so is every other one, and the list ends here
      if (kGuided && bv == -INFINITY) bi = 0x7fffffff;
    }
    if (tid == 0) {
      const bool ok = bi != 0x7fffffff;
      top_ids[row * kTopLp + j] = ok ? bi : -1;
      top_lp[row * kTopLp + j] = ok ? (bv - mx) - lz : -INFINITY;
    }
    pv = bv;
    pi = bi;
  }
  const int s = slot[row];
  if (tid == 0 && s >= 0 && s < S) {  // after everything above; rows of a launch never share a slot
    int* c = counts + s * (long)V + tok;
    *c = *c + 1;
  }
  if constexpr (kGuided) {
    int g, gs, st, C;
    if (tid == 0 && tok >= 0 && tok < V && guide_of(ga, row, g, gs, st, C)) {
      const int c = ga.cls[(long)g * V + tok];
      const int nxt = (unsigned)c < (unsigned)C ? ga.next[(long)g * ga.W + (long)st * C + c] : -1;
      if (nxt >= 0) ga.state[gs] = nxt;  // a negative result cannot happen with a well-formed guide
    }
  }
}

}  // namespace

at::Tensor sample(const at::Tensor& logits, const at::Tensor& temperature, const at::Tensor& top_k,
                  const at::Tensor& top_p, const at::Tensor& uniform) {
  LLMCTL_CHECK(logits.dim() == 2 && logits.is_contiguous(), "logits: contiguous [N, V]");
  const int N = logits.size(0), V = logits.size(1);
  LLMCTL_CHECK(temperature.scalar_type() == at::kFloat && top_p.scalar_type() == at::kFloat &&
                   uniform.scalar_type() == at::kFloat && top_k.scalar_type() == at::kInt,
               "temperature/top_p/uniform fp32, top_k int32");
  LLMCTL_CHECK(temperature.numel() == N && top_k.numel() == N && top_p.numel() == N && uniform.numel() == N,
               "per-row parameter tensors must have N elements");
  const c10::DeviceGuard g(logits.device());
  auto out = at::empty({N}, logits.options().dtype(at::kLong));
  if (N == 0) return out;
  if (logits.scalar_type() == at::kBFloat16)
    hipLaunchKernelGGL(sample_kernel<unsigned short>, dim3(N), dim3(256), 0, stream(), bf_ptr(logits),
                       temperature.data_ptr<float>(), top_k.data_ptr<int>(), top_p.data_ptr<float>(),
                       uniform.data_ptr<float>(), out.data_ptr<int64_t>(), V);
  else if (logits.scalar_type() == at::kFloat)
    hipLaunchKernelGGL(sample_kernel<float>, dim3(N), dim3(256), 0, stream(), logits.data_ptr<float>(),
                       temperature.data_ptr<float>(), top_k.data_ptr<int>(), top_p.data_ptr<float>(),
                       uniform.data_ptr<float>(), out.data_ptr<int64_t>(), V);
  else
    LLMCTL_CHECK(false, "logits must be bf16 or fp32");
  return out;
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> sample_ext(
    const at::Tensor& logits, const at::Tensor& temperature, const at::Tensor& top_k, const at::Tensor& top_p,
    const at::Tensor& uniform, const at::Tensor& slot, const at::Tensor& rep, const at::Tensor& freq,
    const at::Tensor& pres, const at::Tensor& nlp, at::Tensor& counts, const at::Tensor& prompt_mask) {
  LLMCTL_CHECK(logits.dim() == 2 && logits.is_contiguous(), "logits: contiguous [N, V]");
  const int N = logits.size(0), V = logits.size(1);
  LLMCTL_CHECK(V >= 1, "logits: V >= 1");
  LLMCTL_CHECK(temperature.scalar_type() == at::kFloat && top_p.scalar_type() == at::kFloat &&
                   uniform.scalar_type() == at::kFloat && top_k.scalar_type() == at::kInt,
               "temperature/top_p/uniform fp32, top_k int32");
  LLMCTL_CHECK(rep.scalar_type() == at::kFloat && freq.scalar_type() == at::kFloat &&
                   pres.scalar_type() == at::kFloat && slot.scalar_type() == at::kInt && nlp.scalar_type() == at::kInt,
               "rep/freq/pres fp32, slot/nlp int32");
  for (const at::Tensor* t : {&temperature, &top_k, &top_p, &uniform, &slot, &rep, &freq, &pres, &nlp})
    LLMCTL_CHECK(t->numel() == N && t->is_contiguous() && t->device() == logits.device(),
                 "per-row parameter tensors must have N elements on the logits' device");
  LLMCTL_CHECK(counts.dim() == 2 && counts.size(1) == V && counts.scalar_type() == at::kInt && counts.is_contiguous() &&
                   counts.device() == logits.device(),
               "counts: contiguous int32 [S, V] on the logits' device");
  LLMCTL_CHECK(prompt_mask.dim() == 2 && prompt_mask.size(0) == counts.size(0) && prompt_mask.size(1) == V &&
                   prompt_mask.scalar_type() == at::kByte && prompt_mask.is_contiguous() &&
                   prompt_mask.device() == logits.device(),
               "prompt_mask: contiguous uint8 [S, V] on the logits' device");
  const int S = counts.size(0);
  const c10::DeviceGuard g(logits.device());
  auto toks = at::empty({N}, logits.options().dtype(at::kLong));
  auto logprob = at::empty({N}, logits.options().dtype(at::kFloat));
  auto top_ids = at::empty({N, kTopLp}, logits.options().dtype(at::kInt));
  auto top_lp = at::empty({N, kTopLp}, logits.options().dtype(at::kFloat));
  if (N == 0) return {toks, logprob, top_ids, top_lp};
  auto x = at::empty({N, V}, logits.options().dtype(at::kFloat));  // the penalized rows
  const hipStream_t st = stream();
  if (logits.scalar_type() == at::kBFloat16)
    hipLaunchKernelGGL(penalize_kernel<unsigned short>, dim3(N), dim3(256), 0, st, bf_ptr(logits),
                       slot.data_ptr<int>(), rep.data_ptr<float>(), freq.data_ptr<float>(), pres.data_ptr<float>(),
                       counts.data_ptr<int>(), prompt_mask.data_ptr<unsigned char>(), x.data_ptr<float>(), V, S);
  else if (logits.scalar_type() == at::kFloat)
    hipLaunchKernelGGL(penalize_kernel<float>, dim3(N), dim3(256), 0, st, logits.data_ptr<float>(),
                       slot.data_ptr<int>(), rep.data_ptr<float>(), freq.data_ptr<float>(), pres.data_ptr<float>(),
                       counts.data_ptr<int>(), prompt_mask.data_ptr<unsigned char>(), x.data_ptr<float>(), V, S);
  else
    LLMCTL_CHECK(false, "logits must be bf16 or fp32");
  hipLaunchKernelGGL(sample_kernel<float>, dim3(N), dim3(256), 0, st, x.data_ptr<float>(),
                     temperature.data_ptr<float>(), top_k.data_ptr<int>(), top_p.data_ptr<float>(),
                     uniform.data_ptr<float>(), toks.data_ptr<int64_t>(), V);
  hipLaunchKernelGGL(logprob_topk_kernel<false>, dim3(N), dim3(256), 0, st, x.data_ptr<float>(), toks.data_ptr<int64_t>(),
                     slot.data_ptr<int>(), nlp.data_ptr<int>(), counts.data_ptr<int>(), logprob.data_ptr<float>(),
                     top_ids.data_ptr<int>(), top_lp.data_ptr<float>(), V, S, GuideArgs{});
  return {toks, logprob, top_ids, top_lp};
}

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> sample_guided(
    const at::Tensor& logits, const at::Tensor& temperature, const at::Tensor& top_k, const at::Tensor& top_p,
    const at::Tensor& uniform, const at::Tensor& slot, const at::Tensor& rep, const at::Tensor& freq,
    const at::Tensor& pres, const at::Tensor& nlp, at::Tensor& counts, const at::Tensor& prompt_mask,
    const at::Tensor& guide, const at::Tensor& gslot, const at::Tensor& guide_cls, const at::Tensor& guide_next,
    const at::Tensor& guide_meta, at::Tensor& guide_state) {
  LLMCTL_CHECK(logits.dim() == 2 && logits.is_contiguous(), "logits: contiguous [N, V]");
  const int N = logits.size(0), V = logits.size(1);
  LLMCTL_CHECK(V >= 1, "logits: V >= 1");
  LLMCTL_CHECK(temperature.scalar_type() == at::kFloat && top_p.scalar_type() == at::kFloat &&
                   uniform.scalar_type() == at::kFloat && top_k.scalar_type() == at::kInt,
               "temperature/top_p/uniform fp32, top_k int32");
  LLMCTL_CHECK(rep.scalar_type() == at::kFloat && freq.scalar_type() == at::kFloat &&
                   pres.scalar_type() == at::kFloat && slot.scalar_type() == at::kInt && nlp.scalar_type() == at::kInt &&
                   guide.scalar_type() == at::kInt && gslot.scalar_type() == at::kInt,
               "rep/freq/pres fp32, slot/nlp/guide/gslot int32");
  for (const at::Tensor* t : {&temperature, &top_k, &top_p, &uniform, &slot, &rep, &freq, &pres, &nlp, &guide, &gslot})
    LLMCTL_CHECK(t->numel() == N && t->is_contiguous() && t->device() == logits.device(),
                 "per-row parameter tensors must have N elements on the logits' device");
  LLMCTL_CHECK(counts.dim() == 2 && counts.size(1) == V && counts.scalar_type() == at::kInt && counts.is_contiguous() &&
                   counts.device() == logits.device(),
               "counts: contiguous int32 [S, V] on the logits' device");
  LLMCTL_CHECK(prompt_mask.dim() == 2 && prompt_mask.size(0) == counts.size(0) && prompt_mask.size(1) == V &&
                   prompt_mask.scalar_type() == at::kByte && prompt_mask.is_contiguous() &&
                   prompt_mask.device() == logits.device(),
               "prompt_mask: contiguous uint8 [S, V] on the logits' device");
  for (const at::Tensor* t : {&guide_cls, &guide_next, &guide_meta, static_cast<const at::Tensor*>(&guide_state)})
    LLMCTL_CHECK(t->scalar_type() == at::kInt && t->is_contiguous() && t->device() == logits.device(),
                 "guide_cls/guide_next/guide_meta/guide_state: contiguous int32 on the logits' device");
  LLMCTL_CHECK(guide_cls.dim() == 2 && guide_cls.size(1) == V, "guide_cls: [G, V]");
  const int G = guide_cls.size(0);
  LLMCTL_CHECK(guide_next.dim() == 2 && guide_next.size(0) == G && guide_next.size(1) < (1LL << 31), "guide_next: [G, W]");
  LLMCTL_CHECK(guide_meta.dim() == 2 && guide_meta.size(0) == G && guide_meta.size(1) == 2, "guide_meta: [G, 2]");
  LLMCTL_CHECK(guide_state.dim() == 1 && guide_state.size(0) < (1LL << 31), "guide_state: [Sg]");
  const int S = counts.size(0);
  const c10::DeviceGuard g(logits.device());
  auto toks = at::empty({N}, logits.options().dtype(at::kLong));
  auto logprob = at::empty({N}, logits.options().dtype(at::kFloat));
  auto top_ids = at::empty({N, kTopLp}, logits.options().dtype(at::kInt));
  auto top_lp = at::empty({N, kTopLp}, logits.options().dtype(at::kFloat));
  if (N == 0) return {toks, logprob, top_ids, top_lp};
  auto x = at::empty({N, V}, logits.options().dtype(at::kFloat));  // the penalized and masked rows
  const GuideArgs ga{guide.data_ptr<int>(),      gslot.data_ptr<int>(),      guide_cls.data_ptr<int>(),
                     guide_next.data_ptr<int>(), guide_meta.data_ptr<int>(), guide_state.data_ptr<int>(),
                     G,                          (int)guide_next.size(1),    (int)guide_state.size(0)};
  const hipStream_t st = stream();
  if (logits.scalar_type() == at::kBFloat16)
    hipLaunchKernelGGL(penalize_mask_kernel<unsigned short>, dim3(N), dim3(256), 0, st, bf_ptr(logits),
                       slot.data_ptr<int>(), rep.data_ptr<float>(), freq.data_ptr<float>(), pres.data_ptr<float>(),
                       counts.data_ptr<int>(), prompt_mask.data_ptr<unsigned char>(), x.data_ptr<float>(), V, S, ga);
  else if (logits.scalar_type() == at::kFloat)
    hipLaunchKernelGGL(penalize_mask_kernel<float>, dim3(N), dim3(256), 0, st, logits.data_ptr<float>(),
                       slot.data_ptr<int>(), rep.data_ptr<float>(), freq.data_ptr<float>(), pres.data_ptr<float>(),
                       counts.data_ptr<int>(), prompt_mask.data_ptr<unsigned char>(), x.data_ptr<float>(), V, S, ga);
  else
    LLMCTL_CHECK(false, "logits must be bf16 or fp32");
  hipLaunchKernelGGL((sample_kernel<float, true>), dim3(N), dim3(256), 0, st, x.data_ptr<float>(),
                     temperature.data_ptr<float>(), top_k.data_ptr<int>(), top_p.data_ptr<float>(),
                     uniform.data_ptr<float>(), toks.data_ptr<int64_t>(), V);
  hipLaunchKernelGGL(logprob_topk_kernel<true>, dim3(N), dim3(256), 0, st, x.data_ptr<float>(),
                     toks.data_ptr<int64_t>(), slot.data_ptr<int>(), nlp.data_ptr<int>(), counts.data_ptr<int>(),
                     logprob.data_ptr<float>(), top_ids.data_ptr<int>(), top_lp.data_ptr<float>(), V, S, ga);
  return {toks, logprob, top_ids, top_lp};
}

TORCH_LIBRARY_IMPL(llmctl, CUDA, m) {
  m.impl("sample", &sample);
  m.impl("sample_ext", &sample_ext);
  m.impl("sample_guided", &sample_guided);
}

}  // namespace llmctl
