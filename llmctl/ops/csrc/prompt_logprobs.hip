// Prompt scoring: per row of a [R, V] block of logits the target token's logprob, its rank and the
// nlp most likely tokens, in one launch (gfx950).
//
// ``logprob_topk_kernel`` (sampling.hip) serves the decode step: a handful of fp32 scratch rows,
// read once for the max, once for the sum and once per listed entry.  Scoring a prompt runs
// thousands of bf16 rows per prefill chunk, so here a row is read from memory ONCE: one 256-thread
// workgroup per row streams it in 16-byte vectors and keeps, per thread,
//   * the online max / sum-exp (rescaled once per vector, not per element),
//   * the count of entries that precede the target in the (value descending, index ascending)
//     order -- the target's own value is one broadcast element load up front,
//   * its nlp best entries, sorted, in registers (static indices only: no scratch).
// The per-thread lists are merged by nlp rounds of a workgroup arg-max over the threads' heads.
// No atomics, no host sync, no allocation; semantics: ``ref.prompt_logprobs``.
#include <type_traits>

#include "common.h"

namespace llmctl {
namespace {

constexpr int kTop = 8;  // width of the top lists (ref.TOP_LOGPROBS)
constexpr int kNone = 0x7fffffff;

template <typename T>
struct RowVec;
template <>
struct RowVec<unsigned short> {
  using type = bf16x8;
  static constexpr int N = 8;
  static __device__ __forceinline__ float at(const type& v, int e) { return bf2f(v[e]); }
  static __device__ __forceinline__ float one(const unsigned short* p, long i) { return bf2f(p[i]); }
};
template <>
struct RowVec<float> {
  using type = f32x4;
  static constexpr int N = 4;
  static __device__ __forceinline__ float at(const type& v, int e) { return v[e]; }
  static __device__ __forceinline__ float one(const float* p, long i) { return p[i]; }
};

// (value, index) a before b in the list order: larger value first, lower index on ties
__device__ __forceinline__ bool before(float av, int ai, float bv, int bi) { return av > bv || (av == bv && ai < bi); }

// What one thread carries through its share of the row.  ``tv`` / ``ti`` hold its n best entries
// ascending: slot 0 is the worst kept one (the threshold a new entry must beat), slot n - 1 the
// best; unused slots hold (-inf, kNone).  A thread meets its entries in ascending index order, so
// a new entry goes before a kept one only with a strictly larger value.
struct RowState {
  float m = -INFINITY, s = 0.f;
  int ahead = 0;
  float tv[kTop];
  int ti[kTop];
};

template <int NE>
__device__ __forceinline__ void take(RowState& st, const float (&x)[NE], int i0, int n, bool valid, float xt, int t) {
  float vm = x[0];
#pragma unroll
  for (int e = 1; e < NE; ++e) vm = fmaxf(vm, x[e]);
  if (vm > st.m) {  // first vector: m = -inf, s = 0 and __expf(-inf) = 0
    st.s *= __expf(st.m - vm);
    st.m = vm;
  }
  float acc = 0.f;
#pragma unroll
  for (int e = 0; e < NE; ++e) acc += __expf(x[e] - st.m);
  st.s += acc;
  if (valid) {
#pragma unroll
    for (int e = 0; e < NE; ++e) st.ahead += before(x[e], i0 + e, xt, t) ? 1 : 0;
  }
  if (n > 0 && vm > st.tv[0]) {
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      if (x[e] > st.tv[0]) {
        st.tv[0] = x[e];
        st.ti[0] = i0 + e;
#pragma unroll
        for (int j = 0; j + 1 < kTop; ++j) {
          if (j + 1 < n && st.tv[j] > st.tv[j + 1]) {
            const float fv = st.tv[j];
            const int fi = st.ti[j];
            st.tv[j] = st.tv[j + 1];
            st.ti[j] = st.ti[j + 1];
            st.tv[j + 1] = fv;
            st.ti[j + 1] = fi;
          }
        }
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void prompt_logprob_kernel(const T* __restrict__ logits,
                                                              const int64_t* __restrict__ target,
                                                              const int* __restrict__ nlp, float* __restrict__ logprob,
                                                              int* __restrict__ rank, int* __restrict__ top_ids,
                                                              float* __restrict__ top_lp, int V) {
  using RV = RowVec<T>;
  using Vec = typename RV::type;
  constexpr int NE = RV::N;
  __shared__ float sm[8];
  __shared__ int smc[4];
  __shared__ float smv[2][4];
  __shared__ int smi[2][4];
  const long row = blockIdx.x;
  const T* lr = logits + row * (long)V;
  const int tid = threadIdx.x;
  const int n = min(max(nlp[row], 0), kTop);
  // the target is range-checked here: no index taken from the input leaves the row
  const int64_t t64 = target[row];
  const bool valid = t64 >= 0 && t64 < (int64_t)V;
  const int t = valid ? (int)t64 : 0;
  const float xt = valid ? RV::one(lr, t) : 0.f;

  RowState st;
#pragma unroll
  for (int j = 0; j < kTop; ++j) {
    st.tv[j] = -INFINITY;
    st.ti[j] = kNone;
  }
  // scalar head up to the first 16-byte boundary, vector body, scalar tail: every row takes the
  // vector loads, whatever V does to its base.  Per thread the indices ascend: head < body < tail.
  const int mis = (int)((reinterpret_cast<uintptr_t>(lr) / sizeof(T)) % NE);
  const int head = min((NE - mis) % NE, V);
  const int nvec = (V - head) / NE;
  const int tail0 = head + nvec * NE;
  if (tid < head) {
    const float x1[1] = {RV::one(lr, tid)};
    take<1>(st, x1, tid, n, valid, xt, t);
  }
  const Vec* lv = reinterpret_cast<const Vec*>(lr + head);
  if (tid < nvec) {
    Vec cur = lv[tid];
    for (int c = tid; c < nvec; c += 256) {
      const int cn = c + 256;
      Vec nxt = cur;
      if (cn < nvec) nxt = lv[cn];  // the next vector is in flight while this one is worked on
      float x[NE];
#pragma unroll
      for (int e = 0; e < NE; ++e) x[e] = RV::at(cur, e);
      take<NE>(st, x, head + c * NE, n, valid, xt, t);
      cur = nxt;
    }
  }
  if (tail0 + tid < V) {  // fewer than NE entries
    const float x1[1] = {RV::one(lr, tail0 + tid)};
    take<1>(st, x1, tail0 + tid, n, valid, xt, t);
  }

  // the row's max, sum-exp and the target's rank
  const int w = tid >> 6, lane = tid & 63;
  float M = wave_max(st.m);
  if (lane == 0) sm[w] = M;
  __syncthreads();
  M = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
  float z = st.s * __expf(st.m - M);  // a thread without entries: 0 * 0
  int ahead = st.ahead;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    z += __shfl_xor(z, o);
    ahead += __shfl_xor(ahead, o);
  }
  if (lane == 0) {
    sm[4 + w] = z;
    smc[w] = ahead;
  }
  __syncthreads();
  z = (sm[4] + sm[5]) + (sm[6] + sm[7]);
  ahead = (smc[0] + smc[1]) + (smc[2] + smc[3]);
  const float lz = logf(z);  // logsumexp = M + lz; a logprob is (x - M) - lz, for the target and the lists alike
  if (tid == 0) {
    logprob[row] = valid ? (xt - M) - lz : __builtin_nanf("");
    rank[row] = valid ? ahead + 1 : 0;
  }

  // the list: round j takes the best head among the threads' lists; its owner moves to its next entry
  int left = n;  // this thread's entries not yet taken are slots 0 .. left - 1
  for (int j = 0; j < kTop; ++j) {
    float bv = -INFINITY;
    int bi = kNone;
    if (j < n) {  // uniform over the workgroup
      float hv = -INFINITY;
      int hi = kNone;
#pragma unroll
      for (int k = 0; k < kTop; ++k) {
        if (k == left - 1) {
          hv = st.tv[k];
          hi = st.ti[k];
        }
      }
      bv = hv;
      bi = hi;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        if (before(ov, oi, bv, bi)) {
          bv = ov;
          bi = oi;
        }
      }
      const int p = j & 1;  // two buffers: one barrier per round
      if (lane == 0) {
        smv[p][w] = bv;
        smi[p][w] = bi;
      }
      __syncthreads();
      bv = smv[p][0];
      bi = smi[p][0];
#pragma unroll
      for (int k = 1; k < 4; ++k) {
        if (before(smv[p][k], smi[p][k], bv, bi)) {
          bv = smv[p][k];
          bi = smi[p][k];
        }
      }
      if (bi != kNone && bi == hi) --left;  // indices are distinct: exactly one owner
    }
    if (tid == 0) {
      const bool ok = bi != kNone;  // fewer than nlp entries in the row: the list ends
      top_ids[row * kTop + j] = ok ? bi : -1;
      top_lp[row * kTop + j] = ok ? (bv - M) - lz : -INFINITY;
    }
  }
}

}  // namespace

std::tuple<at::Tensor, at::Tensor, at::Tensor, at::Tensor> prompt_logprobs(const at::Tensor& logits,
                                                                          const at::Tensor& target,
                                                                          const at::Tensor& nlp) {
  LLMCTL_CHECK(logits.dim() == 2 && logits.is_contiguous(), "logits: contiguous [R, V]");
  LLMCTL_CHECK(logits.size(0) < (1LL << 31) && logits.size(1) >= 1 && logits.size(1) < (1LL << 31),
               "logits: R < 2^31, 1 <= V < 2^31");
  const int R = logits.size(0), V = logits.size(1);
  LLMCTL_CHECK(target.scalar_type() == at::kLong && target.numel() == R && target.is_contiguous() &&
                   target.device() == logits.device(),
               "target: contiguous int64 [R] on the logits' device");
  LLMCTL_CHECK(nlp.scalar_type() == at::kInt && nlp.numel() == R && nlp.is_contiguous() &&
                   nlp.device() == logits.device(),
               "nlp: contiguous int32 [R] on the logits' device");
  const c10::DeviceGuard g(logits.device());
  auto logprob = at::empty({R}, logits.options().dtype(at::kFloat));
  auto rank = at::empty({R}, logits.options().dtype(at::kInt));
  auto top_ids = at::empty({R, kTop}, logits.options().dtype(at::kInt));
  auto top_lp = at::empty({R, kTop}, logits.options().dtype(at::kFloat));
  if (R == 0) return {logprob, rank, top_ids, top_lp};
  if (logits.scalar_type() == at::kBFloat16)
    hipLaunchKernelGGL(prompt_logprob_kernel<unsigned short>, dim3(R), dim3(256), 0, stream(), bf_ptr(logits),
                       target.data_ptr<int64_t>(), nlp.data_ptr<int>(), logprob.data_ptr<float>(),
                       rank.data_ptr<int>(), top_ids.data_ptr<int>(), top_lp.data_ptr<float>(), V);
  else if (logits.scalar_type() == at::kFloat)
    hipLaunchKernelGGL(prompt_logprob_kernel<float>, dim3(R), dim3(256), 0, stream(), logits.data_ptr<float>(),
                       target.data_ptr<int64_t>(), nlp.data_ptr<int>(), logprob.data_ptr<float>(),
                       rank.data_ptr<int>(), top_ids.data_ptr<int>(), top_lp.data_ptr<float>(), V);
  else
    LLMCTL_CHECK(false, "logits must be bf16 or fp32");
  return {logprob, rank, top_ids, top_lp};
}

TORCH_LIBRARY_IMPL(llmctl, CUDA, m) { m.impl("prompt_logprobs", &prompt_logprobs); }

}  // namespace llmctl
