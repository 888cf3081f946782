// Top-p (nucleus) sampling on the device, without a sort (ClipCap head: P/src/clipcap/entrypoint.py:198-311, generate_batched).
//
// One workgroup of 1024 threads per row of scores s[0..V).  With d_i = s_i - max s, T = temperature (<= 0: 1) and w_i = exp(d_i / T)
// (softmax numerators; fp32), the reference sorts the probabilities descending, keeps sorted position 0 and every position whose
// cumulative probability BEFORE it is <= top_p (the shifted mask, :256-258), renormalises over the kept set (the clamp and second
// softmax, :265-267) and draws one token.  Restated without the sort: with S(t) = sum of w_i over s_i > t and Z = sum of all w_i, token i
// is kept iff S(s_i) <= top_p Z.  S is non-increasing, so the kept set is {s_i >= t*} with t* the smallest value whose S(t*) <= top_p Z,
// and the row maximum (S = 0) is always in it.  t* is found by bisection over the order-preserving unsigned image of the fp32 scores:
// at most 32 rounds, each ONE masked reduction over the workgroup.  Tokens whose score EQUALS t* are all kept (the reference's unstable
// sort keeps an arbitrary subset of a tie at the edge).
//
// The draw: u in [0, 1), target = u x (kept mass).  The sampled token is the smallest id v whose kept mass over ids <= v exceeds the
// target; prefix(v) is the same masked reduction (mask: kept and id <= v), monotone in v because every node of a fixed summation tree
// over non-negative terms is, so v is found by bisection over the id, ceil(log2 V) rounds.  If rounding leaves no such id (u x Z == Z),
// the last kept id.
//
// One reduction shape serves every sum: a thread's values (id = tid + 1024 j) as a balanced tree, wave_sum's butterfly, the 16 wave
// partials as a balanced tree read by every thread.  It depends on (V, block shape) alone, so a row gives the same token wherever it
// sits in a launch, and its depth is 6 + 6 + 4 = 16 roundings whatever V <= 51 200 (the bound the tests' delta is derived from).
// V <= 51 200 (GPT-2: 50 257): keys and numerators live in registers, 50 + 50 per lane, one read of the row; above: the same code
// re-reads the row (L2) and recomputes exp in every round -- correct, not fast.
//
// Stop handling: an inactive row emits stop_id and stays inactive; an active row that draws stop_id turns inactive; a row with any
// NaN emits stop_id (:269-273), and so does a row with +-inf (out of contract: no fault, no garbage).
#include "common.h"
#include "kernels.h"

#include <type_traits>

namespace pio {

static constexpr int NS_T = 1024;        // threads per row
static constexpr int NS_VPT = 50;        // values per thread held in registers: V <= 51 200

// order-preserving image of a float: a < b (as floats, no NaN) <=> okey(a) < okey(b)
__device__ __forceinline__ uint32_t okey(float x) {
  const uint32_t b = __float_as_uint(x);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float okey_inv(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }
static constexpr uint32_t NS_KEY_MIN = 0x00800000u;     // okey(-FLT_MAX): every finite score's key is >= this, okey(-inf) (padding) is below

// balanced tree over f(LO) .. f(LO + N - 1), evaluated depth first (few live temporaries)
template <int LO, int N, class F> __device__ __forceinline__ float tree_sum(F&& f) {
  if constexpr (N == 1) return f(std::integral_constant<int, LO>{});
  else return tree_sum<LO, N / 2>(f) + tree_sum<LO + N / 2, N - N / 2>(f);
}

// sum over the workgroup of the threads' values, the same bits in every thread; red: [2][16] floats, `phase` alternates per call
__device__ __forceinline__ float block_sum(float v, float* red, int& phase) {
  v = wave_sum(v);
  float* r = red + 16 * phase;
  if ((threadIdx.x & 63) == 0) r[threadIdx.x >> 6] = v;
  __syncthreads();
  phase ^= 1;
  return (((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))) +
         (((r[8] + r[9]) + (r[10] + r[11])) + ((r[12] + r[13]) + (r[14] + r[15])));
}
__device__ __forceinline__ int block_sum_int(int v, int* red, int& phase) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  int* r = red + 16 * phase;
  if ((threadIdx.x & 63) == 0) r[threadIdx.x >> 6] = v;
  __syncthreads();
  phase ^= 1;
  int t = 0;
  for (int i = 0; i < 16; ++i) t += r[i];
  return t;
}
__device__ __forceinline__ int block_max_int(int v, int* red, int& phase) {
  for (int o = 32; o > 0; o >>= 1) { const int ov = __shfl_xor(v, o); v = ov > v ? ov : v; }
  int* r = red + 16 * phase;
  if ((threadIdx.x & 63) == 0) r[threadIdx.x >> 6] = v;
  __syncthreads();
  phase ^= 1;
  int t = r[0];
  for (int i = 1; i < 16; ++i) t = r[i] > t ? r[i] : t;
  return t;
}

// REG: V <= NS_T * NS_VPT, the row in registers; otherwise re-read per reduction (vpt = ceil(V / 1024) at run time)
template <bool REG>
__global__ __launch_bounds__(NS_T) void k_nucleus_sample(SampleArgs a) {
  __shared__ float s_redf[32];
  __shared__ int s_redi[32];
  const int n = blockIdx.x, tid = threadIdx.x, V = a.V;
  const float* row = a.scores + (size_t)n * a.ld;
  const int vpt = REG ? NS_VPT : (V + NS_T - 1) / NS_T;
  int pf = 0, pi = 0;

  // ---- pass 1: maximum, NaN / inf flag
  uint32_t key[REG ? NS_VPT : 1];      // REG: the row as keys (ids past V: -inf, below every finite key and of zero mass)
  float m = -INFINITY;
  int bad = 0;
  if constexpr (REG) {
#pragma unroll
    for (int j = 0; j < NS_VPT; ++j) {
      const int id = tid + NS_T * j;
      const float x = id < V ? row[id] : -INFINITY;
      bad |= id < V && (__float_as_uint(x) & 0x7F800000u) == 0x7F800000u;
      m = fmaxf(m, x);
      key[j] = okey(x);
    }
  } else {
    for (int j = 0; j < vpt; ++j) {
      const int id = tid + NS_T * j;
      const float x = id < V ? row[id] : -INFINITY;
      bad |= id < V && (__float_as_uint(x) & 0x7F800000u) == 0x7F800000u;
      m = fmaxf(m, x);
    }
  }
  bad = __syncthreads_or(bad);
  const int was_active = a.active[n];
  if (bad || !was_active) {                  // uniform over the workgroup
    if (tid == 0) {
      a.tokens[(size_t)n * a.tok_stride] = a.stop_id;
      a.active[n] = 0;
      if (a.kept) a.kept[n] = 0;
    }
    return;
  }
  m = wave_max(m);
  if ((tid & 63) == 0) s_redf[tid >> 6] = m;
  __syncthreads();
  m = s_redf[0];
  for (int i = 1; i < 16; ++i) m = fmaxf(m, s_redf[i]);
  __syncthreads();
  const float T = a.temperature > 0.f ? a.temperature : 1.0f;
  const uint32_t kmax = okey(m);

  // ---- keys and softmax numerators
  float w[REG ? NS_VPT : 1];
  if constexpr (REG) {
#pragma unroll
    for (int j = 0; j < NS_VPT; ++j) w[j] = expf((okey_inv(key[j]) - m) / T);
  }
  // sum of the numerators under a predicate pred(key, id); the same tree whatever the predicate
  auto msum = [&](auto pred) -> float {
    float v;
    if constexpr (REG) {
      v = tree_sum<0, NS_VPT>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        return pred(key[j], tid + NS_T * j) ? w[j] : 0.f;
      });
    } else {
      v = 0.f;                                   // one chain per thread: this path's depth grows with V (see the header)
      for (int j = 0; j < vpt; ++j) {
        const int id = tid + NS_T * j;
        if (id < V) {
          const float x = row[id];
          if (pred(okey(x), id)) v += expf((x - m) / T);
        }
      }
    }
    return block_sum(v, s_redf, pf);
  };

  const float Z = msum([](uint32_t, int) { return true; });
  const float thr = a.top_p * Z;
  // ---- t*: the smallest key with S(key) <= thr, S(kmax) = 0
  uint32_t lo = NS_KEY_MIN, hi = kmax;
  if (!(thr >= 0.f)) lo = kmax;                  // top_p < 0 (or NaN): the maximum alone, as the reference keeps position 0
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    const float S = msum([mid](uint32_t k, int) { return k > mid; });
    if (S <= thr) hi = mid; else lo = mid + 1u;
  }
  const uint32_t tstar = hi;
  // ---- kept set: size, mass, last id
  int cnt = 0, last = -1;
  if constexpr (REG) {
#pragma unroll
    for (int j = 0; j < NS_VPT; ++j) {
      const bool kp = key[j] >= tstar;           // tstar >= NS_KEY_MIN: the padding is never kept
      cnt += kp;
      last = kp ? tid + NS_T * j : last;         // ids ascend with j
    }
  } else {
    for (int j = 0; j < vpt; ++j) {
      const int id = tid + NS_T * j;
      const bool kp = id < V && okey(row[id]) >= tstar;
      cnt += kp;
      last = kp ? id : last;
    }
  }
  cnt = block_sum_int(cnt, s_redi, pi);
  last = block_max_int(last, s_redi, pi);
  const float Zk = msum([tstar](uint32_t k, int) { return k >= tstar; });
  const float target = a.uniforms[(size_t)n * a.u_stride] * Zk;
  // ---- the draw: the smallest id v with prefix(v) > target
  int token = last;
  if (Zk > target) {                             // prefix(V - 1) = Zk: an answer exists
    int vlo = 0, vhi = V - 1;
    while (vlo < vhi) {
      const int mid = vlo + ((vhi - vlo) >> 1);
      const float P = msum([tstar, mid](uint32_t k, int id) { return k >= tstar && id <= mid; });
      if (P > target) vhi = mid; else vlo = mid + 1;
    }
    token = vhi;
  }
  if (tid == 0) {
    a.tokens[(size_t)n * a.tok_stride] = token;
    a.active[n] = token == a.stop_id ? 0 : 1;
    if (a.kept) a.kept[n] = cnt;
  }
}

hipError_t launch_nucleus_sample(const SampleArgs& a, hipStream_t s) {
  if (a.N < 1 || a.V < 1 || a.ld < a.V || !a.scores || !a.uniforms || !a.active || !a.tokens) return hipErrorInvalidValue;
  if (a.V <= NS_T * NS_VPT) hipLaunchKernelGGL(k_nucleus_sample<true>, dim3(a.N), dim3(NS_T), 0, s, a);
  else hipLaunchKernelGGL(k_nucleus_sample<false>, dim3(a.N), dim3(NS_T), 0, s, a);
  return hipGetLastError();
}

// u[n][k] = philox_uniform(seed, n, k) (common.h)
__global__ __launch_bounds__(256) void k_philox_uniforms(uint64_t seed, int N, int steps, float* u) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N * steps) return;
  const int n = i / steps, k = i - n * steps;
  u[i] = philox_uniform(seed, (uint32_t)n, (uint32_t)k);
}
hipError_t launch_philox_uniforms(uint64_t seed, int N, int steps, float* u, hipStream_t s) {
  if (N < 1 || steps < 1 || !u) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_philox_uniforms, dim3(ceil_div(N * steps, 256)), dim3(256), 0, s, seed, N, steps, u);
  return hipGetLastError();
}

// every row active before the first step
__global__ __launch_bounds__(256) void k_sample_init(int N, int32_t* active) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < N) active[i] = 1;
}
// lens[n] = index of the first stop token + 1, or steps
__global__ __launch_bounds__(64) void k_sample_lens(const int32_t* __restrict__ ids, int steps, int stop_id, int32_t* lens) {
  const int n = blockIdx.x;
  int first = steps;
  for (int k = threadIdx.x; k < steps; k += 64)
    if (ids[(size_t)n * steps + k] == stop_id) { first = k + 1; break; }
  for (int o = 32; o > 0; o >>= 1) { const int ov = __shfl_xor(first, o); first = ov < first ? ov : first; }
  if (threadIdx.x == 0) lens[n] = first;
}
hipError_t launch_sample_init(int N, int32_t* active, hipStream_t s) {
  hipLaunchKernelGGL(k_sample_init, dim3(ceil_div(N, 256)), dim3(256), 0, s, N, active);
  return hipGetLastError();
}
hipError_t launch_sample_lens(const int32_t* ids, int N, int steps, int stop_id, int32_t* lens, hipStream_t s) {
  hipLaunchKernelGGL(k_sample_lens, dim3(N), dim3(64), 0, s, ids, steps, stop_id, lens);
  return hipGetLastError();
}

}  // namespace pio
