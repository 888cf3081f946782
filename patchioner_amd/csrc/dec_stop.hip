// stop_at_eos ("Stopping a greedy decode at the end of every caption"): the bookkeeping of a greedy decode that runs in segments
// of a few steps and ends once every row has emitted a stop id.  The reference cuts every caption at its first end marker on the host
// (P/src/decap/decap.py:173; P/src/viecap/search.py:172-190), so what a row decodes after that column is never read.
//
//   k_dec_stop_scan  after the segment that wrote id columns [s0, s1): first[n] = the first column of row n that holds a stop id (`steps`:
//                    none so far), *live = rows with none.  It reads columns [s0, s1) ONLY: columns >= s1 of the id table still hold what an
//                    earlier decode on the handle left there.  A first stop before s0 is kept; at s0 == 0 whatever first[] held is ignored,
//                    so a decode needs no reset launch.
//   k_dec_stop_pad   out = canon(ids): columns after a row's first stop repeat the stop id, rows without one are copied.  It reads row n
//                    only up to first[n] (all columns of a row without a stop, which the decode then has run to the end).
//
// Both are bookkeeping of <= 256 rows x <= 64 columns: one workgroup walks the rows (scan: the live count is one block reduction, no atomics,
// nothing to zero between launches), a grid-stride loop the table (pad).
#include "common.h"
#include "kernels.h"

namespace pio {

__global__ __launch_bounds__(256) void k_dec_stop_scan(const int32_t* __restrict__ ids, int N, int steps, int s0, int s1, int stop0, int stop1,
                                                       int32_t* first, int32_t* live) {
  __shared__ int s_cnt[4];
  const int tid = threadIdx.x;
  int alive = 0;
  for (int n = tid; n < N; n += 256) {
    int f = first[n];
    if (s0 <= 0 || f < 0 || f >= s0) {                     // no stop before this segment
      f = steps;
      const int32_t* row = ids + (size_t)n * steps;
      for (int j = s0; j < s1; ++j) {
        const int32_t id = row[j];
        if (id == stop0 || id == stop1) { f = j; break; }
      }
      first[n] = f;
    }
    alive += f >= steps ? 1 : 0;
  }
  for (int o = 32; o > 0; o >>= 1) alive += __shfl_xor(alive, o);
  if ((tid & 63) == 0) s_cnt[tid >> 6] = alive;
  __syncthreads();
  if (tid == 0) *live = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
}

__global__ __launch_bounds__(256) void k_dec_stop_pad(const int32_t* __restrict__ ids, const int32_t* __restrict__ first, int N, int steps,
                                                      int32_t* __restrict__ out) {
  const int total = N * steps;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int n = i / steps, j = i - n * steps;
    const int f = first[n];
    out[i] = (f >= 0 && f < j) ? ids[(size_t)n * steps + f] : ids[i];
  }
}

hipError_t launch_dec_stop_scan(const int32_t* ids, int N, int steps, int s0, int s1, int stop0, int stop1, int32_t* first, int32_t* live,
                                hipStream_t s) {
  if (!ids || !first || !live || N < 1 || N > DEC_MAX_PREFIXES || steps < 1 || steps > 64 || s0 < 0 || s1 <= s0 || s1 > steps)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_dec_stop_scan, dim3(1), dim3(256), 0, s, ids, N, steps, s0, s1, stop0, stop1, first, live);
  return hipGetLastError();
}

hipError_t launch_dec_stop_pad(const int32_t* ids, const int32_t* first, int N, int steps, int32_t* out, hipStream_t s) {
  if (!ids || !first || !out || ids == out || N < 1 || N > DEC_MAX_PREFIXES || steps < 1 || steps > 64) return hipErrorInvalidValue;
  const int blocks = ceil_div(N * steps, 256);
  hipLaunchKernelGGL(k_dec_stop_pad, dim3(blocks < 64 ? blocks : 64), dim3(256), 0, s, ids, first, N, steps, out);
  return hipGetLastError();
}

}  // namespace pio
