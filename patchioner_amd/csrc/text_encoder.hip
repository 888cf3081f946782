// The OpenAI-CLIP text transformer (clip.model.CLIP.encode_text, reached from the memory-bank build
// P/src/decap/im2txtprojection/im2txtprojection.py:511-524, 650-657 and the online_texts path :491-493) on gfx950.
//
// The tower is pre-LN (eps 1e-5), causal, QuickGELU, 12 layers of width 512 (8 heads) or 768 (12 heads), head dim 64,
// context 77, vocabulary 49 408; the feature of a caption is ln_final(x[EOT]) @ text_projection, EOT = the first arg-max of
// the id row.  The dense layers are the ViT's GEMMs (launch_vit_gemm: EPI_QKV, EPI_RESIDUAL with nothing to fold, EPI_GELU
// with act = 1) and LayerNorm (launch_layernorm); this file holds what the text side adds:
//   * k_text_embed      x[s Tp + t] = token_embedding[id] + positional_embedding[t] (fp32), rows t >= L zero, bad ids flagged;
//   * k_text_attention  causal attention on MFMA, one workgroup per (caption, head), all of K and V^T in LDS;
//   * k_text_attention_f32  the same rule in plain fp32 (the parity mode, in the style of vit_fp32.hip);
//   * k_text_pool       EOT gather, ln_final on the gathered row only, @ text_projection in fp32.
//
// Layout: caption s occupies rows [s Tp, s Tp + Tp) of the residual stream, Tp = round_up(L, 8) for a launch of ids [N][L].
//
// Invariance.  A caption's feature has the same bits whatever launch holds it (alone / among others; padded to 77 or to
// the longest caption of its bucket).  The GEMMs and LayerNorm already give a row the same bits wherever it sits
// (kernels.h, EPI_RESIDUAL; Tp % 8 == 0).  Attention: query q of wave w (q in [32 w, 32 w + 32)) visits the key tiles
// 0 .. w of 32 keys in ascending order, with keys above the query masked on the diagonal tile only; that sequence depends on q
// alone, never on Tp, Tk or N.  Rows after EOT (padding ids, zero rows up to Tp) are keys only of later queries, so they
// never reach the EOT row.  K rows and V^T columns >= Tp are zero in LDS, so stale workspace bytes never enter a product.
#include "common.h"
#include "kernels.h"

namespace pio {

__global__ __launch_bounds__(128) void k_text_embed(const int32_t* __restrict__ ids, int L, int Tp, int V, int W,
                                                    const float* __restrict__ tok, const float* __restrict__ pos, float* x,
                                                    int32_t* err) {
  const int r = blockIdx.x, s = r / Tp, t = r - s * Tp;
  float* dst = x + (size_t)r * W;
  int id = -1;
  if (t < L) {
    id = ids[(size_t)s * L + t];
    if (id < 0 || id >= V) {
      if (threadIdx.x == 0) atomicOr(err, 1);
      id = -1;
    }
  }
  if (id < 0) {
    for (int d = threadIdx.x; d < W; d += 128) dst[d] = 0.f;
    return;
  }
  const float* e = tok + (size_t)id * W;
  const float* p = pos + (size_t)t * W;
  for (int d = threadIdx.x; d < W; d += 128) dst[d] = e[d] + p[d];
}

hipError_t launch_text_embed(const int32_t* ids, int N, int L, int Tp, int V, int W, const float* tok, const float* pos, float* x,
                             int32_t* err, hipStream_t s) {
  if (N < 1 || L < 1 || Tp < L || Tp % 8 != 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_text_embed, dim3(N * Tp), dim3(128), 0, s, ids, L, Tp, V, W, tok, pos, x, err);
  return hipGetLastError();
}

// ---- causal attention on MFMA ------------------------------------------------------------------------------------------
// Inputs as EPI_QKV writes them: q, k [N*H][Tk][64], v^T [N*H][64][Tk] (operand type).  nk = round_up(Tp, 32) <= Tk keys are
// staged: K as [nk][72] (row pad: 144-B rows spread a fragment read over the banks), V^T as [64][nk + 8].
// Per wave (32 queries q0 .. q0 + 31, the query on the MFMA column = the lane) and key tile kt of 32 keys:
//   S^T[key][q] = K[key][:] . Q[q][:]     4 x v_mfma_f32_32x32x16 (B = Q, in registers for the whole kernel)
//   online softmax in the log2 domain; the row max / sum are 16 in-register values and one exchange with lane ^ 32
//   O^T[dv][q] += V^T[dv][key] . P^T[key][q]   2 k-steps x 2 halves of dv: accumulator registers 8 s2 .. 8 s2 + 7 are the
//   B fragment of k-step s2 with the keys permuted (16 s2 + 4 h + j, j < 4; 16 s2 + 8 + 4 h + j - 4, j >= 4), and the V^T
//   fragment is read with the same permutation (two 8-byte reads).
static constexpr int TXT_KST = 72;

template <typename T>
__global__ __launch_bounds__(256) void k_text_attention(const VitAttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  typedef typename Vec8<T>::type frag_t;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, nthr = blockDim.x;
  const int h = lane >> 5, r31 = lane & 31;
  const int bh = blockIdx.x, b = bh / a.H, head = bh - b * a.H;
  const int nk = (a.Tp + 31) & ~31, vst = nk + 8;
  T* sk = (T*)smem;
  T* sv = sk + nk * TXT_KST;
  const T* qb = (const T*)a.q + (size_t)bh * a.Tk * 64;
  const T* kb = (const T*)a.k + (size_t)bh * a.Tk * 64;
  const T* vb = (const T*)a.vT + (size_t)bh * 64 * a.Tk;
  const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);
  for (int i = tid; i < nk * 8; i += nthr) {
    const int row = i >> 3, c = i & 7;
    *(uint4*)(sk + row * TXT_KST + c * 8) = row < a.Tp ? *(const uint4*)(kb + (size_t)row * 64 + c * 8) : zero4;
  }
  const int vc = nk >> 3;
  for (int i = tid; i < 64 * vc; i += nthr) {
    const int row = i / vc, c = i - row * vc;
    *(uint4*)(sv + row * vst + c * 8) = c * 8 < a.Tp ? *(const uint4*)(vb + (size_t)row * a.Tk + c * 8) : zero4;
  }
  __syncthreads();

  const int q0 = wid * 32;
  frag_t qf[4];
#pragma unroll
  for (int s = 0; s < 4; ++s) qf[s] = *(const frag_t*)(qb + (size_t)(q0 + r31) * 64 + 16 * s + 8 * h);
  const float sl2 = a.scale * 1.44269504088896340736f;
  float m_run = -1e30f, l_run = 0.f;
  f32x16 ot[2];
#pragma unroll
  for (int d = 0; d < 2; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) ot[d][r] = 0.f;

  for (int kt = 0; kt <= wid; ++kt) {        // tiles wholly above the diagonal are never visited
    f32x16 st;
#pragma unroll
    for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const frag_t kf = *(const frag_t*)(sk + (kt * 32 + r31) * TXT_KST + 16 * s + 8 * h);
      st = mfma32(kf, qf[s], st);
    }
    if (kt == wid) {                          // diagonal tile: key (row) above query (column) masked
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (acc_row32(r, lane) > r31) st[r] = -1e30f;
    }
    float mx = st[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, st[r]);
    mx = xor32_max(mx);
    const float m_new = fmaxf(m_run, mx * sl2);
    const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
    l_run *= alpha;
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
      for (int r = 0; r < 16; ++r) ot[d][r] *= alpha;
    m_run = m_new;
    float p[16], rs = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      p[r] = __builtin_amdgcn_exp2f(fmaf(st[r], sl2, -m_run));
      rs += p[r];
    }
    rs = xor32_add(rs);
    l_run += rs;
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
      frag_t pf;
#pragma unroll
      for (int j = 0; j < 8; ++j) pf[j] = (T)p[8 * s2 + j];
#pragma unroll
      for (int d = 0; d < 2; ++d) {
        const T* vr = sv + (d * 32 + r31) * vst + kt * 32 + 16 * s2 + 4 * h;
        const uint2 lo = *(const uint2*)vr, hi = *(const uint2*)(vr + 8);
        const uint4 v4 = make_uint4(lo.x, lo.y, hi.x, hi.y);
        ot[d] = mfma32(__builtin_bit_cast(frag_t, v4), pf, ot[d]);
      }
    }
  }

  const int q = q0 + r31;
  if (q < a.Tp) {
    const float inv = 1.0f / l_run;
    T* orow = (T*)a.out + (size_t)(b * a.Tp + q) * a.D + head * 64;
#pragma unroll
    for (int d = 0; d < 2; ++d)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4)
#pragma unroll
        for (int j = 0; j < 4; ++j) orow[d * 32 + 8 * g4 + 4 * h + j] = (T)(ot[d][4 * g4 + j] * inv);
  }
}

hipError_t launch_text_attention(OperandType t, const VitAttnArgs& a, hipStream_t s) {
  const int nk = round_up(a.Tp, 32);
  if (a.D != a.H * 64 || a.Tp < 1 || a.Tp % 8 != 0 || nk > 128 || a.Tk < nk || a.Tk % 8 != 0) return hipErrorInvalidValue;
  const size_t smem = ((size_t)nk * TXT_KST + (size_t)64 * (nk + 8)) * 2;
  dim3 grid(a.B * a.H), block(64 * (nk / 32));
  if (t == OP_F16) hipLaunchKernelGGL((k_text_attention<f16>), grid, block, smem, s, a);
  else hipLaunchKernelGGL((k_text_attention<bf16>), grid, block, smem, s, a);
  return hipGetLastError();
}

// ---- the parity mode: causal softmax(q k^T / 8) v in plain fp32 -----------------------------------------------------------
// One wave per query t, keys 0 .. t (lane = key in the score pass, lane = channel in the output pass).  qkv [N*Tp][3D], out
// [N*Tp][D].  The key count is t + 1 for every layout, so the sums run in the same order whatever Tp.
__global__ __launch_bounds__(256) void k_text_attention_f32(const float* __restrict__ qkv, int Tp, int D, int H, float scale,
                                                            float* out) {
  extern __shared__ float s_p[];                       // [4 waves][Tp] probabilities
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int bh = blockIdx.y, b = bh / H, h = bh - b * H;
  const int t = blockIdx.x * 4 + wv;
  if (t >= Tp) return;
  const int len = t + 1;
  float* p = s_p + (size_t)wv * Tp;
  const float* base = qkv + (size_t)b * Tp * 3 * D + h * 64;
  float* o = out + ((size_t)b * Tp + t) * D + h * 64;
  const float* q = base + (size_t)t * 3 * D;
  float mx = -INFINITY;
  for (int j = lane; j < len; j += 64) {
    const float* k = base + (size_t)j * 3 * D + D;
    float s = 0.f;
    for (int d = 0; d < 64; ++d) s += q[d] * k[d];
    s *= scale;
    p[j] = s;
    mx = fmaxf(mx, s);
  }
  mx = wave_max(mx);
  float sum = 0.f;
  for (int j = lane; j < len; j += 64) { const float e = expf(p[j] - mx); p[j] = e; sum += e; }
  sum = wave_sum(sum);
  __builtin_amdgcn_s_waitcnt(0xc07f);                  // lgkmcnt(0): this wave's LDS writes are visible to its own later reads
  const float inv = 1.0f / sum;
  float acc = 0.f;
  for (int j = 0; j < len; ++j) acc += p[j] * base[(size_t)j * 3 * D + 2 * D + lane];
  o[lane] = acc * inv;
}

hipError_t launch_text_attention_f32(const float* qkv, int N, int H, int Tp, int D, float scale, float* out, hipStream_t s) {
  if (D != H * 64 || Tp < 1 || (size_t)4 * Tp * sizeof(float) > 64 * 1024) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_text_attention_f32, dim3(ceil_div(Tp, 4), N * H), dim3(256), 4 * Tp * sizeof(float), s, qkv, Tp, D, H, scale, out);
  return hipGetLastError();
}

// ---- pooling: out[s] = LayerNorm(x[s Tp + argmax ids[s]]) @ proj ----------------------------------------------------------
// One workgroup of 256 per caption.  EOT = the FIRST maximum of the id row (torch.argmax).  LayerNorm in fp32 (two passes:
// mean, then the centred second moment; fixed reduction order), then out[e] = sum over k ascending of y[k] proj[k][e].
__global__ __launch_bounds__(256) void k_text_pool(const float* __restrict__ x, const int32_t* __restrict__ ids, int L, int Tp, int W,
                                                   int E, const float* __restrict__ lw, const float* __restrict__ lb, float eps,
                                                   const float* __restrict__ proj, float* out) {
  __shared__ float y[1024];
  __shared__ float red[4];
  __shared__ int eot_s;
  const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid == 0) {
    const int32_t* row = ids + (size_t)s * L;
    int best = 0;
    for (int j = 1; j < L; ++j)
      if (row[j] > row[best]) best = j;
    eot_s = best;
  }
  __syncthreads();
  const float* xr = x + ((size_t)s * Tp + eot_s) * W;
  float acc = 0.f;
  for (int d = tid; d < W; d += 256) { const float v = xr[d]; y[d] = v; acc += v; }
  acc = wave_sum(acc);
  if (lane == 0) red[wv] = acc;
  __syncthreads();
  const float mean = ((red[0] + red[1]) + (red[2] + red[3])) / (float)W;
  __syncthreads();
  float sq = 0.f;
  for (int d = tid; d < W; d += 256) { const float c = y[d] - mean; sq += c * c; }
  sq = wave_sum(sq);
  if (lane == 0) red[wv] = sq;
  __syncthreads();
  const float rstd = 1.0f / sqrtf(((red[0] + red[1]) + (red[2] + red[3])) / (float)W + eps);
  for (int d = tid; d < W; d += 256) y[d] = (y[d] - mean) * rstd * lw[d] + lb[d];
  __syncthreads();
  for (int e = tid; e < E; e += 256) {
    float o = 0.f;
    for (int k = 0; k < W; ++k) o = fmaf(y[k], proj[(size_t)k * E + e], o);
    out[(size_t)s * E + e] = o;
  }
}

hipError_t launch_text_pool(const float* x, const int32_t* ids, int N, int L, int Tp, int W, int E, const float* lw, const float* lb,
                            float eps, const float* proj, float* out, hipStream_t s) {
  if (N < 1 || L < 1 || W > 1024 || Tp < L) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_text_pool, dim3(N), dim3(256), 0, s, x, ids, L, Tp, W, E, lw, lb, eps, proj, out);
  return hipGetLastError();
}

}  // namespace pio
