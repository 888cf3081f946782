// RegionCLIP's CLIP ModifiedResNet tower (vit_arch 3, P/src/regionclip/clip_backbone.py:14-300) on gfx950.
//
//   k_conv_mfma    NHWC implicit-GEMM convolution on v_mfma_f32_32x32x16_{f16,bf16}: M = B Ho Wo output pixels, N = Cout,
//                  K = kh kw Cin ordered (ky, kx, c) with Cin padded to a multiple of 8 (weights [Cout][ky][kx][Cin_pad]), so that
//                  a lane's 8 consecutive k of one MFMA step are 8 channels of ONE input pixel: one 16-byte load.  Taps outside
//                  the image (3x3, pad 1), rows past M, columns past N and k past K are zeros in the registers (masked loads).
//                  The epilogue is the FrozenBN of the reference as a per-channel fp32 scale / shift, the residual and the ReLU.
//   k_conv_f32     the same convolution in exact fp32 (vit_operand_type 2, the parity mode): one thread per output element.
//   k_avgpool2     nn.AvgPool2d(2) in NHWC.
//   k_attnpool_in  AttentionPool2d's input rows: per image the mean over HW in row 0, the HW pixels after it, + the position table,
//                  zero rows up to Tp.
//
// Numerics.  The reference runs the tower on fp16 activations (convert_weights + x.type(conv1.weight.dtype), clip_backbone.py:245):
// every conv output, BN output and residual sum is rounded to fp16.  The epilogue rounds at the same places, in the operand type:
//     a = rnd(acc);  t = rnd(a * scale[n] + shift[n]);  with a residual: t = rnd(t + res[m][n]);  ReLU
// where `a * scale + shift` is evaluated in fp32 (no contraction) and rounded to the operand type ONCE, as the reference's eval
// F.batch_norm does (x * alpha + beta in fp32, one rounding of its fp16 output); tests/regionclip_ref.py states it with one rounding of
// the float64 value.  c_proj (the fp32-output form) is a Linear: rnd(acc + bias), one rounding.  The fp32 mode does the same operations
// without the roundings.  Every output element is ONE sum over k ascending in MFMA steps of 16 (fp32 mode: steps of
// 1) whatever the tile, the grid or the launch size: no split-K, so an image's activations do not depend on what else the launch holds.
#include "common.h"
#include "kernels.h"

namespace pio {

#pragma clang fp contract(off)

template <typename T> __device__ __forceinline__ float rnd(float v) { return (float)(T)v; }
template <> __device__ __forceinline__ float rnd<float>(float v) { return v; }

// The epilogue of one output element (row m, column n).  out_f32: y32[(b out_rows + out_off + p) N + n] for the pixel p < valid of image b
// (pixels per image = Ho Wo): the attnpool's c_proj writing the fp32 tokens.
template <typename T>
__device__ __forceinline__ void conv_store(const ConvArgs& a, int m, int n, float acc) {
  if (a.out_f32) {                   // a Linear (c_proj): the bias joins the fp32 accumulator, one rounding (scale is 1)
    float t = rnd<T>(acc * a.scale[n] + a.shift[n]);
    const int hw = a.Ho * a.Wo, b = m / hw, p = m - b * hw;
    if (p >= a.valid) return;
    if (a.relu) t = fmaxf(t, 0.f);
    a.y32[((size_t)b * a.out_rows + a.out_off + p) * a.Cout + n] = t;
    return;
  }
  float t = rnd<T>(rnd<T>(acc) * a.scale[n] + a.shift[n]);
  if (a.res) t = rnd<T>(t + (float)((const T*)a.res)[(size_t)m * a.Cout + n]);
  if (a.relu) t = fmaxf(t, 0.f);
  ((T*)a.y)[(size_t)m * a.Cout + n] = (T)t;
}

// One workgroup = 4 waves in 2 x 2, wave tile (32 FM) x (32 FN), workgroup tile (64 FM) x (64 FN).  Operands go from global memory
// straight into the MFMA registers (no LDS): the 2 x 2 waves share A rows / W columns through L1 and L2.
template <typename T, int FM, int FN>
__global__ __launch_bounds__(256) void k_conv_mfma(ConvArgs a) {
  typedef typename Vec8<T>::type v8;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int r = lane & 31, h = lane >> 5;
  const int M = a.B * a.Ho * a.Wo, K = a.ks * a.ks * a.Cin;
  const int m0 = blockIdx.x * 64 * FM + (wv & 1) * 32 * FM, n0 = blockIdx.y * 64 * FN + (wv >> 1) * 32 * FN;
  // the pixel of each A row this lane loads
  int pb[FM], py[FM], px[FM];
  bool pv[FM];
#pragma unroll
  for (int i = 0; i < FM; ++i) {
    const int m = m0 + i * 32 + r;
    pv[i] = m < M;
    const int mm = pv[i] ? m : 0, hw = a.Ho * a.Wo;
    pb[i] = mm / hw;
    const int q = mm - pb[i] * hw;
    py[i] = (q / a.Wo) * a.stride - a.pad;
    px[i] = (q % a.Wo) * a.stride - a.pad;
  }
  const T* X = (const T*)a.x;
  const T* Wt = (const T*)a.w;
  f32x16 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  v8 zero;
#pragma unroll
  for (int e = 0; e < 8; ++e) zero[e] = (T)0.f;
  for (int k0 = 0; k0 < K; k0 += 16) {
    const int kk = k0 + 8 * h;
    const bool kv = kk < K;
    const int tap = kv ? kk / a.Cin : 0, c = kk - tap * a.Cin;
    const int ky = tap / a.ks, kx = tap - ky * a.ks;
    v8 fa[FM], fw[FN];
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      const int iy = py[i] + ky, ix = px[i] + kx;
      const bool ok = kv && pv[i] && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
      fa[i] = ok ? *(const v8*)(X + (((size_t)pb[i] * a.H + iy) * a.W + ix) * a.Cin + c) : zero;
    }
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int n = n0 + j * 32 + r;
      fw[j] = (kv && n < a.Cout) ? *(const v8*)(Wt + (size_t)n * K + kk) : zero;
    }
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) acc[i][j] = mfma32(fa[i], fw[j], acc[i][j]);
  }
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      const int n = n0 + j * 32 + r;
      if (n >= a.Cout) continue;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int m = m0 + i * 32 + acc_row32(e, lane);
        if (m < M) conv_store<T>(a, m, n, acc[i][j][e]);
      }
    }
}

// exact fp32: thread = (pixel m, channel n); 64 channels x 4 pixels per workgroup, k ascending
__global__ __launch_bounds__(256) void k_conv_f32(ConvArgs a) {
  const int n = blockIdx.y * 64 + (threadIdx.x & 63);
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int M = a.B * a.Ho * a.Wo;
  if (m >= M || n >= a.Cout) return;
  const int hw = a.Ho * a.Wo, b = m / hw, q = m - b * hw;
  const int y0 = (q / a.Wo) * a.stride - a.pad, x0 = (q % a.Wo) * a.stride - a.pad;
  const float* X = (const float*)a.x;
  const float* Wr = (const float*)a.w + (size_t)n * a.ks * a.ks * a.Cin;
  float acc = 0.f;
  for (int ky = 0; ky < a.ks; ++ky) {
    const int iy = y0 + ky;
    for (int kx = 0; kx < a.ks; ++kx) {
      const int ix = x0 + kx;
      const float* w = Wr + (ky * a.ks + kx) * a.Cin;
      if (iy < 0 || iy >= a.H || ix < 0 || ix >= a.W) continue;     // a zero tap adds +0: the sum is unchanged
      const float* xp = X + (((size_t)b * a.H + iy) * a.W + ix) * a.Cin;
      for (int c = 0; c < a.Cin; ++c) acc = fmaf(xp[c], w[c], acc);
    }
  }
  conv_store<float>(a, m, n, acc);
}

// imgs [B][3][S][S] fp32 -> [B][S][S][8] operand type (channels 3..7 zero): the stem's input, rounded as x.type(fp16) does
template <typename T>
__global__ __launch_bounds__(256) void k_rn_input(const float* __restrict__ imgs, int B, int S, T* out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, npix = (size_t)B * S * S;
  if (i >= npix) return;
  const size_t b = i / ((size_t)S * S), p = i - b * S * S;
  T* o = out + i * 8;
#pragma unroll
  for (int c = 0; c < 8; ++c) o[c] = (T)(c < 3 ? imgs[(b * 3 + c) * S * S + p] : 0.f);
}

// nn.AvgPool2d(2): ((x00 + x01) + x10) + x11 in fp32, / 4, rounded once (torch's CPU kernel sums the window row-major).  The fp32 sum
// of four fp16 (bf16) values is exact only while their exponents span at most ~11 (~14) binades; beyond that it rounds too
template <typename T>
__global__ __launch_bounds__(256) void k_avgpool2(const T* __restrict__ x, int B, int H, int W, int C, T* __restrict__ y) {
  const int Ho = H / 2, Wo = W / 2;
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, total = (size_t)B * Ho * Wo * C;
  if (i >= total) return;
  const int c = (int)(i % C);
  size_t r = i / C;
  const int ox = (int)(r % Wo);
  r /= Wo;
  const int oy = (int)(r % Ho);
  const size_t b = r / Ho;
  const T* p = x + ((b * H + 2 * oy) * W + 2 * ox) * C + c;
  const float s = (((float)p[0] + (float)p[C]) + (float)p[(size_t)W * C]) + (float)p[(size_t)W * C + C];
  y[i] = (T)(s / 4.f);
}

// one workgroup per (image, 256-channel slice): row 0 = rnd(rnd(mean) + rnd(pos[0])), row 1 + p = rnd(x[p] + rnd(pos[1 + p])),
// rows [1 + HW, Tp) zero
template <typename T>
__global__ __launch_bounds__(256) void k_attnpool_in(const T* __restrict__ x, const float* __restrict__ pos, int HW, int C, int Tp,
                                                     T* __restrict__ out) {
  const int b = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  const T* xb = x + (size_t)b * HW * C + c;
  T* ob = out + (size_t)b * Tp * C + c;
  float s = 0.f;
  for (int p = 0; p < HW; ++p) s += (float)xb[(size_t)p * C];
  ob[0] = (T)(rnd<T>(s / (float)HW) + rnd<T>(pos[c]));
  for (int p = 0; p < HW; ++p) ob[(size_t)(1 + p) * C] = (T)((float)xb[(size_t)p * C] + rnd<T>(pos[(size_t)(1 + p) * C + c]));
  for (int t = 1 + HW; t < Tp; ++t) ob[(size_t)t * C] = (T)0.f;
}

// tile choice: 128 x 128 workgroups where they still give two per CU of the 256, else 64 x 64 (layer4 at 7 x 7: M = 49 B)
int route_conv(const ConvArgs& a) {
  const long M = (long)a.B * a.Ho * a.Wo;
  const long big = ((M + 127) / 128) * ((a.Cout + 127) / 128);
  return big >= 512 ? 2 : 1;
}

hipError_t launch_conv(int type, const ConvArgs& a, int tile, hipStream_t s) {
  const int M = a.B * a.Ho * a.Wo;
  if (M <= 0 || a.Cin % 8 != 0 || a.Cout < 1 || (a.ks != 1 && a.ks != 3) || a.stride < 1) return hipErrorInvalidValue;
  if (a.Ho != (a.H + 2 * a.pad - a.ks) / a.stride + 1 || a.Wo != (a.W + 2 * a.pad - a.ks) / a.stride + 1) return hipErrorInvalidValue;
  if ((size_t)M * a.Cout >= ((size_t)1 << 31)) return hipErrorInvalidValue;
  if (type == 2) {
    hipLaunchKernelGGL(k_conv_f32, dim3(ceil_div(M, 4), ceil_div(a.Cout, 64)), dim3(256), 0, s, a);
    return hipGetLastError();
  }
  if (tile == 0) tile = route_conv(a);
  if (tile != 1 && tile != 2) return hipErrorInvalidValue;
  const dim3 grid(ceil_div(M, 64 * tile), ceil_div(a.Cout, 64 * tile));
  if (type == 0) {
    if (tile == 2) hipLaunchKernelGGL((k_conv_mfma<f16, 2, 2>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_conv_mfma<f16, 1, 1>), grid, dim3(256), 0, s, a);
  } else {
    if (tile == 2) hipLaunchKernelGGL((k_conv_mfma<bf16, 2, 2>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_conv_mfma<bf16, 1, 1>), grid, dim3(256), 0, s, a);
  }
  return hipGetLastError();
}

hipError_t launch_rn_input(int type, const float* imgs, int B, int S, void* out, hipStream_t s) {
  const size_t n = (size_t)B * S * S;
  const dim3 grid((unsigned)((n + 255) / 256));
  if (type == 0) hipLaunchKernelGGL((k_rn_input<f16>), grid, dim3(256), 0, s, imgs, B, S, (f16*)out);
  else if (type == 1) hipLaunchKernelGGL((k_rn_input<bf16>), grid, dim3(256), 0, s, imgs, B, S, (bf16*)out);
  else hipLaunchKernelGGL((k_rn_input<float>), grid, dim3(256), 0, s, imgs, B, S, (float*)out);
  return hipGetLastError();
}

hipError_t launch_avgpool2(int type, const void* x, int B, int H, int W, int C, void* y, hipStream_t s) {
  const size_t n = (size_t)B * (H / 2) * (W / 2) * C;
  if (n == 0) return hipErrorInvalidValue;
  const dim3 grid((unsigned)((n + 255) / 256));
  if (type == 0) hipLaunchKernelGGL((k_avgpool2<f16>), grid, dim3(256), 0, s, (const f16*)x, B, H, W, C, (f16*)y);
  else if (type == 1) hipLaunchKernelGGL((k_avgpool2<bf16>), grid, dim3(256), 0, s, (const bf16*)x, B, H, W, C, (bf16*)y);
  else hipLaunchKernelGGL((k_avgpool2<float>), grid, dim3(256), 0, s, (const float*)x, B, H, W, C, (float*)y);
  return hipGetLastError();
}

hipError_t launch_attnpool_in(int type, const void* x, const float* pos, int B, int HW, int C, int Tp, void* out, hipStream_t s) {
  if (Tp < HW + 1 || B < 1) return hipErrorInvalidValue;
  const dim3 grid(ceil_div(C, 256), B);
  if (type == 0) hipLaunchKernelGGL((k_attnpool_in<f16>), grid, dim3(256), 0, s, (const f16*)x, pos, HW, C, Tp, (f16*)out);
  else if (type == 1) hipLaunchKernelGGL((k_attnpool_in<bf16>), grid, dim3(256), 0, s, (const bf16*)x, pos, HW, C, Tp, (bf16*)out);
  else hipLaunchKernelGGL((k_attnpool_in<float>), grid, dim3(256), 0, s, (const float*)x, pos, HW, C, Tp, (float*)out);
  return hipGetLastError();
}

}  // namespace pio
