// AlphaCLIP region inputs (gfx950): the binary region masks and the patch rows of the four-channel patch embedding.
//
//   k_region_masks   bbox_to_alpha_mask / bboxes_to_alpha_mask and trace_to_alpha_mask (P/src/alphaclip/alpha_mask_utils.py;
//                    map_traces_to_grid, P/src/bbox_utils.py:158-168) for many regions in one launch: region r is the union of
//                    its boxes and its trace points, rasterised on a (grid x grid) raster with the reference's arithmetic.  The
//                    same kernel gives the pixel-level mask the tower reads (grid = crop, divisor 1) and the patch-level mask of
//                    the patch average (grid = crop / p, divisor p).
//   k_im2col_alpha   the patch rows of conv1(x) + conv1_alpha(alpha) as ONE GEMM: columns [0, 3p^2) are the image's pixels
//                    (c * p^2 + py * p + px, conv1's flattening) and [3p^2, 4p^2) the mask's (py * p + px, conv1_alpha's); region r
//                    reads image img_of_region[r], so an image with many regions is never copied.
#include "common.h"
#include "kernels.h"

namespace pio {

#pragma clang fp contract(off)
// Python's float floor division as torch computes it for float32 tensors (c10::div_floor_floating): the reference's
// `x_min // patch_size` on a 0-d float tensor.  Not floor(a / b): it rounds the quotient of (a - fmod(a, b)) / b.
__device__ __forceinline__ float py_floordiv(float a, float b) {
  if (b == 0.f) return a / b;
  const float mod = fmodf(a, b);
  float div = (a - mod) / b;
  if (mod != 0.f && ((b < 0.f) != (mod < 0.f))) div -= 1.f;
  float fl;
  if (div != 0.f) {
    fl = floorf(div);
    if (div - fl > 0.5f) fl += 1.f;
  } else {
    fl = copysignf(0.f, a / b);
  }
  return fl;
}

// One workgroup per region.  Pass 1 writes every cell of the region's raster once per chunk of 256 boxes (cell = 1 when it lies in
// one of the chunk's boxes, OR-ed into the earlier chunks'); pass 2 sets the cells the trace points fall in.  Boxes: [x, y, w, h]
// float32, end = x + w in float32, both ends floor-divided by `divisor`, start clamped to [0, grid - 1], end to [0, grid], the end
// EXCLUSIVE and the box empty unless end > start on both axes.  Points: (x, y) float64 inside [0, 1]^2, cell (int)(x / (1 / grid)),
// clamped to grid - 1.
__global__ __launch_bounds__(256) void k_region_masks(const float* __restrict__ boxes, const int32_t* __restrict__ box_off,
                                                      const double* __restrict__ pts, const int32_t* __restrict__ pt_off, int grid,
                                                      float divisor, uint8_t* __restrict__ out) {
  __shared__ int4 s_box[256];
  const int r = blockIdx.x, tid = threadIdx.x;
  const int cells = grid * grid;
  uint8_t* m = out + (size_t)r * cells;
  const int b0 = box_off[r], b1 = box_off[r + 1];
  const float gm1 = (float)(grid - 1), gf = (float)grid;
  for (int c0 = b0; c0 < b1 || c0 == b0; c0 += 256) {
    const int nb = min(256, b1 - c0);
    __syncthreads();                                   // the previous chunk's readers are done with s_box
    if (tid < nb) {
      const float* bx = boxes + 4 * (size_t)(c0 + tid);
      const float x0 = bx[0], y0 = bx[1];
      const float xe = x0 + bx[2], ye = y0 + bx[3];
      const int x1 = (int)fminf(fmaxf(py_floordiv(x0, divisor), 0.f), gm1);
      const int y1 = (int)fminf(fmaxf(py_floordiv(y0, divisor), 0.f), gm1);
      const int x2 = (int)fminf(fmaxf(py_floordiv(xe, divisor), 0.f), gf);
      const int y2 = (int)fminf(fmaxf(py_floordiv(ye, divisor), 0.f), gf);
      s_box[tid] = (x2 > x1 && y2 > y1) ? make_int4(x1, y1, x2, y2) : make_int4(0, 0, 0, 0);
    }
    __syncthreads();
    for (int c = tid; c < cells; c += 256) {
      const int cy = c / grid, cx = c - cy * grid;
      uint8_t v = c0 == b0 ? 0 : m[c];
      for (int j = 0; j < nb && !v; ++j) {
        const int4 q = s_box[j];
        v = (cx >= q.x && cx < q.z && cy >= q.y && cy < q.w) ? 1 : 0;
      }
      m[c] = v;
    }
    if (nb <= 0) break;                                // a region without boxes: one pass of zeros
  }
  __syncthreads();                                     // every cell is written before the points set theirs
  const double patch = 1.0 / (double)grid;             // map_traces_to_grid divides by this double
  for (int i = pt_off[r] + tid; i < pt_off[r + 1]; i += 256) {
    const double x = pts[2 * i], y = pts[2 * i + 1];
    if (x >= 0.0 && x <= 1.0 && y >= 0.0 && y <= 1.0) {
      int gx = (int)(x / patch), gy = (int)(y / patch);
      gx = gx < grid - 1 ? gx : grid - 1;
      gy = gy < grid - 1 ? gy : grid - 1;
      m[gy * grid + gx] = 1;
    }
  }
}
#pragma clang fp contract(on)

template <typename T> __device__ __forceinline__ T to_op(float v) { return (T)v; }

// One thread per (patch row, channel, py) run of p values; channel 3 is the mask (null: ones, the whole-image forward).
template <typename T>
__global__ __launch_bounds__(256) void k_im2col_alpha(const float* __restrict__ imgs, const int32_t* __restrict__ img_of_region,
                                                      const uint8_t* __restrict__ masks, int R, int S, int p, int n, int Kpad,
                                                      T* __restrict__ out) {
  const int total = R * n * n * 4 * p;
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int py = idx % p;
  int row = idx / p;
  const int c = row & 3;
  row >>= 2;                                            // patch row r * n2 + gy * n + gx
  const int gx = row % n, gy = (row / n) % n, r = row / (n * n);
  const int y = gy * p + py, x0 = gx * p;
  T* dst = out + (size_t)row * Kpad + c * p * p + py * p;
  if (c < 3) {
    const int b = img_of_region ? img_of_region[r] : r;
    const float* src = imgs + (((size_t)b * 3 + c) * S + y) * S + x0;
    for (int px = 0; px < p; ++px) dst[px] = to_op<T>(src[px]);
  } else if (masks) {
    const uint8_t* src = masks + ((size_t)r * S + y) * S + x0;
    for (int px = 0; px < p; ++px) dst[px] = to_op<T>(src[px] ? 1.f : 0.f);
  } else {
    for (int px = 0; px < p; ++px) dst[px] = to_op<T>(1.f);
  }
}

hipError_t launch_region_masks(const float* boxes, const int32_t* box_off, const double* pts, const int32_t* pt_off, int R, int grid,
                               float divisor, uint8_t* out, hipStream_t s) {
  if (R < 1 || grid < 1 || grid > 4096 || !(divisor > 0.f) || !box_off || !pt_off || !out) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_region_masks, dim3(R), dim3(256), 0, s, boxes, box_off, pts, pt_off, grid, divisor, out);
  return hipGetLastError();
}

hipError_t launch_im2col_alpha(int type, const float* imgs, const int32_t* img_of_region, const uint8_t* masks, int R, int S, int p,
                               int n, int Kpad, void* out, hipStream_t s) {
  if (R < 1 || Kpad < 4 * p * p) return hipErrorInvalidValue;
  const dim3 grid(ceil_div(R * n * n * 4 * p, 256));
  if (type == 0) hipLaunchKernelGGL((k_im2col_alpha<f16>), grid, dim3(256), 0, s, imgs, img_of_region, masks, R, S, p, n, Kpad, (f16*)out);
  else if (type == 1) hipLaunchKernelGGL((k_im2col_alpha<bf16>), grid, dim3(256), 0, s, imgs, img_of_region, masks, R, S, p, n, Kpad, (bf16*)out);
  else hipLaunchKernelGGL((k_im2col_alpha<float>), grid, dim3(256), 0, s, imgs, img_of_region, masks, R, S, p, n, Kpad, (float*)out);
  return hipGetLastError();
}

}  // namespace pio
