// Host-side row selection for the sparse last ViT block: which rows of the padded token matrix does a trace region read?
//
// k_region_reduce skips every patch whose grid weight is zero, and k_trace_grids leaves every cell no trace point falls into exactly 0.
// The last block's query rows, attention output, proj, LayerNorm 2, fc1, fc2 and the final LayerNorm are therefore needed only for the
// patches with a non-zero count (api.cpp, run_vit_block_rows).  The cell of a point is evaluated here with the arithmetic of
// k_trace_grids (region.hip): the [0, 1] test, the DIVISION by the double 1.0 / n, the clamp to n - 1 -- IEEE double on both sides, so
// the host's cells are the device's.
//
// The unit is a QUAD: four consecutive rows of the padded token matrix whose first row b * Tp + t is a multiple of 4 (Tp % 8 == 0, so
// quads never straddle images).  Whole aligned quads keep `row mod 4` unchanged after compaction, which is all that resid_join_ktile
// (kernels.h) keys the order of the residual sum on.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace pio {

// xy [P][2] (x, y) of all points, offs [B + 1] CSR offsets.  Writes the first rows of the needed quads, ascending, to quads (room for
// `cap`), img_off [B + 1] = offsets of every image's quads in that list.  Returns the number of quads, or -1 when cap is too small or
// an argument is unusable (Tp % 8 != 0, T > Tp, offsets not ascending).
inline int trace_quads(const double* xy, const int32_t* offs, int B, int n, int G, int T, int Tp, int32_t* quads, int cap,
                       int32_t* img_off) {
  if (B < 1 || n < 1 || G < 0 || T != G + n * n || Tp < T || Tp % 8 != 0 || !offs || !quads || !img_off) return -1;
  const double patch = 1.0 / (double)n;   // k_trace_grids divides by this double
  const int qpi = Tp / 4;
  std::vector<uint8_t> need((size_t)qpi);
  int nq = 0;
  for (int b = 0; b < B; ++b) {
    img_off[b] = nq;
    if (offs[b + 1] < offs[b] || offs[b] < 0) return -1;
    std::fill(need.begin(), need.end(), (uint8_t)0);
    for (int i = offs[b]; i < offs[b + 1]; ++i) {
      const double x = xy[2 * (size_t)i], y = xy[2 * (size_t)i + 1];
      if (x >= 0.0 && x <= 1.0 && y >= 0.0 && y <= 1.0) {
        int gx = (int)(x / patch), gy = (int)(y / patch);
        gx = gx < n - 1 ? gx : n - 1;
        gy = gy < n - 1 ? gy : n - 1;
        need[(size_t)(G + gy * n + gx) >> 2] = 1;
      }
    }
    for (int q = 0; q < qpi; ++q) {
      if (!need[q]) continue;
      if (nq >= cap) return -1;
      quads[nq++] = b * Tp + 4 * q;
    }
  }
  img_off[B] = nq;
  return nq;
}

// What pio_vit_forward_rows requires of a quad list (it indexes device memory with it): img_off ascending from 0, every quad of image b a
// multiple of 4 inside [b Tp, (b + 1) Tp), strictly ascending.  *max_per_img = the longest per-image run.
inline bool quads_valid(const int32_t* quads, const int32_t* img_off, int B, int Tp, int* max_per_img) {
  if (!quads || !img_off || img_off[0] != 0) return false;
  int mx = 0;
  for (int b = 0; b < B; ++b) {
    const int q0 = img_off[b], q1 = img_off[b + 1];
    if (q1 < q0 || q1 - q0 > Tp / 4) return false;
    int prev = b * Tp - 4;
    for (int i = q0; i < q1; ++i) {
      const int r = quads[i];
      if ((r & 3) != 0 || r <= prev || r + 4 > (b + 1) * Tp) return false;
      prev = r;
    }
    mx = q1 - q0 > mx ? q1 - q0 : mx;
  }
  *max_per_img = mx;
  return true;
}

}  // namespace pio
