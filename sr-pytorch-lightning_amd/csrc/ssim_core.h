// The SSIM core shared by ssim_loss.hip, ms_ssim_loss.hip and ms_ssim.hip: what the family has in common is stated once, here, and
// the three files hold their loaders, tilings, grids and epilogues.  piq.ssim's defaults: the separable 11-tap Gaussian of sigma 1.5
// over the valid map, data range 1.  Plain fp32 VALU (no MFMA: 11-tap separable filters); the library builds with
// -ffp-contract=off, and every sum below has one fixed order, so the callers are bit-reproducible.
//   constants    the taps kG, K / HALO, C1, C2 and the 1/2 shift of the two losses
//   moments      a tile of both images in LDS (X, Y) -> moments_rows (horizontal pass of x, y, xx, yy, xy) -> moments_at (vertical
//                pass at one map position): m = G*x', G*y', G*x'x', G*y'y', G*x'y'
//   map values   map_values: the contrast-structure value cs and the SSIM value ss = l * cs of a position (the losses' forward)
//   pyramid      MS-SSIM's five levels: level_sizes, layout_levels and workspace_bytes on the host; bin: a tile's sums into its level
// Everything here was moved under one condition: each kernel's device code stays instruction for instruction what it was.  Three
// pieces did not survive a function boundary under that condition and are still written out in the kernels that use them:
//   - the backward's adjoints, their transposed filter passes and dV/dx' = G^T*m + 2x' G^T*a + y' G^T*b (ssim_loss_bwd_kernel,
//     ml_bwd_kernel): the two files state the SSIM adjoints in different statement orders, the register allocation follows the
//     order, and no one order reproduces both kernels; as functions of the tile the passes also change ml_bwd_kernel's index code;
//   - the 2x2 replicate-pad average (ml_pool_kernel, ms_pool_kernel): through a function the column index loses its no-wrap flag
//     and the address arithmetic is scheduled differently;
//   - the lane-strided per-plane sum around `bin` (ml_final_kernel, ms_final_kernel): as a function it moves the loads of the kernel
//     arguments.
// The metric's ms_maps_kernel (run-time taps and constants, a per-tile shift) keeps its own map arithmetic, like ssim_kernel in data.hip.
#pragma once
#include "srk_common.h"

namespace ssim {

constexpr int K = 11, HALO = K - 1;                  // Gaussian taps; a valid map of (H - 10) x (W - 10) positions
constexpr float C1 = 1e-4f, C2 = 9e-4f;              // (0.01)^2, (0.03)^2: data range 1
// The losses hold and filter both images as x' = x - 1/2, y' = y - 1/2 and give the means the 1/2 back: the (co)variances do not see
// a shift, and G*x'^2 - (G*x')^2 loses up to four times fewer digits to cancellation on values in [-1/2, 1/2] than on [0, 1] (bright
// flat areas, where s_xx + s_yy + c2 is about c2, are the worst case).  The gradient is the shifted form's, which is the same function.
constexpr float SHIFT = 0.5f;
// exp(-(k - 5)^2 / (2 * 1.5^2)) / sum, rounded from float64
static __device__ __constant__ float kG[K] = {0.001028380123898387f, 0.0075987582094967365f, 0.036000773310661316f, 0.10936068743467331f,
                                              0.21300554275512695f,  0.26601171493530273f,   0.21300554275512695f,  0.10936068743467331f,
                                              0.036000773310661316f, 0.0075987582094967365f, 0.001028380123898387f};

// horizontal pass: Hm[q][r][c] = sum_k G[k] * moment_q(r, c + k) for the RY rows and the RX - 10 columns
template <int THREADS, int RY, int RX>
SRK_DEV void moments_rows(const float (*X)[RX + 1], const float (*Y)[RX + 1], float (*Hm)[RY][RX - HALO]) {
  constexpr int SX = RX - HALO;
  for (int i = threadIdx.x; i < RY * SX; i += THREADS) {
    const int r = i / SX, c = i - r * SX;
    float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float xv = X[r][c + k], yv = Y[r][c + k], w = kG[k];
      m[0] += w * xv; m[1] += w * yv; m[2] += w * (xv * xv); m[3] += w * (yv * yv); m[4] += w * (xv * yv);
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) Hm[q][r][c] = m[q];
  }
}

// vertical pass at map position (r, c) of the tile
template <int RY, int SX>
SRK_DEV void moments_at(const float (*Hm)[RY][SX], int r, int c, float m[5]) {
#pragma unroll
  for (int q = 0; q < 5; ++q) m[q] = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float w = kG[k];
#pragma unroll
    for (int q = 0; q < 5; ++q) m[q] += w * Hm[q][r + k][c];
  }
}

// the contrast-structure value cs and the SSIM value ss = l * cs of a map position
struct MapValues {
  float ss, cs;
};

SRK_DEV MapValues map_values(const float m[5]) {
  const float sxx = m[2] - m[0] * m[0], syy = m[3] - m[1] * m[1], sxy = m[4] - m[0] * m[1];
  const float mx = m[0] + SHIFT, my = m[1] + SHIFT;
  MapValues v;
  v.cs = (2.f * sxy + C2) / (sxx + syy + C2);
  v.ss = (2.f * mx * my + C1) / (mx * mx + my * my + C1) * v.cs;
  return v;
}

// ---- MS-SSIM's pyramid (piq.multi_scale_ssim): level 0 is the image pair, level k > 0 is level k-1 replicate-padded by
// p = max(H % 2, W % 2) on the top and left and averaged 2x2 / stride 2 (F.pad + F.avg_pool2d) ----
constexpr int LEVELS = 5;
constexpr int TILE = 16;                             // map tile edge: one workgroup of 256 per 16 x 16 valid positions
constexpr int MIN_SIZE = HALO * (1 << (LEVELS - 1)) + 1;      // 161: the last level still has a map position

struct Level {
  const float* x;                 // plane 0 of the level of image x; plane q starts at x + q * H * W
  const float* y;
  int H, W;
  int tilesX;
  int first;                      // first map tile of this level in a plane's tile range
};

inline int level_pad(int h, int w) { return (h % 2) | (w % 2); }

// level sizes, as piq builds them
inline void level_sizes(int H, int W, int (&h)[LEVELS], int (&w)[LEVELS]) {
  h[0] = H; w[0] = W;
  for (int k = 1; k < LEVELS; ++k) {
    const int p = level_pad(h[k - 1], w[k - 1]);
    h[k] = (h[k - 1] + p) / 2;
    w[k] = (w[k - 1] + p) / 2;
  }
}

inline int map_tiles_x(int w) { return (w - HALO + TILE - 1) / TILE; }
inline int map_tiles(int h, int w) { return map_tiles_x(w) * map_tiles_x(h); }

// the levels of both images: level 0 is (x, y), level k >= 1 lies in the workspace, x's planes then y's.  Returns the map tiles per plane.
inline int layout_levels(const float* x, const float* y, float* ws, long long planes, const int (&h)[LEVELS], const int (&w)[LEVELS],
                         Level (&lv)[LEVELS]) {
  lv[0].x = x;
  lv[0].y = y;
  int t = 0;
  for (int k = 0; k < LEVELS; ++k) {
    if (k > 0) {
      const size_t n = (size_t)planes * h[k] * w[k];
      lv[k].x = ws;
      lv[k].y = ws + n;
      ws += 2 * n;
    }
    lv[k].H = h[k];
    lv[k].W = w[k];
    lv[k].tilesX = map_tiles_x(w[k]);
    lv[k].first = t;
    t += map_tiles(h[k], w[k]);
  }
  return t;
}

inline long long workspace_bytes(long long planes, const int (&h)[LEVELS], const int (&w)[LEVELS]) {
  long long floats = 0;
  for (int k = 1; k < LEVELS; ++k) floats += 2LL * planes * h[k] * w[k];
  return (floats * 4 + 255) / 256 * 256;
}

// Per level, the value the product uses: cs (v.y) for levels 0-3, ss (v.x) for the last level, of map tile t; a.first[k] is level k's
// first tile in a plane's range, a.first[LEVELS] the tiles per plane.  Adding 0.0 to the other bins leaves them unchanged.
template <class Args>
SRK_DEV void bin(const Args& a, int t, double2 v, double (&b)[LEVELS]) {
#pragma unroll
  for (int k = 0; k < LEVELS; ++k) {
    const double val = k < LEVELS - 1 ? v.y : v.x;
    b[k] += (t >= a.first[k] && t < a.first[k + 1]) ? val : 0.0;
  }
}

}  // namespace ssim
