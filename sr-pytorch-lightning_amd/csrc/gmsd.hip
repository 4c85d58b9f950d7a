// GMSD loss and metric (gradient magnitude similarity deviation; piq.GMSDLoss): include/srk.h "GMSD loss", sr_amd/gmsd.py.
// "Pooled" pixels are the 2x2 means of the luma of clamp(sr, 0, 1) and of hr, after piq's zero pad at the bottom and right; the map
// has one position per pooled pixel (Hd x Wd).
//   gmsd_fwd_kernel    one workgroup per (image, 16x32 tile of the map): clamp, luma and pool both images into LDS (18x34 pooled
//                      pixels), the Prewitt taps from LDS, d = GMS - 1 per position, and (sum d, sum d^2) of the tile as two doubles
//                      in its own slot (no atomics: bitwise repeatable).
//   gmsd_stats_kernel  one wave per image: the fixed-order fp64 sums of its tiles -> (mean of d, GMSD_n) in `stats`.
//   gmsd_mean_kernel   one workgroup: the fixed-order mean of GMSD_n -> loss.
//   gmsd_bwd_kernel    one workgroup per (image, 16x32 tile of pooled pixels = 32x64 pixels of sr): the pooled luma of the 20x36
//                      pixels around the tile, the adjoints of grad_x x of the 18x34 positions whose taps touch the tile, the transposed
//                      taps per pooled pixel, and the gradient of its 2x2 block in every channel under the clamp's mask.  Gather form:
//                      no atomics, every element of grad written once.
// d = GMS - 1 = -(a - b)^2 / (a^2 + b^2 + c) is formed directly: GMS sits near 1, so the variance of d does not cancel, and d is
// exactly 0 for identical images.  HBM traffic per pixel of a plane: forward reads sr, hr (8 B); backward reads sr, hr (8 B; the
// halo and the mask re-read are served by L2) and writes grad (4 B).  Nothing is kept between forward and backward but 8 B per image.
// LDS rows are RX + 1 floats (35 / 37: odd), a wave reads 32 consecutive floats of a row per 32-lane group: no bank conflicts.
// Plain fp32 VALU (3x3 taps: no MFMA).  The library builds with -ffp-contract=off.
#include <stdint.h>

#include "srk_common.h"

namespace {

constexpr int GM_THREADS = 256;
constexpr int TY = 16, TX = 32;                       // tile of the pooled map, forward and backward
constexpr int FIN_THREADS = 1024;
constexpr float GM_C = 0.0026143790849673202f;        // 170 / 255^2
constexpr float GM_THIRD = 1.0f / 3.0f;
constexpr float GM_R = 0.299f, GM_G = 0.587f, GM_B = 0.114f;
static_assert(GM_THREADS % 64 == 0 && (TY * TX) % GM_THREADS == 0, "whole waves, whole passes over the tile");

SRK_DEV float clamp01(float v) { return fminf(fmaxf(v, 0.f), 1.f); }

// pixels (x, x + 1) of a row starting at element o: one 8-byte load when `vec` (W even and 8-byte aligned bases: x is even), else
// scalar loads, the second only where `two` (x + 1 < W)
SRK_DEV float2 load_pair(const float* p, size_t o, bool vec, bool two) {
  if (vec) return *reinterpret_cast<const float2*>(p + o);
  return make_float2(p[o], two ? p[o + 1] : 0.f);
}

// RY x RX pooled pixels of one image of both inputs, top-left pooled pixel (oy, ox): the 2x2 mean (over the zero pad where the block
// leaves the image) of the luma of clamp(sr, 0, 1) and of hr; zero outside [0, Hd) x [0, Wd): the zero padding of the taps
template <int RY, int RX>
SRK_DEV void load_region(const float* xs, const float* ys, int C, int H, int W, bool vec, int oy, int ox, int Hd, int Wd,
                         float (*X)[RX + 1], float (*Y)[RX + 1]) {
  const size_t plane = (size_t)H * W;
  for (int i = threadIdx.x; i < RY * RX; i += GM_THREADS) {
    const int r = i / RX, c = i - r * RX;
    const int py = oy + r, px = ox + c;
    float vx = 0.f, vy = 0.f;
    if (py >= 0 && py < Hd && px >= 0 && px < Wd) {
      const bool two = 2 * px + 1 < W;
#pragma unroll
      for (int dy = 0; dy < 2; ++dy) {
        if (2 * py + dy >= H) continue;                            // the pad row
        const size_t o = (size_t)(2 * py + dy) * W + (size_t)(2 * px);
        float2 lx, ly;
        if (C == 3) {
          const float2 r0 = load_pair(xs, o, vec, two), g0 = load_pair(xs, o + plane, vec, two), b0 = load_pair(xs, o + 2 * plane, vec, two);
          const float2 r1 = load_pair(ys, o, vec, two), g1 = load_pair(ys, o + plane, vec, two), b1 = load_pair(ys, o + 2 * plane, vec, two);
          lx.x = GM_R * clamp01(r0.x) + GM_G * clamp01(g0.x) + GM_B * clamp01(b0.x);
          lx.y = GM_R * clamp01(r0.y) + GM_G * clamp01(g0.y) + GM_B * clamp01(b0.y);
          ly.x = GM_R * r1.x + GM_G * g1.x + GM_B * b1.x;
          ly.y = GM_R * r1.y + GM_G * g1.y + GM_B * b1.y;
        } else {
          lx = load_pair(xs, o, vec, two);
          ly = load_pair(ys, o, vec, two);
          lx.x = clamp01(lx.x);
          lx.y = clamp01(lx.y);
        }
        if (!two) lx.y = ly.y = 0.f;                               // the pad column
        vx += lx.x + lx.y;
        vy += ly.x + ly.y;
      }
      vx *= 0.25f;
      vy *= 0.25f;
    }
    X[r][c] = vx;
    Y[r][c] = vy;
  }
}

// Prewitt cross-correlation at the pooled pixel P[r + 1][c + 1]: right minus left and bottom minus top columns / rows, over 3
template <int LD>
SRK_DEV void prewitt(const float (*P)[LD], int r, int c, float& gx, float& gy) {
  const float p00 = P[r][c], p01 = P[r][c + 1], p02 = P[r][c + 2];
  const float p10 = P[r + 1][c], p12 = P[r + 1][c + 2];
  const float p20 = P[r + 2][c], p21 = P[r + 2][c + 1], p22 = P[r + 2][c + 2];
  gx = ((p02 - p00) + (p12 - p10) + (p22 - p20)) * GM_THIRD;
  gy = ((p20 - p00) + (p21 - p01) + (p22 - p02)) * GM_THIRD;
}

__global__ __launch_bounds__(GM_THREADS) void gmsd_fwd_kernel(const srk_gmsd_args a, int Hd, int Wd, int tiles_x, int tiles_pi,
                                                               int vec) {
  constexpr int RY = TY + 2, RX = TX + 2;
  __shared__ float X[RY][RX + 1], Y[RY][RX + 1];
  __shared__ double red[2][GM_THREADS / 64];
  const int tid = threadIdx.x;
  const int n = blockIdx.x / tiles_pi, t = blockIdx.x - n * tiles_pi;
  const int i0 = (t / tiles_x) * TY, j0 = (t % tiles_x) * TX;
  const size_t io = (size_t)n * a.C * a.H * a.W;
  load_region<RY, RX>(a.sr + io, a.hr + io, a.C, a.H, a.W, vec != 0, i0 - 1, j0 - 1, Hd, Wd, X, Y);
  __syncthreads();
  double s1 = 0.0, s2 = 0.0;
#pragma unroll
  for (int i = tid; i < TY * TX; i += GM_THREADS) {
    const int r = i / TX, c = i - r * TX;
    if (i0 + r < Hd && j0 + c < Wd) {
      float gxx, gyx, gxy, gyy;
      prewitt<RX + 1>(X, r, c, gxx, gyx);
      prewitt<RX + 1>(Y, r, c, gxy, gyy);
      const float sa = gxx * gxx + gyx * gyx, sb = gxy * gxy + gyy * gyy;
      const float df = sqrtf(sa) - sqrtf(sb);
      const float d = -(df * df) / (sa + sb + GM_C);
      s1 += (double)d;
      s2 += (double)d * (double)d;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s1 += __shfl_down(s1, off, 64);
    s2 += __shfl_down(s2, off, 64);
  }
  if ((tid & 63) == 0) {
    red[0][tid >> 6] = s1;
    red[1][tid >> 6] = s2;
  }
  __syncthreads();
  if (tid == 0) {
    a.partial[2 * (size_t)blockIdx.x] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    a.partial[2 * (size_t)blockIdx.x + 1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  }
}
static_assert(GM_THREADS / 64 == 4, "the forward's last step adds four waves");

// one wave per image: lane-strided over the image's tiles in index order, a fixed shuffle tree
__global__ __launch_bounds__(GM_THREADS) void gmsd_stats_kernel(const srk_gmsd_args a, int tiles_pi, double count) {
  const int lane = threadIdx.x & 63;
  const long long n = (long long)blockIdx.x * (GM_THREADS / 64) + (threadIdx.x >> 6);
  if (n >= a.N) return;                                            // the whole wave leaves
  const double* p = a.partial + 2 * (size_t)n * tiles_pi;
  double s1 = 0.0, s2 = 0.0;
  for (int t = lane; t < tiles_pi; t += 64) {
    s1 += p[2 * (size_t)t];
    s2 += p[2 * (size_t)t + 1];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s1 += __shfl_down(s1, off, 64);
    s2 += __shfl_down(s2, off, 64);
  }
  if (lane == 0) {
    const double m = s1 / count, var = s2 / count - m * m;
    a.stats[2 * n] = (float)m;
    a.stats[2 * n + 1] = var > 0.0 ? (float)sqrt(var) : 0.f;
  }
}

// thread-strided over the images in index order, a fixed shuffle tree, then the 16 waves in order
__global__ __launch_bounds__(FIN_THREADS) void gmsd_mean_kernel(const srk_gmsd_args a) {
  __shared__ double red[FIN_THREADS / 64];
  double t = 0.0;
  for (long long n = threadIdx.x; n < a.N; n += FIN_THREADS) t += (double)a.stats[2 * n + 1];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < FIN_THREADS / 64; ++w) s += red[w];
    *a.loss = (float)(s / (double)a.N);
  }
}

__global__ __launch_bounds__(GM_THREADS) void gmsd_bwd_kernel(const srk_gmsd_args a, int Hd, int Wd, int tiles_x, int tiles_pi,
                                                               float inv_count, int vec) {
  constexpr int SY = TY + 2, SX = TX + 2;                          // map positions whose taps touch the tile
  constexpr int RY = SY + 2, RX = SX + 2;                          // pooled pixels those positions read
  __shared__ float X[RY][RX + 1], Y[RY][RX + 1];
  __shared__ float Ax[SY][SX + 1], Ay[SY][SX + 1];                 // d loss / d (grad_x x), d loss / d (grad_y x); 0 off the map
  const int tid = threadIdx.x;
  const int n = blockIdx.x / tiles_pi, t = blockIdx.x - n * tiles_pi;
  const int i0 = (t / tiles_x) * TY, j0 = (t % tiles_x) * TX;      // the tile's first pooled pixel
  const size_t io = (size_t)n * a.C * a.H * a.W;
  // region pixel (r, c) is pooled pixel (i0 - 2 + r, j0 - 2 + c); position (r, c) of Ax / Ay is map position (i0 - 1 + r, j0 - 1 + c)
  load_region<RY, RX>(a.sr + io, a.hr + io, a.C, a.H, a.W, vec != 0, i0 - 2, j0 - 2, Hd, Wd, X, Y);
  __syncthreads();
  const float mean = a.stats[2 * (size_t)n], sd = a.stats[2 * (size_t)n + 1];
  // d loss / d GMS = k (d - mean); an image of zero deviation gets no gradient.  The upstream gradient multiplies the finished
  // value, once: grad is linear in it to the last bit
  const float k = sd > 0.f ? inv_count / sd : 0.f;
  const float gout = *a.gout;
  for (int i = tid; i < SY * SX; i += GM_THREADS) {
    const int r = i / SX, c = i - r * SX;
    const int pi = i0 - 1 + r, pj = j0 - 1 + c;
    float ax = 0.f, ay = 0.f;
    if (pi >= 0 && pi < Hd && pj >= 0 && pj < Wd) {
      float gxx, gyx, gxy, gyy;
      prewitt<RX + 1>(X, r, c, gxx, gyx);
      prewitt<RX + 1>(Y, r, c, gxy, gyy);
      const float sa = gxx * gxx + gyx * gyx, sb = gxy * gxy + gyy * gyy;
      const float av = sqrtf(sa), bv = sqrtf(sb);
      if (av > 0.f) {                                              // the square root's derivative is taken as 0 at 0
        const float df = av - bv, id = 1.f / (sa + sb + GM_C);
        const float d = -(df * df) * id;
        // d GMS / d a = 2 (b - a GMS) / (a^2 + b^2 + c) with GMS = 1 + d, then d a / d grad = grad / a
        const float u = k * (d - mean) * (2.f * ((bv - av) - av * d) * id) / av;
        ax = u * gxx;
        ay = u * gyx;
      }
    }
    Ax[r][c] = ax;
    Ay[r][c] = ay;
  }
  __syncthreads();
  const float* sr = a.sr + io;
  float* gr = a.grad + io;
  const size_t plane = (size_t)a.H * a.W;
  const float coef[3] = {GM_R, GM_G, GM_B};
#pragma unroll
  for (int i = tid; i < TY * TX; i += GM_THREADS) {
    const int r = i / TX, c = i - r * TX;
    const int pi = i0 + r, pj = j0 + c;
    if (pi >= Hd || pj >= Wd) continue;
    // the transposed taps: pooled pixel (pi, pj) is the right neighbour of the positions in column pj - 1, the left one of column pj + 1
    const float gp = ((Ax[r][c] - Ax[r][c + 2]) + (Ax[r + 1][c] - Ax[r + 1][c + 2]) + (Ax[r + 2][c] - Ax[r + 2][c + 2]) +
                      (Ay[r][c] - Ay[r + 2][c]) + (Ay[r][c + 1] - Ay[r + 2][c + 1]) + (Ay[r][c + 2] - Ay[r + 2][c + 2])) *
                     (GM_THIRD * 0.25f);
    const bool two = 2 * pj + 1 < a.W;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      if (ch >= a.C) break;
      const float g = (a.C == 3 ? gp * coef[ch] : gp) * gout;
#pragma unroll
      for (int dy = 0; dy < 2; ++dy) {
        if (2 * pi + dy >= a.H) continue;
        const size_t o = (size_t)ch * plane + (size_t)(2 * pi + dy) * a.W + (size_t)(2 * pj);
        const float2 s = load_pair(sr, o, vec != 0, two);
        // the clamp passes the gradient on [0, 1]
        const float g0 = (s.x >= 0.f && s.x <= 1.f) ? g : 0.f, g1 = (s.y >= 0.f && s.y <= 1.f) ? g : 0.f;
        if (vec) {
          *reinterpret_cast<float2*>(gr + o) = make_float2(g0, g1);
        } else {
          gr[o] = g0;
          if (two) gr[o + 1] = g1;
        }
      }
    }
  }
}

struct GmGeom {
  int Hd, Wd, tx, ty;              // the pooled map and its tiles per image
};

}  // namespace

static int gm_geometry(int N, int C, int H, int W, GmGeom* g) {
  if (N <= 0 || (C != 1 && C != 3) || H <= 0 || W <= 0) return -1;
  const int p = (H % 2) | (W % 2);
  if (H > INT32_MAX - 1 || W > INT32_MAX - 1) return -1;
  g->Hd = (H + p) / 2;
  g->Wd = (W + p) / 2;
  g->tx = (g->Wd + TX - 1) / TX;
  g->ty = (g->Hd + TY - 1) / TY;
  // one grid dimension carries (image, tile), and a tile index stays an int
  const long long lim = (1LL << 31) - 1;
  if ((long long)g->tx * g->ty > lim || (long long)N > lim / ((long long)g->tx * g->ty)) return -1;
  return 0;
}

extern "C" int srk_gmsd_tiles(int N, int C, int H, int W) {
  GmGeom g;
  if (gm_geometry(N, C, H, W, &g)) return -1;
  return (int)((long long)N * g.tx * g.ty);
}

static int gm_check(const srk_gmsd_args* a, const char* who, GmGeom* g) {
  SRK_CHECK_ARG(a && a->sr, "%s: null pointer", who);
  SRK_CHECK_ARG(a->N > 0 && a->H > 0 && a->W > 0, "%s: bad sizes N=%d C=%d H=%d W=%d", who, a->N, a->C, a->H, a->W);
  SRK_CHECK_ARG(a->C == 1 || a->C == 3, "%s: C=%d (GMSD takes 1 or 3 channels)", who, a->C);
  SRK_CHECK_ARG(gm_geometry(a->N, a->C, a->H, a->W, g) == 0, "%s: %dx%dx%dx%d refused (images x tiles must stay below 2^31)", who, a->N,
                a->C, a->H, a->W);
  return 0;
}

// 8-byte loads and stores of pixel pairs: every row of every plane starts on 8 bytes
static int gm_vec(const srk_gmsd_args* a, const float* extra) {
  return a->W % 2 == 0 && ((uintptr_t)a->sr | (uintptr_t)a->hr | (uintptr_t)extra) % 8 == 0;
}

extern "C" int srk_gmsd_fwd(const srk_gmsd_args* a, srk_stream_t stream) {
  GmGeom g;
  if (int rc = gm_check(a, "srk_gmsd_fwd", &g)) return rc;
  SRK_CHECK_ARG(a->hr && a->partial, "srk_gmsd_fwd: null pointer");
  const int tpi = g.tx * g.ty;
  hipLaunchKernelGGL(gmsd_fwd_kernel, dim3((unsigned)((long long)a->N * tpi)), dim3(GM_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                     *a, g.Hd, g.Wd, g.tx, tpi, gm_vec(a, nullptr));
  SRK_LAUNCH_CHECK();
  return 0;
}

extern "C" int srk_gmsd_finalize(const srk_gmsd_args* a, srk_stream_t stream) {
  GmGeom g;
  if (int rc = gm_check(a, "srk_gmsd_finalize", &g)) return rc;
  SRK_CHECK_ARG(a->partial && a->stats && a->loss, "srk_gmsd_finalize: null pointer");
  const int per = GM_THREADS / 64;
  hipLaunchKernelGGL(gmsd_stats_kernel, dim3((unsigned)((a->N + per - 1) / per)), dim3(GM_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                     *a, g.tx * g.ty, (double)g.Hd * (double)g.Wd);
  SRK_LAUNCH_CHECK();
  hipLaunchKernelGGL(gmsd_mean_kernel, dim3(1), dim3(FIN_THREADS), 0, reinterpret_cast<hipStream_t>(stream), *a);
  SRK_LAUNCH_CHECK();
  return 0;
}

extern "C" int srk_gmsd_bwd(const srk_gmsd_args* a, srk_stream_t stream) {
  GmGeom g;
  if (int rc = gm_check(a, "srk_gmsd_bwd", &g)) return rc;
  SRK_CHECK_ARG(a->hr && a->stats && a->gout && a->grad, "srk_gmsd_bwd: null pointer");
  const int tpi = g.tx * g.ty;
  const float inv_count = (float)(1.0 / ((double)g.Hd * (double)g.Wd * (double)a->N));
  hipLaunchKernelGGL(gmsd_bwd_kernel, dim3((unsigned)((long long)a->N * tpi)), dim3(GM_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                     *a, g.Hd, g.Wd, g.tx, tpi, inv_count, gm_vec(a, a->grad));
  SRK_LAUNCH_CHECK();
  return 0;
}
