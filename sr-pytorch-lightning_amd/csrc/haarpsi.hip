// HaarPSI loss (piq 0.7.0 haarpsi / HaarPSILoss, reference srmodel.py:36): include/srk.h "HaarPSI", sr_amd/haarpsi.py.
//   haarpsi_fwd_kernel       one workgroup per (image, 16x16 half-resolution tile): clamp sr, x255, YIQ and the 2x2 subsampling of
//                            both images into LDS (a 3/4-pixel half-res halo), the three scales' Haar coefficients of Y' from one
//                            8x8 window per pixel (the k = 2, 4, 8 boxes nest), the similarities and weights, and the tile's
//                            sums of sigma(alpha sim) w and w to fixed slots (no float atomics: bitwise repeatable).
//   haarpsi_finalize_kernel  one workgroup: per image a fixed-order fp64 sum of its tiles, r_n, h_n and the per-image factors of
//                            the backward; the loss 1 - mean h_n (and the index).
//   haarpsi_bwd_kernel       one workgroup per tile: recomputes the coefficients on a 7-pixel halo from the subsampled Y', I', Q'
//                            planes the forward kept (the adjoints need r_n and W_n, which exist only after the whole image is
//                            reduced, so no per-pixel adjoint can be stored by the forward; the planes are 6 B per HR pixel where
//                            recomputing them from sr and hr reads 24 B at a 3.5x halo over-read: at 16x3x192x192 that backward
//                            took 56 us, this one 39 us, for 2.4 us more forward), the
//                            adjoints of the coefficients and of the pooled I / Q, the flipped Haar boxes, the 2x2 pools, M^T,
//                            x255 and the clamp mask, times *gout.
// Plain fp32 VALU (a few dozen FLOP per pixel: no MFMA).  The library builds with -ffp-contract=off.
#include "srk_common.h"

namespace {

constexpr int HT = 16;                     // tile edge, half-resolution pixels
constexpr int HP_THREADS = 256;            // one thread per tile pixel
constexpr int FWD_R = HT + 7;              // forward Y' region: rows i0-3 .. i0+HT+3
constexpr int BWD_C = HT + 7;              // backward coefficient region: rows i0-4 .. i0+HT+2
constexpr int BWD_R = HT + 14;             // backward Y' region: rows i0-7 .. i0+HT+6
constexpr float HP_C = 30.f, HP_ALPHA = 4.2f, HP_EPS = 1.1920928955078125e-07f;   // piq: c, alpha, EPS = 2^-23
constexpr double HP_EPS_D = 1.1920928955078125e-07;
constexpr int FIN_THREADS = 1024;
// YIQ rows (Y, I, Q) of piq's rgb2yiq
__device__ __constant__ float kYiq[9] = {0.299f, 0.587f, 0.114f, 0.5959f, -0.2746f, -0.3213f, 0.2115f, -0.5227f, 0.3112f};
static_assert(HT * HT == HP_THREADS, "one thread per tile pixel");

// Y' (and I', Q' when rgb) of both images over an R x R region whose top-left half-res pixel is (oy, ox): planes
// 0: Y'x  1: Y'y  2: I'x  3: Q'x  4: I'y  5: Q'y.  Zero outside [0, H') x [0, W'); inside, the 2x2 mean of x255 YIQ with the
// full-resolution pixels beyond H x W (the bottom / right subsampling pad) counting as 0.  `keep` (nullable): the image's planes in
// global memory ([P][H'][W']), written for the region's central HT x HT tile (the region starts `halo` pixels before the tile).
template <int R>
SRK_DEV void load_region(const srk_haarpsi_args& a, int n, int oy, int ox, int Hh, int Wh, float (*pl)[R][R], float* keep, int halo) {
  const int H = a.H, W = a.W;
  const long long hw = (long long)H * W;
  const bool rgb = a.C == 3;
  for (int i = threadIdx.x; i < R * R; i += HP_THREADS) {
    const int ry = i / R, rx = i - ry * R;
    const int r = oy + ry, c = ox + rx;
    float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (r >= 0 && r < Hh && c >= 0 && c < Wh) {
#pragma unroll
      for (int im = 0; im < 2; ++im) {
        const float* src = (im == 0 ? a.sr : a.hr) + (long long)n * a.C * hw;
        float sy = 0.f, si = 0.f, sq = 0.f;
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          const int y = 2 * r + (d >> 1), x = 2 * c + (d & 1);
          if (y >= H || x >= W) continue;
          const long long o = (long long)y * W + x;
          if (rgb) {
            float v[3];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
              const float t = src[o + ch * hw];
              v[ch] = 255.f * (im == 0 ? fminf(fmaxf(t, 0.f), 1.f) : t);
            }
            sy += kYiq[0] * v[0] + kYiq[1] * v[1] + kYiq[2] * v[2];
            si += kYiq[3] * v[0] + kYiq[4] * v[1] + kYiq[5] * v[2];
            sq += kYiq[6] * v[0] + kYiq[7] * v[1] + kYiq[8] * v[2];
          } else {
            const float t = src[o];
            sy += 255.f * (im == 0 ? fminf(fmaxf(t, 0.f), 1.f) : t);
          }
        }
        acc[im] = 0.25f * sy;
        acc[2 + 2 * im] = 0.25f * si;
        acc[3 + 2 * im] = 0.25f * sq;
      }
    }
    pl[0][ry][rx] = acc[0];
    pl[1][ry][rx] = acc[1];
    if (rgb) {
      pl[2][ry][rx] = acc[2]; pl[3][ry][rx] = acc[3]; pl[4][ry][rx] = acc[4]; pl[5][ry][rx] = acc[5];
    }
    if (keep && ry >= halo && ry < halo + HT && rx >= halo && rx < halo + HT && r < Hh && c < Wh) {
      const long long hhw = (long long)Hh * Wh, o = (long long)r * Wh + c;
      const int np = rgb ? 6 : 2;
      for (int q = 0; q < np; ++q) keep[q * hhw + o] = acc[q];
    }
  }
}

// the same region read back from the planes the forward kept (zero outside [0, H') x [0, W'))
template <int R>
SRK_DEV void load_planes(const float* keep, bool rgb, int oy, int ox, int Hh, int Wh, float (*pl)[R][R]) {
  const long long hhw = (long long)Hh * Wh;
  const int np = rgb ? 6 : 2;
  for (int i = threadIdx.x; i < R * R; i += HP_THREADS) {
    const int ry = i / R, rx = i - ry * R;
    const int r = oy + ry, c = ox + rx;
    const bool in = r >= 0 && r < Hh && c >= 0 && c < Wh;
    const long long o = (long long)r * Wh + c;
    for (int q = 0; q < np; ++q) pl[q][ry][rx] = in ? keep[q * hhw + o] : 0.f;
  }
}

// the six Haar coefficients (orientation-major: o * 3 + s - 1) of the pixel whose 8x8 Y' window starts at (wy, wx): window row /
// column 4 - k/2 .. 3 + k/2 is the k-box; orientation 0 is (upper half - lower half) / k, orientation 1 (left - right) / k
template <int R>
SRK_DEV void haar6(const float (*img)[R], int wy, int wx, float h[6]) {
  float c2[8], c4[8], c8[8], r2[8], r4[8], r8[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) { r2[i] = 0.f; r4[i] = 0.f; r8[i] = 0.f; }
#pragma unroll
  for (int r = 0; r < 8; ++r) {
    float w[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) w[c] = img[wy + r][wx + c];
    c2[r] = w[3] + w[4];
    c4[r] = c2[r] + (w[2] + w[5]);
    c8[r] = c4[r] + ((w[1] + w[6]) + (w[0] + w[7]));
    const bool in2 = r == 3 || r == 4, in4 = r >= 2 && r <= 5;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      if (in2) r2[c] += w[c];
      if (in4) r4[c] += w[c];
      r8[c] += w[c];
    }
  }
  h[0] = 0.5f * (c2[3] - c2[4]);
  h[1] = 0.25f * ((c4[2] + c4[3]) - (c4[4] + c4[5]));
  h[2] = 0.125f * (((c8[0] + c8[1]) + (c8[2] + c8[3])) - ((c8[4] + c8[5]) + (c8[6] + c8[7])));
  h[3] = 0.5f * (r2[3] - r2[4]);
  h[4] = 0.25f * ((r4[2] + r4[3]) - (r4[4] + r4[5]));
  h[5] = 0.125f * (((r8[0] + r8[1]) + (r8[2] + r8[3])) - ((r8[4] + r8[5]) + (r8[6] + r8[7])));
}

SRK_DEV float sim_s(float u, float v) { return (2.f * u * v + HP_C) / (u * u + v * v + HP_C + HP_EPS); }
// d S(u, v) / d u
SRK_DEV float sim_du(float u, float v) {
  const float d = u * u + v * v + HP_C + HP_EPS;
  return (2.f * v * d - (2.f * u * v + HP_C) * (2.f * u)) / (d * d);
}
SRK_DEV float sigm(float z) { return 1.f / (1.f + expf(-z)); }
SRK_DEV float sgnf(float v) { return (v > 0.f) ? 1.f : (v < 0.f ? -1.f : 0.f); }

// everything one coefficient pixel needs: its 8x8 window starts at (wy, wx) of the region, its I / Q 2x2 pool at (wy+3, wx+3)
struct HaarPx {
  float hx[6], hy[6];
  float ix, iy, qx, qy;
  float w[3], sim[3];
};

template <int R>
SRK_DEV void haar_pixel(const float (*pl)[R][R], bool rgb, int wy, int wx, HaarPx& p) {
  haar6<R>(pl[0], wy, wx, p.hx);
  haar6<R>(pl[1], wy, wx, p.hy);
  p.w[0] = fmaxf(fabsf(p.hx[2]), fabsf(p.hy[2]));
  p.w[1] = fmaxf(fabsf(p.hx[5]), fabsf(p.hy[5]));
  p.sim[0] = 0.5f * (sim_s(fabsf(p.hx[0]), fabsf(p.hy[0])) + sim_s(fabsf(p.hx[1]), fabsf(p.hy[1])));
  p.sim[1] = 0.5f * (sim_s(fabsf(p.hx[3]), fabsf(p.hy[3])) + sim_s(fabsf(p.hx[4]), fabsf(p.hy[4])));
  p.ix = p.iy = p.qx = p.qy = 0.f;
  p.w[2] = p.sim[2] = 0.f;
  if (rgb) {
    const int y = wy + 3, x = wx + 3;
    p.ix = 0.25f * ((pl[2][y][x] + pl[2][y][x + 1]) + (pl[2][y + 1][x] + pl[2][y + 1][x + 1]));
    p.qx = 0.25f * ((pl[3][y][x] + pl[3][y][x + 1]) + (pl[3][y + 1][x] + pl[3][y + 1][x + 1]));
    p.iy = 0.25f * ((pl[4][y][x] + pl[4][y][x + 1]) + (pl[4][y + 1][x] + pl[4][y + 1][x + 1]));
    p.qy = 0.25f * ((pl[5][y][x] + pl[5][y][x + 1]) + (pl[5][y + 1][x] + pl[5][y + 1][x + 1]));
    p.sim[2] = 0.5f * (sim_s(fabsf(p.ix), fabsf(p.iy)) + sim_s(fabsf(p.qx), fabsf(p.qy)));
    p.w[2] = 0.5f * (p.w[0] + p.w[1]);
  }
}

__global__ __launch_bounds__(HP_THREADS) void haarpsi_fwd_kernel(const srk_haarpsi_args a, int tiles_x, int Hh, int Wh) {
  __shared__ float pl[6][FWD_R][FWD_R];
  __shared__ double red[HP_THREADS / 64][2];
  const int tid = threadIdx.x, n = blockIdx.y;
  const int i0 = (blockIdx.x / tiles_x) * HT, j0 = (blockIdx.x % tiles_x) * HT;
  const bool rgb = a.C == 3;
  float* keep = a.planes ? a.planes + (long long)n * (rgb ? 6 : 2) * Hh * Wh : nullptr;
  load_region<FWD_R>(a, n, i0 - 3, j0 - 3, Hh, Wh, pl, keep, 3);
  __syncthreads();
  const int ty = tid / HT, tx = tid % HT;
  double sw = 0.0, ws = 0.0;
  if (i0 + ty < Hh && j0 + tx < Wh) {
    HaarPx p;
    haar_pixel<FWD_R>(pl, rgb, ty, tx, p);
    float s = 0.f, t = 0.f;
#pragma unroll
    for (int o = 0; o < 3; ++o) {
      if (o == 2 && !rgb) break;
      s += sigm(HP_ALPHA * p.sim[o]) * p.w[o];
      t += p.w[o];
    }
    sw = (double)s;
    ws = (double)t;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    sw += __shfl_down(sw, off, 64);
    ws += __shfl_down(ws, off, 64);
  }
  if ((tid & 63) == 0) {
    red[tid >> 6][0] = sw;
    red[tid >> 6][1] = ws;
  }
  __syncthreads();
  if (tid == 0) {
    double s = 0.0, t = 0.0;
#pragma unroll
    for (int w = 0; w < HP_THREADS / 64; ++w) { s += red[w][0]; t += red[w][1]; }
    double* dst = a.partial + 2 * ((long long)n * gridDim.x + blockIdx.x);
    dst[0] = s;
    dst[1] = t;
  }
}

// one wave per image (images w, w + 16, ...), its tiles summed lane-strided then by a fixed shuffle tree
__global__ __launch_bounds__(FIN_THREADS) void haarpsi_finalize_kernel(const srk_haarpsi_args a, int tiles) {
  __shared__ double red[FIN_THREADS / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  double hsum = 0.0;
  for (int n = wv; n < a.N; n += FIN_THREADS / 64) {
    const double* p = a.partial + 2LL * n * tiles;
    double s = 0.0, t = 0.0;
    for (int i = lane; i < tiles; i += 64) {
      s += p[2 * i];
      t += p[2 * i + 1];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      s += __shfl_down(s, off, 64);
      t += __shfl_down(t, off, 64);
    }
    if (lane == 0) {
      const double r = (s + HP_EPS_D) / (t + HP_EPS_D);
      const double lg = log(r / (1.0 - r));
      const double h = (lg / (double)HP_ALPHA) * (lg / (double)HP_ALPHA);
      hsum += h;
      float* st = a.stats + 4LL * n;
      st[0] = (float)r;
      st[1] = (float)(1.0 / (t + HP_EPS_D));
      // d loss / d r_n for a unit upstream gradient: loss = 1 - mean h
      st[2] = (float)(-2.0 * lg / ((double)a.N * (double)HP_ALPHA * (double)HP_ALPHA * r * (1.0 - r)));
      st[3] = (float)h;
    }
  }
  if (lane == 0) red[wv] = hsum;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < FIN_THREADS / 64; ++w) t += red[w];
    const double idx = t / (double)a.N;
    *a.loss = (float)(1.0 - idx);
    if (a.index) *a.index = (float)idx;
  }
}

__global__ __launch_bounds__(HP_THREADS) void haarpsi_bwd_kernel(const srk_haarpsi_args a, int tiles_x, int Hh, int Wh) {
  __shared__ float pl[6][BWD_R][BWD_R];
  __shared__ float gh[6][BWD_C][BWD_C];      // d loss / d (Haar coefficient of sr), coefficient rows i0-4 .. i0+HT+2
  __shared__ float gq[2][BWD_C][BWD_C];      // d loss / d (pooled I, Q of sr)
  const int tid = threadIdx.x, n = blockIdx.y;
  const int i0 = (blockIdx.x / tiles_x) * HT, j0 = (blockIdx.x % tiles_x) * HT;
  const bool rgb = a.C == 3;
  const float* st = a.stats + 4LL * n;
  const float rn = st[0], invw = st[1], G = st[2];          // for a unit upstream gradient: *gout scales the result at the end
  load_planes<BWD_R>(a.planes + (long long)n * (rgb ? 6 : 2) * Hh * Wh, rgb, i0 - 7, j0 - 7, Hh, Wh, pl);
  __syncthreads();
  for (int i = tid; i < BWD_C * BWD_C; i += HP_THREADS) {
    const int cy = i / BWD_C, cx = i - cy * BWD_C;
    const int ci = i0 - 4 + cy, cj = j0 - 4 + cx;
    float g[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, gi = 0.f, gqq = 0.f;
    if (ci >= 0 && ci < Hh && cj >= 0 && cj < Wh) {
      HaarPx p;
      haar_pixel<BWD_R>(pl, rgb, cy, cx, p);
      float A[3], B[3];
#pragma unroll
      for (int o = 0; o < 3; ++o) {
        const float s = sigm(HP_ALPHA * p.sim[o]);
        A[o] = G * (HP_ALPHA * (s * (1.f - s))) * p.w[o] * invw;      // d loss / d sim_o
        B[o] = G * (s - rn) * invw;                                      // d loss / d w_o
      }
      if (rgb) {                                                         // w_2 = (w_0 + w_1) / 2
        B[0] += 0.5f * B[2];
        B[1] += 0.5f * B[2];
      }
#pragma unroll
      for (int o = 0; o < 2; ++o) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const float hx = p.hx[3 * o + s], hy = p.hy[3 * o + s];
          g[3 * o + s] = (A[o] * 0.5f) * sim_du(fabsf(hx), fabsf(hy)) * sgnf(hx);
        }
        const float ux = fabsf(p.hx[3 * o + 2]), uy = fabsf(p.hy[3 * o + 2]);
        const float tie = ux > uy ? 1.f : (ux < uy ? 0.f : 0.5f);         // torch.maximum: half to each side on a tie
        g[3 * o + 2] = B[o] * tie * sgnf(p.hx[3 * o + 2]);
      }
      if (rgb) {
        gi = (A[2] * 0.5f) * sim_du(fabsf(p.ix), fabsf(p.iy)) * sgnf(p.ix);
        gqq = (A[2] * 0.5f) * sim_du(fabsf(p.qx), fabsf(p.qy)) * sgnf(p.qx);
      }
    }
#pragma unroll
    for (int c = 0; c < 6; ++c) gh[c][cy][cx] = g[c];
    gq[0][cy][cx] = gi;
    gq[1][cy][cx] = gqq;
  }
  __syncthreads();
  const int ty = tid / HT, tx = tid % HT;
  const int pi = i0 + ty, pj = j0 + tx;
  if (pi >= Hh || pj >= Wh) return;
  // d loss / d Y'(pi, pj): coefficient (pi + d, pj + e), d, e in [-k/2, k/2 - 1], sits at window row / column 4 + d of the 8x8
  // gh window starting at (ty, tx); the flipped kernel weighs it +1/k for d >= 0 (orientation 0) resp. e >= 0 (orientation 1)
  float gy = 0.f;
  {
    float b2 = 0.f, b4 = 0.f, b8 = 0.f;
#pragma unroll
    for (int r = 0; r < 8; ++r) {
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const float s0 = r >= 4 ? 1.f : -1.f, s1 = c >= 4 ? 1.f : -1.f;
        const bool in2 = r >= 3 && r <= 4 && c >= 3 && c <= 4, in4 = r >= 2 && r <= 5 && c >= 2 && c <= 5;
        if (in2) b2 += s0 * gh[0][ty + r][tx + c] + s1 * gh[3][ty + r][tx + c];
        if (in4) b4 += s0 * gh[1][ty + r][tx + c] + s1 * gh[4][ty + r][tx + c];
        b8 += s0 * gh[2][ty + r][tx + c] + s1 * gh[5][ty + r][tx + c];
      }
    }
    gy = 0.5f * b2 + 0.25f * b4 + 0.125f * b8;
  }
  float gI = 0.f, gQ = 0.f;
  if (rgb) {                                 // pooled (pi - a, pj - b), a, b in {0, 1}: coefficient rows ty + 3, ty + 4
    gI = 0.25f * ((gq[0][ty + 3][tx + 3] + gq[0][ty + 3][tx + 4]) + (gq[0][ty + 4][tx + 3] + gq[0][ty + 4][tx + 4]));
    gQ = 0.25f * ((gq[1][ty + 3][tx + 3] + gq[1][ty + 3][tx + 4]) + (gq[1][ty + 4][tx + 3] + gq[1][ty + 4][tx + 4]));
  }
  // the 2x2 / stride-2 pool (taps on the bottom / right pad dropped), YIQ^T, x255, the clamp's mask
  const int H = a.H, W = a.W;
  const long long hw = (long long)H * W;
  const float* sr = a.sr + (long long)n * a.C * hw;
  float* gr = a.grad + (long long)n * a.C * hw;
  const float qy = 0.25f * gy, qi = 0.25f * gI, qq = 0.25f * gQ, gs = *a.gout;
  float gc[3];
  if (rgb) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) gc[ch] = 255.f * ((kYiq[ch] * qy + kYiq[3 + ch] * qi) + kYiq[6 + ch] * qq);
  } else {
    gc[0] = 255.f * qy;
  }
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    const int y = 2 * pi + (d >> 1), x = 2 * pj + (d & 1);
    if (y >= H || x >= W) continue;
    const long long o = (long long)y * W + x;
    for (int ch = 0; ch < a.C; ++ch) {
      const float v = sr[o + ch * hw];
      gr[o + ch * hw] = (v >= 0.f && v <= 1.f) ? gc[ch] * gs : 0.f;
    }
  }
}

}  // namespace

static int hp_geometry(int H, int W, int* Hh, int* Wh, int* tx, int* ty) {
  if (H < 16 || W < 16) return -1;
  const int p = (H % 2) | (W % 2);
  *Hh = (H + p) / 2;
  *Wh = (W + p) / 2;
  *tx = (*Wh + HT - 1) / HT;
  *ty = (*Hh + HT - 1) / HT;
  return 0;
}

extern "C" int srk_haarpsi_tiles(int N, int H, int W) {
  int Hh, Wh, tx, ty;
  if (N <= 0 || hp_geometry(H, W, &Hh, &Wh, &tx, &ty)) return -1;
  const long long t = (long long)N * tx * ty;
  return t < (1LL << 31) ? (int)t : -1;
}

static int hp_check(const srk_haarpsi_args* a, const char* who) {
  SRK_CHECK_ARG(a && a->sr && a->partial && a->stats, "%s: null pointer", who);
  SRK_CHECK_ARG(a->N > 0 && a->N <= 65535 && (a->C == 1 || a->C == 3), "%s: bad sizes N=%d C=%d", who, a->N, a->C);
  SRK_CHECK_ARG(srk_haarpsi_tiles(a->N, a->H, a->W) > 0, "%s: image %dx%d refused (HaarPSI needs H, W >= 16)", who, a->H, a->W);
  return 0;
}

extern "C" int srk_haarpsi_fwd(const srk_haarpsi_args* a, srk_stream_t stream) {
  if (int rc = hp_check(a, "srk_haarpsi_fwd")) return rc;
  SRK_CHECK_ARG(a->hr, "srk_haarpsi_fwd: null pointer");
  int Hh, Wh, tx, ty;
  hp_geometry(a->H, a->W, &Hh, &Wh, &tx, &ty);
  hipLaunchKernelGGL(haarpsi_fwd_kernel, dim3((unsigned)(tx * ty), (unsigned)a->N), dim3(HP_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), *a, tx, Hh, Wh);
  SRK_LAUNCH_CHECK();
  return 0;
}

extern "C" int srk_haarpsi_finalize(const srk_haarpsi_args* a, srk_stream_t stream) {
  if (int rc = hp_check(a, "srk_haarpsi_finalize")) return rc;
  SRK_CHECK_ARG(a->loss, "srk_haarpsi_finalize: null pointer");
  int Hh, Wh, tx, ty;
  hp_geometry(a->H, a->W, &Hh, &Wh, &tx, &ty);
  hipLaunchKernelGGL(haarpsi_finalize_kernel, dim3(1), dim3(FIN_THREADS), 0, reinterpret_cast<hipStream_t>(stream), *a, tx * ty);
  SRK_LAUNCH_CHECK();
  return 0;
}

extern "C" int srk_haarpsi_bwd(const srk_haarpsi_args* a, srk_stream_t stream) {
  if (int rc = hp_check(a, "srk_haarpsi_bwd")) return rc;
  SRK_CHECK_ARG(a->gout && a->grad && a->planes, "srk_haarpsi_bwd: null pointer");
  int Hh, Wh, tx, ty;
  hp_geometry(a->H, a->W, &Hh, &Wh, &tx, &ty);
  hipLaunchKernelGGL(haarpsi_bwd_kernel, dim3((unsigned)(tx * ty), (unsigned)a->N), dim3(HP_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), *a, tx, Hh, Wh);
  SRK_LAUNCH_CHECK();
  return 0;
}
