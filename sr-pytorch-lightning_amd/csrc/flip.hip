// FLIP loss / metric (reference losses/flip.py; Andersson et al., HPG 2020): include/srk.h "FLIP", sr_amd/flip.py.
//   flip_fwd_kernel  one workgroup per (image, 32x32 tile): both images -> YCxCz in LDS (10-pixel replicate-clamped halo), the
//                    separable CSF and feature filters as a horizontal pass into LDS and a vertical pass into registers, then the
//                    per-pixel error, its partial sum (fixed order) and the 7 adjoints of the error for a unit upstream gradient.
//   flip_bwd_kernel  one workgroup per tile: the 7 adjoint planes with a 10-pixel halo in LDS, the transposed filters (horizontal,
//                    then vertical), the colour-space Jacobian of the test image and the input clamp, times *gout * scale.
// Plain fp32 VALU (about 2 kFLOP per pixel: no MFMA).  The library builds with -ffp-contract=off, so every product and sum below is
// rounded as written.
#include "srk_common.h"

namespace {

constexpr int FT = 32;                 // tile edge (output pixels)
constexpr int FR = 10;                 // CSF radius = halo
constexpr int FRF = 9;                 // feature radius
constexpr int FE = FT + 2 * FR;        // 52: tile + halo
constexpr int NCSF = 2 * FR + 1, NFEAT = 2 * FRF + 1;
// the device table (sr_amd/flip.py _TAB_*)
constexpr int T_A = 0, T_RG = 21, T_BY1 = 42, T_BY2 = 63, T_EDGE = 84, T_POINT = 103, T_GAUSS = 122;
constexpr int T_BYW = 141, T_RED = 143, T_M = 147, T_MINV = 156, T_WHITE = 165;
static_assert(SRK_FLIP_TABLE_FLOATS == 176 && SRK_FLIP_ADJ_CHANNELS == 7, "table layout");

constexpr int FWD_THREADS = 512;
// the filter taps are read from LDS (broadcast) inside every outer iteration: without this fence the compiler hoists all ~140 of
// them out of the pixel loops into VGPRs and spills
#define FLIP_RELOAD_TAPS() asm volatile("" ::: "memory")
constexpr int BWD_THREADS = 512;

// sRGB in [0,1] (clamped) -> YCxCz
SRK_DEV void srgb_to_ycxcz(const float* tab, float r, float g, float b, float& oy, float& ocx, float& ocz) {
  float c[3] = {r, g, b}, l[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float v = fminf(fmaxf(c[i], 0.f), 1.f);
    l[i] = v > 0.04045f ? powf((v + 0.055f) / 1.055f, 2.4f) : v / 12.92f;
  }
  float t[3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
    t[i] = (tab[T_M + 3 * i] * l[0] + tab[T_M + 3 * i + 1] * l[1] + tab[T_M + 3 * i + 2] * l[2]) / tab[T_WHITE + i];
  oy = 116.f * t[1] - 16.f;
  ocx = 500.f * (t[0] - t[1]);
  ocz = 200.f * (t[1] - t[2]);
}

// filtered YCxCz -> clamped linear RGB -> Hunt-adjusted L*a*b*; keeps what the adjoint needs
struct LabState {
  float lab[3];          // L, a, b (before the Hunt adjustment)
  float hunt[3];         // L, 0.01 L a, 0.01 L b
  float fp[3];           // d f / d t of the cube-root segment
  float mask[3];         // 1 where the clamp to [0,1] passes the gradient (closed interval)
};

SRK_DEV void filtered_to_lab(const float* tab, const float o[3], LabState& s) {
  const float yy = (o[0] + 16.f) / 116.f;
  const float u[3] = {(yy + o[1] / 500.f) * tab[T_WHITE], yy * tab[T_WHITE + 1], (yy - o[2] / 200.f) * tab[T_WHITE + 2]};
  float lin[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float v = tab[T_MINV + 3 * i] * u[0] + tab[T_MINV + 3 * i + 1] * u[1] + tab[T_MINV + 3 * i + 2] * u[2];
    s.mask[i] = (v >= 0.f && v <= 1.f) ? 1.f : 0.f;
    lin[i] = fminf(fmaxf(v, 0.f), 1.f);
  }
  const float d = 6.f / 29.f, k = 1.f / (3.f * d * d);
  float f[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float t = (tab[T_M + 3 * i] * lin[0] + tab[T_M + 3 * i + 1] * lin[1] + tab[T_M + 3 * i + 2] * lin[2]) / tab[T_WHITE + i];
    if (t > 0.00885f) {
      f[i] = powf(t, 1.f / 3.f);
      s.fp[i] = f[i] / (3.f * t);
    } else {
      f[i] = t * k + 4.f / 29.f;
      s.fp[i] = k;
    }
  }
  s.lab[0] = 116.f * f[1] - 16.f;
  s.lab[1] = 500.f * (f[0] - f[1]);
  s.lab[2] = 200.f * (f[1] - f[2]);
  s.hunt[0] = s.lab[0];
  s.hunt[1] = (0.01f * s.lab[0]) * s.lab[1];
  s.hunt[2] = (0.01f * s.lab[0]) * s.lab[2];
}

SRK_DEV float sgnf(float v) { return (v > 0.f) ? 1.f : (v < 0.f ? -1.f : 0.f); }

// one pixel: colour (filtered YCxCz) and features (edge x, edge y, point x, point y) of the reference and the test image ->
// err, and (want_adj) d err / d(test colour) and d err / d(test features)
SRK_DEV float flip_pixel(const float* tab, const float cr[3], const float fr[4], const float ct[3], const float ft[4], bool want_adj,
                         float gcol[3], float gfeat[4]) {
  LabState R, T;
  filtered_to_lab(tab, cr, R);
  filtered_to_lab(tab, ct, T);
  const float dL = R.hunt[0] - T.hunt[0], da = R.hunt[1] - T.hunt[1], db = R.hunt[2] - T.hunt[2];
  const float nrm = sqrtf(da * da + db * db);
  const float h = fabsf(dL) + nrm;
  const float pcc = tab[T_RED], klo = tab[T_RED + 1], khi = tab[T_RED + 2], pt = tab[T_RED + 3];
  const float p = h > 0.f ? powf(h, 0.7f) : 0.f;
  const bool lo = p < pcc;
  const float c = lo ? klo * p : pt + (p - pcc) * khi;
  // features
  const float enr = sqrtf(fr[0] * fr[0] + fr[1] * fr[1]), ent = sqrtf(ft[0] * ft[0] + ft[1] * ft[1]);
  const float pnr = sqrtf(fr[2] * fr[2] + fr[3] * fr[3]), pnt = sqrtf(ft[2] * ft[2] + ft[3] * ft[3]);
  const float de = fabsf(enr - ent), dp = fabsf(pnt - pnr);
  const float fe = fmaxf(de, dp);
  const float fraw = fe > 0.f ? sqrtf(fe * 0.70710678118654752f) : 0.f;
  const float f = fminf(fraw, 1.f);
  const float err = c > 0.f ? powf(c, 1.f - f) : 0.f;
  if (!want_adj) return err;
#pragma unroll
  for (int i = 0; i < 3; ++i) gcol[i] = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) gfeat[i] = 0.f;
  if (!(c > 0.f)) return err;                  // minimum of the error: zero gradient through the base and the exponent
  const float g_c = (1.f - f) * powf(c, -f);
  const float g_f = -err * logf(c);
  // feature term
  if (fe > 0.f && fraw <= 1.f) {
    const float dfe = g_f * 0.5f * fraw / fe;
    const float gde = de > dp ? dfe : (de < dp ? 0.f : 0.5f * dfe);
    const float gdp = dp > de ? dfe : (dp < de ? 0.f : 0.5f * dfe);
    const float g_ent = -sgnf(enr - ent) * gde, g_pnt = sgnf(pnt - pnr) * gdp;
    if (ent > 0.f) {
      gfeat[0] = g_ent * (ft[0] / ent);
      gfeat[1] = g_ent * (ft[1] / ent);
    }
    if (pnt > 0.f) {
      gfeat[2] = g_pnt * (ft[2] / pnt);
      gfeat[3] = g_pnt * (ft[3] / pnt);
    }
  }
  // colour term
  const float g_p = g_c * (lo ? klo : khi);
  const float g_h = g_p * (0.7f * p / h);
  const float gL_h = -sgnf(dL) * g_h;
  const float ga_h = nrm > 0.f ? -(da / nrm) * g_h : 0.f;
  const float gb_h = nrm > 0.f ? -(db / nrm) * g_h : 0.f;
  const float gL = gL_h + (0.01f * T.lab[1]) * ga_h + (0.01f * T.lab[2]) * gb_h;
  const float ga = (0.01f * T.lab[0]) * ga_h, gb = (0.01f * T.lab[0]) * gb_h;
  const float gf[3] = {500.f * ga, 116.f * gL - 500.f * ga + 200.f * gb, -200.f * gb};
  float gx[3], gl[3], gu[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) gx[i] = gf[i] * T.fp[i] / tab[T_WHITE + i];
#pragma unroll
  for (int j = 0; j < 3; ++j) gl[j] = (tab[T_M + j] * gx[0] + tab[T_M + 3 + j] * gx[1] + tab[T_M + 6 + j] * gx[2]) * T.mask[j];
#pragma unroll
  for (int j = 0; j < 3; ++j) gu[j] = (tab[T_MINV + j] * gl[0] + tab[T_MINV + 3 + j] * gl[1] + tab[T_MINV + 6 + j] * gl[2]) * tab[T_WHITE + j];
  gcol[0] = (gu[0] + gu[1] + gu[2]) / 116.f;
  gcol[1] = gu[0] / 500.f;
  gcol[2] = -gu[2] / 200.f;
  return err;
}

__global__ __launch_bounds__(FWD_THREADS) void flip_fwd_kernel(const srk_flip_args a, int tiles_x) {
  __shared__ float tab[SRK_FLIP_TABLE_FLOATS];
  __shared__ float img[3][FE][FE];            // YCxCz of one image, tile + halo
  __shared__ float hb[7][FE][FT];             // horizontal pass: A, RG, BY1, BY2 (CSF), edge, point, gauss (features)
  __shared__ float refv[7][FT * FT];          // the reference image's filtered colour and features
  __shared__ double red[FWD_THREADS / 64];
  const int tid = threadIdx.x;
  const int n = blockIdx.y;
  const int ty0 = (blockIdx.x / tiles_x) * FT, tx0 = (blockIdx.x % tiles_x) * FT;
  const int H = a.H, W = a.W;
  const long long hw = (long long)H * W;
  for (int i = tid; i < SRK_FLIP_TABLE_FLOATS; i += FWD_THREADS) tab[i] = a.table[i];
  double acc = 0.0;
  for (int im = 0; im < 2; ++im) {
    const float* src = (im == 0 ? a.hr : a.sr) + (long long)n * 3 * hw;
    __syncthreads();
    for (int i = tid; i < FE * FE; i += FWD_THREADS) {
      const int ry = i / FE, rx = i - ry * FE;
      const int gy = min(max(ty0 - FR + ry, 0), H - 1), gx = min(max(tx0 - FR + rx, 0), W - 1);
      const long long o = (long long)gy * W + gx;
      srgb_to_ycxcz(tab, src[o], src[o + hw], src[o + 2 * hw], img[0][ry][rx], img[1][ry][rx], img[2][ry][rx]);
    }
    __syncthreads();
    for (int i = tid; i < FE * FT; i += FWD_THREADS) {
      FLIP_RELOAD_TAPS();
      const int ry = i / FT, cx = i - ry * FT;
      float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f, s5 = 0.f, s6 = 0.f;
#pragma unroll 7
      for (int k = 0; k < NCSF; ++k) {
        s0 += tab[T_A + k] * img[0][ry][cx + k];
        s1 += tab[T_RG + k] * img[1][ry][cx + k];
        s2 += tab[T_BY1 + k] * img[2][ry][cx + k];
        s3 += tab[T_BY2 + k] * img[2][ry][cx + k];
      }
#pragma unroll
      for (int k = 0; k < NFEAT; ++k) {
        const float y = img[0][ry][cx + 1 + k];
        s4 += tab[T_EDGE + k] * y;
        s5 += tab[T_POINT + k] * y;
        s6 += tab[T_GAUSS + k] * y;
      }
      hb[0][ry][cx] = s0; hb[1][ry][cx] = s1; hb[2][ry][cx] = s2; hb[3][ry][cx] = s3;
      hb[4][ry][cx] = s4; hb[5][ry][cx] = s5; hb[6][ry][cx] = s6;
    }
    __syncthreads();
    for (int p = tid; p < FT * FT; p += FWD_THREADS) {
      FLIP_RELOAD_TAPS();
      const int py = p / FT, px = p - py * FT;
      float c0 = 0.f, c1 = 0.f, c2 = 0.f, c3 = 0.f, e0 = 0.f, e1 = 0.f, e2 = 0.f, e3 = 0.f;
#pragma unroll 7
      for (int k = 0; k < NCSF; ++k) {
        c0 += tab[T_A + k] * hb[0][py + k][px];
        c1 += tab[T_RG + k] * hb[1][py + k][px];
        c2 += tab[T_BY1 + k] * hb[2][py + k][px];
        c3 += tab[T_BY2 + k] * hb[3][py + k][px];
      }
#pragma unroll
      for (int k = 0; k < NFEAT; ++k) {
        const int r = py + 1 + k;
        e0 += tab[T_GAUSS + k] * hb[4][r][px];        // edge x: derivative along x, Gaussian along y
        e1 += tab[T_EDGE + k] * hb[6][r][px];         // edge y
        e2 += tab[T_GAUSS + k] * hb[5][r][px];        // point x
        e3 += tab[T_POINT + k] * hb[6][r][px];        // point y
      }
      // features of y = (Y + 16) / 116: the detectors' taps sum to zero, so the offset drops out
      const float col[3] = {c0, c1, tab[T_BYW] * c2 + tab[T_BYW + 1] * c3};
      const float feat[4] = {e0 / 116.f, e1 / 116.f, e2 / 116.f, e3 / 116.f};
      if (im == 0) {                              // the reference image: kept in LDS for the test image's pass
#pragma unroll
        for (int c = 0; c < 3; ++c) refv[c][p] = col[c];
#pragma unroll
        for (int c = 0; c < 4; ++c) refv[3 + c][p] = feat[c];
        continue;
      }
      const int gy = ty0 + py, gx = tx0 + px;
      if (gy >= H || gx >= W) continue;
      const float cr[3] = {refv[0][p], refv[1][p], refv[2][p]}, fr[4] = {refv[3][p], refv[4][p], refv[5][p], refv[6][p]};
      float gcol[3], gfeat[4];
      const float e = flip_pixel(tab, cr, fr, col, feat, a.adj != nullptr, gcol, gfeat);
      acc += (double)e;
      const long long o = (long long)gy * W + gx;
      if (a.err) a.err[(long long)n * hw + o] = e;
      if (a.adj) {
        float* d = a.adj + (long long)n * SRK_FLIP_ADJ_CHANNELS * hw + o;
        d[0] = gcol[0]; d[hw] = gcol[1]; d[2 * hw] = gcol[2];
        d[3 * hw] = gfeat[0]; d[4 * hw] = gfeat[1]; d[5 * hw] = gfeat[2]; d[6 * hw] = gfeat[3];
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < FWD_THREADS / 64; ++w) t += red[w];
    a.partial[(long long)n * gridDim.x + blockIdx.x] = t;
  }
}

// weight of source position p in the adjoint of a replicate-padded 1-D filter at target q (extent len, radius r):
// interior targets take tap q - p + r; the first / last position collects every tap that the clamp folded onto it
template <int R>
SRK_DEV float adj_weight(const float* taps, const float* pre, const float* suf, int p, int q, int len) {
  if (len == 1) return pre[2 * R];
  if (q == 0) return p <= R ? pre[R - p] : 0.f;
  if (q == len - 1) {
    const int j = len - 1 - p + R;
    return j <= 2 * R ? suf[j] : 0.f;
  }
  const int k = q - p + R;
  return (k >= 0 && k <= 2 * R) ? taps[k] : 0.f;
}

__global__ __launch_bounds__(BWD_THREADS) void flip_bwd_kernel(const srk_flip_args a, int tiles_x) {
  __shared__ float tab[SRK_FLIP_TABLE_FLOATS];
  __shared__ float pre[7][NCSF], suf[7][NCSF];   // prefix / suffix sums of each tap set (A, RG, BY1, BY2, edge, point, gauss)
  __shared__ float adj[7][FE][FE];
  __shared__ float hb[7][FE][FT];
  const int tid = threadIdx.x;
  const int n = blockIdx.y;
  const int ty0 = (blockIdx.x / tiles_x) * FT, tx0 = (blockIdx.x % tiles_x) * FT;
  const int H = a.H, W = a.W;
  const long long hw = (long long)H * W;
  for (int i = tid; i < SRK_FLIP_TABLE_FLOATS; i += BWD_THREADS) tab[i] = a.table[i];
  const float* ad = a.adj + (long long)n * SRK_FLIP_ADJ_CHANNELS * hw;
  for (int i = tid; i < FE * FE; i += BWD_THREADS) {
    const int ry = i / FE, rx = i - ry * FE;
    const int gy = ty0 - FR + ry, gx = tx0 - FR + rx;
    const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
    const long long o = (long long)gy * W + gx;
#pragma unroll
    for (int c = 0; c < 7; ++c) adj[c][ry][rx] = in ? ad[o + c * hw] : 0.f;
  }
  __syncthreads();
  if (tid < 7) {
    const int off[7] = {T_A, T_RG, T_BY1, T_BY2, T_EDGE, T_POINT, T_GAUSS};
    const int len = tid < 4 ? NCSF : NFEAT;
    float s = 0.f;
    for (int k = 0; k < len; ++k) { s += tab[off[tid] + k]; pre[tid][k] = s; }
    s = 0.f;
    for (int k = len - 1; k >= 0; --k) { s += tab[off[tid] + k]; suf[tid][k] = s; }
  }
  __syncthreads();
  // horizontal adjoint: region rows x tile columns
  for (int i = tid; i < FE * FT; i += BWD_THREADS) {
    FLIP_RELOAD_TAPS();
    const int ry = i / FT, cx = i - ry * FT;
    const int q = tx0 + cx;
    float s[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (q < W) {
      if (q > 0 && q < W - 1) {                      // interior target: the taps, reversed
#pragma unroll
        for (int k = 0; k < NCSF; ++k) {
          s[0] += tab[T_A + 2 * FR - k] * adj[0][ry][cx + k];
          s[1] += tab[T_RG + 2 * FR - k] * adj[1][ry][cx + k];
          s[2] += tab[T_BY1 + 2 * FR - k] * adj[2][ry][cx + k];
          s[3] += tab[T_BY2 + 2 * FR - k] * adj[2][ry][cx + k];
        }
#pragma unroll
        for (int k = 0; k < NFEAT; ++k) {
          const int c = cx + 1 + k;
          s[4] += tab[T_EDGE + 2 * FRF - k] * adj[3][ry][c] + tab[T_POINT + 2 * FRF - k] * adj[5][ry][c];
          s[5] += tab[T_GAUSS + 2 * FRF - k] * adj[4][ry][c];
          s[6] += tab[T_GAUSS + 2 * FRF - k] * adj[6][ry][c];
        }
      } else {                                       // first / last column: folded taps
        for (int k = 0; k < NCSF; ++k) {
          const int p = q - FR + k;
          if (p < 0 || p >= W) continue;
          s[0] += adj_weight<FR>(tab + T_A, pre[0], suf[0], p, q, W) * adj[0][ry][cx + k];
          s[1] += adj_weight<FR>(tab + T_RG, pre[1], suf[1], p, q, W) * adj[1][ry][cx + k];
          s[2] += adj_weight<FR>(tab + T_BY1, pre[2], suf[2], p, q, W) * adj[2][ry][cx + k];
          s[3] += adj_weight<FR>(tab + T_BY2, pre[3], suf[3], p, q, W) * adj[2][ry][cx + k];
        }
        for (int k = 0; k < NFEAT; ++k) {
          const int p = q - FRF + k, c = cx + 1 + k;
          if (p < 0 || p >= W) continue;
          s[4] += adj_weight<FRF>(tab + T_EDGE, pre[4], suf[4], p, q, W) * adj[3][ry][c]
                + adj_weight<FRF>(tab + T_POINT, pre[5], suf[5], p, q, W) * adj[5][ry][c];
          const float wg = adj_weight<FRF>(tab + T_GAUSS, pre[6], suf[6], p, q, W);
          s[5] += wg * adj[4][ry][c];
          s[6] += wg * adj[6][ry][c];
        }
      }
    }
#pragma unroll
    for (int c = 0; c < 7; ++c) hb[c][ry][cx] = s[c];
  }
  __syncthreads();
  const float* sr = a.sr + (long long)n * 3 * hw;
  float* gr = a.grad + (long long)n * 3 * hw;
  const float gs = *a.gout * a.scale;
  for (int i = tid; i < FT * FT; i += BWD_THREADS) {
    FLIP_RELOAD_TAPS();
    const int py = i / FT, px = i - py * FT;
    const int q = ty0 + py, gx = tx0 + px;
    if (q >= H || gx >= W) continue;
    float gy0 = 0.f, gcx = 0.f, gb1 = 0.f, gb2 = 0.f, gfe = 0.f;
    if (q > 0 && q < H - 1) {
#pragma unroll
      for (int k = 0; k < NCSF; ++k) {
        gy0 += tab[T_A + 2 * FR - k] * hb[0][py + k][px];
        gcx += tab[T_RG + 2 * FR - k] * hb[1][py + k][px];
        gb1 += tab[T_BY1 + 2 * FR - k] * hb[2][py + k][px];
        gb2 += tab[T_BY2 + 2 * FR - k] * hb[3][py + k][px];
      }
#pragma unroll
      for (int k = 0; k < NFEAT; ++k) {
        const int r = py + 1 + k;
        gfe += tab[T_GAUSS + 2 * FRF - k] * hb[4][r][px] + tab[T_EDGE + 2 * FRF - k] * hb[5][r][px]
             + tab[T_POINT + 2 * FRF - k] * hb[6][r][px];
      }
    } else {
      for (int k = 0; k < NCSF; ++k) {
        const int p = q - FR + k;
        if (p < 0 || p >= H) continue;
        gy0 += adj_weight<FR>(tab + T_A, pre[0], suf[0], p, q, H) * hb[0][py + k][px];
        gcx += adj_weight<FR>(tab + T_RG, pre[1], suf[1], p, q, H) * hb[1][py + k][px];
        gb1 += adj_weight<FR>(tab + T_BY1, pre[2], suf[2], p, q, H) * hb[2][py + k][px];
        gb2 += adj_weight<FR>(tab + T_BY2, pre[3], suf[3], p, q, H) * hb[3][py + k][px];
      }
      for (int k = 0; k < NFEAT; ++k) {
        const int p = q - FRF + k, r = py + 1 + k;
        if (p < 0 || p >= H) continue;
        gfe += adj_weight<FRF>(tab + T_GAUSS, pre[6], suf[6], p, q, H) * hb[4][r][px]
             + adj_weight<FRF>(tab + T_EDGE, pre[4], suf[4], p, q, H) * hb[5][r][px]
             + adj_weight<FRF>(tab + T_POINT, pre[5], suf[5], p, q, H) * hb[6][r][px];
      }
    }
    const float gY = gy0 + gfe / 116.f;
    const float gCz = tab[T_BYW] * gb1 + tab[T_BYW + 1] * gb2;
    // YCxCz <- XYZ / white
    const float gX[3] = {500.f * gcx / tab[T_WHITE], (116.f * gY - 500.f * gcx + 200.f * gCz) / tab[T_WHITE + 1],
                         -200.f * gCz / tab[T_WHITE + 2]};
    const long long o = (long long)q * W + gx;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const float gl = tab[T_M + j] * gX[0] + tab[T_M + 3 + j] * gX[1] + tab[T_M + 6 + j] * gX[2];
      const float x = sr[o + j * hw];
      float d = 0.f;
      if (x >= 0.f && x <= 1.f) d = x > 0.04045f ? (2.4f / 1.055f) * powf((x + 0.055f) / 1.055f, 1.4f) : 1.f / 12.92f;
      gr[o + j * hw] = (gl * d) * gs;
    }
  }
}

}  // namespace

extern "C" int srk_flip_blocks(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  return N * ((H + FT - 1) / FT) * ((W + FT - 1) / FT);
}

static int flip_check(const srk_flip_args* a, const char* who) {
  SRK_CHECK_ARG(a && a->sr && a->table, "%s: null pointer", who);
  SRK_CHECK_ARG(a->N > 0 && a->N <= 65535 && a->H > 0 && a->W > 0, "%s: bad sizes N=%d H=%d W=%d", who, a->N, a->H, a->W);
  SRK_CHECK_ARG((long long)((a->H + FT - 1) / FT) * ((a->W + FT - 1) / FT) < (1LL << 31), "%s: image too large", who);
  return 0;
}

extern "C" int srk_flip_fwd(const srk_flip_args* a, srk_stream_t stream) {
  if (int rc = flip_check(a, "srk_flip_fwd")) return rc;
  SRK_CHECK_ARG(a->hr && a->partial, "srk_flip_fwd: null pointer");
  const int tx = (a->W + FT - 1) / FT, ty = (a->H + FT - 1) / FT;
  hipLaunchKernelGGL(flip_fwd_kernel, dim3((unsigned)(tx * ty), (unsigned)a->N), dim3(FWD_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), *a, tx);
  SRK_LAUNCH_CHECK();
  return 0;
}

extern "C" int srk_flip_bwd(const srk_flip_args* a, srk_stream_t stream) {
  if (int rc = flip_check(a, "srk_flip_bwd")) return rc;
  SRK_CHECK_ARG(a->adj && a->gout && a->grad, "srk_flip_bwd: null pointer");
  const int tx = (a->W + FT - 1) / FT, ty = (a->H + FT - 1) / FT;
  hipLaunchKernelGGL(flip_bwd_kernel, dim3((unsigned)(tx * ty), (unsigned)a->N), dim3(BWD_THREADS), 0,
                     reinterpret_cast<hipStream_t>(stream), *a, tx);
  SRK_LAUNCH_CHECK();
  return 0;
}

extern "C" int srk_flip_mean(const double* partial, int nb, long long n, float* out, srk_stream_t stream) {
  return srk_l1_loss_mean(partial, nb, n, out, stream);         // the same fixed-order mean of per-workgroup partial sums
}
