// SSIM loss, 1 - SSIM(clamp(sr, 0, 1), hr) with piq.ssim's defaults (piq.SSIMLoss; the metric twin is ssim_kernel in data.hip):
// include/srk.h "SSIM loss", sr_amd/ssim_loss.py.  The constants, the moment passes and the map value are ssim_core.h's.  One
// (image, channel) plane at a time; "pooled" pixels are the f x f means.
//   ssim_loss_fwd_kernel       one workgroup per (plane, 16x16 tile of the valid SSIM map): clamp sr, pool both images into LDS
//                              (26x26 pooled pixels), the moments and the SSIM value per position, and the tile's sum as one
//                              double in its own slot (no atomics: bitwise repeatable).
//   ssim_loss_finalize_kernel  one workgroup: the fixed-order fp64 sum of every tile, loss = 1 - sum / (N C (Hp-10)(Wp-10)).
//   ssim_loss_bwd_kernel       one workgroup per (plane, 16x32 tile of pooled sr pixels): recomputes the moments of the 26x42 map
//                              positions whose windows touch the tile from a 36x52 haloed tile of both images, the adjoints
//                              a = dS/d(G*xx), b = dS/d(G*xy) and m = dS/d(mu_x) (total), their transposed separable filter
//                              (the same 11 taps: G is symmetric), grad = (G^T*m + 2x' G^T*a + y' G^T*b) * (-*gout / count / f^2)
//                              spread over the f x f block under the clamp's mask.
// Recompute or saved maps, by HBM traffic, in bytes per HR pixel of a plane (f = 1; halo re-reads are served by L2 and not counted):
//   recompute (chosen):  forward reads sr, hr (8 B), writes 8 B per 256 positions;  backward reads sr, hr (8 B), writes grad (4 B)
//                        -> 8 B + 12 B = 20 B, and nothing is kept between forward and backward;
//   saved maps:          forward reads 8 B and writes m, a, b (12 B);  backward reads m, a, b (12 B), sr and hr (8 B: the 2x and y
//                        factors and the clamp mask), writes 4 B  -> 20 B + 24 B = 44 B, and 12 B per pixel stay allocated.
// The recompute costs the backward about 3.7x the forward's filter arithmetic per pixel (the 36x52 region over the 16x32 tile).
#include "ssim_core.h"

namespace {

using ssim::HALO;
constexpr int SL_THREADS = 256;
constexpr int FT = 16;                                // forward tile edge, map positions
constexpr int BTY = 16, BTX = 32;                     // backward tile, pooled pixels
constexpr int FIN_THREADS = 1024;
static_assert(FT * FT == SL_THREADS, "forward: one thread per map position");

// RY x RX pooled pixels of one plane of both images, top-left pooled pixel (oy, ox): x' = mean of clamp(sr, 0, 1) - 1/2, y' = mean of
// hr - 1/2 over the f x f block; zero outside [0, Hp) x [0, Wp) (such pixels only reach map positions that are not valid)
template <int RY, int RX>
SRK_DEV void load_region(const float* xs, const float* ys, int W, int f, int oy, int ox, int Hp, int Wp, float (*X)[RX + 1],
                         float (*Y)[RX + 1]) {
  const float inv = 1.0f / (float)(f * f);
  for (int i = threadIdx.x; i < RY * RX; i += SL_THREADS) {
    const int r = i / RX, c = i - r * RX;
    const int py = oy + r, px = ox + c;
    float vx = 0.f, vy = 0.f;
    if (py >= 0 && py < Hp && px >= 0 && px < Wp) {
      for (int dy = 0; dy < f; ++dy)
        for (int dx = 0; dx < f; ++dx) {
          const size_t o = (size_t)(py * f + dy) * W + (size_t)(px * f + dx);
          vx += fminf(fmaxf(xs[o], 0.f), 1.f);
          vy += ys[o];
        }
      vx = vx * inv - ssim::SHIFT;
      vy = vy * inv - ssim::SHIFT;
    }
    X[r][c] = vx;
    Y[r][c] = vy;
  }
}

__global__ __launch_bounds__(SL_THREADS) void ssim_loss_fwd_kernel(const srk_ssim_loss_args a, int f, int Hp, int Wp, int tiles_x,
                                                                    int tiles_pp) {
  constexpr int R = FT + HALO;
  __shared__ float X[R][R + 1], Y[R][R + 1];
  __shared__ float Hm[5][R][FT];
  __shared__ double red[SL_THREADS / 64];
  const int tid = threadIdx.x;
  const int plane = blockIdx.x / tiles_pp, t = blockIdx.x - plane * tiles_pp;
  const int y0 = (t / tiles_x) * FT, x0 = (t % tiles_x) * FT;
  const size_t po = (size_t)plane * a.H * a.W;
  load_region<R, R>(a.sr + po, a.hr + po, a.W, f, y0, x0, Hp, Wp, X, Y);
  __syncthreads();
  ssim::moments_rows<SL_THREADS, R, R>(X, Y, Hm);
  __syncthreads();
  const int r = tid / FT, c = tid % FT;
  double acc = 0.0;
  if (y0 + r + HALO < Hp && x0 + c + HALO < Wp) {
    float m[5];
    ssim::moments_at<R, FT>(Hm, r, c, m);
    acc = (double)ssim::map_values(m).ss;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) a.partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// thread-strided over the tiles (eight loads in flight, added in index order), a fixed shuffle tree, then the 16 waves in order
__global__ __launch_bounds__(FIN_THREADS) void ssim_loss_finalize_kernel(const srk_ssim_loss_args a, long long tiles, double count) {
  __shared__ double red[FIN_THREADS / 64];
  double t = 0.0;
  long long i = threadIdx.x;
  for (; i + FIN_THREADS * 7LL < tiles; i += FIN_THREADS * 8LL) {
    double v[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = a.partial[i + (long long)FIN_THREADS * k];
#pragma unroll
    for (int k = 0; k < 8; ++k) t += v[k];
  }
  for (; i < tiles; i += FIN_THREADS) t += a.partial[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < FIN_THREADS / 64; ++w) s += red[w];
    *a.loss = (float)(1.0 - s / count);
  }
}

__global__ __launch_bounds__(SL_THREADS) void ssim_loss_bwd_kernel(const srk_ssim_loss_args a, int f, int Hp, int Wp, int tiles_x,
                                                                    int tiles_pp, float scale) {
  constexpr int SY = BTY + HALO, SX = BTX + HALO;                // map positions whose windows touch the tile
  constexpr int RY = SY + HALO, RX = SX + HALO;                  // pooled pixels those positions read
  __shared__ float X[RY][RX + 1], Y[RY][RX + 1];
  __shared__ float Hm[5][RY][SX];
  __shared__ float adj[3][SY][SX + 1];                           // m, a, b of the map positions (0 where not valid)
  float (*Ha)[SY][BTX] = reinterpret_cast<float (*)[SY][BTX]>(&Hm[0][0][0]);   // their horizontal pass: reuses Hm once it is consumed
  static_assert(3 * SY * BTX <= 5 * RY * SX, "Ha fits in Hm");
  const int tid = threadIdx.x;
  const int plane = blockIdx.x / tiles_pp, t = blockIdx.x - plane * tiles_pp;
  const int i0 = (t / tiles_x) * BTY, j0 = (t % tiles_x) * BTX;  // the tile's first pooled pixel
  const size_t po = (size_t)plane * a.H * a.W;
  // region pixel (r, c) is pooled pixel (i0 - 10 + r, j0 - 10 + c); map position (r, c) of the tile is (i0 - 10 + r, j0 - 10 + c) too
  load_region<RY, RX>(a.sr + po, a.hr + po, a.W, f, i0 - HALO, j0 - HALO, Hp, Wp, X, Y);
  __syncthreads();
  ssim::moments_rows<SL_THREADS, RY, RX>(X, Y, Hm);
  __syncthreads();
  for (int i = tid; i < SY * SX; i += SL_THREADS) {
    const int r = i / SX, c = i - r * SX;
    const int pi = i0 - HALO + r, pj = j0 - HALO + c;
    float gm = 0.f, ga = 0.f, gb = 0.f;
    if (pi >= 0 && pi + HALO < Hp && pj >= 0 && pj + HALO < Wp) {
      float m[5];
      ssim::moments_at<RY, SX>(Hm, r, c, m);
      const float ux = m[0], uy = m[1];                          // the shifted means: what s_xx, s_xy see
      const float mx = ux + ssim::SHIFT, my = uy + ssim::SHIFT;
      const float sxx = m[2] - ux * ux, syy = m[3] - uy * uy, sxy = m[4] - ux * uy;
      const float ib1 = 1.f / (mx * mx + my * my + ssim::C1), ib2 = 1.f / (sxx + syy + ssim::C2);
      const float l = (2.f * mx * my + ssim::C1) * ib1, cs = (2.f * sxy + ssim::C2) * ib2;      // S = l * cs
      ga = -(l * cs) * ib2;                                      // through sigma_xx
      gb = 2.f * l * ib2;                                        // through sigma_xy
      // d S / d (G*x') in full: 2 mu_y cs / B1 - 2 mu_x S / B1 - u_y b - 2 u_x a, grouped so that each difference is taken once
      gm = 2.f * cs * ib1 * (my - mx * l) + 2.f * l * ib2 * (ux * cs - uy);
    }
    adj[0][r][c] = gm;
    adj[1][r][c] = ga;
    adj[2][r][c] = gb;
  }
  __syncthreads();                                               // adj complete, Hm consumed
  // grad(q) = sum_k G[k] adj(q - k), k = 0..10: pixel column c of the tile reads map columns c .. c + 10 of the tile (G symmetric)
  for (int i = tid; i < SY * BTX; i += SL_THREADS) {
    const int r = i / BTX, c = i - r * BTX;
    float v[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < ssim::K; ++k) {
      const float w = ssim::kG[k];
#pragma unroll
      for (int q = 0; q < 3; ++q) v[q] += w * adj[q][r][c + k];
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) Ha[q][r][c] = v[q];
  }
  __syncthreads();
  const float gs = *a.gout * scale;
  const float* sr = a.sr + po;
  float* gr = a.grad + po;
  for (int i = tid; i < BTY * BTX; i += SL_THREADS) {
    const int r = i / BTX, c = i - r * BTX;
    const int pi = i0 + r, pj = j0 + c;
    if (pi >= Hp || pj >= Wp) continue;
    float v[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < ssim::K; ++k) {
      const float w = ssim::kG[k];
#pragma unroll
      for (int q = 0; q < 3; ++q) v[q] += w * Ha[q][r + k][c];
    }
    const float x = X[r + HALO][c + HALO], y = Y[r + HALO][c + HALO];            // x', y': the shifted pixels
    const float g = (v[0] + 2.f * x * v[1] + y * v[2]) * gs;
    for (int dy = 0; dy < f; ++dy)
      for (int dx = 0; dx < f; ++dx) {
        const size_t o = (size_t)(pi * f + dy) * a.W + (size_t)(pj * f + dx);
        const float s = sr[o];
        gr[o] = (s >= 0.f && s <= 1.f) ? g : 0.f;                // the clamp passes the gradient on [0, 1]
      }
  }
}

struct SlGeom {
  int f, Hp, Wp;
  int ftx, fty, btx, bty;          // forward / backward tiles per plane
  long long planes;
};

}  // namespace

// Python's round(min(H, W) / 256) (halves to the even neighbour), at least 1
static int sl_pool(int H, int W) {
  const int m = H < W ? H : W, q = m / 256, r = m % 256;
  const int f = q + ((r > 128 || (r == 128 && (q & 1))) ? 1 : 0);
  return f < 1 ? 1 : f;
}

static int sl_geometry(int N, int C, int H, int W, SlGeom* g) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0) return -1;
  g->f = sl_pool(H, W);
  g->Hp = H / g->f;
  g->Wp = W / g->f;
  if (g->Hp < ssim::K || g->Wp < ssim::K) return -1;
  g->ftx = (g->Wp - HALO + FT - 1) / FT;
  g->fty = (g->Hp - HALO + FT - 1) / FT;
  g->btx = (g->Wp + BTX - 1) / BTX;
  g->bty = (g->Hp + BTY - 1) / BTY;
  g->planes = (long long)N * C;
  // one grid dimension carries (plane, tile): both launches must fit it
  const long long lim = (1LL << 31) - 1;
  if (g->planes > lim / ((long long)g->ftx * g->fty) || g->planes > lim / ((long long)g->btx * g->bty)) return -1;
  return 0;
}

extern "C" int srk_ssim_loss_tiles(int N, int C, int H, int W) {
  SlGeom g;
  if (sl_geometry(N, C, H, W, &g)) return -1;
  return (int)(g.planes * g.ftx * g.fty);
}

static int sl_check(const srk_ssim_loss_args* a, const char* who, SlGeom* g) {
  SRK_CHECK_ARG(a && a->sr, "%s: null pointer", who);
  SRK_CHECK_ARG(a->N > 0 && a->C > 0 && a->H > 0 && a->W > 0, "%s: bad sizes N=%d C=%d H=%d W=%d", who, a->N, a->C, a->H, a->W);
  SRK_CHECK_ARG(sl_geometry(a->N, a->C, a->H, a->W, g) == 0,
                "%s: %dx%dx%dx%d refused (the pooled image must be at least 11x11, and planes x tiles must stay below 2^31)", who, a->N,
                a->C, a->H, a->W);
  return 0;
}

extern "C" int srk_ssim_loss_fwd(const srk_ssim_loss_args* a, srk_stream_t stream) {
  SlGeom g;
  if (int rc = sl_check(a, "srk_ssim_loss_fwd", &g)) return rc;
  SRK_CHECK_ARG(a->hr && a->partial, "srk_ssim_loss_fwd: null pointer");
  const int tpp = g.ftx * g.fty;
  hipLaunchKernelGGL(ssim_loss_fwd_kernel, dim3((unsigned)(g.planes * tpp)), dim3(SL_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                     *a, g.f, g.Hp, g.Wp, g.ftx, tpp);
  SRK_LAUNCH_CHECK();
  return 0;
}

extern "C" int srk_ssim_loss_finalize(const srk_ssim_loss_args* a, srk_stream_t stream) {
  SlGeom g;
  if (int rc = sl_check(a, "srk_ssim_loss_finalize", &g)) return rc;
  SRK_CHECK_ARG(a->partial && a->loss, "srk_ssim_loss_finalize: null pointer");
  const double count = (double)g.planes * (double)(g.Hp - HALO) * (double)(g.Wp - HALO);
  hipLaunchKernelGGL(ssim_loss_finalize_kernel, dim3(1), dim3(FIN_THREADS), 0, reinterpret_cast<hipStream_t>(stream), *a,
                     g.planes * g.ftx * g.fty, count);
  SRK_LAUNCH_CHECK();
  return 0;
}

extern "C" int srk_ssim_loss_bwd(const srk_ssim_loss_args* a, srk_stream_t stream) {
  SlGeom g;
  if (int rc = sl_check(a, "srk_ssim_loss_bwd", &g)) return rc;
  SRK_CHECK_ARG(a->hr && a->gout && a->grad, "srk_ssim_loss_bwd: null pointer");
  const int tpp = g.btx * g.bty;
  const double count = (double)g.planes * (double)(g.Hp - HALO) * (double)(g.Wp - HALO);
  const float scale = (float)(-1.0 / (count * (double)g.f * (double)g.f));
  hipLaunchKernelGGL(ssim_loss_bwd_kernel, dim3((unsigned)(g.planes * tpp)), dim3(SL_THREADS), 0, reinterpret_cast<hipStream_t>(stream),
                     *a, g.f, g.Hp, g.Wp, g.btx, tpp, scale);
  SRK_LAUNCH_CHECK();
  return 0;
}
