// MS-SSIM loss, 1 - MS-SSIM(clamp(sr, 0, 1), hr) with piq.multi_scale_ssim's defaults (piq.MultiScaleSSIMLoss; the metric twin is
// ms_ssim.hip, the single-scale loss ssim_loss.hip): include/srk.h "MS-SSIM loss", sr_amd/ms_ssim_loss.py.  The constants, the moment
// passes, the map values and the levels' geometry are ssim_core.h's.  One (image, channel) plane at a time; level 0 is
// (clamp(sr), hr), level k > 0 is level k-1 replicate-padded by p = max(H % 2, W % 2) on the top and left and averaged 2x2 / stride 2.
//   ml_pool_kernel      level k of both images from level k-1 (ms_pool_kernel's arithmetic); the clamp of sr is folded into the reads
//                       of level 0, so no clamped copy of the image exists; one launch per level, levels 1-4 in the caller's workspace
//   ml_maps_kernel      one launch for all five levels: one workgroup per (plane, 16x16 tile of a level's valid map) stages the tile +
//                       10-pixel halo of both images in LDS (level 0: sr clamped on load) and writes (sum ss, sum cs) over its tile
//                       to a fixed slot
//   ml_final_kernel     one workgroup, one wave per plane at a time: the plane's partials summed per level in a fixed order, the level
//                       means m_k (cs for k < 4, ss for k = 4), v = prod m_k^w_k (0 if any m_k <= 0), loss = 1 - mean v, and the
//                       table[plane][k] = w_k v / (m_k count_k planes) the backward scales by (all 0 for a plane with any m_k <= 0:
//                       piq's relu(m)^w has an infinite slope there and autograd returns NaN)
//   ml_bwd_kernel       one launch per level, coarse to fine; one workgroup per (plane, 16x32 pixel tile of level k) recomputes the
//                       moments of the 26x42 map positions whose windows touch the tile from a 36x52 haloed tile of the saved pyramid
//                       (ssim_loss_bwd_kernel's scheme), the adjoints of cs (levels 0-3) or ss (level 4), their transposed separable
//                       filter, scales by the plane's negated table entry, GATHERS 1/4 of the parent pixel's already-final
//                       gradient of level k+1 (parent ((i + p) / 2, (j + p) / 2), none if that lies outside level k+1: the row or
//                       column the pooling's floor drops; twice the share on row / column 0 when p = 1: the replicated pad) and
//                       writes level k's gradient once.  Level 0 multiplies the sum by *gout, applies the clamp's mask and writes grad.
// No atomics anywhere and fixed-order sums: bit-reproducible.  (plane, tile) share blockIdx.x in every launch.  fp32 maps (like piq),
// double sums.  The backward is bound, like the SSIM loss's, by LDS reads of the 11-tap passes (one dword per multiply-add), not by HBM.
#include <math.h>
#include "ssim_core.h"

namespace {

using ssim::HALO;
constexpr int ML_LEVELS = ssim::LEVELS;
constexpr int ML_THREADS = 256;
constexpr int ML_FT = ssim::TILE;                      // forward tile edge, map positions
constexpr int ML_BTY = 16, ML_BTX = 32;                // backward tile, pixels of the level
constexpr int ML_FIN_THREADS = 512;
static_assert(ML_FT * ML_FT == ML_THREADS, "maps: one thread per map position");
const double kMlWeight[ML_LEVELS] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};      // piq.multi_scale_ssim's scale_weights

struct MlMapsArgs {
  ssim::Level lv[ML_LEVELS];
  int tiles;                      // map tiles per plane, all levels
  double* partials;               // [planes][tiles][2]: (sum ss, sum cs)
};

struct MlFinalArgs {
  const double* partials;
  int first[ML_LEVELS + 1];       // first[ML_LEVELS] = tiles per plane
  float count[ML_LEVELS];         // valid map positions per plane, per level (exact in fp32: < 2^24 is checked)
  float weight[ML_LEVELS];
  int planes;
  float* table;                   // [planes][ML_LEVELS]
  float* loss;
};

struct MlBwdArgs {
  const float* x;                 // level k of both images
  const float* y;
  int H, W;
  const float* table;             // [planes][ML_LEVELS]
  int k;
  const float* gout;
  const float* gpar;              // gradient of level k + 1 [planes][Hn][Wn]; null at the last level
  int Hn, Wn, p;                  // level k + 1's size and the pad that built it
  float* gdst;                    // gradient of level k [planes][H][W]
  int tiles_x, tiles_pp;
  int level0;                     // clamp x on load, mask the gradient on store
};

__global__ __launch_bounds__(ML_THREADS) void ml_pool_kernel(const float* __restrict__ xs, const float* __restrict__ ys, int Hs, int Ws,
                                                             float* __restrict__ xd, float* __restrict__ yd, int Hd, int Wd, int p,
                                                             int blocks_pp, int clampx) {
  const int plane = blockIdx.x / blocks_pp;
  const int q = (blockIdx.x - plane * blocks_pp) * ML_THREADS + threadIdx.x;
  if (q >= Hd * Wd) return;
  const int i = q / Wd, j = q - i * Wd;
  // padded row 2i (2i + 1) is source row max(2i - p, 0) (2i + 1 - p <= Hs - 1 since Hd = (Hs + p) / 2); columns alike
  const int r0 = max(2 * i - p, 0), r1 = 2 * i + 1 - p;
  const int c0 = max(2 * j - p, 0), c1 = 2 * j + 1 - p;
  const size_t so = (size_t)plane * Hs * Ws, d = (size_t)plane * Hd * Wd + q;
  const float* a = xs + so;
  const float* b = ys + so;
  float a00 = a[r0 * Ws + c0], a01 = a[r0 * Ws + c1], a10 = a[r1 * Ws + c0], a11 = a[r1 * Ws + c1];
  if (clampx) {
    a00 = fminf(fmaxf(a00, 0.f), 1.f); a01 = fminf(fmaxf(a01, 0.f), 1.f);
    a10 = fminf(fmaxf(a10, 0.f), 1.f); a11 = fminf(fmaxf(a11, 0.f), 1.f);
  }
  xd[d] = 0.25f * (((a00 + a01) + a10) + a11);
  yd[d] = 0.25f * (((b[r0 * Ws + c0] + b[r0 * Ws + c1]) + b[r1 * Ws + c0]) + b[r1 * Ws + c1]);
}

// RY x RX pixels of one plane of both images of a level, top-left pixel (oy, ox), as x' = x - 1/2, y' = y - 1/2 (x clamped to
// [0, 1] first when `clampx`); zero outside [0, H) x [0, W) (such pixels only reach map positions that are not valid)
template <int RY, int RX>
SRK_DEV void ml_load_region(const float* xs, const float* ys, int H, int W, int oy, int ox, int clampx, float (*X)[RX + 1],
                            float (*Y)[RX + 1]) {
  for (int i = threadIdx.x; i < RY * RX; i += ML_THREADS) {
    const int r = i / RX, c = i - r * RX;
    const int py = oy + r, px = ox + c;
    float vx = 0.f, vy = 0.f;
    if (py >= 0 && py < H && px >= 0 && px < W) {
      const size_t o = (size_t)py * W + px;
      vx = xs[o];
      if (clampx) vx = fminf(fmaxf(vx, 0.f), 1.f);
      vx -= ssim::SHIFT;
      vy = ys[o] - ssim::SHIFT;
    }
    X[r][c] = vx;
    Y[r][c] = vy;
  }
}

__global__ __launch_bounds__(ML_THREADS) void ml_maps_kernel(const MlMapsArgs a) {
  constexpr int R = ML_FT + HALO;
  __shared__ float X[R][R + 1], Y[R][R + 1];
  __shared__ float Hm[5][R][ML_FT];
  __shared__ double red[ML_THREADS / 64][2];
  const int tid = threadIdx.x;
  const int plane = blockIdx.x / a.tiles, t = blockIdx.x - plane * a.tiles;
  // this tile's level: uniform selects over the table (no dynamic index into the kernel arguments)
  const float* xs = a.lv[0].x;
  const float* ys = a.lv[0].y;
  int H = a.lv[0].H, W = a.lv[0].W, tilesX = a.lv[0].tilesX, first = 0, level0 = 1;
#pragma unroll
  for (int k = 1; k < ML_LEVELS; ++k)
    if (t >= a.lv[k].first) { xs = a.lv[k].x; ys = a.lv[k].y; H = a.lv[k].H; W = a.lv[k].W; tilesX = a.lv[k].tilesX; first = a.lv[k].first; level0 = 0; }
  const int lt = t - first;
  const int y0 = (lt / tilesX) * ML_FT, x0 = (lt % tilesX) * ML_FT;
  const size_t po = (size_t)plane * H * W;
  ml_load_region<R, R>(xs + po, ys + po, H, W, y0, x0, level0, X, Y);
  __syncthreads();
  ssim::moments_rows<ML_THREADS, R, R>(X, Y, Hm);
  __syncthreads();
  const int r = tid / ML_FT, c = tid % ML_FT;
  // cs before ss: declared the other way round the two sums swap registers behind map_values; the order is kept so the kernel's
  // instructions stay as they were
  double cs_acc = 0.0, ss_acc = 0.0;
  if (y0 + r + HALO < H && x0 + c + HALO < W) {
    float m[5];
    ssim::moments_at<R, ML_FT>(Hm, r, c, m);
    const ssim::MapValues v = ssim::map_values(m);
    ss_acc = (double)v.ss;
    cs_acc = (double)v.cs;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    ss_acc += __shfl_down(ss_acc, off, 64);
    cs_acc += __shfl_down(cs_acc, off, 64);
  }
  if ((tid & 63) == 0) { red[tid >> 6][0] = ss_acc; red[tid >> 6][1] = cs_acc; }
  __syncthreads();
  if (tid == 0) {
    double2 v;
    v.x = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
    v.y = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
    reinterpret_cast<double2*>(a.partials)[blockIdx.x] = v;
  }
}

__global__ __launch_bounds__(ML_FIN_THREADS) void ml_final_kernel(const MlFinalArgs a) {
  __shared__ double red[ML_FIN_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int T = a.first[ML_LEVELS];
  double wsum = 0.0;                                     // lane 0: this wave's planes, in plane order
  for (int plane = wave; plane < a.planes; plane += ML_FIN_THREADS / 64) {
    const double2* p = reinterpret_cast<const double2*>(a.partials) + (size_t)plane * T;
    double bin[ML_LEVELS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    // lane-strided with eight loads in flight per lane, added in index order, then a fixed shuffle tree (ms_final_kernel).  A slot
    // past the plane's last tile is loaded as zero and lands in no level.
    for (int i = lane; i < T; i += 64 * 8) {
      double2 v[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = i + 64 * k < T ? p[i + 64 * k] : make_double2(0.0, 0.0);
#pragma unroll
      for (int k = 0; k < 8; ++k) ssim::bin(a, i + 64 * k, v[k], bin);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
      for (int k = 0; k < ML_LEVELS; ++k) bin[k] += __shfl_down(bin[k], off, 64);
    // lane k < 5 takes level k's mean m_k and factor m_k^w_k; every lane multiplies them in level order
    double tot = 0.0, cnt = 1.0, wt = 0.0;
#pragma unroll
    for (int k = 0; k < ML_LEVELS; ++k) {
      const double b = __shfl(bin[k], 0, 64);
      if (lane == k) { tot = b; cnt = (double)a.count[k]; wt = (double)a.weight[k]; }
    }
    const double m = lane < ML_LEVELS ? tot / cnt : 1.0;
    const double f = lane < ML_LEVELS ? pow(fmax(m, 0.0), wt) : 1.0;
    double v = 1.0;
    bool positive = true;
#pragma unroll
    for (int k = 0; k < ML_LEVELS; ++k) {
      v *= __shfl(f, k, 64);
      positive = positive && (__shfl(m, k, 64) > 0.0);
    }
    if (!positive) v = 0.0;
    // d v / d m_k = w_k v / m_k, spread over the level's map positions and the planes; zero for the whole plane when v = 0
    if (lane < ML_LEVELS) a.table[(size_t)plane * ML_LEVELS + lane] = positive ? (float)(wt * v / (m * cnt * (double)a.planes)) : 0.f;
    if (lane == 0) wsum += v;
  }
  if (lane == 0) red[wave] = wsum;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < ML_FIN_THREADS / 64; ++w) s += red[w];
    *a.loss = (float)(1.0 - s / (double)a.planes);     // every image has C planes: the mean over C, then over N
  }
}

// SS: the adjoint of the SSIM map (last level); otherwise of the contrast-structure map
template <bool SS>
__global__ __launch_bounds__(ML_THREADS) void ml_bwd_kernel(const MlBwdArgs a) {
  constexpr int SY = ML_BTY + HALO, SX = ML_BTX + HALO;          // map positions whose windows touch the tile
  constexpr int RY = SY + HALO, RX = SX + HALO;                  // pixels those positions read
  __shared__ float X[RY][RX + 1], Y[RY][RX + 1];
  __shared__ float Hm[5][RY][SX];
  __shared__ float adj[3][SY][SX + 1];                           // m, a, b of the map positions (0 where not valid)
  float (*Ha)[SY][ML_BTX] = reinterpret_cast<float (*)[SY][ML_BTX]>(&Hm[0][0][0]);   // their horizontal pass: reuses Hm once it is consumed
  static_assert(3 * SY * ML_BTX <= 5 * RY * SX, "Ha fits in Hm");
  const int tid = threadIdx.x;
  const int plane = blockIdx.x / a.tiles_pp, t = blockIdx.x - plane * a.tiles_pp;
  const int i0 = (t / a.tiles_x) * ML_BTY, j0 = (t % a.tiles_x) * ML_BTX;      // the tile's first pixel
  const int H = a.H, W = a.W;
  const size_t po = (size_t)plane * H * W;
  // region pixel (r, c) is pixel (i0 - 10 + r, j0 - 10 + c); map position (r, c) of the tile is (i0 - 10 + r, j0 - 10 + c) too
  ml_load_region<RY, RX>(a.x + po, a.y + po, H, W, i0 - HALO, j0 - HALO, a.level0, X, Y);
  __syncthreads();
  ssim::moments_rows<ML_THREADS, RY, RX>(X, Y, Hm);
  __syncthreads();
  for (int i = tid; i < SY * SX; i += ML_THREADS) {
    const int r = i / SX, c = i - r * SX;
    const int pi = i0 - HALO + r, pj = j0 - HALO + c;
    float gm = 0.f, ga = 0.f, gb = 0.f;
    if (pi >= 0 && pi + HALO < H && pj >= 0 && pj + HALO < W) {
      float m[5];
      ssim::moments_at<RY, SX>(Hm, r, c, m);
      const float ux = m[0], uy = m[1];                          // the shifted means: what s_xx, s_xy see
      const float sxx = m[2] - ux * ux, syy = m[3] - uy * uy, sxy = m[4] - ux * uy;
      const float ib2 = 1.f / (sxx + syy + ssim::C2);
      const float cs = (2.f * sxy + ssim::C2) * ib2;
      if (SS) {
        const float mx = ux + ssim::SHIFT, my = uy + ssim::SHIFT;
        const float ib1 = 1.f / (mx * mx + my * my + ssim::C1);
        const float l = (2.f * mx * my + ssim::C1) * ib1;        // S = l * cs
        ga = -(l * cs) * ib2;                                    // through sigma_xx
        gb = 2.f * l * ib2;                                      // through sigma_xy
        // d S / d (G*x') in full: 2 mu_y cs / B1 - 2 mu_x S / B1 - u_y b - 2 u_x a, grouped so that each difference is taken once
        gm = 2.f * cs * ib1 * (my - mx * l) + 2.f * l * ib2 * (ux * cs - uy);
      } else {
        ga = -cs * ib2;
        gb = 2.f * ib2;
        gm = 2.f * ib2 * (ux * cs - uy);                         // - u_y b - 2 u_x a
      }
    }
    adj[0][r][c] = gm;
    adj[1][r][c] = ga;
    adj[2][r][c] = gb;
  }
  __syncthreads();                                               // adj complete, Hm consumed
  // grad(q) = sum_k G[k] adj(q - k), k = 0..10: pixel column c of the tile reads map columns c .. c + 10 of the tile (G symmetric)
  for (int i = tid; i < SY * ML_BTX; i += ML_THREADS) {
    const int r = i / ML_BTX, c = i - r * ML_BTX;
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
  const float tk = a.table[(size_t)plane * ML_LEVELS + a.k];     // 0 for a plane whose value is 0: its whole gradient is 0
  // loss = 1 - mean v.  Levels 1-4 carry the gradient per unit of the upstream gradient; level 0 multiplies the finished sum by *gout
  // once, so the result is linear in *gout to the last bit (scaling every level's term instead rounds each differently, and the
  // terms of different levels partly cancel)
  const float gs = -tk;
  const float go = a.level0 ? *a.gout : 1.f;
  const float* gp = a.gpar ? a.gpar + (size_t)plane * a.Hn * a.Wn : nullptr;
  const float* xr = a.x + po;
  float* gd = a.gdst + po;
  for (int i = tid; i < ML_BTY * ML_BTX; i += ML_THREADS) {
    const int r = i / ML_BTX, c = i - r * ML_BTX;
    const int pi = i0 + r, pj = j0 + c;
    if (pi >= H || pj >= W) continue;
    float v[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < ssim::K; ++k) {
      const float w = ssim::kG[k];
#pragma unroll
      for (int q = 0; q < 3; ++q) v[q] += w * Ha[q][r + k][c];
    }
    const float x = X[r + HALO][c + HALO], y = Y[r + HALO][c + HALO];            // x', y': the shifted pixels
    float g = tk != 0.f ? (v[0] + 2.f * x * v[1] + y * v[2]) * gs : 0.f;
    if (gp) {
      // padded row pi + p lies in parent row (pi + p) / 2; with p = 1 the replicated padded row 0 is source row 0 as well and
      // lies in parent row 0 too.  A parent index past the level is the padded row / column the pooling's floor dropped.
      const int pr = (pi + a.p) >> 1, pc = (pj + a.p) >> 1;
      if (pr < a.Hn && pc < a.Wn) {
        const float share = 0.25f * ((a.p && pi == 0) ? 2.f : 1.f) * ((a.p && pj == 0) ? 2.f : 1.f);
        g += share * gp[(size_t)pr * a.Wn + pc];
      }
    }
    const size_t o = (size_t)pi * W + pj;
    if (a.level0) {
      const float s = xr[o];
      g = (s >= 0.f && s <= 1.f) ? g * go : 0.f;                 // the clamp passes the gradient on [0, 1]
    }
    gd[o] = g;
  }
}

struct MlGeom {
  int h[ML_LEVELS], w[ML_LEVELS];
  int first[ML_LEVELS + 1];        // map tiles per plane: level boundaries
  int btx[ML_LEVELS], bty[ML_LEVELS];
  long long planes;
};

}  // namespace

// level sizes as piq builds them, the tilings of every launch, and the refusals: 0, or -1 when the kernels cannot run the sizes
static int ml_geometry(int N, int C, int H, int W, MlGeom* g) {
  if (N <= 0 || C <= 0 || H < ssim::MIN_SIZE || W < ssim::MIN_SIZE) return -1;
  const long long lim = (1LL << 31) - 1;
  if ((long long)H * W > (1LL << 24)) return -1;         // in-plane offsets are ints, and the map counts are exact in fp32
  g->planes = (long long)N * C;
  ssim::level_sizes(H, W, g->h, g->w);
  int t = 0;
  long long most = 1;                                    // the most blocks per plane of any launch
  for (int k = 0; k < ML_LEVELS; ++k) {
    g->first[k] = t;
    t += ssim::map_tiles(g->h[k], g->w[k]);
    g->btx[k] = (g->w[k] + ML_BTX - 1) / ML_BTX;
    g->bty[k] = (g->h[k] + ML_BTY - 1) / ML_BTY;
    const long long b = (long long)g->btx[k] * g->bty[k], pool = ((long long)g->h[k] * g->w[k] + ML_THREADS - 1) / ML_THREADS;
    if (b > most) most = b;
    if (k > 0 && pool > most) most = pool;
  }
  g->first[ML_LEVELS] = t;
  if (t > most) most = t;
  // one grid dimension carries (plane, tile): every launch must fit it
  if (g->planes > lim / most) return -1;
  return 0;
}

extern "C" long long srk_ms_ssim_loss_workspace_bytes(int N, int C, int H, int W) {
  MlGeom g;
  if (ml_geometry(N, C, H, W, &g)) return -1;
  return ssim::workspace_bytes(g.planes, g.h, g.w);
}

extern "C" int srk_ms_ssim_loss_tiles(int N, int C, int H, int W, int* first) {
  MlGeom g;
  if (ml_geometry(N, C, H, W, &g)) return -1;
  if (first)
    for (int k = 0; k <= ML_LEVELS; ++k) first[k] = g.first[k];
  return g.first[ML_LEVELS];
}

static int ml_check(const srk_ms_ssim_loss_args* a, const char* who, MlGeom* g) {
  SRK_CHECK_ARG(a, "%s: null pointer", who);
  SRK_CHECK_ARG(ml_geometry(a->N, a->C, a->H, a->W, g) == 0,
                "%s: %dx%dx%dx%d refused (N, C > 0, H and W at least %d, and planes x tiles must stay below 2^31)", who, a->N, a->C,
                a->H, a->W, ssim::MIN_SIZE);
  return 0;
}

extern "C" int srk_ms_ssim_loss_fwd(const srk_ms_ssim_loss_args* a, srk_stream_t stream) {
  MlGeom g;
  if (int rc = ml_check(a, "srk_ms_ssim_loss_fwd", &g)) return rc;
  SRK_CHECK_ARG(a->sr && a->hr && a->workspace && a->partials, "srk_ms_ssim_loss_fwd: null pointer");
  SRK_CHECK_ARG((uintptr_t)a->partials % 16 == 0 && (uintptr_t)a->workspace % 4 == 0, "srk_ms_ssim_loss_fwd: workspace alignment");
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  MlMapsArgs m;
  m.tiles = ssim::layout_levels(a->sr, a->hr, a->workspace, g.planes, g.h, g.w, m.lv);
  m.partials = a->partials;
  for (int k = 1; k < ML_LEVELS; ++k) {
    const int p = ssim::level_pad(g.h[k - 1], g.w[k - 1]);
    const int bpp = (g.h[k] * g.w[k] + ML_THREADS - 1) / ML_THREADS;
    hipLaunchKernelGGL(ml_pool_kernel, dim3((unsigned)(g.planes * bpp)), dim3(ML_THREADS), 0, s, m.lv[k - 1].x, m.lv[k - 1].y, g.h[k - 1],
                       g.w[k - 1], const_cast<float*>(m.lv[k].x), const_cast<float*>(m.lv[k].y), g.h[k], g.w[k], p, bpp, k == 1 ? 1 : 0);
    SRK_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(ml_maps_kernel, dim3((unsigned)(g.planes * m.tiles)), dim3(ML_THREADS), 0, s, m);
  SRK_LAUNCH_CHECK();
  return 0;
}

extern "C" int srk_ms_ssim_loss_finalize(const srk_ms_ssim_loss_args* a, srk_stream_t stream) {
  MlGeom g;
  if (int rc = ml_check(a, "srk_ms_ssim_loss_finalize", &g)) return rc;
  SRK_CHECK_ARG(a->partials && a->table && a->loss, "srk_ms_ssim_loss_finalize: null pointer");
  SRK_CHECK_ARG((uintptr_t)a->partials % 16 == 0, "srk_ms_ssim_loss_finalize: partials alignment");
  MlFinalArgs f;
  f.partials = a->partials;
  for (int k = 0; k <= ML_LEVELS; ++k) f.first[k] = g.first[k];
  for (int k = 0; k < ML_LEVELS; ++k) {
    f.count[k] = (float)((g.h[k] - HALO) * (g.w[k] - HALO));
    f.weight[k] = (float)kMlWeight[k];
  }
  f.planes = (int)g.planes;
  f.table = a->table;
  f.loss = a->loss;
  hipLaunchKernelGGL(ml_final_kernel, dim3(1), dim3(ML_FIN_THREADS), 0, reinterpret_cast<hipStream_t>(stream), f);
  SRK_LAUNCH_CHECK();
  return 0;
}

extern "C" int srk_ms_ssim_loss_bwd(const srk_ms_ssim_loss_args* a, srk_stream_t stream) {
  MlGeom g;
  if (int rc = ml_check(a, "srk_ms_ssim_loss_bwd", &g)) return rc;
  SRK_CHECK_ARG(a->sr && a->hr && a->workspace && a->table && a->gout && a->gwork && a->grad, "srk_ms_ssim_loss_bwd: null pointer");
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  ssim::Level lv[ML_LEVELS];
  ssim::layout_levels(a->sr, a->hr, a->workspace, g.planes, g.h, g.w, lv);
  // the gradients of levels 1-4 of x in gwork, in level order
  float* gl[ML_LEVELS];
  gl[0] = a->grad;
  float* gw = a->gwork;
  for (int k = 1; k < ML_LEVELS; ++k) {
    gl[k] = gw;
    gw += (size_t)g.planes * g.h[k] * g.w[k];
  }
  for (int k = ML_LEVELS - 1; k >= 0; --k) {
    MlBwdArgs b;
    b.x = lv[k].x;
    b.y = lv[k].y;
    b.H = g.h[k];
    b.W = g.w[k];
    b.table = a->table;
    b.k = k;
    b.gout = a->gout;
    const bool last = k == ML_LEVELS - 1;
    b.gpar = last ? nullptr : gl[k + 1];
    b.Hn = last ? 0 : g.h[k + 1];
    b.Wn = last ? 0 : g.w[k + 1];
    b.p = ssim::level_pad(g.h[k], g.w[k]);
    b.gdst = gl[k];
    b.tiles_x = g.btx[k];
    b.tiles_pp = g.btx[k] * g.bty[k];
    b.level0 = k == 0 ? 1 : 0;
    const dim3 grid((unsigned)(g.planes * b.tiles_pp));
    if (last) hipLaunchKernelGGL(ml_bwd_kernel<true>, grid, dim3(ML_THREADS), 0, s, b);
    else hipLaunchKernelGGL(ml_bwd_kernel<false>, grid, dim3(ML_THREADS), 0, s, b);
    SRK_LAUNCH_CHECK();
  }
  return 0;
}
