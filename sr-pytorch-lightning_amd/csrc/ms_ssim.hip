// MS-SSIM with piq.multi_scale_ssim's defaults (reference configs/train_default_sr.yml `metrics`), on the device (the levels' geometry
// and `bin` are ssim_core.h's):
//   ms_pool_kernel     level k of both images from level k-1: replicate-pad p = max(H % 2, W % 2) on the top and left, then a
//                      2x2 / stride-2 average (F.pad + F.avg_pool2d); one launch per level, levels 1-4 in the caller's workspace
//   ms_maps_kernel     one launch for all five levels: the block index runs over every level's 16x16 valid-map tiles; each
//                      workgroup stages its tile + 10-pixel halo of both images in LDS, runs the separable 11-tap Gaussian (run-time
//                      taps and constants) over the five moments of the tile shifted by one of its pixels (otherwise as ssim_kernel
//                      in data.hip) and writes (sum ss, sum cs) over its tile to a fixed slot
//   ms_final_kernel    one wave per (image, channel) plane (8 waves): the plane's partials summed per level in a fixed order (lane-strided,
//                      then a shuffle tree), divided by the valid counts, relu / pow / product, then the mean over all planes
// No float atomics anywhere: the result is bit-reproducible.  fp32 maps (like piq), double sums.
#include <math.h>
#include "ssim_core.h"

namespace {

constexpr int MS_LEVELS = ssim::LEVELS;
constexpr int MS_TILE = ssim::TILE;
constexpr int MS_FINAL_THREADS = 512;

struct MsMapsArgs {
  ssim::Level lv[MS_LEVELS];
  float g[11];                    // normalised Gaussian taps
  float c1, c2;
  int tiles;                      // tiles per plane, all levels
  double* partials;               // [planes][tiles][2]: (sum ss, sum cs)
};

struct MsFinalArgs {
  const double* partials;
  int first[MS_LEVELS + 1];       // first[MS_LEVELS] = tiles per plane
  float count[MS_LEVELS];         // valid map positions per plane, per level (exact in fp32: < 2^24)
  float weight[MS_LEVELS];
  int planes;
  float* out;
};

__global__ __launch_bounds__(256) void ms_pool_kernel(const float* __restrict__ xs, const float* __restrict__ ys, int Hs, int Ws,
                                                      float* __restrict__ xd, float* __restrict__ yd, int Hd, int Wd, int p) {
  const int plane = blockIdx.y;
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q >= Hd * Wd) return;
  const int i = q / Wd, j = q - i * Wd;
  // padded row 2i (2i + 1) is source row max(2i - p, 0) (2i + 1 - p <= Hs - 1 since Hd = (Hs + p) / 2); columns alike
  const int r0 = max(2 * i - p, 0), r1 = 2 * i + 1 - p;
  const int c0 = max(2 * j - p, 0), c1 = 2 * j + 1 - p;
  const size_t so = (size_t)plane * Hs * Ws, d = (size_t)plane * Hd * Wd + q;
  const float* a = xs + so;
  const float* b = ys + so;
  xd[d] = 0.25f * (((a[r0 * Ws + c0] + a[r0 * Ws + c1]) + a[r1 * Ws + c0]) + a[r1 * Ws + c1]);
  yd[d] = 0.25f * (((b[r0 * Ws + c0] + b[r0 * Ws + c1]) + b[r1 * Ws + c0]) + b[r1 * Ws + c1]);
}

__global__ __launch_bounds__(256) void ms_maps_kernel(const MsMapsArgs a) {
  __shared__ float X[26][27], Y[26][27];
  __shared__ float Hm[5][26][16];
  __shared__ double red[4][2];
  const int tid = threadIdx.x;
  const int plane = blockIdx.y;
  const int t = blockIdx.x;
  // this tile's level: uniform selects over the table (no dynamic index into the kernel arguments)
  const float* xs = a.lv[0].x;
  const float* ys = a.lv[0].y;
  int H = a.lv[0].H, W = a.lv[0].W, tilesX = a.lv[0].tilesX, first = 0;
#pragma unroll
  for (int k = 1; k < MS_LEVELS; ++k)
    if (t >= a.lv[k].first) { xs = a.lv[k].x; ys = a.lv[k].y; H = a.lv[k].H; W = a.lv[k].W; tilesX = a.lv[k].tilesX; first = a.lv[k].first; }
  const int lt = t - first;
  const int tX = lt % tilesX, tY = lt / tilesX;
  const int y0 = tY * MS_TILE, x0 = tX * MS_TILE;
  xs += (size_t)plane * H * W;
  ys += (size_t)plane * H * W;
  for (int i = tid; i < 26 * 26; i += 256) {
    const int r = i / 26, c = i - r * 26;
    const int py = y0 + r, px = x0 + c;
    float vx = 0.f, vy = 0.f;
    if (py < H && px < W) {
      const size_t o = (size_t)py * W + px;
      vx = xs[o];
      vy = ys[o];
    }
    X[r][c] = vx; Y[r][c] = vy;
  }
  __syncthreads();
  // moments of the tile shifted by one of its pixels (inside the image: y0 + 10 < H): the variances lose no digits to
  // cancellation in fp32, and constant images give exactly zero
  const float kx = X[5][5], ky = Y[5][5];
  for (int i = tid; i < 26 * 16; i += 256) {
    const int r = i >> 4, c = i & 15;
    float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      const float xv = X[r][c + k] - kx, yv = Y[r][c + k] - ky, w = a.g[k];
      m[0] += w * xv; m[1] += w * yv; m[2] += w * (xv * xv); m[3] += w * (yv * yv); m[4] += w * (xv * yv);
    }
#pragma unroll
    for (int q = 0; q < 5; ++q) Hm[q][r][c] = m[q];
  }
  __syncthreads();
  const int r = tid >> 4, c = tid & 15;
  double ss_acc = 0.0, cs_acc = 0.0;
  if (y0 + r + 10 < H && x0 + c + 10 < W) {
    float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      const float w = a.g[k];
#pragma unroll
      for (int q = 0; q < 5; ++q) m[q] += w * Hm[q][r + k][c];
    }
    const float sxx = m[2] - m[0] * m[0], syy = m[3] - m[1] * m[1], sxy = m[4] - m[0] * m[1];
    const float mx = m[0] + kx, my = m[1] + ky;
    const float cs = (2.f * sxy + a.c2) / (sxx + syy + a.c2);
    const float ss = (2.f * mx * my + a.c1) / (mx * mx + my * my + a.c1) * cs;
    ss_acc = (double)ss;
    cs_acc = (double)cs;
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
    reinterpret_cast<double2*>(a.partials)[(size_t)plane * a.tiles + t] = v;
  }
}

__global__ __launch_bounds__(MS_FINAL_THREADS) void ms_final_kernel(const MsFinalArgs a) {
  __shared__ double red[MS_FINAL_THREADS / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int T = a.first[MS_LEVELS];
  double wsum = 0.0;                                     // lane 0: this wave's planes, in plane order
  for (int plane = wave; plane < a.planes; plane += MS_FINAL_THREADS / 64) {
    const double2* p = reinterpret_cast<const double2*>(a.partials) + (size_t)plane * T;
    double bin[MS_LEVELS] = {0.0, 0.0, 0.0, 0.0, 0.0};
    // lane-strided with eight loads in flight per lane, added in index order, then a fixed shuffle tree (l1_mean_kernel).  A slot
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
      for (int k = 0; k < MS_LEVELS; ++k) bin[k] += __shfl_down(bin[k], off, 64);
    // lane k < 5 takes level k's factor relu(mean)^w_k; lane 0 multiplies them in level order
    double tot = 0.0, cnt = 1.0, wt = 0.0;
#pragma unroll
    for (int k = 0; k < MS_LEVELS; ++k) {
      const double b = __shfl(bin[k], 0, 64);
      if (lane == k) { tot = b; cnt = (double)a.count[k]; wt = (double)a.weight[k]; }
    }
    const double f = lane < MS_LEVELS ? pow(fmax(tot / cnt, 0.0), wt) : 1.0;
    double v = f;
#pragma unroll
    for (int k = 1; k < MS_LEVELS; ++k) v *= __shfl(f, k, 64);
    if (lane == 0) wsum += v;
  }
  if (lane == 0) red[wave] = wsum;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < MS_FINAL_THREADS / 64; ++w) s += red[w];
    *a.out = (float)(s / (double)a.planes);            // every image has C planes: the mean over C, then over N
  }
}

}  // namespace

extern "C" long long srk_ms_ssim_workspace_bytes(int N, int C, int H, int W) {
  if (N <= 0 || C <= 0 || H < ssim::MIN_SIZE || W < ssim::MIN_SIZE) return -1;
  int h[MS_LEVELS], w[MS_LEVELS];
  ssim::level_sizes(H, W, h, w);
  return ssim::workspace_bytes((long long)N * C, h, w);
}

extern "C" int srk_ms_ssim_tiles(int H, int W, int* first) {
  if (H < ssim::MIN_SIZE || W < ssim::MIN_SIZE) return -1;
  int h[MS_LEVELS], w[MS_LEVELS];
  ssim::level_sizes(H, W, h, w);
  int t = 0;
  for (int k = 0; k < MS_LEVELS; ++k) {
    if (first) first[k] = t;
    t += ssim::map_tiles(h[k], w[k]);
  }
  if (first) first[MS_LEVELS] = t;
  return t;
}

extern "C" int srk_ms_ssim(const srk_ms_ssim_args* a, srk_stream_t stream) {
  SRK_CHECK_ARG(a && a->x && a->y && a->workspace && a->partials && a->out, "srk_ms_ssim: null pointer");
  SRK_CHECK_ARG(a->N > 0 && a->C > 0 && (long long)a->N * a->C <= 65535, "srk_ms_ssim: bad sizes N=%d C=%d", a->N, a->C);
  SRK_CHECK_ARG(a->H >= ssim::MIN_SIZE && a->W >= ssim::MIN_SIZE, "srk_ms_ssim: image %dx%d is smaller than %dx%d", a->H, a->W,
                ssim::MIN_SIZE, ssim::MIN_SIZE);
  SRK_CHECK_ARG(a->sigma > 0.f, "srk_ms_ssim: sigma must be positive");
  SRK_CHECK_ARG((uintptr_t)a->partials % 16 == 0 && (uintptr_t)a->workspace % 4 == 0, "srk_ms_ssim: workspace alignment");
  const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int planes = a->N * a->C;
  int h[MS_LEVELS], w[MS_LEVELS];
  ssim::level_sizes(a->H, a->W, h, w);
  MsMapsArgs m;
  MsFinalArgs f;
  const int t = ssim::layout_levels(a->x, a->y, a->workspace, planes, h, w, m.lv);
  for (int k = 0; k < MS_LEVELS; ++k) {
    f.first[k] = m.lv[k].first;
    f.count[k] = (float)((h[k] - ssim::HALO) * (w[k] - ssim::HALO));
  }
  f.first[MS_LEVELS] = t;
  double g[11], gs = 0.0;
  for (int i = 0; i < 11; ++i) {
    const double co = i - 5.0;
    g[i] = exp(-(co * co) / (2.0 * (double)a->sigma * (double)a->sigma));
    gs += g[i];
  }
  for (int i = 0; i < 11; ++i) m.g[i] = (float)(g[i] / gs);
  m.c1 = a->k1 * a->k1;
  m.c2 = a->k2 * a->k2;
  m.tiles = t;
  m.partials = a->partials;
  f.partials = a->partials;
  const float wt[MS_LEVELS] = {a->w0, a->w1, a->w2, a->w3, a->w4};
  for (int k = 0; k < MS_LEVELS; ++k) f.weight[k] = wt[k];
  f.planes = planes;
  f.out = a->out;

  for (int k = 1; k < MS_LEVELS; ++k) {
    const int p = ssim::level_pad(h[k - 1], w[k - 1]);
    hipLaunchKernelGGL(ms_pool_kernel, dim3((unsigned)((h[k] * w[k] + 255) / 256), (unsigned)planes), dim3(256), 0, s,
                       m.lv[k - 1].x, m.lv[k - 1].y, h[k - 1], w[k - 1], const_cast<float*>(m.lv[k].x), const_cast<float*>(m.lv[k].y),
                       h[k], w[k], p);
    SRK_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(ms_maps_kernel, dim3((unsigned)t, (unsigned)planes), dim3(256), 0, s, m);
  SRK_LAUNCH_CHECK();
  hipLaunchKernelGGL(ms_final_kernel, dim3(1), dim3(MS_FINAL_THREADS), 0, s, f);
  SRK_LAUNCH_CHECK();
  return 0;
}
