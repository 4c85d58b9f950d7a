// Tiled / self-ensemble inference (tiling.py): the two data movements around the model's forward, each ONE launch for any number of tiles.
//   srk_tile_gather  LR image [1,C,H,W] -> batch of tiles [N,C,th,tw], each already transformed (one of the 8 flips / transposes)
//   srk_tile_place   batch of SR tiles [N,C,s*th,s*tw] -> each entry's owned rectangle of the HR image [1,C,sH,sW], transform undone;
//                    store, or out += weight * v (the ensemble's sum)
// Transform id k: bit 0 reverses W, bit 1 reverses H, bit 2 transposes H and W after the flips.  A tile lives in the TRANSFORMED frame
// (rows Y, columns X of transform_k(image)); pixel (Y, X) of that frame is pixel (y, x) of the image with
//     (y1, x1) = bit 2 ? (X, Y) : (Y, X);   y = bit 1 ? H-1-y1 : y1;   x = bit 0 ? W-1-x1 : x1
// and the same with sH, sW for the HR frames.
// Both kernels are pure fp32 copies, HBM-bound.  A workgroup moves one 32 x 32 block of one channel of one entry, 32 lanes along the
// WRITTEN side's W.  Without the transpose the read side runs along W as well (forwards or backwards: coalesced either way); with it the
// block is read with the lanes along the READ side's W into a 32 x 33 LDS tile and written transposed out of it (pitch 33: a column read
// of 32 lanes touches 32 banks).  All element offsets are 64-bit: the HR image is the one tensor here that may pass 2^31 elements.
#include "srk_common.h"

namespace {

constexpr int TB = 32;          // block edge

// image pixel (y, x) -> transformed-frame pixel (Y, X) and back; H, W are the IMAGE's sides in both (the flips act on the image's axes)
__device__ __forceinline__ void to_frame(int id, int H, int W, int y, int x, int& Y, int& X) {
  const int y1 = (id & 2) ? H - 1 - y : y, x1 = (id & 1) ? W - 1 - x : x;
  Y = (id & 4) ? x1 : y1;
  X = (id & 4) ? y1 : x1;
}
__device__ __forceinline__ void to_image(int id, int H, int W, int Y, int X, int& y, int& x) {
  const int y1 = (id & 4) ? X : Y, x1 = (id & 4) ? Y : X;
  y = (id & 2) ? H - 1 - y1 : y1;
  x = (id & 1) ? W - 1 - x1 : x1;
}

// blockIdx.x = ((n * C + c) * nbh + bi) * nbw + bj
__device__ __forceinline__ void decode_block(int C, int nbh, int nbw, int& n, int& c, int& bi, int& bj) {
  unsigned b = blockIdx.x;
  bj = (int)(b % (unsigned)nbw); b /= (unsigned)nbw;
  bi = (int)(b % (unsigned)nbh); b /= (unsigned)nbh;
  c = (int)(b % (unsigned)C);
  n = (int)(b / (unsigned)C);
}

__global__ __launch_bounds__(256) void tile_gather_kernel(const srk_tile_args a, int nbh, int nbw) {
  __shared__ float lds[TB][TB + 1];
  int n, c, bi, bj;
  decode_block(a.C, nbh, nbw, n, c, bi, bj);
  const srk_tile_desc d = a.table[n];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int i0 = bi * TB, j0 = bj * TB;                           // block origin inside the tile (rows i, columns j)
  const float* src = a.src + (long long)c * a.H * a.W;
  float* dst = a.dst + ((long long)n * a.C + c) * a.th * a.tw;
  if (d.id & 4) {
    // the image's W runs along the tile's rows: read with tx along i, write with tx along j
#pragma unroll
    for (int r = 0; r < TB; r += 8) {
      const int i = i0 + tx, j = j0 + ty + r;
      int y, x;
      to_image(d.id, a.H, a.W, d.y0 + i, d.x0 + j, y, x);
      float v = 0.f;
      if (i < a.th && j < a.tw && y >= 0 && y < a.H && x >= 0 && x < a.W) v = src[(long long)y * a.W + x];
      lds[ty + r][tx] = v;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < TB; r += 8) {
      const int i = i0 + ty + r, j = j0 + tx;
      if (i < a.th && j < a.tw) dst[(long long)i * a.tw + j] = lds[tx][ty + r];
    }
  } else {
#pragma unroll
    for (int r = 0; r < TB; r += 8) {
      const int i = i0 + ty + r, j = j0 + tx;
      int y, x;
      to_image(d.id, a.H, a.W, d.y0 + i, d.x0 + j, y, x);
      if (i < a.th && j < a.tw && y >= 0 && y < a.H && x >= 0 && x < a.W) dst[(long long)i * a.tw + j] = src[(long long)y * a.W + x];
    }
  }
}

__global__ __launch_bounds__(256) void tile_place_kernel(const srk_tile_args a, int nbh, int nbw) {
  __shared__ float lds[TB][TB + 1];
  int n, c, bi, bj;
  decode_block(a.C, nbh, nbw, n, c, bi, bj);
  const srk_tile_desc d = a.table[n];
  const int i0 = bi * TB, j0 = bj * TB;                           // block origin inside the owned rectangle (HR image rows / columns)
  if (i0 >= d.oh || j0 >= d.ow) return;                           // (the grid covers the largest owned rectangle; block-uniform exit)
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int s = a.scale;
  const int sH = a.H * s, sW = a.W * s, sth = a.th * s, stw = a.tw * s;
  const int ly0 = d.y0 * s, lx0 = d.x0 * s;                       // tile origin in the transformed HR frame
  const float* src = a.src + ((long long)n * a.C + c) * sth * stw;
  float* dst = a.dst + (long long)c * sH * sW;
  float v[TB / 8];
  if (d.id & 4) {
    // the tile's W runs along the image's rows: read with tx along i, write with tx along j
#pragma unroll
    for (int r = 0; r < TB; r += 8) {
      const int i = i0 + tx, j = j0 + ty + r;
      int Y, X;
      to_frame(d.id, sH, sW, d.oy + i, d.ox + j, Y, X);
      Y -= ly0; X -= lx0;
      float t = 0.f;
      if (i < d.oh && j < d.ow && Y >= 0 && Y < sth && X >= 0 && X < stw) t = src[(long long)Y * stw + X];
      lds[ty + r][tx] = t;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < TB; r += 8) v[r / 8] = lds[tx][ty + r];
  } else {
#pragma unroll
    for (int r = 0; r < TB; r += 8) {
      const int i = i0 + ty + r, j = j0 + tx;
      int Y, X;
      to_frame(d.id, sH, sW, d.oy + i, d.ox + j, Y, X);
      Y -= ly0; X -= lx0;
      v[r / 8] = (i < d.oh && j < d.ow && Y >= 0 && Y < sth && X >= 0 && X < stw) ? src[(long long)Y * stw + X] : 0.f;
    }
  }
#pragma unroll
  for (int r = 0; r < TB; r += 8) {
    const int i = i0 + ty + r, j = j0 + tx;
    const int y = d.oy + i, x = d.ox + j;
    if (i < d.oh && j < d.ow && y >= 0 && y < sH && x >= 0 && x < sW) {
      // the rectangle must also lie inside the tile: a pixel whose source is outside it is left alone (never read out of bounds)
      int Y, X;
      to_frame(d.id, sH, sW, y, x, Y, X);
      Y -= ly0; X -= lx0;
      if (Y >= 0 && Y < sth && X >= 0 && X < stw) {
        float* o = dst + (long long)y * sW + x;
        *o = a.accumulate ? *o + a.weight * v[r / 8] : v[r / 8];
      }
    }
  }
}

int check_common(const srk_tile_args* a, const char* who) {
  SRK_CHECK_ARG(a && a->src && a->dst && a->table, "%s: null pointer", who);
  SRK_CHECK_ARG(a->N > 0 && a->C > 0 && a->H > 0 && a->W > 0 && a->th > 0 && a->tw > 0, "%s: bad sizes", who);
  return 0;
}

int blocks_of(const srk_tile_args* a, int h, int w, int& nbh, int& nbw, unsigned& total, const char* who) {
  nbh = (h + TB - 1) / TB;
  nbw = (w + TB - 1) / TB;
  const long long t = (long long)a->N * a->C * nbh * nbw;
  SRK_CHECK_ARG(t <= 0x7fffffffLL, "%s: %lld blocks in one launch", who, t);
  total = (unsigned)t;
  return 0;
}

}  // namespace

extern "C" int srk_tile_gather(const srk_tile_args* a, srk_stream_t stream) {
  if (int rc = check_common(a, "srk_tile_gather")) return rc;
  SRK_CHECK_ARG((long long)a->th * a->tw * a->C <= 0x7fffffffLL, "srk_tile_gather: tile too large");
  int nbh, nbw;
  unsigned total;
  if (int rc = blocks_of(a, a->th, a->tw, nbh, nbw, total, "srk_tile_gather")) return rc;
  hipLaunchKernelGGL(tile_gather_kernel, dim3(total), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), *a, nbh, nbw);
  SRK_LAUNCH_CHECK();
  return 0;
}

extern "C" int srk_tile_place(const srk_tile_args* a, srk_stream_t stream) {
  if (int rc = check_common(a, "srk_tile_place")) return rc;
  SRK_CHECK_ARG(a->scale > 0 && a->max_oh > 0 && a->max_ow > 0, "srk_tile_place: bad scale / owned extent");
  SRK_CHECK_ARG((long long)a->H * a->scale <= 0x7fffffffLL && (long long)a->W * a->scale <= 0x7fffffffLL &&
                (long long)a->th * a->scale <= 0x7fffffffLL && (long long)a->tw * a->scale <= 0x7fffffffLL, "srk_tile_place: an HR side passes 2^31");
  int nbh, nbw;
  unsigned total;
  if (int rc = blocks_of(a, a->max_oh, a->max_ow, nbh, nbw, total, "srk_tile_place")) return rc;
  hipLaunchKernelGGL(tile_place_kernel, dim3(total), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), *a, nbh, nbw);
  SRK_LAUNCH_CHECK();
  return 0;
}
