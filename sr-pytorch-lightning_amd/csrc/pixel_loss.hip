// Pixel-domain losses of the training step (include/srk.h, "pixel losses"): Charbonnier, Huber, smooth-L1, Barron's general robust
// loss with fixed alpha and c, and the PSNR loss.  All HBM streams shaped like the L1 loss of data.hip: float4 loads of both images,
// an fp32 sum of at most four values per thread then double, wave shuffle + LDS, one double per block in a fixed slot (no atomics:
// bit-identical run to run), the upstream gradient read from the device.  Unlike L1 (a sign in a byte) none of these has a derivative
// that fits a byte, and a 16-bit one would miss the fp32 limits of the tests, so every backward RECOMPUTES psi(d) from the two saved
// images: forward 8 B per element, backward 12 B, no buffer besides the gradient.
#include "srk_common.h"

namespace {

constexpr int PL_THREADS = 256;
static_assert(PL_THREADS * 4 == SRK_PIXEL_LOSS_BLOCK_ELEMS, "one float4 per thread and pass");

// the launch's constants, derived once per thread from (p0, p1); uniform, so they live in scalar registers
struct pl_consts {
  float k0, k1, k2, k3;
};

template <int KIND>
__device__ __forceinline__ pl_consts pl_prepare(float p0, float p1) {
  pl_consts c = {0.f, 0.f, 0.f, 0.f};
  if constexpr (KIND == SRK_PIXEL_CHARBONNIER) {
    c.k0 = p0 * p0;                                 // eps^2
  } else if constexpr (KIND == SRK_PIXEL_HUBER) {
    c.k0 = p0;                                      // delta
    c.k1 = 0.5f * p0;
  } else if constexpr (KIND == SRK_PIXEL_SMOOTH_L1) {
    c.k0 = p0;                                      // beta
    c.k1 = 0.5f * p0;
  } else {
    // the robust kinds divide every element by the launch's constants c, c^2 and b: they multiply by the fp32 reciprocals instead
    // (one more rounding each, well inside the tests' limits).  The host sends only constants whose reciprocals and quotient are
    // finite, normal fp32 numbers (pixel_loss.py: _kind_of)
    c.k0 = 1.f / p1;                                // 1 / c
    c.k1 = 1.f / (p1 * p1);                         // 1 / c^2
    if constexpr (KIND == SRK_PIXEL_ROBUST_GENERAL) {
      const float b = fabsf(p0 - 2.f);
      c.k2 = 1.f / b;                               // 1 / b
      c.k3 = b / p0;                                // b / alpha
    }
  }
  return c;
}

// value and psi = d value / d d of one element.  `alpha` is p0 (read by ROBUST_GENERAL only)
template <int KIND>
__device__ __forceinline__ float pl_value(float d, const pl_consts& c, float alpha) {
  if constexpr (KIND == SRK_PIXEL_CHARBONNIER) {
    return sqrtf(d * d + c.k0);
  } else if constexpr (KIND == SRK_PIXEL_HUBER) {
    const float ad = fabsf(d);
    return ad <= c.k0 ? 0.5f * d * d : c.k0 * (ad - c.k1);
  } else if constexpr (KIND == SRK_PIXEL_SMOOTH_L1) {
    const float ad = fabsf(d);
    return ad < c.k0 ? 0.5f * d * d / c.k0 : ad - c.k1;
  } else {
    const float q = d * c.k0;
    const float z = q * q;
    if constexpr (KIND == SRK_PIXEL_ROBUST_A2) return 0.5f * z;
    else if constexpr (KIND == SRK_PIXEL_ROBUST_A0) return log1pf(0.5f * z);
    else if constexpr (KIND == SRK_PIXEL_ROBUST_NEG_INF) return -expm1f(-0.5f * z);
    else return c.k3 * expm1f(0.5f * alpha * log1pf(z * c.k2));
  }
}

template <int KIND>
__device__ __forceinline__ float pl_psi(float d, const pl_consts& c, float alpha) {
  if constexpr (KIND == SRK_PIXEL_CHARBONNIER) {
    return d / sqrtf(d * d + c.k0);
  } else if constexpr (KIND == SRK_PIXEL_HUBER) {
    return fabsf(d) <= c.k0 ? d : copysignf(c.k0, d);
  } else if constexpr (KIND == SRK_PIXEL_SMOOTH_L1) {
    // (d == 0 with beta == 0 takes the second branch: the sign of 0 is 0, as torch's l1 gradient)
    return fabsf(d) < c.k0 ? d / c.k0 : (float)((d > 0.f) - (d < 0.f));
  } else {
    const float q = d * c.k0;
    const float z = q * q;
    const float lin = d * c.k1;                     // d / c^2
    if constexpr (KIND == SRK_PIXEL_ROBUST_A2) return lin;
    else if constexpr (KIND == SRK_PIXEL_ROBUST_A0) return lin / (0.5f * z + 1.f);
    else if constexpr (KIND == SRK_PIXEL_ROBUST_NEG_INF) return lin * expf(-0.5f * z);
    else return lin * expf((0.5f * alpha - 1.f) * log1pf(z * c.k2));
  }
}

__device__ __forceinline__ void pl_block_sum(double acc, double* slot) {
  __shared__ double red[PL_THREADS / 64];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = red[0];
#pragma unroll
    for (int w = 1; w < PL_THREADS / 64; ++w) t += red[w];
    *slot = t;
  }
}

template <int KIND>
__global__ __launch_bounds__(PL_THREADS) void pixel_fwd_kernel(const srk_pixel_loss_args a) {
  const pl_consts c = pl_prepare<KIND>(a.p0, a.p1);
  const long long n4 = a.n >> 2;
  double acc = 0.0;
  for (long long i = (long long)blockIdx.x * PL_THREADS + threadIdx.x; i < n4; i += (long long)gridDim.x * PL_THREADS) {
    const float4 s = reinterpret_cast<const float4*>(a.sr)[i], h = reinterpret_cast<const float4*>(a.hr)[i];
    const float t = (pl_value<KIND>(s.x - h.x, c, a.p0) + pl_value<KIND>(s.y - h.y, c, a.p0)) +
                    (pl_value<KIND>(s.z - h.z, c, a.p0) + pl_value<KIND>(s.w - h.w, c, a.p0));
    acc += (double)t;
  }
  if (blockIdx.x == 0 && threadIdx.x < (a.n & 3)) {            // tail (n not a multiple of 4)
    const long long i = (n4 << 2) + threadIdx.x;
    acc += (double)pl_value<KIND>(a.sr[i] - a.hr[i], c, a.p0);
  }
  pl_block_sum(acc, a.partial + blockIdx.x);
}

template <int KIND>
__global__ __launch_bounds__(PL_THREADS) void pixel_bwd_kernel(const srk_pixel_loss_args a) {
  const pl_consts c = pl_prepare<KIND>(a.p0, a.p1);
  const float g = *a.gout * a.scale;
  const long long n4 = a.n >> 2;
  for (long long i = (long long)blockIdx.x * PL_THREADS + threadIdx.x; i < n4; i += (long long)gridDim.x * PL_THREADS) {
    const float4 s = reinterpret_cast<const float4*>(a.sr)[i], h = reinterpret_cast<const float4*>(a.hr)[i];
    float4 o;
    o.x = g * pl_psi<KIND>(s.x - h.x, c, a.p0);
    o.y = g * pl_psi<KIND>(s.y - h.y, c, a.p0);
    o.z = g * pl_psi<KIND>(s.z - h.z, c, a.p0);
    o.w = g * pl_psi<KIND>(s.w - h.w, c, a.p0);
    reinterpret_cast<float4*>(a.grad)[i] = o;
  }
  if (blockIdx.x == 0 && threadIdx.x < (a.n & 3)) {
    const long long i = (n4 << 2) + threadIdx.x;
    a.grad[i] = g * pl_psi<KIND>(a.sr[i] - a.hr[i], c, a.p0);
  }
}

template <int KIND>
void pixel_launch(bool bwd, const srk_pixel_loss_args& a, hipStream_t s) {
  const dim3 grid(srk_pixel_loss_blocks(a.n)), block(PL_THREADS);
  if (bwd) hipLaunchKernelGGL(pixel_bwd_kernel<KIND>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(pixel_fwd_kernel<KIND>, grid, block, 0, s, a);
}

bool pixel_dispatch(bool bwd, const srk_pixel_loss_args& a, hipStream_t s) {
  switch (a.kind) {
    case SRK_PIXEL_CHARBONNIER: pixel_launch<SRK_PIXEL_CHARBONNIER>(bwd, a, s); return true;
    case SRK_PIXEL_HUBER: pixel_launch<SRK_PIXEL_HUBER>(bwd, a, s); return true;
    case SRK_PIXEL_SMOOTH_L1: pixel_launch<SRK_PIXEL_SMOOTH_L1>(bwd, a, s); return true;
    case SRK_PIXEL_ROBUST_A2: pixel_launch<SRK_PIXEL_ROBUST_A2>(bwd, a, s); return true;
    case SRK_PIXEL_ROBUST_A0: pixel_launch<SRK_PIXEL_ROBUST_A0>(bwd, a, s); return true;
    case SRK_PIXEL_ROBUST_NEG_INF: pixel_launch<SRK_PIXEL_ROBUST_NEG_INF>(bwd, a, s); return true;
    case SRK_PIXEL_ROBUST_GENERAL: pixel_launch<SRK_PIXEL_ROBUST_GENERAL>(bwd, a, s); return true;
    default: return false;
  }
}

// ---- PSNR loss -----------------------------------------------------------------------------------------------------------------
constexpr double PSNR_K = 4.342944819032518;        // 10 / ln 10

// blocks per image: one per SRK_PIXEL_LOSS_BLOCK_ELEMS elements, as long as the whole grid stays near L1's SRK_PIXEL_LOSS_BLOCKS_MAX
// (a block then walks its image with a stride); at least one
long long psnr_bpi(int N, long long per) {
  long long want = (per + SRK_PIXEL_LOSS_BLOCK_ELEMS - 1) / SRK_PIXEL_LOSS_BLOCK_ELEMS;
  const long long cap = SRK_PIXEL_LOSS_BLOCKS_MAX / N;
  if (want > cap) want = cap;
  return want < 1 ? 1 : want;
}

// The three pieces of image n, which starts at element n * per of a 16-byte-aligned tensor: `head` scalars up to the next 16-byte
// boundary (at most 3, at most per), `n4` float4s, `tail` scalars.  None of the float4s holds a pixel of another image.
struct psnr_span {
  long long base, n4;
  int head, tail;
};
__device__ __forceinline__ psnr_span psnr_span_of(long long n, long long per) {
  psnr_span s;
  s.base = n * per;
  long long head = (4 - (s.base & 3)) & 3;
  if (head > per) head = per;
  s.head = (int)head;
  s.n4 = (per - head) >> 2;
  s.tail = (int)((per - head) & 3);
  return s;
}

__global__ __launch_bounds__(PL_THREADS) void psnr_fwd_kernel(const srk_psnr_loss_args a, int bpi) {
  const unsigned n = blockIdx.x / (unsigned)bpi;
  const int b = (int)(blockIdx.x - n * (unsigned)bpi);
  const psnr_span sp = psnr_span_of(n, a.per);
  const float* sr = a.sr + sp.base;
  const float* hr = a.hr + sp.base;
  double acc = 0.0;
  const float4* s4 = reinterpret_cast<const float4*>(sr + sp.head);
  const float4* h4 = reinterpret_cast<const float4*>(hr + sp.head);
  for (long long i = (long long)b * PL_THREADS + threadIdx.x; i < sp.n4; i += (long long)bpi * PL_THREADS) {
    const float4 s = s4[i], h = h4[i];
    const float dx = s.x - h.x, dy = s.y - h.y, dz = s.z - h.z, dw = s.w - h.w;
    acc += (double)((dx * dx + dy * dy) + (dz * dz + dw * dw));
  }
  if (b == 0) {                                       // the scalar head and tail of the image: threads 0-2 and 64-66
    if ((int)threadIdx.x < sp.head) {
      const float d = sr[threadIdx.x] - hr[threadIdx.x];
      acc += (double)(d * d);
    }
    const int t = (int)threadIdx.x - 64;
    if (t >= 0 && t < sp.tail) {
      const long long i = sp.head + (sp.n4 << 2) + t;
      const float d = sr[i] - hr[i];
      acc += (double)(d * d);
    }
  }
  pl_block_sum(acc, a.partial + blockIdx.x);
}

// one workgroup; the image's partials in a fixed order -> mse_n -> coef[n] and ln(mse_n + eps); the logarithms are summed per thread in
// image order, then by the fixed shuffle / LDS tree.  Few images with many blocks each (bpi >= 64, so at most 32 images): a WAVE takes
// images w, w + 4, ..., its lanes the partials l, l + 64, ... in index order, then the shuffle tree.  Otherwise a THREAD takes images
// t, t + 256, ... and adds the image's fewer than 64 partials in index order.  `bpi` is the launch's, so the choice is uniform.
__global__ __launch_bounds__(PL_THREADS) void psnr_finalize_kernel(const srk_psnr_loss_args a, int bpi) {
  double acc = 0.0;
  if (bpi >= 64) {
    const int lane = threadIdx.x & 63;
    for (int n = threadIdx.x >> 6; n < a.N; n += PL_THREADS / 64) {
      const double* p = a.partial + (long long)n * bpi;
      double s = 0.0;
      for (int b = lane; b < bpi; b += 64) s += p[b];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
      if (lane == 0) {
        const double m = s / (double)a.per + (double)a.eps;
        a.coef[n] = (float)(PSNR_K / (double)a.N * 2.0 / ((double)a.per * m));
        acc += log(m);
      }
    }
  } else {
    for (int n = threadIdx.x; n < a.N; n += PL_THREADS) {
      const double* p = a.partial + (long long)n * bpi;
      double s = 0.0;
#pragma unroll 8
      for (int b = 0; b < bpi; ++b) s += p[b];
      const double m = s / (double)a.per + (double)a.eps;
      a.coef[n] = (float)(PSNR_K / (double)a.N * 2.0 / ((double)a.per * m));
      acc += log(m);
    }
  }
  __shared__ double total;
  pl_block_sum(acc, &total);
  if (threadIdx.x == 0) *a.loss = (float)(PSNR_K * total / (double)a.N);
}

__global__ __launch_bounds__(PL_THREADS) void psnr_bwd_kernel(const srk_psnr_loss_args a, int bpi) {
  const unsigned n = blockIdx.x / (unsigned)bpi;
  const int b = (int)(blockIdx.x - n * (unsigned)bpi);
  const psnr_span sp = psnr_span_of(n, a.per);
  const float g = *a.gout * a.coef[n];
  const float* sr = a.sr + sp.base;
  const float* hr = a.hr + sp.base;
  float* grad = a.grad + sp.base;
  const float4* s4 = reinterpret_cast<const float4*>(sr + sp.head);
  const float4* h4 = reinterpret_cast<const float4*>(hr + sp.head);
  float4* g4 = reinterpret_cast<float4*>(grad + sp.head);
  for (long long i = (long long)b * PL_THREADS + threadIdx.x; i < sp.n4; i += (long long)bpi * PL_THREADS) {
    const float4 s = s4[i], h = h4[i];
    float4 o;
    o.x = g * (s.x - h.x);
    o.y = g * (s.y - h.y);
    o.z = g * (s.z - h.z);
    o.w = g * (s.w - h.w);
    g4[i] = o;
  }
  if (b == 0) {
    if ((int)threadIdx.x < sp.head) grad[threadIdx.x] = g * (sr[threadIdx.x] - hr[threadIdx.x]);
    const int t = (int)threadIdx.x - 64;
    if (t >= 0 && t < sp.tail) {
      const long long i = sp.head + (sp.n4 << 2) + t;
      grad[i] = g * (sr[i] - hr[i]);
    }
  }
}

}  // namespace

extern "C" int srk_pixel_loss_blocks(long long n) {
  const long long b = (n / 4 + PL_THREADS - 1) / PL_THREADS;
  return (int)(b < 1 ? 1 : (b > SRK_PIXEL_LOSS_BLOCKS_MAX ? SRK_PIXEL_LOSS_BLOCKS_MAX : b));
}
extern "C" int srk_pixel_loss_fwd(const srk_pixel_loss_args* a, srk_stream_t stream) {
  SRK_CHECK_ARG(a && a->sr && a->hr && a->partial && a->n > 0, "srk_pixel_loss_fwd: null pointer / empty");
  SRK_CHECK_ARG(((uintptr_t)a->sr | (uintptr_t)a->hr) % 16 == 0, "srk_pixel_loss_fwd: 16-byte alignment");
  const bool known = pixel_dispatch(false, *a, reinterpret_cast<hipStream_t>(stream));
  SRK_CHECK_ARG(known, "srk_pixel_loss_fwd: unknown kind %d", a->kind);
  SRK_LAUNCH_CHECK();
  return 0;
}
extern "C" int srk_pixel_loss_bwd(const srk_pixel_loss_args* a, srk_stream_t stream) {
  SRK_CHECK_ARG(a && a->sr && a->hr && a->gout && a->grad && a->n > 0, "srk_pixel_loss_bwd: null pointer / empty");
  SRK_CHECK_ARG(((uintptr_t)a->sr | (uintptr_t)a->hr | (uintptr_t)a->grad) % 16 == 0, "srk_pixel_loss_bwd: 16-byte alignment");
  const bool known = pixel_dispatch(true, *a, reinterpret_cast<hipStream_t>(stream));
  SRK_CHECK_ARG(known, "srk_pixel_loss_bwd: unknown kind %d", a->kind);
  SRK_LAUNCH_CHECK();
  return 0;
}

extern "C" long long srk_psnr_loss_blocks(int N, long long per) {
  if (N <= 0 || per <= 0) return -1;
  // HIP launches a grid of fewer than 2^32 threads: fewer than 2^24 blocks of 256 (more images than that take the torch path)
  const long long total = (long long)N * psnr_bpi(N, per);
  return total < (1LL << 32) / PL_THREADS ? total : -1;
}
extern "C" int srk_psnr_loss_fwd(const srk_psnr_loss_args* a, srk_stream_t stream) {
  SRK_CHECK_ARG(a && a->sr && a->hr && a->partial, "srk_psnr_loss_fwd: null pointer");
  SRK_CHECK_ARG(srk_psnr_loss_blocks(a->N, a->per) > 0, "srk_psnr_loss_fwd: empty / too many blocks");
  SRK_CHECK_ARG(((uintptr_t)a->sr | (uintptr_t)a->hr) % 16 == 0, "srk_psnr_loss_fwd: 16-byte alignment");
  const int bpi = (int)psnr_bpi(a->N, a->per);
  hipLaunchKernelGGL(psnr_fwd_kernel, dim3((unsigned)(a->N * (long long)bpi)), dim3(PL_THREADS), 0, reinterpret_cast<hipStream_t>(stream), *a, bpi);
  SRK_LAUNCH_CHECK();
  return 0;
}
extern "C" int srk_psnr_loss_finalize(const srk_psnr_loss_args* a, srk_stream_t stream) {
  SRK_CHECK_ARG(a && a->partial && a->coef && a->loss, "srk_psnr_loss_finalize: null pointer");
  SRK_CHECK_ARG(srk_psnr_loss_blocks(a->N, a->per) > 0 && a->eps > 0.f, "srk_psnr_loss_finalize: empty / too many blocks / eps <= 0");
  hipLaunchKernelGGL(psnr_finalize_kernel, dim3(1), dim3(PL_THREADS), 0, reinterpret_cast<hipStream_t>(stream), *a, (int)psnr_bpi(a->N, a->per));
  SRK_LAUNCH_CHECK();
  return 0;
}
extern "C" int srk_psnr_loss_bwd(const srk_psnr_loss_args* a, srk_stream_t stream) {
  SRK_CHECK_ARG(a && a->sr && a->hr && a->coef && a->gout && a->grad, "srk_psnr_loss_bwd: null pointer");
  SRK_CHECK_ARG(srk_psnr_loss_blocks(a->N, a->per) > 0, "srk_psnr_loss_bwd: empty / too many blocks");
  SRK_CHECK_ARG(((uintptr_t)a->sr | (uintptr_t)a->hr | (uintptr_t)a->grad) % 16 == 0, "srk_psnr_loss_bwd: 16-byte alignment");
  const int bpi = (int)psnr_bpi(a->N, a->per);
  hipLaunchKernelGGL(psnr_bwd_kernel, dim3((unsigned)(a->N * (long long)bpi)), dim3(PL_THREADS), 0, reinterpret_cast<hipStream_t>(stream), *a, bpi);
  SRK_LAUNCH_CHECK();
  return 0;
}
