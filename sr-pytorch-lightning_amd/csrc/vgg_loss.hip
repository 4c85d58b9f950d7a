// The glue of the VGG perceptual loss (include/srk.h, "VGG perceptual loss"; vgg_loss.py): everything between the srk_conv2d launches of the
// frozen feature stack.  Seven bandwidth-bound streams over DENSE NHWC tensors in the storage dtype: a lane moves one 16-byte channel
// chunk (8 x 16-bit or 4 x fp32) per access, a grid of at most SRK_VGG_BLOCKS_MAX workgroups walks the chunks with its stride, nothing
// is indexed at run time inside a register array (no scratch), and the one reduction keeps a double per workgroup in a fixed slot that
// one finalize workgroup adds in a fixed order (no atomics: bit-identical run to run).
//   prepare     8 B read + 32 / 64 B written per pixel and image      pool_fwd   4 chunks read, 1 written per output chunk
//   feat_fwd    2 chunks read per chunk                               pool_bwd   the window (4 chunks, 3 of them cache hits) + 1 read, 1 written
//   feat_grad   2 chunks read, 1 written                              image_grad 1 chunk read, 12 B written per pixel
#include "srk_common.h"

namespace {

constexpr int VG_THREADS = 256;
// torchvision's ImageNet statistics, the constants of VGGLoss (losses/losses.py:80-90)
#define VG_MEAN0 0.485f
#define VG_MEAN1 0.456f
#define VG_MEAN2 0.406f
#define VG_STD0 0.229f
#define VG_STD1 0.224f
#define VG_STD2 0.225f

// one 16-byte chunk <-> its CH floats (constant indices only: the arrays stay in registers)
template <int DT> SRK_DEV void chunk_decode(const i32x4 raw, float (&v)[DTraits<DT>::CH]) {
  if constexpr (DTraits<DT>::IS16) {
    unpack2<DT>((uint32_t)raw.x, v[0], v[1]);
    unpack2<DT>((uint32_t)raw.y, v[2], v[3]);
    unpack2<DT>((uint32_t)raw.z, v[4], v[5]);
    unpack2<DT>((uint32_t)raw.w, v[6], v[7]);
  } else {
    v[0] = __int_as_float(raw.x);
    v[1] = __int_as_float(raw.y);
    v[2] = __int_as_float(raw.z);
    v[3] = __int_as_float(raw.w);
  }
}
template <int DT> SRK_DEV i32x4 chunk_encode(const float (&v)[DTraits<DT>::CH]) {
  i32x4 raw;
  if constexpr (DTraits<DT>::IS16) {
    raw.x = (int)pack2<DT>(v[0], v[1]);
    raw.y = (int)pack2<DT>(v[2], v[3]);
    raw.z = (int)pack2<DT>(v[4], v[5]);
    raw.w = (int)pack2<DT>(v[6], v[7]);
  } else {
    raw.x = __float_as_int(v[0]);
    raw.y = __float_as_int(v[1]);
    raw.z = __float_as_int(v[2]);
    raw.w = __float_as_int(v[3]);
  }
  return raw;
}
SRK_DEV void gstore16(void* p, i32x4 v) { *reinterpret_cast<i32x4*>(p) = v; }

// first / stride of a grid-stride walk
SRK_DEV long long vg_first() { return (long long)blockIdx.x * VG_THREADS + threadIdx.x; }
SRK_DEV long long vg_stride() { return (long long)gridDim.x * VG_THREADS; }

// ---- prepare: both images, normalised, into one NHWC batch of 16 channels ------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(VG_THREADS) void vgg_prepare_kernel(const srk_vgg_prepare_args a) {
  typedef DTraits<DT> Tr;
  const long long hw = (long long)a.H * a.W, total = (a.hr ? 2LL : 1LL) * a.N * hw;
  const i32x4 zero = {0, 0, 0, 0};
  for (long long p = vg_first(); p < total; p += vg_stride()) {
    const long long n = p / hw, r = p - n * hw;
    const float* src = n < a.N ? a.sr + n * 3 * hw : a.hr + (n - a.N) * 3 * hw;
    const float c0 = (src[r] - VG_MEAN0) / VG_STD0;
    const float c1 = (src[hw + r] - VG_MEAN1) / VG_STD1;
    const float c2 = (src[2 * hw + r] - VG_MEAN2) / VG_STD2;
    char* d = reinterpret_cast<char*>(a.dst) + p * (16 * (long long)sizeof(typename Tr::elem));
    if constexpr (Tr::IS16) {
      i32x4 lo = zero;
      lo.x = (int)pack2<DT>(c0, c1);
      lo.y = (int)pack2<DT>(c2, 0.f);
      gstore16(d, lo);
      gstore16(d + 16, zero);
    } else {
      i32x4 lo = zero;
      lo.x = __float_as_int(c0);
      lo.y = __float_as_int(c1);
      lo.z = __float_as_int(c2);
      gstore16(d, lo);
      gstore16(d + 16, zero);
      gstore16(d + 32, zero);
      gstore16(d + 48, zero);
    }
  }
}

// ---- 2 x 2 / stride 2 max-pool ------------------------------------------------------------------------------------------------
template <int DT>
__global__ __launch_bounds__(VG_THREADS) void vgg_pool_fwd_kernel(const srk_vgg_pool_args a) {
  typedef DTraits<DT> Tr;
  const int cpp = a.C / Tr::CH, Ho = a.H >> 1, Wo = a.W >> 1;
  const long long total = (long long)a.N * Ho * Wo * cpp;
  const long long col = 16LL * cpp, row = col * a.W;          // bytes to the next pixel / the next image row of x
  for (long long i = vg_first(); i < total; i += vg_stride()) {
    long long t = i / cpp;
    const int c = (int)(i - t * cpp);
    const int xo = (int)(t % Wo);
    t /= Wo;
    const int yo = (int)(t % Ho);
    const long long n = t / Ho;
    const char* w0 = reinterpret_cast<const char*>(a.x) + ((n * a.H + 2 * yo) * a.W + 2 * xo) * col + 16LL * c;
    float v0[Tr::CH], v1[Tr::CH], v2[Tr::CH], v3[Tr::CH], m[Tr::CH];
    chunk_decode<DT>(gload16(w0), v0);
    chunk_decode<DT>(gload16(w0 + col), v1);
    chunk_decode<DT>(gload16(w0 + row), v2);
    chunk_decode<DT>(gload16(w0 + row + col), v3);
#pragma unroll
    for (int e = 0; e < Tr::CH; ++e) m[e] = fmaxf(fmaxf(v0[e], v1[e]), fmaxf(v2[e], v3[e]));
    gstore16(reinterpret_cast<char*>(a.y) + 16 * i, chunk_encode<DT>(m));          // (a maximum is one of its inputs: exact)
  }
}

template <int DT>
__global__ __launch_bounds__(VG_THREADS) void vgg_pool_bwd_kernel(const srk_vgg_pool_args a) {
  typedef DTraits<DT> Tr;
  const int cpp = a.C / Tr::CH, Ho = a.H >> 1, Wo = a.W >> 1;
  const long long total = (long long)a.N * a.H * a.W * cpp;
  const long long col = 16LL * cpp, row = col * a.W;
  const i32x4 zero = {0, 0, 0, 0};
  for (long long i = vg_first(); i < total; i += vg_stride()) {
    long long t = i / cpp;
    const int c = (int)(i - t * cpp);
    const int x = (int)(t % a.W);
    t /= a.W;
    const int y = (int)(t % a.H);
    const long long n = t / a.H;
    const int yo = y >> 1, xo = x >> 1;
    i32x4 out = zero;
    if (yo < Ho && xo < Wo) {                      // (an odd last row / column belongs to no window)
      const char* w0 = reinterpret_cast<const char*>(a.x) + ((n * a.H + 2 * yo) * a.W + 2 * xo) * col + 16LL * c;
      const i32x4 r0 = gload16(w0), r1 = gload16(w0 + col), r2 = gload16(w0 + row), r3 = gload16(w0 + row + col);
      const i32x4 gr = gload16(reinterpret_cast<const char*>(a.gy) + (((n * Ho + yo) * Wo + xo) * cpp + c) * 16LL);
      const int k = ((y & 1) << 1) | (x & 1);      // this position's place in the window, row-major
      const i32x4 rk = k == 0 ? r0 : (k == 1 ? r1 : (k == 2 ? r2 : r3));
      float v0[Tr::CH], v1[Tr::CH], v2[Tr::CH], v3[Tr::CH], mine[Tr::CH], g[Tr::CH], o[Tr::CH];
      chunk_decode<DT>(r0, v0);
      chunk_decode<DT>(r1, v1);
      chunk_decode<DT>(r2, v2);
      chunk_decode<DT>(r3, v3);
      chunk_decode<DT>(rk, mine);
      chunk_decode<DT>(gr, g);
#pragma unroll
      for (int e = 0; e < Tr::CH; ++e) {
        const float m = fmaxf(fmaxf(v0[e], v1[e]), fmaxf(v2[e], v3[e]));
        // the FIRST maximum takes the gradient: no earlier position of the window holds the maximum too
        const bool earlier = (k > 0 && v0[e] == m) || (k > 1 && v1[e] == m) || (k > 2 && v2[e] == m);
        const bool take = mine[e] == m && !earlier && (!a.relu_mask || mine[e] > 0.f);
        o[e] = take ? g[e] : 0.f;
      }
      out = chunk_encode<DT>(o);                   // (g or 0: exact)
    }
    gstore16(reinterpret_cast<char*>(a.gx) + 16 * i, out);
  }
}

// ---- feature loss ----------------------------------------------------------------------------------------------------------------
SRK_DEV void vg_block_sum(double acc, double* slot) {
  __shared__ double red[VG_THREADS / 64];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = red[0];
#pragma unroll
    for (int w = 1; w < VG_THREADS / 64; ++w) t += red[w];
    *slot = t;
  }
}

template <int DT, int CRIT>
__global__ __launch_bounds__(VG_THREADS) void vgg_feat_fwd_kernel(const srk_vgg_feat_args a) {
  typedef DTraits<DT> Tr;
  const long long chunks = a.n / Tr::CH;
  double acc = 0.0;
  for (long long i = vg_first(); i < chunks; i += vg_stride()) {
    float s[Tr::CH], h[Tr::CH];
    chunk_decode<DT>(gload16(reinterpret_cast<const char*>(a.fs) + 16 * i), s);
    chunk_decode<DT>(gload16(reinterpret_cast<const char*>(a.fh) + 16 * i), h);
#pragma unroll
    for (int e = 0; e < Tr::CH; ++e) {
      const double d = (double)s[e] - (double)h[e];
      acc += CRIT == SRK_VGG_L2 ? d * d : fabs(d);
    }
  }
  vg_block_sum(acc, a.partial + blockIdx.x);
}

// one workgroup: thread t adds partials t, t + 256, ... in index order, then the fixed shuffle / LDS tree
__global__ __launch_bounds__(VG_THREADS) void vgg_feat_finalize_kernel(const srk_vgg_feat_args a, int nblocks) {
  double acc = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += VG_THREADS) acc += a.partial[b];
  __shared__ double total;
  vg_block_sum(acc, &total);
  if (threadIdx.x == 0) *a.loss = (float)((double)a.rescale * total / (double)a.n);
}

template <int DT, int CRIT>
__global__ __launch_bounds__(VG_THREADS) void vgg_feat_grad_kernel(const srk_vgg_feat_args a) {
  typedef DTraits<DT> Tr;
  const long long chunks = a.n / Tr::CH;
  for (long long i = vg_first(); i < chunks; i += vg_stride()) {
    float s[Tr::CH], h[Tr::CH], o[Tr::CH];
    chunk_decode<DT>(gload16(reinterpret_cast<const char*>(a.fs) + 16 * i), s);
    chunk_decode<DT>(gload16(reinterpret_cast<const char*>(a.fh) + 16 * i), h);
#pragma unroll
    for (int e = 0; e < Tr::CH; ++e) {
      const float d = s[e] - h[e];
      const float t = CRIT == SRK_VGG_L2 ? d : (float)((d > 0.f) - (d < 0.f));
      o[e] = s[e] > 0.f ? t : 0.f;                 // fs is a post-ReLU activation: the gradient with respect to its pre-activation
    }
    gstore16(reinterpret_cast<char*>(a.gf) + 16 * i, chunk_encode<DT>(o));
  }
}

// ---- ReLU in place: the end of a conv that fp32 storage runs as several launches over slices of its input channels ------------------------
template <int DT>
__global__ __launch_bounds__(VG_THREADS) void vgg_relu_kernel(const srk_vgg_relu_args a) {
  typedef DTraits<DT> Tr;
  const long long chunks = a.n / Tr::CH;
  for (long long i = vg_first(); i < chunks; i += vg_stride()) {
    float v[Tr::CH];
    char* p = reinterpret_cast<char*>(a.x) + 16 * i;
    chunk_decode<DT>(gload16(p), v);
#pragma unroll
    for (int e = 0; e < Tr::CH; ++e) v[e] = relu_f32(v[e]);
    gstore16(p, chunk_encode<DT>(v));
  }
}

// ---- the end of the backward chain: NHWC 16 channels -> NCHW fp32, every scalar applied here ------------------------------------------
template <int DT>
__global__ __launch_bounds__(VG_THREADS) void vgg_image_grad_kernel(const srk_vgg_image_grad_args a) {
  typedef DTraits<DT> Tr;
  const long long hw = (long long)a.H * a.W, total = (long long)a.N * hw;
  const float gs = *a.gout * a.scale;
  const float k0 = gs / VG_STD0, k1 = gs / VG_STD1, k2 = gs / VG_STD2;
  for (long long p = vg_first(); p < total; p += vg_stride()) {
    const long long n = p / hw, r = p - n * hw;
    float v[Tr::CH];
    chunk_decode<DT>(gload16(reinterpret_cast<const char*>(a.g) + p * (16 * (long long)sizeof(typename Tr::elem))), v);
    float* dst = a.grad + n * 3 * hw + r;
    dst[0] = v[0] * k0;
    dst[hw] = v[1] * k1;
    dst[2 * hw] = v[2] * k2;
  }
}

dim3 vg_grid(long long work) { return dim3((unsigned)srk_vgg_blocks(work)); }
bool vg_dtype_ok(int dt) { return dt == SRK_BF16 || dt == SRK_F16 || dt == SRK_F32; }
long long vg_elem_bytes(int dt) { return dt == SRK_F32 ? 4 : 2; }
bool vg_aligned(const void* p) { return (uintptr_t)p % 16 == 0; }

// launch KERNEL<dtype, ...> for the three storage dtypes
#define VG_LAUNCH_DT(KERNEL, dt, grid, st, ...)                                                              \
  do {                                                                                                       \
    if ((dt) == SRK_BF16) hipLaunchKernelGGL((KERNEL<SRK_BF16>), grid, dim3(VG_THREADS), 0, st, __VA_ARGS__); \
    else if ((dt) == SRK_F16) hipLaunchKernelGGL((KERNEL<SRK_F16>), grid, dim3(VG_THREADS), 0, st, __VA_ARGS__); \
    else hipLaunchKernelGGL((KERNEL<SRK_F32>), grid, dim3(VG_THREADS), 0, st, __VA_ARGS__);                   \
  } while (0)
#define VG_LAUNCH_DT_CRIT(KERNEL, dt, crit, grid, st, ...)                                                                  \
  do {                                                                                                                      \
    if ((crit) == SRK_VGG_L2) {                                                                                             \
      if ((dt) == SRK_BF16) hipLaunchKernelGGL((KERNEL<SRK_BF16, SRK_VGG_L2>), grid, dim3(VG_THREADS), 0, st, __VA_ARGS__);   \
      else if ((dt) == SRK_F16) hipLaunchKernelGGL((KERNEL<SRK_F16, SRK_VGG_L2>), grid, dim3(VG_THREADS), 0, st, __VA_ARGS__); \
      else hipLaunchKernelGGL((KERNEL<SRK_F32, SRK_VGG_L2>), grid, dim3(VG_THREADS), 0, st, __VA_ARGS__);                    \
    } else {                                                                                                                \
      if ((dt) == SRK_BF16) hipLaunchKernelGGL((KERNEL<SRK_BF16, SRK_VGG_L1>), grid, dim3(VG_THREADS), 0, st, __VA_ARGS__);   \
      else if ((dt) == SRK_F16) hipLaunchKernelGGL((KERNEL<SRK_F16, SRK_VGG_L1>), grid, dim3(VG_THREADS), 0, st, __VA_ARGS__); \
      else hipLaunchKernelGGL((KERNEL<SRK_F32, SRK_VGG_L1>), grid, dim3(VG_THREADS), 0, st, __VA_ARGS__);                    \
    }                                                                                                                       \
  } while (0)

}  // namespace

extern "C" int srk_vgg_blocks(long long chunks) {
  const long long b = (chunks + VG_THREADS - 1) / VG_THREADS;
  return (int)(b < 1 ? 1 : (b > SRK_VGG_BLOCKS_MAX ? SRK_VGG_BLOCKS_MAX : b));
}

extern "C" int srk_vgg_relu(const srk_vgg_relu_args* a, srk_stream_t stream) {
  SRK_CHECK_ARG(a && a->x && a->n > 0 && a->n % 16 == 0 && vg_dtype_ok(a->dtype), "srk_vgg_relu: null pointer / n not a positive multiple of 16 / unknown dtype");
  SRK_CHECK_ARG(vg_aligned(a->x), "srk_vgg_relu: 16-byte alignment");
  VG_LAUNCH_DT(vgg_relu_kernel, a->dtype, vg_grid(a->n * vg_elem_bytes(a->dtype) / 16), reinterpret_cast<hipStream_t>(stream), *a);
  SRK_LAUNCH_CHECK();
  return 0;
}

extern "C" int srk_vgg_prepare(const srk_vgg_prepare_args* a, srk_stream_t stream) {
  SRK_CHECK_ARG(a && a->sr && a->dst, "srk_vgg_prepare: null pointer");
  SRK_CHECK_ARG(a->N > 0 && a->H > 0 && a->W > 0 && vg_dtype_ok(a->dtype), "srk_vgg_prepare: empty image / unknown dtype %d", a->dtype);
  SRK_CHECK_ARG(vg_aligned(a->dst), "srk_vgg_prepare: 16-byte alignment");
  const long long pixels = (a->hr ? 2LL : 1LL) * a->N * a->H * a->W;
  VG_LAUNCH_DT(vgg_prepare_kernel, a->dtype, vg_grid(pixels), reinterpret_cast<hipStream_t>(stream), *a);
  SRK_LAUNCH_CHECK();
  return 0;
}

static int vg_pool_check(const srk_vgg_pool_args* a, const char* who) {
  SRK_CHECK_ARG(a && a->x, "%s: null pointer", who);
  SRK_CHECK_ARG(a->N > 0 && a->H >= 2 && a->W >= 2 && a->C >= 16 && a->C % 16 == 0 && vg_dtype_ok(a->dtype),
                "%s: needs N > 0, H, W >= 2, C a multiple of 16 and a known dtype (N %d H %d W %d C %d dtype %d)", who, a->N, a->H, a->W, a->C, a->dtype);
  return 0;
}
extern "C" int srk_vgg_pool_fwd(const srk_vgg_pool_args* a, srk_stream_t stream) {
  if (int rc = vg_pool_check(a, "srk_vgg_pool_fwd")) return rc;
  SRK_CHECK_ARG(a->y && vg_aligned(a->x) && vg_aligned(a->y), "srk_vgg_pool_fwd: null pointer / 16-byte alignment");
  const long long chunks = (long long)a->N * (a->H / 2) * (a->W / 2) * (a->C * vg_elem_bytes(a->dtype) / 16);
  VG_LAUNCH_DT(vgg_pool_fwd_kernel, a->dtype, vg_grid(chunks), reinterpret_cast<hipStream_t>(stream), *a);
  SRK_LAUNCH_CHECK();
  return 0;
}
extern "C" int srk_vgg_pool_bwd(const srk_vgg_pool_args* a, srk_stream_t stream) {
  if (int rc = vg_pool_check(a, "srk_vgg_pool_bwd")) return rc;
  SRK_CHECK_ARG(a->gy && a->gx && vg_aligned(a->x) && vg_aligned(a->gy) && vg_aligned(a->gx), "srk_vgg_pool_bwd: null pointer / 16-byte alignment");
  const long long chunks = (long long)a->N * a->H * a->W * (a->C * vg_elem_bytes(a->dtype) / 16);
  VG_LAUNCH_DT(vgg_pool_bwd_kernel, a->dtype, vg_grid(chunks), reinterpret_cast<hipStream_t>(stream), *a);
  SRK_LAUNCH_CHECK();
  return 0;
}

static int vg_feat_check(const srk_vgg_feat_args* a, const char* who) {
  SRK_CHECK_ARG(a && a->n > 0 && a->n % 16 == 0 && vg_dtype_ok(a->dtype) && (a->criterion == SRK_VGG_L2 || a->criterion == SRK_VGG_L1),
                "%s: needs n > 0, a multiple of 16, a known dtype and criterion", who);
  return 0;
}
extern "C" int srk_vgg_feat_fwd(const srk_vgg_feat_args* a, srk_stream_t stream) {
  if (int rc = vg_feat_check(a, "srk_vgg_feat_fwd")) return rc;
  SRK_CHECK_ARG(a->fs && a->fh && a->partial && vg_aligned(a->fs) && vg_aligned(a->fh), "srk_vgg_feat_fwd: null pointer / 16-byte alignment");
  const long long chunks = a->n * vg_elem_bytes(a->dtype) / 16;
  VG_LAUNCH_DT_CRIT(vgg_feat_fwd_kernel, a->dtype, a->criterion, vg_grid(chunks), reinterpret_cast<hipStream_t>(stream), *a);
  SRK_LAUNCH_CHECK();
  return 0;
}
extern "C" int srk_vgg_feat_finalize(const srk_vgg_feat_args* a, srk_stream_t stream) {
  if (int rc = vg_feat_check(a, "srk_vgg_feat_finalize")) return rc;
  SRK_CHECK_ARG(a->partial && a->loss, "srk_vgg_feat_finalize: null pointer");
  const int nblocks = srk_vgg_blocks(a->n * vg_elem_bytes(a->dtype) / 16);
  hipLaunchKernelGGL(vgg_feat_finalize_kernel, dim3(1), dim3(VG_THREADS), 0, reinterpret_cast<hipStream_t>(stream), *a, nblocks);
  SRK_LAUNCH_CHECK();
  return 0;
}
extern "C" int srk_vgg_feat_grad(const srk_vgg_feat_args* a, srk_stream_t stream) {
  if (int rc = vg_feat_check(a, "srk_vgg_feat_grad")) return rc;
  SRK_CHECK_ARG(a->fs && a->fh && a->gf && vg_aligned(a->fs) && vg_aligned(a->fh) && vg_aligned(a->gf), "srk_vgg_feat_grad: null pointer / 16-byte alignment");
  const long long chunks = a->n * vg_elem_bytes(a->dtype) / 16;
  VG_LAUNCH_DT_CRIT(vgg_feat_grad_kernel, a->dtype, a->criterion, vg_grid(chunks), reinterpret_cast<hipStream_t>(stream), *a);
  SRK_LAUNCH_CHECK();
  return 0;
}

extern "C" int srk_vgg_image_grad(const srk_vgg_image_grad_args* a, srk_stream_t stream) {
  SRK_CHECK_ARG(a && a->g && a->gout && a->grad, "srk_vgg_image_grad: null pointer");
  SRK_CHECK_ARG(a->N > 0 && a->H > 0 && a->W > 0 && vg_dtype_ok(a->dtype), "srk_vgg_image_grad: empty image / unknown dtype %d", a->dtype);
  SRK_CHECK_ARG(vg_aligned(a->g), "srk_vgg_image_grad: 16-byte alignment");
  VG_LAUNCH_DT(vgg_image_grad_kernel, a->dtype, vg_grid((long long)a->N * a->H * a->W), reinterpret_cast<hipStream_t>(stream), *a);
  SRK_LAUNCH_CHECK();
  return 0;
}
