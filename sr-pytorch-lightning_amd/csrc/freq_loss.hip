// Frequency-domain losses: the FFT loss (BasicSR's FFTLoss) and the focal frequency loss (Jiang et al., ICCV 2021): include/srk.h
// "frequency losses", sr_amd/freq_loss.py.  A direct matrix DFT of d = sr - hr per plane on the fp32 matrix pipe
// (v_mfma_f32_32x32x2_f32: A lane l holds A[l & 31][l >> 5], B lane l holds B[l >> 5][l & 31], C/D lane l holds column l & 31 and rows
// (r & 3) + 8 (r >> 2) + 4 (l >> 5) in register r; exact fp32, a k-ordered fmaf chain).
//   freq_spectrum_kernel<KIND, BWD>
//       one workgroup per (plane, block of 32 spectrum rows k of the half k = 0 .. H / 2), one wave per 32 columns (ceil(W / 32) waves):
//         stage 1   T[k][w] = sum_h e^{-2 pi i k h / H} d[h][w]: A = the H twiddles (LDS table, index (k h) mod H kept by integer
//                   steps), B = d read from sr and hr, 32 consecutive floats of a row per half wave; T (32 x W complex) to LDS;
//         stage 2   D[k][l] = sum_w T[k][w] e^{-2 pi i l w / W}: A = T from LDS (row pitch odd: no bank conflicts between rows),
//                   B = the W twiddles; Re D and Im D of a 32 x 32 tile in the wave's accumulators;
//         forward   the elementwise term on the accumulators, a fixed-order sum (and max) over the workgroup, two doubles per workgroup;
//         backward  G (the signs / 2 w D / (H W), times the row's count) over T in LDS, V[k][w] = sum_l G[k][l] e^{+2 pi i l w / W}
//                   (the same loop as stage 2 with the sine's sign turned) to the scratch buffer.
//   freq_adjoint_kernel   one workgroup per (plane, 32 columns w), one wave per 32 rows h: grad[h][w] = sum_k Re(e^{+2 pi i k h / H}
//                   V[k][w]) * scale * gout: A = the H twiddles, B = V, rows of 32 consecutive floats; every element written once.
//   freq_finalize_kernel  one workgroup: per plane the fixed-order double sum of its blocks (ffl: the max, q_max, the division by
//                   q_max^(alpha / 2)), then the fixed-order sum over planes.
// Ragged sizes are predicated: operands outside the plane are zeros, results outside it are dropped; the transform is never padded.
// Rows k > H / 2 follow from d being real (D[H - k][W - l] = conj D[k][l]): a row with 0 < 2k < H counts twice.
// No atomics, nothing read back on the host.  The library builds with -ffp-contract=off.
#include <math.h>
#include <stdint.h>

#include "srk_common.h"

namespace {

constexpr int KB = 32;                                // spectrum rows per workgroup; columns per wave
constexpr int MAX_WAVES = SRK_FREQ_MAX_SIZE / 32;     // 16 waves: 1024 threads
constexpr int FIN_THREADS = 1024;
enum { KIND_FFT = 0, KIND_FFL = 1 };

struct FreqArgs {                                     // what both losses' argument structs carry
  const float *sr, *hr;
  int N, C, H, W;
  float alpha;
  const float *tw_h, *tw_w;
  double* partial;
  float *qmax, *loss, *scratch;
  const float* gout;
  float* grad;
};

SRK_DEV f32x16 mma(float a, float b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0); }
SRK_DEV int acc_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// X[row][col] = sum_m (Pr + i Pi)[row][m] e^{-+ 2 pi i m col / n} for 32 rows held in LDS (pitch ld) and the wave's 32 columns
// col0 .. col0 + 31; `sgn` = 1: e^{-i} (the forward transform), -1: e^{+i} (its adjoint).  m runs to n in steps of 2; column m = n of
// an odd n is a zero column of P.
SRK_DEV void row_transform(const float* Pr, const float* Pi, int ld, const float* tc, const float* ts, int n, int col0, float sgn,
                           f32x16& xr, f32x16& xi) {
  const int lane = threadIdx.x & 63, i = lane & 31, half = lane >> 5;
  const int col = (col0 + i) % n;
  const int step = (2 * col) % n;
  int idx = half ? col : 0;                           // (m col) mod n at m = half
  const float* pr = Pr + i * ld + half;
  const float* pi = Pi + i * ld + half;
  // two steps per trip, unrolled by hand (a loop of MFMAs with a run-time trip count is not unrolled by the compiler): the second
  // step's reads are in flight under the first step's MFMAs.  Columns n .. of P are zeros up to the pitch.
  for (int m0 = 0; m0 < n; m0 += 4) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int m = m0 + 2 * u;
      const float c = tc[idx], s = sgn * ts[idx];
      const float ar = pr[m], ai = pi[m];
      xr = mma(ar, c, xr);
      xr = mma(ai, s, xr);
      xi = mma(ai, c, xi);
      xi = mma(ar, -s, xi);
      idx += step;
      if (idx >= n) idx -= n;
    }
  }
}

template <int KIND, bool BWD>
__global__ __launch_bounds__(MAX_WAVES * 64) void freq_spectrum_kernel(const FreqArgs a, int Hh, int kblocks, int ld) {
  extern __shared__ float lds[];
  float* Tr = lds;
  float* Ti = Tr + KB * ld;
  float* hc = Ti + KB * ld;
  float* hs = hc + a.H;
  float* wc = hs + a.H;
  float* ws = wc + a.W;
  __shared__ double red_s[MAX_WAVES];
  __shared__ float red_m[MAX_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  const int i = lane & 31, half = lane >> 5;
  const int H = a.H, W = a.W;
  // the row blocks of a plane read the same sr and hr: neighbours in `bid` share an XCD, and with it that L2
  const long long bid = xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const long long plane = bid / kblocks;
  const int k0 = (int)(bid - plane * kblocks) * KB;
  for (int t = tid; t < 2 * H; t += blockDim.x) hc[t] = a.tw_h[t];       // (hc, hs) and (wc, ws) are contiguous like the tables
  for (int t = tid; t < 2 * W; t += blockDim.x) wc[t] = a.tw_w[t];
  __syncthreads();

  // stage 1: the wave's 32 columns of T.  Lane (i, half) supplies the twiddle of row k0 + i at h + half and d[h + half][w0 + i].
  const int w0 = wave * 32;
  {
    const size_t base = (size_t)plane * H * W;
    const float* s = a.sr + base;
    const float* t = a.hr + base;
    const int kr = (k0 + i) % H;
    const int step = (2 * kr) % H;
    int idx = half ? kr : 0;
    const int w = w0 + i;
    const bool wok = w < W;
    const int wl = wok ? w : W - 1;                              // loads stay inside the plane and unconditional: four steps,
    f32x16 tr = {0}, ti = {0};                                   // unrolled by hand, keep their loads in flight
    for (int h0 = 0; h0 < H; h0 += 8) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {                              // (a step past H multiplies zeros)
        const int hh = h0 + 2 * u + half;
        const size_t o = (size_t)(hh < H ? hh : H - 1) * W + wl;
        const float v = s[o] - t[o];
        const float dv = (wok && hh < H) ? v : 0.f;
        tr = mma(hc[idx], dv, tr);
        ti = mma(-hs[idx], dv, ti);
        idx += step;
        if (idx >= H) idx -= H;
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = acc_row(r, half);
      Tr[row * ld + w] = tr[r];
      Ti[row * ld + w] = ti[r];
    }
  }
  __syncthreads();

  // stage 2: the wave's 32 x 32 tile of D
  f32x16 dr = {0}, di = {0};
  row_transform(Tr, Ti, ld, wc, ws, W, w0, 1.f, dr, di);

  const int l = w0 + i;
  const float inv_hw = 1.f / ((float)H * (float)W);
  const float ha = 0.5f * a.alpha;
  double sum = 0.0;
  float qm = 0.f;
  float gr[16], gi[16];
  float qplane = 0.f;
  if (BWD && KIND == KIND_FFL) qplane = a.qmax[plane];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int k = k0 + acc_row(r, half);
    const bool valid = k < Hh && l < W;
    const bool edge = k == 0 || 2 * k == H;                      // the row is its own mirror: it counts once
    const float cnt = edge ? 1.f : 2.f;
    const float re = dr[r];
    const float im = (edge && (2 * l) % W == 0) ? 0.f : di[r];   // a self-conjugate bin: Im D is 0, not a rounding residue
    if (KIND == KIND_FFT) {
      if (!BWD) {
        if (valid) sum += (double)(cnt * (fabsf(re) + fabsf(im)));
      } else {
        gr[r] = valid ? cnt * ((re > 0.f) - (re < 0.f)) : 0.f;
        gi[r] = valid ? cnt * ((im > 0.f) - (im < 0.f)) : 0.f;
      }
    } else {
      const float q = (re * re + im * im) * inv_hw;
      if (!BWD) {
        if (valid && q > 0.f) {
          sum += (double)cnt * ((double)q * (double)powf(q, ha));
          qm = fmaxf(qm, q);
        }
      } else {
        const float wgt = (valid && qplane > 0.f) ? powf(fminf(q / qplane, 1.f), ha) : 0.f;
        const float g = cnt * 2.f * wgt * inv_hw;
        gr[r] = g * re;
        gi[r] = g * im;
      }
    }
  }

  if (!BWD) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      sum += __shfl_down(sum, off, 64);
      qm = fmaxf(qm, __shfl_down(qm, off, 64));
    }
    if (lane == 0) {
      red_s[wave] = sum;
      red_m[wave] = qm;
    }
    __syncthreads();
    if (tid == 0) {
      double tot = 0.0;
      float m = 0.f;
      for (int v = 0; v < nw; ++v) {
        tot += red_s[v];
        m = fmaxf(m, red_m[v]);
      }
      a.partial[2 * (size_t)bid] = tot;
      a.partial[2 * (size_t)bid + 1] = (double)m;
    }
  } else {
    __syncthreads();                                             // every wave has read T
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int row = acc_row(r, half);
      Tr[row * ld + l] = gr[r];
      Ti[row * ld + l] = gi[r];
    }
    __syncthreads();
    f32x16 vr = {0}, vi = {0};
    row_transform(Tr, Ti, ld, wc, ws, W, w0, -1.f, vr, vi);
    if (l < W) {
      float* out = a.scratch + (size_t)plane * 2 * Hh * W;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int k = k0 + acc_row(r, half);
        if (k < Hh) {
          out[(size_t)k * W + l] = vr[r];
          out[((size_t)Hh + k) * W + l] = vi[r];
        }
      }
    }
  }
}

// grad[h][w] = scale * gout * sum_{k <= H / 2} (cos(2 pi k h / H) Vr[k][w] - sin(2 pi k h / H) Vi[k][w])
__global__ __launch_bounds__(MAX_WAVES * 64) void freq_adjoint_kernel(const FreqArgs a, int Hh, int wblocks, float scale) {
  __shared__ float hc[2 * SRK_FREQ_MAX_SIZE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = lane & 31, half = lane >> 5;
  const int H = a.H, W = a.W;
  const float* hs = hc + H;
  const long long plane = blockIdx.x / wblocks;
  const int w0 = (int)(blockIdx.x - plane * wblocks) * 32;
  for (int t = tid; t < 2 * H; t += blockDim.x) hc[t] = a.tw_h[t];
  __syncthreads();
  const float* Vr = a.scratch + (size_t)plane * 2 * Hh * W;
  const float* Vi = Vr + (size_t)Hh * W;
  const int h0 = wave * 32;
  const int hr = (h0 + i) % H;
  const int step = (2 * hr) % H;
  int idx = half ? hr : 0;
  const int w = w0 + i;
  const bool wok = w < W;
  const int wl = wok ? w : W - 1;                                // (unconditional loads inside the plane, as in stage 1)
  f32x16 g = {0};
  for (int k0 = 0; k0 < Hh; k0 += 8) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int kk = k0 + 2 * u + half;
      const bool in = wok && kk < Hh;
      const size_t o = (size_t)(kk < Hh ? kk : Hh - 1) * W + wl;
      const float vr = Vr[o], vi = Vi[o];
      const float br = in ? vr : 0.f, bi = in ? vi : 0.f;
      g = mma(hc[idx], br, g);
      g = mma(-hs[idx], bi, g);
      idx += step;
      if (idx >= H) idx -= H;
    }
  }
  if (wok) {
    const float gout = *a.gout;
    float* out = a.grad + (size_t)plane * H * W;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int h = h0 + acc_row(r, half);
      if (h < H) out[(size_t)h * W + w] = (g[r] * scale) * gout;   // the upstream gradient last, once: grad is linear in it
    }
  }
}

// thread-strided over the planes in index order, each plane's blocks in index order, a fixed shuffle tree, then the 16 waves in order
template <int KIND>
__global__ __launch_bounds__(FIN_THREADS) void freq_finalize_kernel(const FreqArgs a, long long planes, int kblocks, double denom) {
  __shared__ double red[FIN_THREADS / 64];
  double t = 0.0;
  for (long long p = threadIdx.x; p < planes; p += FIN_THREADS) {
    const double* q = a.partial + 2 * (size_t)p * kblocks;
    double s = 0.0, m = 0.0;
    for (int b = 0; b < kblocks; ++b) {
      s += q[2 * b];
      m = fmax(m, q[2 * b + 1]);
    }
    if (KIND == KIND_FFL) {
      a.qmax[p] = (float)m;                                      // (the max of fp32 values: exact)
      s = m > 0.0 ? s / pow(m, 0.5 * (double)a.alpha) : 0.0;
    }
    t += s;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) t += __shfl_down(t, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
#pragma unroll
    for (int v = 0; v < FIN_THREADS / 64; ++v) s += red[v];
    *a.loss = (float)(s / denom);
  }
}

struct FreqGeom {
  int Hh, kblocks, wblocks, hblocks, ld, lds_bytes;
  long long planes;
};

constexpr int lds_bytes_for(int H, int ld, int W) { return (2 * KB * ld + 2 * H + 2 * W) * (int)sizeof(float); }
constexpr int LDS_MAX = lds_bytes_for(SRK_FREQ_MAX_SIZE, SRK_FREQ_MAX_SIZE + 1, SRK_FREQ_MAX_SIZE);
static_assert(LDS_MAX <= 160 * 1024, "T, and the four tables, of the largest plane fit the CU's LDS");

int geometry(int N, int C, int H, int W, FreqGeom* g) {
  if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || H > SRK_FREQ_MAX_SIZE || W > SRK_FREQ_MAX_SIZE) return -1;
  g->planes = (long long)N * C;
  g->Hh = H / 2 + 1;
  g->kblocks = (g->Hh + KB - 1) / KB;
  g->wblocks = (W + 31) / 32;
  g->hblocks = (H + 31) / 32;
  g->ld = g->wblocks * 32 + 1;                       // odd: the 32 rows of an A operand fall into 32 different banks
  g->lds_bytes = lds_bytes_for(H, g->ld, W);
  // (plane, block) share one grid dimension, in either launch
  const long long lim = (1LL << 31) - 1;
  const int per = g->kblocks > g->wblocks ? g->kblocks : g->wblocks;
  if (g->planes > lim / per) return -1;
  return 0;
}

template <typename A> FreqArgs common(const A* a, float alpha, float* qmax) {
  return FreqArgs{a->sr, a->hr, a->N, a->C, a->H, a->W, alpha, a->tw_h, a->tw_w, a->partial, qmax, a->loss, a->scratch, a->gout, a->grad};
}

int check(const FreqArgs& a, const char* who, FreqGeom* g) {
  SRK_CHECK_ARG(a.sr && a.hr && a.tw_h && a.tw_w, "%s: null pointer", who);
  SRK_CHECK_ARG(geometry(a.N, a.C, a.H, a.W, g) == 0, "%s: %dx%dx%dx%d refused (1 <= H, W <= %d; planes x blocks below 2^31)", who, a.N, a.C,
                a.H, a.W, SRK_FREQ_MAX_SIZE);
  SRK_CHECK_ARG(a.alpha >= 0.f && a.alpha <= (float)SRK_FREQ_MAX_ALPHA, "%s: alpha=%g (0 <= alpha <= %d)", who, (double)a.alpha,
                SRK_FREQ_MAX_ALPHA);
  return 0;
}

template <int KIND, bool BWD> int launch_spectrum(const FreqArgs& a, const FreqGeom& g, hipStream_t st, const char* who) {
  // once per instantiation: the largest plane's T needs more than the 64 KiB a kernel gets by default
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(&freq_spectrum_kernel<KIND, BWD>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX);
  if (attr != hipSuccess) {
    srk_set_error("%s: cannot reserve %d bytes of LDS: %s", who, LDS_MAX, hipGetErrorString(attr));
    return (int)attr;
  }
  hipLaunchKernelGGL((freq_spectrum_kernel<KIND, BWD>), dim3((unsigned)(g.planes * g.kblocks)), dim3(64 * g.wblocks), g.lds_bytes, st, a,
                     g.Hh, g.kblocks, g.ld);
  SRK_LAUNCH_CHECK();
  return 0;
}

template <int KIND> int forward(const FreqArgs& a, srk_stream_t stream, const char* who) {
  FreqGeom g;
  if (int rc = check(a, who, &g)) return rc;
  SRK_CHECK_ARG(a.partial, "%s: null pointer", who);
  return launch_spectrum<KIND, false>(a, g, reinterpret_cast<hipStream_t>(stream), who);
}

template <int KIND> int finalize(const FreqArgs& a, srk_stream_t stream, const char* who) {
  FreqGeom g;
  if (int rc = check(a, who, &g)) return rc;
  SRK_CHECK_ARG(a.partial && a.loss && (KIND == KIND_FFT || a.qmax), "%s: null pointer", who);
  const double count = (double)g.planes * (double)a.H * (double)a.W;
  hipLaunchKernelGGL(freq_finalize_kernel<KIND>, dim3(1), dim3(FIN_THREADS), 0, reinterpret_cast<hipStream_t>(stream), a, g.planes, g.kblocks,
                     KIND == KIND_FFT ? 2.0 * count : count);
  SRK_LAUNCH_CHECK();
  return 0;
}

template <int KIND> int backward(const FreqArgs& a, srk_stream_t stream, const char* who) {
  FreqGeom g;
  if (int rc = check(a, who, &g)) return rc;
  SRK_CHECK_ARG(a.scratch && a.gout && a.grad && (KIND == KIND_FFT || a.qmax), "%s: null pointer", who);
  if (int rc = launch_spectrum<KIND, true>(a, g, reinterpret_cast<hipStream_t>(stream), who)) return rc;
  const double count = (double)g.planes * (double)a.H * (double)a.W;
  const float scale = (float)(1.0 / (KIND == KIND_FFT ? 2.0 * count : count));
  hipLaunchKernelGGL(freq_adjoint_kernel, dim3((unsigned)(g.planes * g.wblocks)), dim3(64 * g.hblocks), 0, reinterpret_cast<hipStream_t>(stream),
                     a, g.Hh, g.wblocks, scale);
  SRK_LAUNCH_CHECK();
  return 0;
}

}  // namespace

extern "C" int srk_freq_loss_tiles(int N, int C, int H, int W) {
  FreqGeom g;
  if (geometry(N, C, H, W, &g)) return -1;
  return (int)(g.planes * g.kblocks);
}

extern "C" int srk_fft_loss_fwd(const srk_fft_loss_args* a, srk_stream_t stream) {
  SRK_CHECK_ARG(a, "srk_fft_loss_fwd: null pointer");
  return forward<KIND_FFT>(common(a, 0.f, nullptr), stream, "srk_fft_loss_fwd");
}
extern "C" int srk_fft_loss_finalize(const srk_fft_loss_args* a, srk_stream_t stream) {
  SRK_CHECK_ARG(a, "srk_fft_loss_finalize: null pointer");
  return finalize<KIND_FFT>(common(a, 0.f, nullptr), stream, "srk_fft_loss_finalize");
}
extern "C" int srk_fft_loss_bwd(const srk_fft_loss_args* a, srk_stream_t stream) {
  SRK_CHECK_ARG(a, "srk_fft_loss_bwd: null pointer");
  return backward<KIND_FFT>(common(a, 0.f, nullptr), stream, "srk_fft_loss_bwd");
}
extern "C" int srk_ffl_loss_fwd(const srk_ffl_loss_args* a, srk_stream_t stream) {
  SRK_CHECK_ARG(a, "srk_ffl_loss_fwd: null pointer");
  return forward<KIND_FFL>(common(a, a->alpha, a->qmax), stream, "srk_ffl_loss_fwd");
}
extern "C" int srk_ffl_loss_finalize(const srk_ffl_loss_args* a, srk_stream_t stream) {
  SRK_CHECK_ARG(a, "srk_ffl_loss_finalize: null pointer");
  return finalize<KIND_FFL>(common(a, a->alpha, a->qmax), stream, "srk_ffl_loss_finalize");
}
extern "C" int srk_ffl_loss_bwd(const srk_ffl_loss_args* a, srk_stream_t stream) {
  SRK_CHECK_ARG(a, "srk_ffl_loss_bwd: null pointer");
  return backward<KIND_FFL>(common(a, a->alpha, a->qmax), stream, "srk_ffl_loss_bwd");
}
