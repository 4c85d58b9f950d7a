// Gradient clipping by norm and by value as launches of the training step (torch.nn.utils.clip_grad_norm_ with norm_type 2 /
// clip_grad_value_): the gradients are those of the optimizers' device table (srk_adam_slot / srk_adam_block, param_table.h), one
// workgroup per block of at most 4096 elements of ONE tensor, clipped in place.
//
// The thresholds, the last norm and coefficient and two counters live in DEVICE memory (srk.h: SRK_CLIP_*), so a captured hipGraph
// recomputes the norm of whatever its static gradients hold, counts its own clips and follows a threshold written between two replays.
//
//   sumsq : partials[base + b] = sum of g*g over block b, in double                                4 B per parameter
//   coef  : norm = sqrt(sum of every partial) / loss scale;  coef = min(1, max_norm / (norm + 1e-6))   one workgroup
//   apply : g *= coef; a workgroup that reads coef == 1 returns at once                           8 B per parameter, 0 B when nothing clips
//   value : g = clamp(g, -b, b) with a NaN kept                                                   8 B
// The sums use no atomics and need nothing zeroed: every partial is rewritten by its own workgroup, every order of addition is fixed,
// and the same gradients give the same bits, eager or replayed.  apply and value are streams over ONE array (the gradient) through
// param_table.h's table_walk; sumsq reads with the same alignment rule (16-byte loads when the block's gradient address allows).
#include "param_table.h"

namespace {

// The sum of one double per thread over the TABLE_NT threads of a workgroup in ONE fixed order (a pairwise tree in LDS); every thread
// returns it.
__device__ __forceinline__ double block_sum(double v, double* s) {
  s[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int w = TABLE_NT / 2; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) s[threadIdx.x] += s[threadIdx.x + w];
    __syncthreads();
  }
  return s[0];
}

// Thread t owns the 4-element groups t, t + TABLE_NT, ... of the block and, behind them, the tail elements 4 * n4 + t, ...; it adds
// their squares in that order.  The aligned path loads a group as 16 bytes (a full block: 4 loads per thread, all issued before the
// first use), the unaligned path (a gradient that is a view into a larger storage) as four scalars: the same values in the same order.
__global__ __launch_bounds__(TABLE_NT) void grad_sumsq_kernel(const srk_adam_slot* __restrict__ slots, const srk_adam_block* __restrict__ blocks,
                                                              double* __restrict__ partials) {
  __shared__ double s[TABLE_NT];
  const TableRange r = table_range(slots, blocks);
  const float* const g = r.sl.g + r.e0;
  const int n = (int)(r.e1 - r.e0), n4 = n >> 2;
  double acc = 0.0;
  auto add = [&](float v) { const double d = (double)v; acc += d * d; };
  if (((uintptr_t)g & 15) == 0) {
    for (int i0 = 0; i0 < n4; i0 += 4 * TABLE_NT) {
      f32x4 g4[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = i0 + u * TABLE_NT + threadIdx.x;
        g4[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (i < n4) g4[u] = *reinterpret_cast<const f32x4*>(g + 4 * i);
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (i0 + u * TABLE_NT + (int)threadIdx.x < n4) {
#pragma unroll
          for (int k = 0; k < 4; ++k) add(g4[u][k]);
        }
      }
    }
  } else {
    for (int i = threadIdx.x; i < n4; i += TABLE_NT) {
#pragma unroll
      for (int k = 0; k < 4; ++k) add(g[4 * i + k]);
    }
  }
  for (int e = 4 * n4 + threadIdx.x; e < n; e += TABLE_NT) add(g[e]);
  const double sum = block_sum(acc, s);
  if (threadIdx.x == 0) partials[blockIdx.x] = sum;
}

__global__ __launch_bounds__(TABLE_NT) void grad_clip_coef_kernel(float* __restrict__ state, const double* __restrict__ partials, int n,
                                                                  const float* __restrict__ scaler_state) {
  __shared__ double s[TABLE_NT];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += TABLE_NT) acc += partials[i];
  const double sum = block_sum(acc, s);
  if (threadIdx.x != 0) return;                              // one thread reads and writes the state: ordinary loads and stores
  const double scale = scaler_state ? (double)scaler_state[0] : 1.0;
  const double norm = sqrt(sum) / scale;
  float coef = 1.f;
  if (isfinite(norm)) {
    const double c = (double)state[SRK_CLIP_MAX_NORM] / (norm + 1e-6);
    coef = (float)(c < 1.0 ? c : 1.0);
    if (coef < 1.f) state[SRK_CLIP_NUM_CLIPPED] += 1.f;      // counted where apply will multiply: a double just below 1 may round to 1.f
  } else {
    state[SRK_CLIP_NUM_NONFINITE] += 1.f;
  }
  state[SRK_CLIP_TOTAL_NORM] = (float)norm;
  state[SRK_CLIP_COEF] = coef;
}

__global__ __launch_bounds__(TABLE_NT) void grad_clip_apply_kernel(const srk_adam_slot* __restrict__ slots, const srk_adam_block* __restrict__ blocks,
                                                                   const float* __restrict__ state) {
  const float c = state[SRK_CLIP_COEF];
  if (c == 1.f) return;                                      // nothing to clip: the gradient is not touched
  const TableRange r = table_range(slots, blocks);
  float* const x[1] = {const_cast<float*>(r.sl.g)};
  table_walk<1u, 1u, false>(x, nullptr, r.e0, r.e1, [&](float (&v)[1], float) { v[0] = v[0] * c; });
}

__global__ __launch_bounds__(TABLE_NT) void grad_clip_value_kernel(const srk_adam_slot* __restrict__ slots, const srk_adam_block* __restrict__ blocks,
                                                                   const float* __restrict__ state, const float* __restrict__ scaler_state) {
  float b = state[SRK_CLIP_CLIP_VALUE];
  if (scaler_state) b = b * scaler_state[0];                 // the gradients still carry the loss scale
  const float lo = -b;
  // Under the loss scaler an infinite gradient stays infinite: its check runs BEHIND this launch and must still skip the step, as
  // GradScaler.unscale_ (which records the overflow) runs before the clip in the torch recipe.  Without a scaler: torch.clamp's +-b.
  const float keep = scaler_state ? __builtin_inff() : __builtin_nanf("");   // |g| == keep passes unchanged (nothing equals a NaN)
  const TableRange r = table_range(slots, blocks);
  float* const x[1] = {const_cast<float*>(r.sl.g)};
  // compares and selects, not fminf / fmaxf: a NaN fails every compare and stays (torch.clamp; the loss scaler's check must still see it)
  table_walk<1u, 1u, false>(x, nullptr, r.e0, r.e1, [&](float (&v)[1], float) {
    const float gv = v[0];
    const float c = gv < lo ? lo : (gv > b ? b : gv);
    v[0] = __builtin_fabsf(gv) == keep ? gv : c;
  });
}

}  // namespace

#define SRK_CLIP_CHECK_TABLE(name)                                                                                          \
  SRK_CHECK_ARG(a && a->slots && a->blocks && a->state, name ": null pointer");                                             \
  SRK_CHECK_ARG(a->nblocks > 0 && a->nslots > 0, name ": %d blocks, %d tensors", a->nblocks, a->nslots)

extern "C" int srk_grad_sumsq(const srk_grad_clip_args* a, srk_stream_t stream) {
  SRK_CLIP_CHECK_TABLE("srk_grad_sumsq");
  SRK_CHECK_ARG(a->partials, "srk_grad_sumsq: no partials buffer");
  SRK_CHECK_ARG(a->base >= 0 && (long long)a->base + a->nblocks <= a->nblocks_total,
                "srk_grad_sumsq: blocks [%d, %d + %d) of %d partials", a->base, a->base, a->nblocks, a->nblocks_total);
  hipLaunchKernelGGL(grad_sumsq_kernel, dim3((unsigned)a->nblocks), dim3(TABLE_NT), 0, reinterpret_cast<hipStream_t>(stream), a->slots, a->blocks,
                     a->partials + a->base);
  SRK_LAUNCH_CHECK();
  return 0;
}

extern "C" int srk_grad_clip_coef(const srk_grad_clip_args* a, srk_stream_t stream) {
  SRK_CHECK_ARG(a && a->state && a->partials, "srk_grad_clip_coef: null pointer");
  SRK_CHECK_ARG(a->nblocks_total > 0, "srk_grad_clip_coef: %d partials", a->nblocks_total);
  hipLaunchKernelGGL(grad_clip_coef_kernel, dim3(1), dim3(TABLE_NT), 0, reinterpret_cast<hipStream_t>(stream), a->state, a->partials,
                     a->nblocks_total, a->scaler_state);
  SRK_LAUNCH_CHECK();
  return 0;
}

extern "C" int srk_grad_clip_apply(const srk_grad_clip_args* a, srk_stream_t stream) {
  SRK_CLIP_CHECK_TABLE("srk_grad_clip_apply");
  hipLaunchKernelGGL(grad_clip_apply_kernel, dim3((unsigned)a->nblocks), dim3(TABLE_NT), 0, reinterpret_cast<hipStream_t>(stream), a->slots,
                     a->blocks, a->state);
  SRK_LAUNCH_CHECK();
  return 0;
}

extern "C" int srk_grad_clip_value(const srk_grad_clip_args* a, srk_stream_t stream) {
  SRK_CLIP_CHECK_TABLE("srk_grad_clip_value");
  hipLaunchKernelGGL(grad_clip_value_kernel, dim3((unsigned)a->nblocks), dim3(TABLE_NT), 0, reinterpret_cast<hipStream_t>(stream), a->slots,
                     a->blocks, a->state, a->scaler_state);
  SRK_LAUNCH_CHECK();
  return 0;
}
