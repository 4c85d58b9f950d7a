// Adam update of every parameter tensor of a model in ONE launch.
//
// Replaces torch.optim.Adam.step() as the reference configures it (models/srmodel.py:145-154: `optim.Adam(trainable)` at
// torch's defaults; :602-603 drops every user-supplied hyper-parameter).  torch's fused implementation packs at most a few
// dozen tensors into one launch's arguments: RCAN's ~1,600 parameter tensors are 45 launches of ~28 us (1.3 ms of a 15 ms
// batch-16 step), EDSR-baseline's 4 launches are 7 % of its step.  Here the tensor list lives in a device table that is
// uploaded when the set of (parameter, gradient) addresses changes, and one grid walks all of it: HBM-bound
// (7 floats of traffic per parameter), ~0.1 ms for RCAN.
//
//   m = beta1*m + (1-beta1)*g;  v = beta2*v + (1-beta2)*g*g;
//   p -= lr/(1-beta1^t) * m / (sqrt(v)/sqrt(1-beta2^t) + eps)          (t = step count after this step, fp32 like torch)
// `weight_decay` is the L2 form (g += wd*p), `maximize` negates g: torch.optim.Adam's semantics.  The step counts (per tensor, as
// torch keeps them) live on the device so that hipGraph replays advance them: the update reads its tensor's count, a second
// tiny launch increments the counts of all tensors in the table.
#include "srk_common.h"

namespace {

constexpr int ADAM_NT = 256;

// Dynamic loss scaling on the DEVICE (fp16 training, the reference's `precision: 16` = Lightning's "16-mixed": autocast +
// torch.amp.GradScaler, configs/all.yml:122): state = {scale, growth tracker, found_inf, growth factor, backoff factor, growth
// interval, skipped steps}.  GradScaler reads found_inf on the HOST every step (`optimizer.step` is skipped from Python), which a
// hipGraph replay cannot do; here the check, the skip and the scale update are launches of the captured step:
//   adam_check_kernel  : found_inf = any gradient not finite           (the gradients are still multiplied by `scale`)
//   adam_group_kernel  : found_inf ? nothing : the update on g / scale
//   adam_bump_kernel   : found_inf ? nothing : step counts += 1
//   scaler_update      : found_inf ? (scale *= backoff, tracker = 0) : (++tracker == interval ? scale *= growth, tracker = 0); found_inf = 0
// -- torch.amp.GradScaler.step / update, same constants, same order.
__global__ __launch_bounds__(ADAM_NT) void adam_check_kernel(const srk_adam_args a, float* __restrict__ state) {
  const srk_adam_block blk = a.blocks[blockIdx.x];
  const srk_adam_slot sl = a.slots[blk.slot];
  const long long e0 = blk.start, e1 = (e0 + blk.count < sl.n) ? e0 + blk.count : sl.n;
  bool bad = false;
  for (long long e = e0 + threadIdx.x; e < e1; e += ADAM_NT) bad |= !isfinite(sl.g[e]);
  if (bad) state[2] = 1.f;                  // every writer stores the same value
}

__global__ void scaler_update_kernel(float* __restrict__ state) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (state[2] != 0.f) {
    state[0] *= state[4];
    state[1] = 0.f;
    state[6] += 1.f;
  } else {
    const float t = state[1] + 1.f;
    if (t >= state[5]) { state[0] *= state[3]; state[1] = 0.f; }
    else state[1] = t;
  }
  state[2] = 0.f;
}

template <bool SCALED>
__global__ __launch_bounds__(ADAM_NT) void adam_group_kernel(const srk_adam_args a, const float* __restrict__ state) {
  float inv_scale = 1.f;
  if constexpr (SCALED) {
    if (state[2] != 0.f) return;            // a non-finite gradient somewhere: the whole step is skipped
    inv_scale = 1.f / state[0];
  }
  const srk_adam_block blk = a.blocks[blockIdx.x];
  const srk_adam_slot sl = a.slots[blk.slot];
  const float t = a.steps[sl.step_idx] + 1.f;
  const float bc1 = 1.f - powf(a.beta1, t), bc2 = 1.f - powf(a.beta2, t);
  const float step_size = a.lr / bc1, bc2s = sqrtf(bc2);
  const float b2 = a.beta2, eps = a.eps, wd = a.weight_decay, omb1 = a.one_minus_beta1, omb2 = a.one_minus_beta2;
  const long long e0 = blk.start, e1 = (e0 + blk.count < sl.n) ? e0 + blk.count : sl.n;
  float* const p = sl.p;
  const float* const g = sl.g;
  float* const m = a.m + sl.state_off;
  float* const v = a.v + sl.state_off;
  auto upd = [&](float& pv, float gv, float& mv, float& vv) {
    if constexpr (SCALED) gv *= inv_scale;
    if (a.maximize) gv = -gv;
    if (wd != 0.f) gv += wd * pv;
    mv = mv + (gv - mv) * omb1;                             // torch: exp_avg.lerp_(grad, 1 - beta1)
    vv = b2 * vv + omb2 * gv * gv;                          //        exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    const float denom = sqrtf(vv) / bc2s + eps;
    pv -= step_size * (mv / denom);
  };
  // 16-byte accesses when all four arrays allow it (tensor starts inside the flat state buffers are 4-float aligned)
  const bool vec = ((((uintptr_t)p | (uintptr_t)g) & 15) == 0) && (sl.state_off & 3) == 0 && (e0 & 3) == 0;
  if (vec) {
    // 4 x float4 per array and thread, all 16 loads issued before the first use (a 4096-element block is one pass)
    const long long n4 = (e1 - e0) >> 2;
    for (long long i0 = 0; i0 < n4; i0 += 4 * ADAM_NT) {
      f32x4 p4[4], m4[4], v4[4], g4[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long long i = i0 + u * ADAM_NT + threadIdx.x;
        if (i < n4) {
          const long long e = e0 + 4 * i;
          p4[u] = *reinterpret_cast<const f32x4*>(p + e); g4[u] = *reinterpret_cast<const f32x4*>(g + e);
          m4[u] = *reinterpret_cast<const f32x4*>(m + e); v4[u] = *reinterpret_cast<const f32x4*>(v + e);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long long i = i0 + u * ADAM_NT + threadIdx.x;
        if (i < n4) {
          const long long e = e0 + 4 * i;
          float pv[4] = {p4[u].x, p4[u].y, p4[u].z, p4[u].w}, mv[4] = {m4[u].x, m4[u].y, m4[u].z, m4[u].w};
          float vv[4] = {v4[u].x, v4[u].y, v4[u].z, v4[u].w};
          const float gv[4] = {g4[u].x, g4[u].y, g4[u].z, g4[u].w};
#pragma unroll
          for (int k = 0; k < 4; ++k) upd(pv[k], gv[k], mv[k], vv[k]);
          *reinterpret_cast<f32x4*>(p + e) = f32x4{pv[0], pv[1], pv[2], pv[3]};
          *reinterpret_cast<f32x4*>(m + e) = f32x4{mv[0], mv[1], mv[2], mv[3]};
          *reinterpret_cast<f32x4*>(v + e) = f32x4{vv[0], vv[1], vv[2], vv[3]};
        }
      }
    }
    for (long long e = e0 + 4 * n4 + threadIdx.x; e < e1; e += ADAM_NT) upd(p[e], g[e], m[e], v[e]);
  } else {
    for (long long e = e0 + threadIdx.x; e < e1; e += ADAM_NT) upd(p[e], g[e], m[e], v[e]);
  }
}

// second launch of a step: the update has read every count, advance the counts of the tensors in the table.  (A "last block
// bumps" ticket inside the update costs one same-address atomic per block: 5k blocks serialise to 0.3 ms.)
__global__ __launch_bounds__(ADAM_NT) void adam_bump_kernel(const srk_adam_args a, const float* __restrict__ state) {
  if (state && state[2] != 0.f) return;
  for (int i = blockIdx.x * ADAM_NT + threadIdx.x; i < a.nslots; i += gridDim.x * ADAM_NT) a.steps[a.slots[i].step_idx] += 1.f;
}


// ---- Ranger (torch_optimizer 0.3.0 `Ranger` = RAdam + Lookahead) over the same table ---------------------------------------
// Per tensor, t = its step count after this step (srk.h has the rule).  The branches -- rectified or not (N_sma > threshold) and
// the Lookahead sync (t % k == 0) -- are decided HERE from the device count, so a replayed hipGraph takes the branch of the
// step it replays, not the one of the step it was captured at.  N_sma and the step size are formed in DOUBLE from double
// hyper-parameters (N_sma cancels: 1999 - 1993.0 at t = 6, so fp32 scalars are off by 0.57 %), then -s*lr is rounded to fp32
// once, as torch rounds a Python scalar; the per-element arithmetic is fp32 in the package's order.
// Traffic: p, m, v read + written, g read = 28 B per parameter; a sync step adds the slow buffer (36 B).  Both branches are
// uniform per block (one tensor per block), so the slow buffer is touched only on sync steps and at t = 1 (slow = p).

// the element arithmetic of one block, with the block-uniform decisions made
struct RangerBlock {
  float* p; const float* g; float* m; float* v; float* slow;
  long long e0, e1;
  float inv_scale, step, decay, b1, b2, omb1, omb2, eps, alpha;
  bool wd, rect, sync, first;
};

// READ_SLOW (a sync step after the first): the slow weights are loaded.  A template, not a runtime select on the load: the
// conditional 16-byte loads doubled the register count (210 VGPRs, occupancy 2 against 130 / 3 this way).
template <bool SCALED, bool READ_SLOW>
__device__ __forceinline__ void ranger_block(const RangerBlock& b) {
  const bool write_slow = b.sync || b.first;
  // sv: the slow weight on entry (READ_SLOW), written back when write_slow.  Selects, not branches: the flags are block-uniform
  auto upd = [&](float& pv, float gv, float& mv, float& vv, float& sv) {
    if constexpr (SCALED) gv *= b.inv_scale;
    sv = b.first ? pv : sv;                                  // slow_buffer.copy_(p) at the tensor's first step
    vv = vv * b.b2 + b.omb2 * gv * gv;                       // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    mv = mv * b.b1 + b.omb1 * gv;                            // exp_avg.mul_(beta1).add_(grad, alpha=1 - beta1)
    pv = b.wd ? pv + b.decay * pv : pv;                      // p.add_(p, alpha=-wd * lr)
    const float u = b.rect ? mv / (sqrtf(vv) + b.eps) : mv;  // p.addcdiv_(exp_avg, exp_avg_sq.sqrt().add_(eps), value=-s * lr)
    pv = pv + b.step * u;                                    //   or p.add_(exp_avg, alpha=-s * lr)
    sv = b.sync ? sv + b.alpha * (pv - sv) : sv;             // slow.add_(p - slow, alpha=alpha); p.copy_(slow)
    pv = b.sync ? sv : pv;
  };
  float* const p = b.p;
  const float* const g = b.g;
  float* const m = b.m;
  float* const v = b.v;
  float* const slow = b.slow;
  auto upd1 = [&](long long e) {
    float pv = p[e], mv = m[e], vv = v[e], sv = 0.f;
    if constexpr (READ_SLOW) sv = slow[e];
    upd(pv, g[e], mv, vv, sv);
    p[e] = pv; m[e] = mv; v[e] = vv;
    if (write_slow) slow[e] = sv;
  };
  const long long e0 = b.e0, e1 = b.e1;
  const bool vec = ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)slow) & 15) == 0) && (e0 & 3) == 0;
  if (vec) {
    const long long n4 = (e1 - e0) >> 2;
    for (long long i0 = 0; i0 < n4; i0 += 4 * ADAM_NT) {
      f32x4 p4[4], m4[4], v4[4], g4[4], s4[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long long i = i0 + u * ADAM_NT + threadIdx.x;
        s4[u] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (i < n4) {
          const long long e = e0 + 4 * i;
          p4[u] = *reinterpret_cast<const f32x4*>(p + e); g4[u] = *reinterpret_cast<const f32x4*>(g + e);
          m4[u] = *reinterpret_cast<const f32x4*>(m + e); v4[u] = *reinterpret_cast<const f32x4*>(v + e);
          if constexpr (READ_SLOW) s4[u] = *reinterpret_cast<const f32x4*>(slow + e);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long long i = i0 + u * ADAM_NT + threadIdx.x;
        if (i < n4) {
          const long long e = e0 + 4 * i;
          float pv[4] = {p4[u].x, p4[u].y, p4[u].z, p4[u].w}, mv[4] = {m4[u].x, m4[u].y, m4[u].z, m4[u].w};
          float vv[4] = {v4[u].x, v4[u].y, v4[u].z, v4[u].w}, sv[4] = {s4[u].x, s4[u].y, s4[u].z, s4[u].w};
          const float gv[4] = {g4[u].x, g4[u].y, g4[u].z, g4[u].w};
#pragma unroll
          for (int k = 0; k < 4; ++k) upd(pv[k], gv[k], mv[k], vv[k], sv[k]);
          *reinterpret_cast<f32x4*>(p + e) = f32x4{pv[0], pv[1], pv[2], pv[3]};
          *reinterpret_cast<f32x4*>(m + e) = f32x4{mv[0], mv[1], mv[2], mv[3]};
          *reinterpret_cast<f32x4*>(v + e) = f32x4{vv[0], vv[1], vv[2], vv[3]};
          if (write_slow) *reinterpret_cast<f32x4*>(slow + e) = f32x4{sv[0], sv[1], sv[2], sv[3]};
        }
      }
    }
    for (long long e = e0 + 4 * n4 + threadIdx.x; e < e1; e += ADAM_NT) upd1(e);
  } else {
    for (long long e = e0 + threadIdx.x; e < e1; e += ADAM_NT) upd1(e);
  }
}

template <bool SCALED>
__global__ __launch_bounds__(ADAM_NT) void ranger_group_kernel(const srk_ranger_args a, const float* __restrict__ state) {
  RangerBlock b;
  b.inv_scale = 1.f;
  if constexpr (SCALED) {
    if (state[2] != 0.f) return;            // a non-finite gradient somewhere: the whole step is skipped
    b.inv_scale = 1.f / state[0];
  }
  const srk_adam_block blk = a.blocks[blockIdx.x];
  const srk_adam_slot sl = a.slots[blk.slot];
  const long long t = (long long)a.steps[sl.step_idx] + 1;
  const double td = (double)t, b2t = pow(a.beta2, td);
  const double n_max = 2.0 / (1.0 - a.beta2) - 1.0;
  const double n_sma = n_max - 2.0 * td * b2t / (1.0 - b2t);
  b.rect = n_sma > a.n_sma_threshold;
  const double s = b.rect ? sqrt((1.0 - b2t) * (n_sma - 4.0) / (n_max - 4.0) * (n_sma - 2.0) / n_sma * n_max / (n_max - 2.0)) / (1.0 - pow(a.beta1, td))
                          : 1.0 / (1.0 - pow(a.beta1, td));
  b.step = (float)(-s * a.lr);
  b.decay = (float)(-a.weight_decay * a.lr);
  b.b1 = (float)a.beta1; b.b2 = (float)a.beta2; b.omb1 = (float)(1.0 - a.beta1); b.omb2 = (float)(1.0 - a.beta2);
  b.eps = (float)a.eps; b.alpha = (float)a.alpha;
  b.wd = a.weight_decay != 0.0; b.sync = t % a.k == 0; b.first = t == 1;
  b.e0 = blk.start; b.e1 = (b.e0 + blk.count < sl.n) ? b.e0 + blk.count : sl.n;
  b.p = sl.p; b.g = sl.g;
  b.m = a.m + sl.state_off; b.v = a.v + sl.state_off; b.slow = a.slow + sl.state_off;
  if (b.sync && !b.first) ranger_block<SCALED, true>(b);
  else ranger_block<SCALED, false>(b);
}

// second launch of a Ranger step: advance the counts of the tensors in the table (adam_bump_kernel's job, on the Ranger table)
__global__ __launch_bounds__(ADAM_NT) void ranger_bump_kernel(const srk_ranger_args a, const float* __restrict__ state) {
  if (state && state[2] != 0.f) return;
  for (int i = blockIdx.x * ADAM_NT + threadIdx.x; i < a.nslots; i += gridDim.x * ADAM_NT) a.steps[a.slots[i].step_idx] += 1.f;
}

}  // namespace

extern "C" int srk_adam_step(const srk_adam_args* a, srk_stream_t stream) {
  SRK_CHECK_ARG(a && a->slots && a->blocks && a->m && a->v && a->steps, "srk_adam_step: null pointer");
  SRK_CHECK_ARG(a->nblocks > 0 && a->nslots > 0, "srk_adam_step: %d blocks, %d tensors", a->nblocks, a->nslots);
  SRK_CHECK_ARG(a->beta1 >= 0.f && a->beta1 < 1.f && a->beta2 >= 0.f && a->beta2 < 1.f && a->eps >= 0.f && a->lr >= 0.f,
                "srk_adam_step: lr=%g betas=(%g, %g) eps=%g", a->lr, a->beta1, a->beta2, a->eps);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(adam_group_kernel<false>, dim3((unsigned)a->nblocks), dim3(ADAM_NT), 0, st, *a, (const float*)nullptr);
  hipLaunchKernelGGL(adam_bump_kernel, dim3((unsigned)((a->nslots + ADAM_NT - 1) / ADAM_NT)), dim3(ADAM_NT), 0, st, *a, (const float*)nullptr);
  SRK_LAUNCH_CHECK();
  return 0;
}

extern "C" int srk_adam_step_scaled(const srk_adam_args* a, float* scaler_state, srk_stream_t stream) {
  SRK_CHECK_ARG(a && a->slots && a->blocks && a->m && a->v && a->steps && scaler_state, "srk_adam_step_scaled: null pointer");
  SRK_CHECK_ARG(a->nblocks > 0 && a->nslots > 0, "srk_adam_step_scaled: %d blocks, %d tensors", a->nblocks, a->nslots);
  SRK_CHECK_ARG(a->beta1 >= 0.f && a->beta1 < 1.f && a->beta2 >= 0.f && a->beta2 < 1.f && a->eps >= 0.f && a->lr >= 0.f,
                "srk_adam_step_scaled: lr=%g betas=(%g, %g) eps=%g", a->lr, a->beta1, a->beta2, a->eps);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(adam_check_kernel, dim3((unsigned)a->nblocks), dim3(ADAM_NT), 0, st, *a, scaler_state);
  hipLaunchKernelGGL(adam_group_kernel<true>, dim3((unsigned)a->nblocks), dim3(ADAM_NT), 0, st, *a, (const float*)scaler_state);
  hipLaunchKernelGGL(adam_bump_kernel, dim3((unsigned)((a->nslots + ADAM_NT - 1) / ADAM_NT)), dim3(ADAM_NT), 0, st, *a, (const float*)scaler_state);
  SRK_LAUNCH_CHECK();
  return 0;
}

/* Several parameter groups: GradScaler.step unscales and checks EVERY group before any is updated -- an inf in group 1
 * must not leave group 0 already stepped.  srk_adam_check_scaled over all groups first, then srk_adam_update_scaled per group. */
extern "C" int srk_adam_check_scaled(const srk_adam_args* a, float* scaler_state, srk_stream_t stream) {
  SRK_CHECK_ARG(a && a->slots && a->blocks && scaler_state, "srk_adam_check_scaled: null pointer");
  SRK_CHECK_ARG(a->nblocks > 0 && a->nslots > 0, "srk_adam_check_scaled: %d blocks, %d tensors", a->nblocks, a->nslots);
  hipLaunchKernelGGL(adam_check_kernel, dim3((unsigned)a->nblocks), dim3(ADAM_NT), 0, reinterpret_cast<hipStream_t>(stream), *a, scaler_state);
  SRK_LAUNCH_CHECK();
  return 0;
}

extern "C" int srk_adam_update_scaled(const srk_adam_args* a, const float* scaler_state, srk_stream_t stream) {
  SRK_CHECK_ARG(a && a->slots && a->blocks && a->m && a->v && a->steps && scaler_state, "srk_adam_update_scaled: null pointer");
  SRK_CHECK_ARG(a->nblocks > 0 && a->nslots > 0, "srk_adam_update_scaled: %d blocks, %d tensors", a->nblocks, a->nslots);
  SRK_CHECK_ARG(a->beta1 >= 0.f && a->beta1 < 1.f && a->beta2 >= 0.f && a->beta2 < 1.f && a->eps >= 0.f && a->lr >= 0.f,
                "srk_adam_update_scaled: lr=%g betas=(%g, %g) eps=%g", a->lr, a->beta1, a->beta2, a->eps);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(adam_group_kernel<true>, dim3((unsigned)a->nblocks), dim3(ADAM_NT), 0, st, *a, scaler_state);
  hipLaunchKernelGGL(adam_bump_kernel, dim3((unsigned)((a->nslots + ADAM_NT - 1) / ADAM_NT)), dim3(ADAM_NT), 0, st, *a, scaler_state);
  SRK_LAUNCH_CHECK();
  return 0;
}

/* after the LAST parameter group's srk_adam_step_scaled of a step: the scale / growth-tracker update (one thread) */
extern "C" int srk_loss_scale_update(float* scaler_state, srk_stream_t stream) {
  SRK_CHECK_ARG(scaler_state, "srk_loss_scale_update: null pointer");
  hipLaunchKernelGGL(scaler_update_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), scaler_state);
  SRK_LAUNCH_CHECK();
  return 0;
}


// ---- Ranger entry points: the same four shapes as Adam's (one group; one group under loss scaling; check / update halves) ----
namespace {
int ranger_check_args(const srk_ranger_args* a, const char* fn) {
  SRK_CHECK_ARG(a && a->slots && a->blocks && a->m && a->v && a->slow && a->steps, "%s: null pointer", fn);
  SRK_CHECK_ARG(a->nblocks > 0 && a->nslots > 0, "%s: %d blocks, %d tensors", fn, a->nblocks, a->nslots);
  SRK_CHECK_ARG(a->lr > 0.0 && a->alpha >= 0.0 && a->alpha <= 1.0 && a->k >= 1 && a->beta1 >= 0.0 && a->beta1 < 1.0 &&
                a->beta2 >= 0.0 && a->beta2 < 1.0 && a->eps >= 0.0 && a->weight_decay >= 0.0,
                "%s: lr=%g alpha=%g k=%d betas=(%g, %g) eps=%g weight_decay=%g", fn, a->lr, a->alpha, a->k, a->beta1, a->beta2,
                a->eps, a->weight_decay);
  return 0;
}

void ranger_launch(const srk_ranger_args* a, const float* scaler_state, hipStream_t st) {
  if (scaler_state) hipLaunchKernelGGL(ranger_group_kernel<true>, dim3((unsigned)a->nblocks), dim3(ADAM_NT), 0, st, *a, scaler_state);
  else hipLaunchKernelGGL(ranger_group_kernel<false>, dim3((unsigned)a->nblocks), dim3(ADAM_NT), 0, st, *a, scaler_state);
  hipLaunchKernelGGL(ranger_bump_kernel, dim3((unsigned)((a->nslots + ADAM_NT - 1) / ADAM_NT)), dim3(ADAM_NT), 0, st, *a, scaler_state);
}

// the gradient check is Adam's: it reads the table only
void ranger_check_launch(const srk_ranger_args* a, float* scaler_state, hipStream_t st) {
  srk_adam_args c{};
  c.slots = a->slots; c.blocks = a->blocks; c.nslots = a->nslots; c.nblocks = a->nblocks;
  hipLaunchKernelGGL(adam_check_kernel, dim3((unsigned)a->nblocks), dim3(ADAM_NT), 0, st, c, scaler_state);
}
}  // namespace

extern "C" int srk_ranger_step(const srk_ranger_args* a, srk_stream_t stream) {
  if (int rc = ranger_check_args(a, "srk_ranger_step")) return rc;
  ranger_launch(a, nullptr, reinterpret_cast<hipStream_t>(stream));
  SRK_LAUNCH_CHECK();
  return 0;
}

extern "C" int srk_ranger_step_scaled(const srk_ranger_args* a, float* scaler_state, srk_stream_t stream) {
  if (int rc = ranger_check_args(a, "srk_ranger_step_scaled")) return rc;
  SRK_CHECK_ARG(scaler_state, "srk_ranger_step_scaled: null scaler state");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  ranger_check_launch(a, scaler_state, st);
  ranger_launch(a, scaler_state, st);
  SRK_LAUNCH_CHECK();
  return 0;
}

extern "C" int srk_ranger_check_scaled(const srk_ranger_args* a, float* scaler_state, srk_stream_t stream) {
  SRK_CHECK_ARG(a && a->slots && a->blocks && scaler_state, "srk_ranger_check_scaled: null pointer");
  SRK_CHECK_ARG(a->nblocks > 0 && a->nslots > 0, "srk_ranger_check_scaled: %d blocks, %d tensors", a->nblocks, a->nslots);
  ranger_check_launch(a, scaler_state, reinterpret_cast<hipStream_t>(stream));
  SRK_LAUNCH_CHECK();
  return 0;
}

extern "C" int srk_ranger_update_scaled(const srk_ranger_args* a, const float* scaler_state, srk_stream_t stream) {
  if (int rc = ranger_check_args(a, "srk_ranger_update_scaled")) return rc;
  SRK_CHECK_ARG(scaler_state, "srk_ranger_update_scaled: null scaler state");
  ranger_launch(a, scaler_state, reinterpret_cast<hipStream_t>(stream));
  SRK_LAUNCH_CHECK();
  return 0;
}


// ---- SGD and RMSprop (torch.optim.SGD / torch.optim.RMSprop) over the same table ---------------------------------------------
// The models' `optimizer="SGD"` / `"RMSprop"` (reference models/srmodel.py:57-64).  torch's foreach step packs a few dozen tensors
// per launch and makes one pass per _foreach_* op: for RCAN's ~1,600 tensors that is Adam's launch storm once per pass.  Here:
// one launch over Adam's table, one tensor per block, so every per-tensor decision is block-uniform.  srk.h has the rules; the
// element arithmetic is fp32 in the order of torch's _single_tensor_sgd / _single_tensor_rmsprop, and every scalar (-lr,
// 1 - dampening, 1 - alpha) is formed in double and rounded to fp32 once, as torch rounds a Python scalar.
// Only the state a configuration uses is touched: SGD 12 B per parameter (p read + written, g read), 20 B with momentum;
// RMSprop 20 B (square_avg too), +8 B with momentum, +8 B centered.
namespace {

// The elements [e0, e1) of one tensor with NS flat state arrays beside p and g: 16-byte accesses when every address allows it,
// 4 x float4 per array and thread with all loads issued before the first use (a 4096-element block is one pass), scalar tail.
// upd(p, g, s[NS]) is the element rule.  READ0 = false: state array 0 is written without being read (SGD's momentum buffer at a
// tensor's first step) -- a template, not a runtime select on the load, for the reason given at ranger_block.
template <int NS, bool READ0, class F>
__device__ __forceinline__ void state_block(float* const p, const float* const g, float* const (&s)[NS > 0 ? NS : 1],
                                            const long long e0, const long long e1, F upd) {
  constexpr int NA = NS > 0 ? NS : 1;
  auto upd1 = [&](long long e) {
    float pv = p[e], sv[NA] = {};
#pragma unroll
    for (int j = 0; j < NS; ++j)
      if (READ0 || j > 0) sv[j] = s[j][e];
    upd(pv, g[e], sv);
    p[e] = pv;
#pragma unroll
    for (int j = 0; j < NS; ++j) s[j][e] = sv[j];
  };
  uintptr_t bits = (uintptr_t)p | (uintptr_t)g;
#pragma unroll
  for (int j = 0; j < NS; ++j) bits |= (uintptr_t)s[j];
  const bool vec = (bits & 15) == 0 && (e0 & 3) == 0;
  if (vec) {
    const long long n4 = (e1 - e0) >> 2;
    for (long long i0 = 0; i0 < n4; i0 += 4 * ADAM_NT) {
      f32x4 p4[4], g4[4], s4[NA][4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long long i = i0 + u * ADAM_NT + threadIdx.x;
#pragma unroll
        for (int j = 0; j < NA; ++j) s4[j][u] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (i < n4) {
          const long long e = e0 + 4 * i;
          p4[u] = *reinterpret_cast<const f32x4*>(p + e); g4[u] = *reinterpret_cast<const f32x4*>(g + e);
#pragma unroll
          for (int j = 0; j < NS; ++j)
            if (READ0 || j > 0) s4[j][u] = *reinterpret_cast<const f32x4*>(s[j] + e);
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const long long i = i0 + u * ADAM_NT + threadIdx.x;
        if (i < n4) {
          const long long e = e0 + 4 * i;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            float pv = p4[u][k], sv[NA] = {};
#pragma unroll
            for (int j = 0; j < NS; ++j) sv[j] = s4[j][u][k];
            upd(pv, g4[u][k], sv);
            p4[u][k] = pv;
#pragma unroll
            for (int j = 0; j < NS; ++j) s4[j][u][k] = sv[j];
          }
          *reinterpret_cast<f32x4*>(p + e) = p4[u];
#pragma unroll
          for (int j = 0; j < NS; ++j) *reinterpret_cast<f32x4*>(s[j] + e) = s4[j][u];
        }
      }
    }
    for (long long e = e0 + 4 * n4 + threadIdx.x; e < e1; e += ADAM_NT) upd1(e);
  } else {
    for (long long e = e0 + threadIdx.x; e < e1; e += ADAM_NT) upd1(e);
  }
}

// torch.optim.SGD.  "first" -- torch creates momentum_buffer as a clone of the first gradient a tensor ever receives, whatever
// `dampening` says -- is read from the tensor's DEVICE count, so a replayed hipGraph gives a tensor whose first gradient arrives
// at a later step the right branch, and a step skipped under loss scaling leaves the tensor "first".
template <bool SCALED, bool MOM>
__global__ __launch_bounds__(ADAM_NT) void sgd_group_kernel(const srk_sgd_args a, const float* __restrict__ state) {
  float inv_scale = 1.f;
  if constexpr (SCALED) {
    if (state[2] != 0.f) return;            // a non-finite gradient somewhere: the whole step is skipped
    inv_scale = 1.f / state[0];
  }
  const srk_adam_block blk = a.blocks[blockIdx.x];
  const srk_adam_slot sl = a.slots[blk.slot];
  const float mom = (float)a.momentum, omd = (float)(1.0 - a.dampening), wd = (float)a.weight_decay, nlr = (float)(-a.lr);
  const bool has_wd = a.weight_decay != 0.0, nesterov = a.nesterov != 0, maximize = a.maximize != 0;
  bool first = false;
  if constexpr (MOM) first = a.steps[sl.step_idx] == 0.f;
  const long long e0 = blk.start, e1 = (e0 + blk.count < sl.n) ? e0 + blk.count : sl.n;
  auto upd = [&](float& pv, float gv, float (&sv)[1]) {
    if constexpr (SCALED) gv *= inv_scale;
    gv = maximize ? -gv : gv;
    gv = has_wd ? gv + wd * pv : gv;                          // grad.add(param, alpha=weight_decay)
    if constexpr (MOM) {
      const float b = first ? gv : sv[0] * mom + omd * gv;    // buf = grad.clone()  or  buf.mul_(momentum).add_(grad, alpha=1 - dampening)
      sv[0] = b;
      gv = nesterov ? gv + mom * b : b;                       // grad.add(buf, alpha=momentum)  or  buf
    }
    pv = pv + nlr * gv;                                       // param.add_(grad, alpha=-lr)
  };
  if constexpr (MOM) {
    float* const s[1] = {a.buf + sl.state_off};
    if (first) state_block<1, false>(sl.p, sl.g, s, e0, e1, upd);
    else state_block<1, true>(sl.p, sl.g, s, e0, e1, upd);
  } else {
    float* const s[1] = {nullptr};
    state_block<0, false>(sl.p, sl.g, s, e0, e1, upd);
  }
}

// torch.optim.RMSprop.  State arrays in the order square_avg, [momentum_buffer], [grad_avg].
template <bool SCALED, bool MOM, bool CENTERED>
__global__ __launch_bounds__(ADAM_NT) void rmsprop_group_kernel(const srk_rmsprop_args a, const float* __restrict__ state) {
  float inv_scale = 1.f;
  if constexpr (SCALED) {
    if (state[2] != 0.f) return;            // a non-finite gradient somewhere: the whole step is skipped
    inv_scale = 1.f / state[0];
  }
  constexpr int NS = 1 + (MOM ? 1 : 0) + (CENTERED ? 1 : 0);
  const srk_adam_block blk = a.blocks[blockIdx.x];
  const srk_adam_slot sl = a.slots[blk.slot];
  const float alpha = (float)a.alpha, oma = (float)(1.0 - a.alpha), eps = (float)a.eps, mom = (float)a.momentum;
  const float wd = (float)a.weight_decay, nlr = (float)(-a.lr);
  const bool has_wd = a.weight_decay != 0.0, maximize = a.maximize != 0;
  const bool lerp_low = oma < 0.5f;          // at::lerp's two forms
  const float omw = 1.f - oma;
  const long long e0 = blk.start, e1 = (e0 + blk.count < sl.n) ? e0 + blk.count : sl.n;
  auto upd = [&](float& pv, float gv, float (&sv)[NS]) {
    if constexpr (SCALED) gv *= inv_scale;
    gv = maximize ? -gv : gv;
    gv = has_wd ? gv + wd * pv : gv;                          // grad.add(param, alpha=weight_decay)
    float& sq = sv[0];
    sq = sq * alpha + oma * gv * gv;                          // square_avg.mul_(alpha).addcmul_(grad, grad, value=1 - alpha)
    float avg;
    if constexpr (CENTERED) {
      float& ga = sv[NS - 1];
      const float d = gv - ga;
      ga = lerp_low ? ga + oma * d : gv - d * omw;            // grad_avg.lerp_(grad, 1 - alpha)
      avg = sqrtf(sq - ga * ga);                              // square_avg.addcmul(grad_avg, grad_avg, value=-1).sqrt_()
    } else {
      avg = sqrtf(sq);
    }
    avg += eps;
    if constexpr (MOM) {
      float& b = sv[1];
      b = b * mom + gv / avg;                                 // buf.mul_(momentum).addcdiv_(grad, avg)
      pv = pv + nlr * b;                                      // param.add_(buf, alpha=-lr)
    } else {
      pv = pv + nlr * (gv / avg);                             // param.addcdiv_(grad, avg, value=-lr)
    }
  };
  float* s[NS];
  s[0] = a.sq + sl.state_off;
  if constexpr (MOM) s[1] = a.buf + sl.state_off;
  if constexpr (CENTERED) s[NS - 1] = a.ga + sl.state_off;
  float* const (&sc)[NS] = s;
  state_block<NS, true>(sl.p, sl.g, sc, e0, e1, upd);
}

// the gradient check and the count bump are Adam's kernels: they read the table (and `steps`) only
void table_check_launch(const srk_adam_slot* slots, const srk_adam_block* blocks, int nslots, int nblocks, float* scaler_state, hipStream_t st) {
  srk_adam_args c{};
  c.slots = slots; c.blocks = blocks; c.nslots = nslots; c.nblocks = nblocks;
  hipLaunchKernelGGL(adam_check_kernel, dim3((unsigned)nblocks), dim3(ADAM_NT), 0, st, c, scaler_state);
}

void table_bump_launch(const srk_adam_slot* slots, int nslots, float* steps, const float* scaler_state, hipStream_t st) {
  srk_adam_args c{};
  c.slots = slots; c.nslots = nslots; c.steps = steps;
  hipLaunchKernelGGL(adam_bump_kernel, dim3((unsigned)((nslots + ADAM_NT - 1) / ADAM_NT)), dim3(ADAM_NT), 0, st, c, scaler_state);
}

int sgd_check_args(const srk_sgd_args* a, const char* fn) {
  SRK_CHECK_ARG(a && a->slots && a->blocks, "%s: null table", fn);
  SRK_CHECK_ARG(a->nblocks > 0 && a->nslots > 0, "%s: %d blocks, %d tensors", fn, a->nblocks, a->nslots);
  SRK_CHECK_ARG(a->momentum == 0.0 || (a->buf && a->steps), "%s: momentum=%g needs the momentum buffer and the counts", fn, a->momentum);
  SRK_CHECK_ARG(a->lr >= 0.0 && a->momentum >= 0.0 && a->weight_decay >= 0.0 && (!a->nesterov || (a->momentum > 0.0 && a->dampening == 0.0)),
                "%s: lr=%g momentum=%g dampening=%g weight_decay=%g nesterov=%d", fn, a->lr, a->momentum, a->dampening, a->weight_decay, a->nesterov);
  return 0;
}

// momentum == 0: no count is kept (nothing is "first"), so the update is the only launch
void sgd_launch(const srk_sgd_args* a, const float* scaler_state, hipStream_t st) {
  const dim3 grid((unsigned)a->nblocks), block(ADAM_NT);
  const bool mom = a->momentum != 0.0;
  if (scaler_state) {
    if (mom) hipLaunchKernelGGL((sgd_group_kernel<true, true>), grid, block, 0, st, *a, scaler_state);
    else hipLaunchKernelGGL((sgd_group_kernel<true, false>), grid, block, 0, st, *a, scaler_state);
  } else {
    if (mom) hipLaunchKernelGGL((sgd_group_kernel<false, true>), grid, block, 0, st, *a, scaler_state);
    else hipLaunchKernelGGL((sgd_group_kernel<false, false>), grid, block, 0, st, *a, scaler_state);
  }
  if (mom) table_bump_launch(a->slots, a->nslots, a->steps, scaler_state, st);
}

int rmsprop_check_args(const srk_rmsprop_args* a, const char* fn) {
  SRK_CHECK_ARG(a && a->slots && a->blocks, "%s: null table", fn);
  SRK_CHECK_ARG(a->nblocks > 0 && a->nslots > 0, "%s: %d blocks, %d tensors", fn, a->nblocks, a->nslots);
  SRK_CHECK_ARG(a->sq && a->steps && (a->momentum <= 0.0 || a->buf) && (!a->centered || a->ga), "%s: null state pointer", fn);
  SRK_CHECK_ARG(a->lr >= 0.0 && a->alpha >= 0.0 && a->eps >= 0.0 && a->momentum >= 0.0 && a->weight_decay >= 0.0,
                "%s: lr=%g alpha=%g eps=%g momentum=%g weight_decay=%g", fn, a->lr, a->alpha, a->eps, a->momentum, a->weight_decay);
  return 0;
}

template <bool SCALED>
void rmsprop_launch_as(const srk_rmsprop_args* a, const float* scaler_state, hipStream_t st) {
  const dim3 grid((unsigned)a->nblocks), block(ADAM_NT);
  const bool mom = a->momentum > 0.0, cen = a->centered != 0;
  if (mom && cen) hipLaunchKernelGGL((rmsprop_group_kernel<SCALED, true, true>), grid, block, 0, st, *a, scaler_state);
  else if (mom) hipLaunchKernelGGL((rmsprop_group_kernel<SCALED, true, false>), grid, block, 0, st, *a, scaler_state);
  else if (cen) hipLaunchKernelGGL((rmsprop_group_kernel<SCALED, false, true>), grid, block, 0, st, *a, scaler_state);
  else hipLaunchKernelGGL((rmsprop_group_kernel<SCALED, false, false>), grid, block, 0, st, *a, scaler_state);
}

void rmsprop_launch(const srk_rmsprop_args* a, const float* scaler_state, hipStream_t st) {
  if (scaler_state) rmsprop_launch_as<true>(a, scaler_state, st);
  else rmsprop_launch_as<false>(a, scaler_state, st);
  table_bump_launch(a->slots, a->nslots, a->steps, scaler_state, st);
}
}  // namespace

// The four shapes of Adam's entry points (one group; one group under loss scaling; the check / update halves for several groups)
#define SRK_TABLE_STEP_ENTRIES(NAME, ARGS)                                                                              \
  extern "C" int srk_##NAME##_step(const ARGS* a, srk_stream_t stream) {                                               \
    if (int rc = NAME##_check_args(a, "srk_" #NAME "_step")) return rc;                                                \
    NAME##_launch(a, nullptr, reinterpret_cast<hipStream_t>(stream));                                                  \
    SRK_LAUNCH_CHECK();                                                                                                \
    return 0;                                                                                                          \
  }                                                                                                                    \
  extern "C" int srk_##NAME##_step_scaled(const ARGS* a, float* scaler_state, srk_stream_t stream) {                   \
    if (int rc = NAME##_check_args(a, "srk_" #NAME "_step_scaled")) return rc;                                         \
    SRK_CHECK_ARG(scaler_state, "srk_" #NAME "_step_scaled: null scaler state");                                       \
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);                                                            \
    table_check_launch(a->slots, a->blocks, a->nslots, a->nblocks, scaler_state, st);                                  \
    NAME##_launch(a, scaler_state, st);                                                                                \
    SRK_LAUNCH_CHECK();                                                                                                \
    return 0;                                                                                                          \
  }                                                                                                                    \
  extern "C" int srk_##NAME##_check_scaled(const ARGS* a, float* scaler_state, srk_stream_t stream) {                  \
    SRK_CHECK_ARG(a && a->slots && a->blocks && scaler_state, "srk_" #NAME "_check_scaled: null pointer");             \
    SRK_CHECK_ARG(a->nblocks > 0 && a->nslots > 0, "srk_" #NAME "_check_scaled: %d blocks, %d tensors", a->nblocks, a->nslots); \
    table_check_launch(a->slots, a->blocks, a->nslots, a->nblocks, scaler_state, reinterpret_cast<hipStream_t>(stream)); \
    SRK_LAUNCH_CHECK();                                                                                                \
    return 0;                                                                                                          \
  }                                                                                                                    \
  extern "C" int srk_##NAME##_update_scaled(const ARGS* a, const float* scaler_state, srk_stream_t stream) {           \
    if (int rc = NAME##_check_args(a, "srk_" #NAME "_update_scaled")) return rc;                                       \
    SRK_CHECK_ARG(scaler_state, "srk_" #NAME "_update_scaled: null scaler state");                                     \
    NAME##_launch(a, scaler_state, reinterpret_cast<hipStream_t>(stream));                                             \
    SRK_LAUNCH_CHECK();                                                                                                \
    return 0;                                                                                                          \
  }

SRK_TABLE_STEP_ENTRIES(sgd, srk_sgd_args)
SRK_TABLE_STEP_ENTRIES(rmsprop, srk_rmsprop_args)
#undef SRK_TABLE_STEP_ENTRIES
